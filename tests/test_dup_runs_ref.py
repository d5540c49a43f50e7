"""CPU checks of tests/dup_runs_ref.py: the oracle agrees with numpy on every
duplicate-bearing case, the host model of the union walk equals np.unique,
every ablation of its seed is caught by a named case, and each construction
puts its run where its name says.  No GPU: the evidence that the cases of
test_dup_runs_gpu.py can fail is obtained here, not by altering kernels."""
import numpy as np
import pytest

import dup_runs_ref as R
from oracle import bind as orc

TILE = R.TILE
X = R.X

# the case each ablation must change, and why
CATCHERS = {
    # tile 1 starts right behind u's X and v has nothing below X
    1: "allB_after_ua",
    # a tile head inside v's run, and u has no X: b_before alone holds X.  (With
    # A first on ties the mirror of allB_after_ua cannot do this: there u's
    # copies precede v's, so a_before is X wherever b_before is.)
    2: f"run_u_L{TILE - 1}_mirror",
    # a tile head inside u's run: last B before is a smaller value
    3: f"run_u_L{TILE - 1}",
    # path positions 39 and 40 lie in two thread segments
    4: "run_u_L2",
    # the run of 0 is longer than thread 0's segment
    5: "zero_head_u",
}


def test_case_inventory():
    names = set(R.UNION_BY_NAME)
    for L in R.RUN_LENS:
        assert f"run_u_L{L}" in names and f"run_u_L{L}_mirror" in names
    for a, b in R.BOTH_COPIES:
        for before in R.BEFORES:
            for pu, pv in R.PARITIES[1:]:
                assert f"both_a{a}_b{b}_before{before}_p{pu}{pv}" in names
                assert f"both_a{a}_b{b}_before{before}_p{pu}{pv}_mirror" in names
    for c in R.UNION_CASES:
        assert c.u.size <= 4 * TILE + 8 and c.v.size <= 4 * TILE + 8, c.name
    for lists in R.tree_cases().values():
        assert len(lists) <= 33 and all(x.size <= R.TREE_N for x in lists)
    assert sorted({R.sort_rounds(n) for n in R.SORT_NS}) == [0, 1, 2, 3]


def test_oracle_equals_numpy_union():
    for c in R.UNION_CONTENT_CASES:
        want = c.want["merge"]
        assert np.array_equal(orc.merge_sorted([c.u, c.v]), want), c.name
        assert np.array_equal(orc.merge_sorted([c.u]), np.unique(c.u)), c.name
    for name, lists in R.tree_cases().items():
        want = R.want_union(*lists)
        assert np.array_equal(orc.merge_sorted(lists), want), name
        k = len(lists)
        distinct = 3 if name.startswith("three") else k if name.startswith("ragged") \
            else k - (k - 1) % 2  # gaps: the last non-empty list is the widest
        assert want.size == distinct, name


def test_oracle_equals_numpy_index_of():
    for name, u, q in R.index_cases():
        want = R.want_index_of(u, q)
        assert [orc.index_of(u, int(x)) for x in q] == want.tolist(), name
    # the first index of a run, not any index of it
    _, u, _ = R.index_cases()[0]
    assert R.want_index_of(u, [2**63, 5, 2**40]).tolist() == [708, 0, 4]


def test_oracle_equals_numpy_fold():
    cases = R.fold_cases()
    for name, lists in cases.items():
        want = R.want_fold(lists)
        assert np.array_equal(orc.intersect_sorted(lists), want), name
        for x in lists:
            assert np.all(x[1:] > x[:-1]), name  # the fold's domain is duplicate-free
    for k in (9, 150):
        want = R.want_fold(cases[f"planted_k{k}"])
        assert want.size >= 300 and want[0] == 0 and want[-1] == R.U64_MAX
    assert R.want_fold(cases["to_one_k9"]).tolist() == [2**63]
    assert len({x.size for x in cases["equal_len_k9"]}) == 1
    assert R.want_fold(cases["equal_len_k9"]).size >= 200
    # smallest first, stable: the six B - C_j lists come first, one chunk goes
    # per round (two in the first), nothing is left after round 5 of 9
    lists = cases["empties_at_round5_k10"]
    order = sorted(range(len(lists)), key=lambda i: lists[i].size)
    assert order == list(range(10))
    cur, sizes = lists[0], []
    for x in lists[1:]:
        cur = np.intersect1d(cur, x)
        sizes.append(cur.size)
    assert sizes[:5] == [2000, 1500, 1000, 500, 0] and len(sizes) == 9


def test_model_equals_unique():
    for c in R.UNION_CONTENT_CASES:
        assert np.array_equal(R.model_union(c.u, c.v), c.want["merge"]), c.name


def test_every_ablation_is_caught(capsys):
    """Each broken seed changes the output of the case named for it; the full
    list of catching cases is printed (pytest -s)."""
    caught = {a: [] for a in R.ABLATIONS if a}
    for c in R.UNION_CONTENT_CASES:
        for a in caught:
            if not np.array_equal(R.model_union(c.u, c.v, a), c.want["merge"]):
                caught[a].append(c.name)
    with capsys.disabled():
        for a, names in caught.items():
            print(f"\nablation {a} ({R.ABLATIONS[a]}): caught by {len(names)}: "
                  + ", ".join(names))
    for a, name in CATCHERS.items():
        assert name in caught[a], f"ablation {a} ({R.ABLATIONS[a]}) passes {name}"
    # the two sides are told apart: a_before's case does not need b_before
    assert CATCHERS[1] not in caught[2] and CATCHERS[2] not in caught[1]


def test_run_positions():
    """Host arithmetic: every run sits where the case's name says."""
    for L in R.RUN_LENS:
        c = R.UNION_BY_NAME[f"run_u_L{L}"]
        assert R.run_span(c.u, c.v, X) == (R.RUN_START, R.RUN_START + L - 1)
        assert np.count_nonzero(c.v == X) == 0 and np.count_nonzero(c.u == X) == L
    assert R.RUN_START % R.WPT == R.WPT - 1  # L = 2 lies in two thread segments
    starts, ends = set(), set()
    for a, b in R.BOTH_COPIES:
        for before in R.BEFORES:
            c = R.UNION_BY_NAME[f"both_a{a}_b{b}_before{before}"]
            first, last = R.run_span(c.u, c.v, X)
            assert (first, last) == (before, before + a + b - 1)
            assert np.count_nonzero(c.u == X) == a and np.count_nonzero(c.v == X) == b
            starts.add(first)
            ends.add((last + 1) % TILE)
    assert starts == {TILE - 1, TILE, TILE + 1}
    assert 0 in ends  # a run whose last element is the last of a tile
    c = R.UNION_BY_NAME[f"both_a2048_b2048_before{TILE}"]
    assert R.run_span(c.u, c.v, X) == (TILE, 3 * TILE - 1)


def test_whole_tiles_inside_runs():
    # tiles 1 and 2 of the longest run are X only, all from u: they emit nothing
    c = R.UNION_BY_NAME[f"run_u_L{3 * TILE + 5}"]
    merged, from_a = R.merge_path(c.u, c.v)
    assert np.all(merged[TILE:3 * TILE] == X) and np.all(from_a[TILE:3 * TILE])
    geo = R.tile_geometry(c.u, c.v)
    assert geo[1][1:] == (TILE, 19, 0) and geo[2][1:] == (TILE, 19, 0)
    # the last partial tile is UINT64_MAX only
    for name, start in (("max_tail_fill", TILE), ("max_tail_over", TILE - 48)):
        c = R.UNION_BY_NAME[name]
        merged, _ = R.merge_path(c.u, c.v)
        assert TILE < merged.size < 2 * TILE and np.all(merged[TILE:] == R.U64_MAX)
        assert R.run_span(c.u, c.v, R.U64_MAX)[0] == start
    # the sort path's packed words: top bit set on ascending keys
    top = [bool(np.all(a >= np.uint64(2**63))) for a in R.packed_segments()]
    assert sorted(top) == [False, False, True, True]
    c = R.UNION_BY_NAME["doubles_triples"]
    assert 3 * TILE <= c.u.size + c.v.size
    assert np.all(np.unique(c.u, return_counts=True)[1] >= 2)
    assert np.all(np.unique(c.v, return_counts=True)[1] >= 2)
    c = R.UNION_BY_NAME["zero_head_both"]
    assert c.u[0] == 0 and c.v[0] == 0 and R.run_span(c.u, c.v, 0) == (0, TILE + 61)


def test_all_b_tiles():
    """Tiles with alen == 0 and a0 > 0 (has_ab with an empty A range)."""
    c = R.UNION_BY_NAME["allB_after_ua"]
    geo = R.tile_geometry(c.u, c.v)
    assert c.u.size == TILE and c.u[-1] == X
    assert geo[1] == (TILE, 0, 0, TILE)  # a_before = X is the only seed: b0 == 0
    assert geo[2] == (TILE, 0, TILE, 3000 - TILE)
    # mirrored, A first on ties: v's low values, then u's 3000 X, v's X last;
    # tile 1 is all-A with blen == 0 and has_bb
    assert R.tile_geometry(c.v, c.u)[1] == (1, TILE, TILE - 1, 0)
    c = R.UNION_BY_NAME["allB_after_ua_short"]
    assert R.tile_geometry(c.u, c.v)[1] == (101, 0, TILE - 101, 3101 - TILE)
    # u's X last in tile 0, v's 2048 copies are tile 1: a0 > 0, alen == 0, b0 > 0
    c = R.UNION_BY_NAME[f"both_a1_b2048_before{TILE - 1}"]
    a0, alen, b0, blen = R.tile_geometry(c.u, c.v)[1]
    assert a0 > 0 and alen == 0 and b0 > 0 and blen == TILE


@pytest.mark.parametrize("name", ["both_a1_b2048_before2047", "allB_after_ua",
                                  "allB_after_ua_mirror", "equal_n5000_m0"])
def test_guards(name):
    """The slice guards: own[0] before, a value of the other list after."""
    c = R.UNION_BY_NAME[name]
    for own, other in ((c.u, c.v), (c.v, c.u)):
        for par in (0, 1):
            big, off = R.guarded(own, other, par)
            assert off == 2 - par and np.array_equal(big[off:off + own.size], own)
            if own.size:
                assert np.all(big[:off] == own[0])
            if other.size:
                assert np.all(np.isin(big[off + own.size:], other))
