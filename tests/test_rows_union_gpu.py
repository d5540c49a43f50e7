"""GPU parity of the flat sort-unique DestUIDs path (Engine.union_rows,
dest_uids, update_dest_uids): the ascending duplicate-free set of a CSR UID
matrix's flat element array.  Expected values come from the CPU oracle's
merge_sorted for sorted rows and from numpy's unique otherwise; every
comparison is exact.

The leaf is 2048 flat elements and the union tree pairs leaves, so the shapes
are the smallest that reach each boundary: the 64-lane keep-word, the leaf,
odd leaf counts at one and at several tree levels.  One moderate shape
(4096 short rows, 65 leaves, 7 rounds) runs a deeper tree once.
"""
import json
import os

import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth
from oracle import bind as orc

pytestmark = pytest.mark.gpu

LEAF = 2048
TOP = (1 << 64) - 1
GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))


def u64(x):
    return np.asarray(x, dtype=np.uint64)


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.empty(0, dtype=torch.int64, device="cuda:0")
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def flat(rows):
    rows = [u64(r) for r in rows]
    return np.concatenate(rows) if rows else np.empty(0, dtype=np.uint64)


def union_dev(eng, vals):
    return to_np(eng.union_rows(to_dev(vals)))


def check_rows(eng, rows, want, what=""):
    """Both entry points against one expected set."""
    want = u64(want)
    got = union_dev(eng, flat(rows))
    assert np.array_equal(got, want), f"union_rows {what}"
    got = algo.dest_uids(eng, rows)
    assert got.dtype == np.uint64 and np.array_equal(got, want), f"dest_uids {what}"


def rows_of(vals, n):
    return [vals[i:i + n] for i in range(0, vals.size, n)]


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


# ---------- 1. the reference's MergeSorted tables ----------

@pytest.mark.parametrize("case", GOLDEN["merge_sorted"], ids=lambda c: c["name"])
def test_golden_merge_sorted_tables(eng, case):
    rows = [u64(l) for l in case["input"]]
    assert orc.merge_sorted(rows).tolist() == case["out"]
    check_rows(eng, rows, case["out"], case["name"])


# ---------- 2. leaf boundaries ----------

TOTALS = [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4096, 4097]


@pytest.mark.parametrize("total", TOTALS)
def test_leaf_boundaries_one_ascending_row(eng, total):
    """Strictly ascending: every leaf skips the sort network."""
    vals = np.arange(total, dtype=np.uint64) * np.uint64(3) + np.uint64(5)
    check_rows(eng, [vals], orc.merge_sorted([vals]), f"total={total}")
    assert union_dev(eng, vals).size == total


@pytest.mark.parametrize("total", TOTALS)
def test_leaf_boundaries_rows_of_three(eng, total):
    """Sorted rows of length 3: leaves straddle rows, so the sort is taken."""
    rng = np.random.default_rng(synth.SEED + 600 + total)
    vals = rng.integers(0, max(2 * total, 4), size=total, dtype=np.uint64)
    rows = [np.sort(r) for r in rows_of(vals, 3)]
    check_rows(eng, rows, orc.merge_sorted(rows), f"total={total}")


# ---------- 3. tree shapes: odd items at one and at several levels ----------

@pytest.mark.parametrize("total", [3 * LEAF - 7, 4 * LEAF + 1, 5 * LEAF + 1, 33 * LEAF])
def test_tree_shapes(eng, total):
    """3, 5, 6 and 33 leaves: 3 -> 2 -> 1, 5 -> 3 -> 2 -> 1, 6 -> 3 -> 2 -> 1 and
    33 -> 17 -> 9 -> 5 -> 3 -> 2 -> 1."""
    rng = np.random.default_rng(synth.SEED + 610 + total)
    vals = rng.integers(0, total // 2, size=total, dtype=np.uint64)
    want = np.unique(vals)
    assert want.size < total
    assert np.array_equal(union_dev(eng, vals), want)
    rows = [np.sort(r) for r in rows_of(vals, 1000)]
    assert np.array_equal(orc.merge_sorted(rows), want)
    assert np.array_equal(algo.dest_uids(eng, rows), want)


# ---------- 4. duplicates ----------

def test_duplicates(eng):
    one = np.full(LEAF, 42, dtype=np.uint64)
    check_rows(eng, [one], [42], "a tile of one value")
    check_rows(eng, [np.full(3 * LEAF, 42, dtype=np.uint64)], [42], "3 leaves of one value")
    check_rows(eng, [np.full(2 * LEAF + 9, 0, dtype=np.uint64)], [0], "3 leaves of zero")
    # non-decreasing, not strict: the sort is skipped, the dedup must still run
    pairs = np.repeat(np.arange(1, LEAF // 2 + 1, dtype=np.uint64), 2)
    assert pairs.size == LEAF and pairs[:4].tolist() == [1, 1, 2, 2]
    check_rows(eng, [pairs], orc.merge_sorted([pairs]), "[1,1,2,2,...]")
    twice = np.repeat(np.arange(LEAF + 100, dtype=np.uint64), 2)  # 2 leaves and 200
    check_rows(eng, [twice], np.arange(LEAF + 100), "pairs across leaves")
    # one value as the last element of leaf i and the first of leaf i + 1
    asc = np.arange(3 * LEAF, dtype=np.uint64)
    asc[LEAF] = asc[LEAF - 1]
    asc[2 * LEAF] = asc[2 * LEAF - 1]
    want = orc.merge_sorted([asc])
    assert want.size == 3 * LEAF - 2
    check_rows(eng, [asc], want, "equal across a leaf boundary")
    # all rows identical
    row = synth.gen_sorted_unique(np.random.default_rng(synth.SEED + 620), 700, 5000)
    check_rows(eng, [row] * 9, orc.merge_sorted([row] * 9), "identical rows")
    assert np.array_equal(orc.merge_sorted([row] * 9), row)


# ---------- 5. u64 extremes ----------

def test_u64_extremes_in_a_partial_last_tile(eng):
    """A signed compare would put 2^63.. before 0; the UINT64_MAX padding of
    the last tile must neither swallow nor duplicate a real UINT64_MAX."""
    b63 = 1 << 63
    ext = [0, b63 - 1, b63, TOP - 1, TOP]
    rng = np.random.default_rng(synth.SEED + 630)
    body = rng.integers(1, 1 << 40, size=LEAF, dtype=np.uint64)
    rows = [body[:1000], body[1000:],
            u64([TOP, 0, b63, TOP]),            # unsorted, UINT64_MAX twice
            u64([b63 - 1, TOP - 1, 7, TOP])]    # partial last tile: 8 elements
    vals = flat(rows)
    assert vals.size == LEAF + 8
    want = np.unique(vals)
    assert want[0] == 0 and want[-5:].tolist()[1:] == ext[1:] and want[-1] == TOP
    got = union_dev(eng, vals)
    assert np.array_equal(got, want)
    assert got[-4:].tolist() == ext[1:] and got[0] == 0
    assert np.array_equal(algo.dest_uids(eng, rows), want)
    # sorted rows of extremes only, against the oracle
    srows = [u64([0, b63 - 1, b63, TOP]), u64([0, TOP - 1, TOP, TOP]), u64([TOP])]
    check_rows(eng, srows, orc.merge_sorted(srows), "sorted extremes")
    assert orc.merge_sorted(srows).tolist() == ext


@pytest.mark.parametrize("n", [1, 5, LEAF - 1, LEAF, LEAF + 1])
def test_only_uint64_max(eng, n):
    check_rows(eng, [np.full(n, TOP, dtype=np.uint64)], [TOP], f"{n} x UINT64_MAX")


# ---------- 6. unsorted rows ----------

def test_shuffled_rows_with_duplicates(eng):
    rng = np.random.default_rng(synth.SEED + 640)
    rows = [rng.integers(0, 9000, size=n, dtype=np.uint64)
            for n in [0, 5, 64, 100, 2048, 3000, 1, 4097]]
    rows[3][:50] = rows[3][50:]  # guaranteed repeats inside a row
    want = np.unique(flat(rows))
    assert want.size < flat(rows).size
    check_rows(eng, rows, want, "shuffled rows")


def ref_update_dest_uids(rows, dest):
    """query/query.go:2594-2609, restated with the oracle's IndexOf/ApplyFilter."""
    included = np.zeros(dest.size, dtype=bool)
    for row in rows:
        for uid in row:
            idx = orc.index_of(dest, int(uid))
            if idx >= 0:
                included[idx] = True
    return orc.apply_filter(dest, included)


def test_update_dest_uids(eng):
    rng = np.random.default_rng(synth.SEED + 650)
    dest = synth.gen_sorted_unique(rng, 1500, 6000)   # holds uids absent from the matrix
    rows = [rng.integers(0, 8000, size=n, dtype=np.uint64)  # and the matrix, uids
            for n in [300, 0, 64, 1, 700, 65]]               # absent from dest
    rows[0][:20] = rows[4][:20]
    in_matrix = np.isin(dest, flat(rows))
    assert in_matrix.any() and not in_matrix.all()
    assert not np.isin(flat(rows), dest).all()
    want = ref_update_dest_uids(rows, dest)
    assert np.array_equal(want, dest[in_matrix])
    got = algo.update_dest_uids(eng, rows, dest)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert algo.update_dest_uids(eng, [], dest).size == 0
    assert algo.update_dest_uids(eng, rows, u64([])).size == 0
    ext = [u64([TOP, 0, 1 << 63]), u64([5, TOP])]
    edest = u64([0, 4, (1 << 63) - 1, 1 << 63, TOP])
    assert algo.update_dest_uids(eng, ext, edest).tolist() == \
        ref_update_dest_uids(ext, edest).tolist() == [0, 1 << 63, TOP]


# ---------- 7. empty rows ----------

def test_empty_rows(eng):
    e = u64([])
    rows = [e, u64([4, 9]), e, e, u64([1, 9, 30]), e]
    check_rows(eng, rows, orc.merge_sorted(rows), "empty rows between")
    assert orc.merge_sorted(rows).tolist() == [1, 4, 9, 30]
    check_rows(eng, [], [], "n_rows = 0")
    check_rows(eng, [e] * 7, [], "all rows empty")


# ---------- 8. aliasing and capacity ----------

def test_aliasing_and_capacity(eng):
    rng = np.random.default_rng(synth.SEED + 660)
    total = 2 * LEAF + 77
    vals = rng.integers(0, 3000, size=total, dtype=np.uint64)
    want = np.unique(vals)
    dv = to_dev(vals)
    got = eng.union_rows(dv, out=dv)          # out is vals
    assert got.data_ptr() == dv.data_ptr()
    assert np.array_equal(to_np(got), want)

    buf = torch.zeros(total + 8, dtype=torch.int64, device="cuda:0")
    buf[:total] = to_dev(vals)
    before = buf.clone()
    with pytest.raises(RuntimeError, match="uidalgo error 3"):  # UA_ERR_INVALID
        eng.union_rows(buf[:total], out=buf[8:])
    with pytest.raises(RuntimeError, match="uidalgo error 3"):
        eng.union_rows(buf[8:], out=buf[:total])
    with pytest.raises(ValueError):
        eng.union_rows(buf[:total],
                       out=torch.empty(total - 1, dtype=torch.int64, device="cuda:0"))
    assert torch.equal(buf, before)  # rejected calls wrote nothing
    out = torch.empty(total + 5, dtype=torch.int64, device="cuda:0")
    assert np.array_equal(to_np(eng.union_rows(buf[:total], out=out)), want)


# ---------- 9. determinism and workspace reuse ----------

def test_determinism_and_workspace_reuse(eng):
    rng = np.random.default_rng(synth.SEED + 670)
    vals = rng.integers(0, 20_000, size=5 * LEAF + 300, dtype=np.uint64)
    want = np.unique(vals)
    dv = to_dev(vals)
    lists = [synth.gen_sorted_unique(rng, n, 30_000) for n in (5000, 0, 2049, 7000)]
    dl = [to_dev(x) for x in lists]
    want_m = orc.merge_sorted(lists)
    rows = [synth.gen_sorted_unique(rng, n, 9000) for n in (3000, 0, 2500)]
    shared = synth.gen_sorted_unique(rng, 3000, 9000)
    offs = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.uint64)
    d_rv, d_ro, d_sh = to_dev(flat(rows)), to_dev(offs), to_dev(shared)
    want_f = flat([orc.intersect_with(r, shared) for r in rows])

    first = to_np(eng.union_rows(dv))
    assert np.array_equal(to_np(eng.merge_sorted(dl)), want_m)
    fv, _ = eng.filter_rows(d_rv, d_ro, d_sh)
    assert np.array_equal(to_np(fv), want_f)
    second = to_np(eng.union_rows(dv))
    assert np.array_equal(to_np(eng.merge_sorted(dl)), want_m)
    assert np.array_equal(first, want) and np.array_equal(second, want)
    assert np.array_equal(to_np(dv), vals)  # the input is left alone


# ---------- 10. statistics ----------

def test_stats_of_a_five_leaf_call(eng):
    total = 4 * LEAF + 100   # 5 leaves: 5 -> 3 -> 2 -> 1, R = 3 rounds
    R = 3
    vals = np.random.default_rng(synth.SEED + 680).integers(
        0, 50_000, size=total, dtype=np.uint64)
    dv = to_dev(vals)
    eng.union_rows(dv)  # workspace growth is not part of the count
    eng.stats_reset()
    got = to_np(eng.union_rows(dv))
    st = eng.stats()
    assert np.array_equal(got, np.unique(vals))
    # the leaf pass, then count + write per round
    assert st["launches"] == 1 + 2 * R
    # leaf pass 16 B per element; the tree's capacity bound: every round moves
    # every item, 8 * 3 B per element of capacity
    assert st["bytes_algorithmic"] == 16 * total + 24 * R * total
    assert st["kernel_ms"] > 0

    eng.stats_reset()
    assert eng.union_rows(to_dev([])).numel() == 0
    st = eng.stats()
    assert (st["launches"], st["bytes_algorithmic"], st["kernel_ms"]) == (0, 0, 0)


# ---------- 11. equivalence with the existing path ----------

def test_equals_merge_sorted_on_zipf_rows(eng):
    rng = np.random.default_rng(synth.SEED + 690)
    lens = np.clip(rng.zipf(1.4, size=300) - 1, 0, 2000)
    total = int(lens.sum())
    assert (lens == 0).any() and (lens == 2000).any() and 10_000 < total <= 80_000
    rows = [synth.gen_sorted_unique(rng, int(n), 30_000) for n in lens]
    want = orc.merge_sorted(rows)
    assert want.size < total
    got_new = union_dev(eng, flat(rows))
    got_old = to_np(eng.merge_sorted([to_dev(r) for r in rows]))
    assert np.array_equal(got_new, want)
    assert np.array_equal(got_old, want)


# ---------- 12. ua_merge_k_dev after the refactor ----------

@pytest.mark.parametrize("lens", [(3000,), (0,), (2500, 1), (0, 4097), (2049, 0, 6000),
                                  (1, 0, 2048, 5000, 63, 64, 65, 3001, 700)],
                         ids=lambda l: f"k{len(l)}-{sum(l)}")
def test_merge_sorted_unchanged(eng, lens):
    rng = np.random.default_rng(synth.SEED + 700 + sum(lens))
    lists = [synth.gen_sorted_unique(rng, n, 12_000) for n in lens]
    want = orc.merge_sorted(lists)
    assert np.array_equal(to_np(eng.merge_sorted([to_dev(x) for x in lists])), want)
    assert np.array_equal(algo.merge_sorted(eng, lists), want)


# ---------- 13. one moderate shape: a tree of 65 leaves and 7 rounds ----------

def test_many_short_rows(eng):
    rng = np.random.default_rng(synth.SEED + 710)
    lens = rng.integers(1, 65, size=4096)
    total = int(lens.sum())
    assert 32 * LEAF < total <= 80 * LEAF
    vals = rng.integers(0, total // 3, size=total, dtype=np.uint64)
    row_id = np.repeat(np.arange(lens.size), lens)
    vals = vals[np.lexsort((vals, row_id))]  # sorted inside each row
    want = np.unique(vals)
    assert np.array_equal(union_dev(eng, vals), want)
    offs = np.concatenate([[0], np.cumsum(lens)])
    rows = [vals[offs[r]:offs[r + 1]] for r in range(4096)]
    assert np.array_equal(orc.merge_sorted(rows), want)
