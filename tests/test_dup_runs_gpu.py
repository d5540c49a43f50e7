"""The duplicate half of the contract on the GPU: MergeSorted's dedup on long
equal runs (k_tiles<OP_UNION>: the per-thread previous value seeded from
a_before / b_before), the k-way union tree on lists that collapse after round
0, the keep-all merge and the segmented sort on ties that span tiles
(MODE_DIRECT), k_index_of on runs and at its edges, and the IntersectSorted
fold with a result that stays non-empty.  The cases and what each is for are
in dup_runs_ref.py; test_dup_runs_ref.py shows on the host that each of five
plausible seed bugs changes the output of one of them.

Expected values come from numpy (np.unique / np.sort / np.searchsorted) and
are compared with the oracle too where it has the call.  Outputs are
pre-filled with -1 and one element longer than their capacity, and that cell
must keep its fill.  No list is longer than about 8 200 elements,
except the fold's random lists (those of test_parity_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import dup_runs_ref as R
from dgraph_amd import algo
from dgraph_amd._lib import check, lib
from oracle import bind as orc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CAP_FILL = 0x5A5A5A5A5A5A5A5A  # no case holds it (the union fill, -1, is UINT64_MAX)


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


_DEV = {}


def dev(c):
    """(du, dv): slices of larger device tensors at the case's parities, with
    guards around them (R.guarded); uploaded once per case."""
    if c.name not in _DEV:
        out = []
        for own, other, par in ((c.u, c.v, c.pu), (c.v, c.u, c.pv)):
            big, off = R.guarded(own, other, par)
            t = to_dev(big)
            s = t[off:off + own.size]
            assert own.size == 0 or (s.data_ptr() >> 3) & 1 == par
            out.append(s)
        _DEV[c.name] = tuple(out)
    return _DEV[c.name]


def new_outs(cases, fill=-1):
    return [torch.full((c.u.size + c.v.size + 1,), fill, dtype=torch.int64, device=DEV)
            for c in cases]


def check_outs(cases, outs, lens, key, what):
    for c, o, n in zip(cases, outs, lens):
        w = c.want[key]
        got = to_np(o)
        assert int(n) == w.size, f"{what}: {c.name}: length {n} != {w.size}"
        assert np.array_equal(got[:w.size], w), f"{what}: {c.name}"
        # the cell behind the capacity n + m (for the keep-all merge, behind the result)
        assert got[-1] == R.U64_MAX, f"{what}: {c.name}: wrote past its capacity"


def run_union_paths(eng, cases):
    du = [dev(c)[0] for c in cases]
    dv = [dev(c)[1] for c in cases]
    outs = new_outs(cases)
    _, lens = eng.merge_pairs(du, dv, outs)
    check_outs(cases, outs, lens, "merge", "one-shot merge")
    outs = new_outs(cases)
    _, lens = eng.merge_all_pairs(du, dv, outs)
    check_outs(cases, outs, lens, "merge_all", "keep-all merge")
    outs = new_outs(cases)
    b = eng.make_batch(du, dv, outs)
    try:
        for what, run in (("prepared merge 1 (computes splits)", lambda: b.run(algo.OP_MERGE)),
                          ("prepared merge 2 (cached splits)", lambda: b.run(algo.OP_MERGE)),
                          ("prepared merge x3, one sync", lambda: b.run_n(algo.OP_MERGE, 3))):
            for o in outs:
                o.fill_(-1)
            check_outs(cases, outs, run(), "merge", what)
    finally:
        b.close()


BASE_NAMES = [c.name for c in R.UNION_CASES if not c.name.endswith("_mirror")]


@pytest.mark.parametrize("name", BASE_NAMES)
def test_union_single_pair(eng, name):
    """The case and its mirror, each alone: one-shot union, keep-all merge,
    prepared union (splits computed, cached, and three passes under one sync),
    MergeSorted with k = 1 and the host form."""
    for c in (R.UNION_BY_NAME[name], R.UNION_BY_NAME[name + "_mirror"]):
        run_union_paths(eng, [c])
        du, dv = dev(c)
        assert np.array_equal(to_np(eng.merge_sorted([du])), np.unique(c.u)), f"k=1: {c.name}"
        assert np.array_equal(to_np(eng.merge_sorted([du, dv])), c.want["merge"]), \
            f"k=2 tree: {c.name}"
        if (c.pu, c.pv) == (0, 0):
            assert np.array_equal(algo.merge_sorted(eng, [c.u, c.v]), c.want["merge"]), \
                f"host form: {c.name}"


def test_union_mixed_batch(eng):
    """Every case in one grid: tiles that emit nothing next to other pairs'
    tiles, pairs without tiles in between."""
    run_union_paths(eng, R.UNION_CASES)


# ---- k-way union tree ----

@pytest.mark.parametrize("name", list(R.tree_cases()))
def test_union_tree(eng, name):
    """Round 0 leaves a handful of values per pair; every later round is tiled
    by capacity, so almost all of its tiles lie past the path."""
    lists = R.tree_cases()[name]
    want = R.want_union(*lists)
    assert np.array_equal(orc.merge_sorted(lists), want)
    got = to_np(eng.merge_sorted([to_dev(x) for x in lists]))
    assert np.array_equal(got, want), name
    assert np.array_equal(algo.merge_sorted(eng, lists), want), f"host form: {name}"


# ---- segmented sort (bitonic chunks + MODE_DIRECT merge rounds) ----

def sort_and_check(eng, arrs, what):
    tensors = [to_dev(a) for a in arrs]
    eng.sort_segments(tensors)
    for i, (a, t) in enumerate(zip(arrs, tensors)):
        assert np.array_equal(to_np(t), np.sort(a)), f"{what}: segment {i} (n = {a.size})"


@pytest.mark.parametrize("n", R.SORT_NS)
def test_sort_few_distinct(eng, n):
    """1, 2 and 3 distinct values: every merge round is ties across tiles."""
    sort_and_check(eng, [R.sort_segments()[(n, d)] for d in (1, 2, 3)], f"n{n}")


def test_sort_mixed_rounds(eng):
    """Segments with 0, 1, 2 and 3 merge rounds in one call: each starts on
    the side it will end on."""
    segs = R.sort_segments()
    arrs = [segs[(n, d)] for d in (3, 1, 2) for n in R.SORT_NS]
    assert {R.sort_rounds(a.size) for a in arrs} == {0, 1, 2, 3}
    sort_and_check(eng, arrs, "mixed")


def test_sort_packed_words(eng):
    """key << 32 | pos with the top bit set, ascending keys and flipped ones."""
    arrs = R.packed_segments()
    assert any(np.all(a >= np.uint64(2**63)) for a in arrs)
    sort_and_check(eng, arrs, "packed")


# ---- IndexOf ----

@pytest.mark.parametrize("name", [c[0] for c in R.index_cases()])
def test_index_of(eng, name):
    _, u, q = next(c for c in R.index_cases() if c[0] == name)
    want = R.want_index_of(u, q)
    du, dq = to_dev(u), to_dev(q)
    out = torch.full((q.size + 1,), -7, dtype=torch.int64, device=DEV)
    check(lib().ua_index_of_batch_dev(eng._ctx, C.c_void_p(du.data_ptr()), u.size,
                                      C.c_void_p(dq.data_ptr()), q.size,
                                      C.c_void_p(out.data_ptr())))
    got = out.cpu().numpy()
    assert got[:q.size].tolist() == want.tolist()
    assert got[q.size] == -7, "wrote past out[nq - 1]"
    assert eng.index_of_batch(du, dq).cpu().numpy().tolist() == want.tolist()


# ---- IntersectSorted fold ----

@pytest.mark.parametrize("name", list(R.fold_cases()))
def test_intersect_fold(eng, name):
    lists = R.fold_cases()[name]
    want = orc.intersect_sorted(lists)
    assert np.array_equal(want, R.want_fold(lists))
    if not name.startswith("empties"):
        assert want.size > 0
    got = to_np(eng.intersect_sorted([to_dev(x) for x in lists]))
    assert np.array_equal(got, want), name


# ---- capacity promise on duplicates (uidalgo.h: all writes stay within each
# pair's out capacity; the values are unspecified and not asserted) ----

CAP_PAD = 8


def cap_outs(cases, cap_of):
    return [torch.full((cap_of(c) + CAP_PAD,), CAP_FILL, dtype=torch.int64, device=DEV)
            for c in cases]


def check_caps(cases, outs, lens, cap_of, what):
    for c, o, n in zip(cases, outs, lens):
        cap = cap_of(c)
        assert int(n) <= cap, f"{what}: {c.name}: length {n} > capacity {cap}"
        assert np.all(o[cap:].cpu().numpy() == CAP_FILL), f"{what}: {c.name}: wrote past capacity"


CAP_OPS = (("intersect", algo.OP_INTERSECT, lambda c: min(c.u.size, c.v.size)),
           ("difference", algo.OP_DIFFERENCE, lambda c: c.u.size))


@pytest.mark.parametrize("opname", ["intersect", "difference"])
def test_capacity_on_duplicates(eng, opname):
    _, op, cap_of = next(x for x in CAP_OPS if x[0] == opname)
    cases = R.UNION_CASES
    assert all(CAP_FILL not in c.want["merge"] for c in R.UNION_CONTENT_CASES)
    du = [dev(c)[0] for c in cases]
    dv = [dev(c)[1] for c in cases]
    fn = eng.intersect_pairs if op == algo.OP_INTERSECT else eng.difference_pairs
    outs = cap_outs(cases, cap_of)
    _, lens = fn(du, dv, outs)
    check_caps(cases, outs, lens, cap_of, f"one-shot {opname}")
    outs = cap_outs(cases, cap_of)
    b = eng.make_batch(du, dv, outs)
    try:
        for what in ("prepared run 1", "prepared run 2 (cached splits)"):
            for o in outs:
                o.fill_(CAP_FILL)
            check_caps(cases, outs, b.run(op), cap_of, f"{what} {opname}")
    finally:
        b.close()


@pytest.mark.parametrize("opname", ["intersect", "difference"])
def test_capacity_on_narrow_tiles(eng, opname):
    """All values share their upper 32 bits, so the prepared batch walks the
    32-bit copy: full tiles of one repeated value, with and without the
    sentinel walk."""
    _, op, cap_of = next(x for x in CAP_OPS if x[0] == opname)
    cases = [R.UNION_BY_NAME[n] for n in (f"both_a2048_b2048_before{R.TILE}",
                                          f"both_a2048_b2048_before{R.TILE}_mirror",
                                          f"both_a1_b2048_before{R.TILE - 1}",
                                          "doubles_triples", "equal_n5000_m5000")]
    for c in cases:
        assert max(int(c.u[-1]), int(c.v[-1])) < 2**32
    du = [dev(c)[0] for c in cases]
    dv = [dev(c)[1] for c in cases]
    outs = cap_outs(cases, cap_of)
    b = eng.make_batch(du, dv, outs)
    try:
        for what in ("narrow run 1", "narrow run 2"):
            for o in outs:
                o.fill_(CAP_FILL)
            check_caps(cases, outs, b.run(op), cap_of, f"{what} {opname}")
            assert b.info()["narrow_tiles"] > 0
    finally:
        b.close()
