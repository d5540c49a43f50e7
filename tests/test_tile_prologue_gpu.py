"""Edges of the tile kernel's fill (k_tiles prologue): the LDS-DMA bodies, the
per-side remainders (< 128 elements, one register per thread), the parity
heads, B's lookahead element and union's a_before / b_before are all issued
before one wait.  What can go wrong sits at tile and list edges, so every
list here has at most a few thousand elements.

Every case is a (u, v) pair of duplicate-free sorted uint64 lists, each a
slice of a larger device tensor: the slice offset gives the pointer parity
(ashift / bshift) and the elements just outside the slice are guards whose
values would create a false match or a wrong dedup if the kernel read them.
Expected values come from numpy on the slices alone (the k-way cases use the
oracle fold).  Each case runs through the four one-shot pair ops and through
one prepared batch three times: intersect (writes the split cache), intersect
(reads it), merge (reads the cache the intersect wrote).

Tile = 2048 merge-path elements, A (u) first on ties.
"""
import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth
from oracle import bind as orc

pytestmark = pytest.mark.gpu

TILE = 2048
EDGE_LENS = [0, 1, 2, 127, 128, 129, 255, 256, 257]
PARITIES = [(0, 0), (0, 1), (1, 0), (1, 1)]


def arr(x):
    return np.asarray(x, dtype=np.uint64)


def first_above(src, floor, avoid):
    """Smallest value of src above floor that is not in avoid (else None)."""
    for x in src:
        if x > floor and x not in avoid:
            return int(x)
    return None


def guarded(own, other, parity):
    """Host array [guards | own | guards] and the slice offset of `own`.
    Before: own[0] again (a union that read it would drop own[0]).  After: a
    value of `other` that `own` lacks (reading it as the lookahead would turn
    it into a match), else other's last value."""
    own_set = set(own.tolist())
    before = int(own[0]) if own.size else (int(other[0]) if other.size else 7)
    floor = int(own[-1]) if own.size else -1
    after = first_above(other.tolist(), floor, own_set)
    if after is None:
        after = int(other[-1]) if other.size else before
    off = 2 - parity  # even offset -> 16B aligned slice, odd -> not
    big = np.concatenate([arr([before] * off), own, arr([after] * 2)])
    return big, off


class Case:
    def __init__(self, name, u, v, pu=0, pv=0):
        self.name, self.u, self.v, self.pu, self.pv = name, arr(u), arr(v), pu, pv
        for a in (self.u, self.v):
            assert a.size < 2 or np.all(a[1:] > a[:-1]), name
        self.want = {
            "intersect": np.intersect1d(self.u, self.v),
            "difference": np.setdiff1d(self.u, self.v),
            "merge": np.union1d(self.u, self.v),
            "merge_all": np.sort(np.concatenate([self.u, self.v])),
        }
        self._dev = None

    def dev(self):
        """(du, dv): slices of larger device tensors, uploaded once."""
        if self._dev is None:
            out = []
            for own, other, par in ((self.u, self.v, self.pu), (self.v, self.u, self.pv)):
                big, off = guarded(own, other, par)
                t = torch.from_numpy(big.view(np.int64)).to("cuda:0")
                s = t[off:off + own.size]
                assert own.size == 0 or (s.data_ptr() >> 3) & 1 == par
                out.append(s)
            self._dev = tuple(out)
        return self._dev


def low_high(L, other_len, shared, rng):
    """`low`: L values below 10_000; `high`: other_len values, the first
    `shared` of them taken from low, the rest above 20_000.  On the merge
    path all of low is consumed before the first value above 20_000."""
    low = np.sort(rng.choice(10_000, size=L, replace=False)).astype(np.uint64)
    k = min(shared, L)
    common = np.sort(rng.choice(low, size=k, replace=False)) if k else arr([])
    rest = 20_000 + np.sort(rng.choice(50_000, size=other_len - k, replace=False))
    return low, np.concatenate([common, rest.astype(np.uint64)])


def build_cases():
    rng = np.random.default_rng(synth.SEED + 97)
    cases = []
    # remainder lengths: tile 0 has alen == L (resp. blen == L) by construction
    # (the short list and at most 5 shared values of the long one come first)
    for L in EDGE_LENS:
        for pu, pv in PARITIES:
            u, v = low_high(L, 3000, 5, rng)
            cases.append(Case(f"alen{L}_p{pu}{pv}", u, v, pu, pv))
            v, u = low_high(L, 3000, 5, rng)
            cases.append(Case(f"blen{L}_p{pu}{pv}", u, v, pu, pv))
    # one-sided tiles and empty lists
    lo = arr(np.arange(3000) * 3 + 1)
    hi = arr(np.arange(3000) * 3 + 100_000)
    for pu, pv in ((0, 0), (1, 1)):
        cases.append(Case(f"u_below_v_p{pu}{pv}", lo, hi, pu, pv))
        cases.append(Case(f"v_below_u_p{pu}{pv}", hi, lo, pu, pv))
    cases.append(Case("n0", [], lo[:2500], 0, 1))
    cases.append(Case("m0", lo[:2500], [], 1, 0))
    cases.append(Case("n0_m0", [], []))
    # path lengths: last tile empty, full, or one element
    for path in (1, 2047, 2048, 2049, 4096, 4097):
        n = path // 2
        span = 3 * path
        u = np.sort(rng.choice(span, size=n, replace=False))
        v = np.sort(rng.choice(span, size=path - n, replace=False))
        cases.append(Case(f"path{path}", u, v, path & 1, (path >> 1) & 1))
    # lookahead: value X sits in both lists with `before` path elements ahead
    # of it.  before == TILE-1 puts u's X last in tile 0 and v's X first in
    # tile 1: only the lookahead element makes tile 0 see the match, and only
    # a_before lets tile 1's union drop the duplicate.
    X = 50_000
    for before in (TILE - 2, TILE - 1, TILE):
        nu = before // 2
        low = rng.choice(X, size=before - 3, replace=False)  # 3 values shared
        ul, vl = np.sort(low[:nu]), np.sort(np.concatenate([low[:3], low[nu:]]))
        uh = X + 1 + np.sort(rng.choice(5000, size=600, replace=False))
        vh = X + 1 + np.sort(rng.choice(5000, size=600, replace=False))
        u = np.concatenate([ul, [X], uh])
        v = np.concatenate([vl, [X], vh])
        for pu, pv in ((0, 0), (1, 0), (0, 1)):
            cases.append(Case(f"straddle{before}_p{pu}{pv}", u, v, pu, pv))
            cases.append(Case(f"straddle{before}_swapped_p{pu}{pv}", v, u, pu, pv))
        # same shape, but v ends where tile 0's B range ends: no lookahead
        # exists, and the guard after v's slice is X's successor in u or X
        cases.append(Case(f"b_ends_at_m_{before}", u, vl, 1, 1))
        cases.append(Case(f"b_ends_at_m_{before}_x", np.concatenate([ul, [X]]), vl, 0, 1))
    return cases


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def new_outs(cases):
    return [torch.full((c.u.size + c.v.size + 1,), -1, dtype=torch.int64, device="cuda:0")
            for c in cases]


def check(cases, outs, lens, key, what):
    for c, o, n in zip(cases, outs, lens):
        w = c.want[key]
        assert int(n) == w.size, f"{what}: {c.name}: length {n} != {w.size}"
        assert np.array_equal(to_np(o[:n]), w), f"{what}: {c.name}"


def run_all(eng, cases):
    du = [c.dev()[0] for c in cases]
    dv = [c.dev()[1] for c in cases]
    for key, fn in (("intersect", eng.intersect_pairs), ("difference", eng.difference_pairs),
                    ("merge", eng.merge_pairs), ("merge_all", eng.merge_all_pairs)):
        outs = new_outs(cases)
        _, lens = fn(du, dv, outs)
        check(cases, outs, lens, key, f"one-shot {key}")
    outs = new_outs(cases)
    b = eng.make_batch(du, dv, outs)
    try:
        for key, op, what in (("intersect", algo.OP_INTERSECT, "prepared run 1 (computes splits)"),
                              ("intersect", algo.OP_INTERSECT, "prepared run 2 (cached splits)"),
                              ("merge", algo.OP_MERGE, "prepared run 3 (merge on cached splits)")):
            for o in outs:
                o.fill_(-1)
            lens = b.run(op)
            check(cases, outs, lens, key, what)
    finally:
        b.close()


def test_case_shapes():
    """The constructions give the tile shapes they claim (host arithmetic)."""
    for L in EDGE_LENS:
        c = BY_NAME[f"alen{L}_p00"]
        assert c.u.size == L and np.searchsorted(c.v, 10_000) + L <= TILE
        c = BY_NAME[f"blen{L}_p00"]
        assert c.v.size == L and np.searchsorted(c.u, 10_000) + L <= TILE
    c = BY_NAME[f"straddle{TILE - 1}_p00"]
    i = int(np.searchsorted(c.u, 50_000))
    j = int(np.searchsorted(c.v, 50_000))
    assert c.u[i] == 50_000 == c.v[j] and i + j == TILE - 1
    assert BY_NAME[f"b_ends_at_m_{TILE - 1}"].v.size == j
    assert all(c.u.size + c.v.size <= 6100 for c in CASES)


@pytest.mark.parametrize("name", list(BY_NAME))
def test_single_pair(eng, name):
    run_all(eng, [BY_NAME[name]])


def test_mixed_batch(eng):
    """28 pairs in one grid: tile->pair boundaries next to each other, pairs
    without tiles in between, and a one-element pair as the last tile."""
    names = ([f"alen{L}_p01" for L in (1, 127, 129, 257)] +
             [f"blen{L}_p10" for L in (0, 2, 128, 255)] +
             ["n0_m0", "u_below_v_p11", "n0", "v_below_u_p00", "m0"] +
             [f"path{p}" for p in (2047, 2048, 2049, 4096, 4097)] +
             ["n0_m0"] +
             [f"straddle{b}_p10" for b in (TILE - 2, TILE - 1, TILE)] +
             [f"straddle{TILE - 1}_swapped_p01", f"b_ends_at_m_{TILE - 1}",
              f"b_ends_at_m_{TILE - 1}_x", "blen256_p11", "alen256_p00", "path1"])
    assert 16 <= len(names) <= 32
    run_all(eng, [BY_NAME[n] for n in names])


@pytest.mark.parametrize("order", ["shrinking", "growing"])
def test_kway(eng, order):
    """k-way rounds: the tile words come from descriptors whose lengths were
    written on the device, and capacity-tiled rounds overshoot the path."""
    rng = np.random.default_rng(synth.SEED + 98)
    sizes = [4097, 3000, 2049, 2048, 1500, 129, 2, 1]
    if order == "growing":
        sizes = sizes[::-1]
    lists = [np.sort(rng.choice(6000, size=n, replace=False)).astype(np.uint64)
             for n in sizes]
    common = arr([11, 2047, 2048, 5999])  # keeps the k-way intersection non-empty
    lists = [np.union1d(x, common) for x in lists]
    dev = [torch.from_numpy(x.view(np.int64)).to("cuda:0") for x in lists]
    want_m, want_i = orc.merge_sorted(lists), orc.intersect_sorted(lists)
    assert want_i.size >= common.size
    assert np.array_equal(to_np(eng.merge_sorted(dev)), want_m), "merge_sorted"
    assert np.array_equal(to_np(eng.intersect_sorted(dev)), want_i), "intersect_sorted"
