"""The prepared batch's split cache: the first run of any op searches, per
(tile, thread), the merge-path splits i0 (at the thread's first diagonal) and
i0b (at its middle one) and stores them; every later run of any op loads them
instead of searching.

What can go wrong is a split at an extreme (a thread that consumes only A or
only B, in its first or second half), a wave or tile edge, the last thread of
a tile, a partial tile whose trailing threads all sit at the tile's end, and
a cache written by one op and read by another.  The cases are chosen for
those and do not depend on how the cache packs the two values.  Every case is
a pair of duplicate-free sorted uint64 lists of at most about 6000 elements;
expected values come from numpy.  Each set of pairs goes through one prepared
batch per op order, and every run is checked, so each op is seen writing the
cache and reading one that another op wrote.

Tile = 2048 merge-path elements, 256 threads x 8 path steps, 4 waves of 512
steps; A (u) goes first on ties.
"""
import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth

pytestmark = pytest.mark.gpu

TILE = 2048
ORDERS = [
    ("intersect", "intersect", "merge", "difference"),
    ("merge", "merge", "intersect", "difference"),
    ("difference", "intersect", "merge"),
]
OPS = {"intersect": algo.OP_INTERSECT, "merge": algo.OP_MERGE,
       "difference": algo.OP_DIFFERENCE}
GUARD = 8  # sentinel elements behind each out tensor's capacity


def arr(x):
    return np.asarray(x, dtype=np.uint64)


def guarded(own, other, parity):
    """Host array [guards | own | guards] and the slice offset of `own`: the
    offset sets the pointer parity, and the guards are values that would
    change a result if the kernel read them (own[0] again in front; behind, a
    value of `other` that `own` lacks)."""
    before = int(own[0]) if own.size else (int(other[0]) if other.size else 7)
    later = np.setdiff1d(other[other > own[-1]] if own.size else other, own)
    after = int(later[0]) if later.size else (int(other[-1]) if other.size else before)
    off = 2 - parity  # even offset -> 16-byte aligned slice, odd -> not
    return np.concatenate([arr([before] * off), own, arr([after] * 2)]), off


class Case:
    def __init__(self, name, u, v, pu=0, pv=0):
        self.name, self.u, self.v, self.pu, self.pv = name, arr(u), arr(v), pu, pv
        for a in (self.u, self.v):
            assert a.size < 2 or np.all(a[1:] > a[:-1]), name
        assert self.u.size + self.v.size <= 6200, name
        self.want = {
            "intersect": np.intersect1d(self.u, self.v),
            "difference": np.setdiff1d(self.u, self.v),
            "merge": np.union1d(self.u, self.v),
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


def alternating(run, shift, share, total=5200):
    """The merge path is `shift` elements of v, then runs of `run` elements
    taken alternately from u and v.  With share, each v-run opens with the
    value that closed the u-run before it (a tie, which A wins), so intersect
    and difference have something to find at every run boundary."""
    u, v = [], []
    x = 10
    for _ in range(shift):
        v.append(x)
        x += 2
    side = 0
    while len(u) + len(v) + run <= total:
        dst = u if side == 0 else v
        if side == 1 and share and u:
            x = u[-1]
        for _ in range(run):
            dst.append(x)
            x += 2
        side ^= 1
    return arr(u), arr(v)


def build_runs():
    cases = []
    k = 0
    for run in (512, 8, 4, 1):
        for shift in (0, 1, 3, 7):
            for share in (False, True):
                u, v = alternating(run, shift, share)
                cases.append(Case(f"run{run}_shift{shift}_{'tie' if share else 'plain'}",
                                  u, v, k & 1, (k >> 1) & 1))
                k += 1
    lo = arr(np.arange(2600) * 3 + 1)
    hi = arr(np.arange(2600) * 3 + 100_000)
    cases.append(Case("u_below_v", lo, hi, 0, 1))
    cases.append(Case("v_below_u", hi, lo, 1, 0))
    return cases


def build_partial():
    rng = np.random.default_rng(synth.SEED + 211)
    cases = []
    for path in (1, 2047, 2048, 2049, 4097):
        n = path // 2
        span = 2 * path + 3
        u = np.sort(rng.choice(span, size=n, replace=False))
        v = np.sort(rng.choice(span, size=path - n, replace=False))
        cases.append(Case(f"path{path}", u, v, path & 1, (path >> 1) & 1))
        cases.append(Case(f"path{path}_swapped", v, u, (path >> 1) & 1, path & 1))
    # tile 0 is all A and tile 1 all B (v sits inside a gap of u); swapped,
    # tile 0 is all B and tile 1 all A
    u = np.concatenate([np.arange(TILE) * 2 + 1, 50_000 + np.arange(300) * 2])
    v = 10_000 + np.arange(TILE + 100) * 3
    cases.append(Case("all_a_then_all_b", u, v, 1, 1))
    cases.append(Case("all_b_then_all_a", v, u, 0, 0))
    some = arr(np.arange(2500) * 5 + 3)
    cases.append(Case("n0", [], some, 0, 1))
    cases.append(Case("m0", some, [], 1, 0))
    cases.append(Case("n0_m0", [], []))
    return cases


def build_random():
    """20 pairs, lengths in [0, 5000]: the universe is cut into runs of random
    length that go to u, to v or to both."""
    rng = np.random.default_rng(synth.SEED + 212)
    cases = []
    for k in range(20):
        size = int(rng.integers(0, 7001)) if k else 0
        p_both = float(rng.choice([0.0, 0.01, 0.2, 0.6, 1.0]))
        mean = int(rng.choice([1, 3, 8, 40, 600]))
        vals = np.cumsum(rng.integers(1, 4, size=size) +
                         (rng.random(size) < 0.01) * rng.integers(0, 100_000, size=size))
        side = np.empty(size, dtype=np.int8)
        i = 0
        while i < size:
            ln = int(rng.geometric(1.0 / mean))
            r = rng.random()
            side[i:i + ln] = 2 if r < p_both else (0 if r < p_both + (1 - p_both) / 2 else 1)
            i += ln
        u = vals[(side == 0) | (side == 2)][:5000]
        v = vals[(side == 1) | (side == 2)][:5000]
        # keep the pair within about 6000 path elements
        while u.size + v.size > 6000:
            u, v = u[:u.size * 3 // 4], v[:v.size * 3 // 4]
        cases.append(Case(f"random{k}", u, v, k & 1, (k >> 1) & 1))
    return cases


RUNS = build_runs()
PARTIAL = build_partial()
RANDOM = build_random()
BY_NAME = {c.name: c for c in RUNS + PARTIAL + RANDOM}
assert len(BY_NAME) == len(RUNS) + len(PARTIAL) + len(RANDOM)


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def new_outs(cases):
    return [torch.full((c.u.size + c.v.size + GUARD,), -1, dtype=torch.int64,
                       device="cuda:0") for c in cases]


def check(cases, outs, lens, key, what):
    for c, o, n in zip(cases, outs, lens):
        w = c.want[key]
        assert int(n) == w.size, f"{what}: {c.name}: length {n} != {w.size}"
        assert np.array_equal(to_np(o[:n]), w), f"{what}: {c.name}"
        cap = c.u.size + c.v.size
        assert bool((o[cap:] == -1).all()), f"{what}: {c.name}: wrote past the capacity"


def run_orders(eng, cases):
    """One fresh prepared batch per op order; every run checked."""
    du = [c.dev()[0] for c in cases]
    dv = [c.dev()[1] for c in cases]
    for order in ORDERS:
        outs = new_outs(cases)
        b = eng.make_batch(du, dv, outs)
        try:
            for i, key in enumerate(order):
                for o in outs:
                    o.fill_(-1)
                lens = b.run(OPS[key])
                check(cases, outs, lens, key,
                      f"order {'/'.join(order)}, run {i + 1} ({key})")
        finally:
            b.close()


def test_case_shapes():
    """The constructions give the shapes they claim (host arithmetic)."""
    u, v = alternating(512, 0, False)
    # the path is u[0:512], v[0:512], ...: every wave of tile 0 is one run
    assert u[511] < v[0] < v[511] < u[512]
    u, v = alternating(8, 3, True)
    assert np.all(v[:3] < u[0]) and v[3] == u[7] and v[4] > u[7]
    assert np.intersect1d(u, v).size >= 300
    u, v = alternating(1, 0, True)
    assert np.intersect1d(u, v).size >= 2000
    c = BY_NAME["all_a_then_all_b"]
    assert c.u[TILE - 1] < c.v[0] and c.v[-1] < c.u[TILE] and c.v.size > TILE
    for path in (1, 2047, 2048, 2049, 4097):
        c = BY_NAME[f"path{path}"]
        assert c.u.size + c.v.size == path
    assert max(c.u.size for c in RANDOM) > 2048 and RANDOM[0].u.size == 0
    assert any(c.want["intersect"].size > 100 for c in RANDOM)


def test_runs(eng):
    """Threads that take 0 or 8 elements of A (0 or 4 in their first half), run
    edges on and off thread and wave edges."""
    run_orders(eng, RUNS)


def test_partial_and_degenerate(eng):
    run_orders(eng, PARTIAL)


def test_random(eng):
    run_orders(eng, RANDOM)


def test_mixed_batch(eng):
    """About 24 pairs in one grid with empty pairs in between: a tile's cached
    splits sit next to those of another pair's tile."""
    names = ["run512_shift0_plain", "n0_m0", "run8_shift1_tie", "path1", "run4_shift3_tie",
             "n0", "run1_shift7_tie", "u_below_v", "n0_m0", "v_below_u", "path2047",
             "m0", "path2048_swapped", "path2049", "n0_m0", "path4097", "all_a_then_all_b",
             "all_b_then_all_a", "random3", "n0_m0", "random7", "run512_shift7_tie",
             "run1_shift0_plain", "random12", "path1_swapped", "run8_shift3_plain"]
    cases = [BY_NAME[n] for n in names]
    assert {(c.pu, c.pv) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    run_orders(eng, cases)


@pytest.mark.parametrize("key", ["intersect", "merge", "difference"])
def test_run_n_on_fresh_batch(eng, key):
    """Three passes in one enqueue: the first writes the cache, the others
    read it; the lengths and outputs are the last pass's."""
    cases = [BY_NAME[n] for n in ("run512_shift3_tie", "path4097", "n0_m0", "random5",
                                  "run4_shift1_plain", "all_b_then_all_a")]
    du = [c.dev()[0] for c in cases]
    dv = [c.dev()[1] for c in cases]
    outs = new_outs(cases)
    b = eng.make_batch(du, dv, outs)
    try:
        lens = b.run_n(OPS[key], 3)
        check(cases, outs, lens, key, f"run_n({key}, 3)")
    finally:
        b.close()


@pytest.mark.parametrize("key", ["intersect", "merge", "difference"])
def test_invalid_input_stays_in_bounds(eng, key):
    """Lists that repeat every value three times break the input contract:
    results are unspecified, but the call succeeds, no length exceeds the op's
    capacity and nothing behind the capacity is written — on the run that
    searches the splits and on the run that reads them back."""
    u = np.repeat(arr(np.arange(900) * 4 + 2), 3)
    v = np.repeat(arr(np.arange(900) * 6), 3)
    du = torch.from_numpy(u.view(np.int64)).to("cuda:0")
    dv = torch.from_numpy(v.view(np.int64)).to("cuda:0")
    cap = {"intersect": min(u.size, v.size), "merge": u.size + v.size,
           "difference": u.size}[key]
    out = torch.full((cap + GUARD,), -1, dtype=torch.int64, device="cuda:0")
    b = eng.make_batch([du], [dv], [out])
    try:
        for run in (1, 2):
            lens = b.run(OPS[key])  # raises unless the call returns UA_OK
            assert lens[0] <= cap, f"run {run}: length {lens[0]} > capacity {cap}"
            assert bool((out[cap:] == -1).all()), f"run {run}: guard overwritten"
    finally:
        b.close()
