"""GPU behaviour of the host pipeline that drives the pair kernels: the
one-shot calls (ctx workspace), the prepared batch (its own allocation, graph
captured tail) and the k-way union tree (one view per round) share one engine
and one set of stage functions.  These tests pin what the three owners must
agree on: nobody aliases another owner's buffers, rounds without tiles publish
zero lengths, and each path books the same statistics.

Expected values come from the CPU oracle only.  Tile = 2048 merge-path
elements; lists hold 0 to 6000 elements, so a pair spans 0 to 5 tiles.
"""
import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth
from oracle import bind as orc

pytestmark = pytest.mark.gpu

TILE = 2048


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.empty(0, dtype=torch.int64, device="cuda:0")
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def sorted_list(rng, n, span):
    """n distinct sorted values below span (span ~ 3n: about a third shared
    between two such lists)."""
    return np.sort(rng.choice(span, size=n, replace=False)).astype(np.uint64)


class Pairs:
    """Pairs on the device with their oracle results, computed once."""

    def __init__(self, rng, sizes):
        self.u, self.v = [], []
        for n, m in sizes:
            span = 3 * max(n, m, 1)
            self.u.append(sorted_list(rng, n, span))
            self.v.append(sorted_list(rng, m, span))
        self.du = [to_dev(u) for u in self.u]
        self.dv = [to_dev(v) for v in self.v]
        uv = list(zip(self.u, self.v))
        self.want = {
            algo.OP_INTERSECT: [orc.intersect_with(u, v) for u, v in uv],
            algo.OP_DIFFERENCE: [orc.difference(u, v) for u, v in uv],
            algo.OP_MERGE: [orc.merge_sorted([u, v]) for u, v in uv],
        }
        self.sum_nm = sum(u.size + v.size for u, v in uv)

    def new_outs(self):
        # n+m + 1 fits every op; the +1 keeps empty pairs a real allocation
        return [torch.full((u.size + v.size + 1,), -1, dtype=torch.int64,
                           device="cuda:0") for u, v in zip(self.u, self.v)]

    def check(self, outs, lens, op, what):
        want = self.want[op]
        assert [int(x) for x in lens] == [w.size for w in want], what
        for i, w in enumerate(want):
            assert np.array_equal(to_np(outs[i][:lens[i]]), w), f"{what}: pair {i}"


# 0 to 3 tiles per pair, one empty pair, odd sizes around the tile edges
SMALL_SIZES = [(1000, 1047), (0, 0), (TILE, 1), (3000, 3100), (0, 2500), (4097, 2047)]


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def small():
    return Pairs(np.random.default_rng(synth.SEED + 81), SMALL_SIZES)


@pytest.fixture(scope="module")
def large():
    """40 pairs of up to 5 tiles: more pairs and more tiles than `small`, so
    every ctx workspace slot grows when these run after it."""
    rng = np.random.default_rng(synth.SEED + 82)
    sizes = [(int(rng.integers(0, 5121)), int(rng.integers(0, 5121))) for _ in range(38)]
    sizes += [(5120, 5120), (0, 0)]
    return Pairs(rng, sizes)


def test_shapes(small, large):
    tiles = lambda c: [(u.size + v.size + TILE - 1) // TILE for u, v in zip(c.u, c.v)]
    assert sorted(set(tiles(small))) == [0, 1, 2, 3]
    assert max(tiles(large)) == 5 and sum(tiles(large)) > 4 * sum(tiles(small))
    assert all(a.size <= 6000 for c in (small, large) for a in c.u + c.v)


def test_interleaved_owners(eng, small, large):
    rng = np.random.default_rng(synth.SEED + 83)
    kway = [sorted_list(rng, n, 9000) for n in (2500, 0, 3001, 1, 2048)]
    want_kway = orc.merge_sorted(kway)

    outs = small.new_outs()
    b = eng.make_batch(small.du, small.dv, outs)
    try:
        lens = b.run(algo.OP_INTERSECT)  # captures the tail graph
        small.check(outs, lens, algo.OP_INTERSECT, "prepared intersect, first run")

        louts = large.new_outs()
        _, llens = eng.difference_pairs(large.du, large.dv, louts)
        large.check(louts, llens, algo.OP_DIFFERENCE, "one-shot difference")

        for o in outs:
            o.fill_(-1)
        lens = b.run_n(algo.OP_INTERSECT, 3)
        small.check(outs, lens, algo.OP_INTERSECT, "prepared run_n after one-shot")
        lens = b.run(algo.OP_DIFFERENCE)
        small.check(outs, lens, algo.OP_DIFFERENCE, "prepared difference")
        lens = b.run(algo.OP_MERGE)
        small.check(outs, lens, algo.OP_MERGE, "prepared merge")

        louts = large.new_outs()
        _, llens = eng.merge_pairs(large.du, large.dv, louts)
        large.check(louts, llens, algo.OP_MERGE, "one-shot merge")
        got = to_np(eng.merge_sorted([to_dev(x) for x in kway]))
        assert np.array_equal(got, want_kway), "merge_sorted of 5 lists"

        for o in outs:
            o.fill_(-1)
        lens = b.run(algo.OP_INTERSECT)
        small.check(outs, lens, algo.OP_INTERSECT, "prepared intersect, last run")
    finally:
        b.close()


KWAY_CASES = {
    "four_empty": [[], [], [], []],
    "two_empty_and_one": [[], [], [7]],
    "single_with_duplicates": [[1, 1, 1]],
}


@pytest.mark.parametrize("name", list(KWAY_CASES) + ["five_with_empty_pair"])
def test_kway_empty_rounds(eng, name):
    if name == "five_with_empty_pair":
        # lists 0 and 1 are empty: pair 0 of round 1 has no tiles, the others do
        rng = np.random.default_rng(synth.SEED + 84)
        lists = [sorted_list(rng, n, 12000) for n in (0, 0, 3000, 2049, 4000)]
    else:
        lists = [np.array(x, dtype=np.uint64) for x in KWAY_CASES[name]]
    dev = [to_dev(x) for x in lists]
    want_m = orc.merge_sorted(lists)
    want_i = orc.intersect_sorted(lists)
    if name in KWAY_CASES:  # the oracle's answers, restated
        assert want_m.tolist() == {"four_empty": [], "two_empty_and_one": [7],
                                   "single_with_duplicates": [1]}[name]
    assert np.array_equal(to_np(eng.merge_sorted(dev)), want_m), "merge_sorted"
    assert np.array_equal(to_np(eng.intersect_sorted(dev)), want_i), "intersect_sorted"


def _stats_after(eng, fn):
    eng.stats_reset()
    res = fn()
    return res, eng.stats()


def test_stats_by_path(eng, small):
    c = small
    nm = c.sum_nm

    def expect(st, launches, nbytes, what, timed=True):
        assert st["launches"] == launches, what
        assert st["bytes_algorithmic"] == nbytes, what
        if timed:
            assert st["kernel_ms"] > 0, what
        else:
            assert st["kernel_ms"] == 0, what

    (_, lens), st = _stats_after(eng, lambda: eng.intersect_pairs(c.du, c.dv, c.new_outs()))
    expect(st, 1, 8 * (nm + sum(lens)), "one-shot intersect")
    (_, lens), st = _stats_after(eng, lambda: eng.difference_pairs(c.du, c.dv, c.new_outs()))
    expect(st, 1, 8 * (nm + sum(lens)), "one-shot difference")
    (_, lens), st = _stats_after(eng, lambda: eng.merge_pairs(c.du, c.dv, c.new_outs()))
    expect(st, 2, 8 * (nm + sum(lens)), "one-shot merge")
    (_, lens), st = _stats_after(eng, lambda: eng.merge_all_pairs(c.du, c.dv, c.new_outs()))
    assert lens == [u.size + v.size for u, v in zip(c.u, c.v)]
    expect(st, 1, 16 * nm, "merge_all_pairs")

    b = eng.make_batch(c.du, c.dv, c.new_outs())
    try:
        lens, st = _stats_after(eng, lambda: b.run(algo.OP_INTERSECT))
        expect(st, 1, 8 * (nm + sum(lens)), "prepared intersect")
        lens, st = _stats_after(eng, lambda: b.run_n(algo.OP_INTERSECT, 3))
        expect(st, 1, 3 * 8 * (nm + sum(lens)), "prepared run_n x3")
        lens, st = _stats_after(eng, lambda: b.run(algo.OP_MERGE))
        expect(st, 2, 8 * (nm + sum(lens)), "prepared merge")
    finally:
        b.close()

    three = [c.du[0], c.dv[0], c.du[3]]  # non-empty: a tree of 2 rounds
    total = sum(t.numel() for t in three)
    _, st = _stats_after(eng, lambda: eng.merge_sorted(three))
    expect(st, 4, 48 * total, "merge_sorted of 3 lists")

    empty = [to_dev([]), to_dev([])]
    (_, lens), st = _stats_after(eng, lambda: eng.intersect_pairs(empty, empty))
    assert lens == [0, 0]
    expect(st, 0, 0, "one-shot intersect of two empty pairs", timed=False)
