"""GPU parity of the fused per-pair tail (k_tail_fused) that follows the staged
intersect/difference tile kernel: chunk map, chunk base, sparse and dense copy,
primary-vs-overflow staging, lengths.  Expected values come from the CPU
oracle only; the shapes are the smallest at which each path can go wrong.

Tile = 2048 merge-path elements, chunk = 64 tiles, primary staging = 64.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:  # for the child-process entry at the bottom
    sys.path.insert(0, REPO_ROOT)

import torch  # noqa: E402

from dgraph_amd import algo, synth  # noqa: E402
from oracle import bind as orc  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 2048
CHUNK = 64  # UA_TAIL_C
STAGE_P = 64  # UA_STAGE_P
BLOCK_SPAN = 1 << 20  # value range owned by one planted tile


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.empty(0, dtype=torch.int64, device="cuda:0")
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


# ---------- input construction ----------

def rand_pair(rng, n, m, k):
    """Sorted duplicate-free u (n) and v (m) sharing exactly k values."""
    assert k <= min(n, m)
    d = n + m - k
    vals = np.uint64(rng.integers(0, 1000)) + np.cumsum(
        rng.integers(1, 50, size=d, dtype=np.uint64))
    role = rng.permutation(d)
    common, uo, vo = role[:k], role[k:n], role[n:]
    u = np.sort(vals[np.concatenate([common, uo])])
    v = np.sort(vals[np.concatenate([common, vo])])
    return u.astype(np.uint64), v.astype(np.uint64)


def planted_pair(rng, tiles, tail=0):
    """tiles: list of (c, a) per merge tile — c values common to u and v, a
    values only in u, and 2048 - 2c - a only in v, all inside the tile's own
    value range, so tile k of the merge path is exactly block k: intersect
    emits c there and difference emits a.  tail extra u-only values follow
    (a final partial tile)."""
    us, vs = [], []
    for k, (c, a) in enumerate(tiles):
        b = TILE - 2 * c - a
        assert b >= 0
        d = c + a + b
        vals = np.uint64(k * BLOCK_SPAN) + np.cumsum(
            rng.integers(1, 400, size=d, dtype=np.uint64))
        role = rng.permutation(d)
        us.append(np.sort(vals[role[:c + a]]))
        vs.append(np.sort(vals[np.concatenate([role[:c], role[c + a:]])]))
    if tail:
        us.append(np.uint64(len(tiles) * BLOCK_SPAN) +
                  np.arange(1, tail + 1, dtype=np.uint64))
    cat = lambda xs: (np.concatenate(xs) if xs else np.empty(0)).astype(np.uint64)
    return cat(us), cat(vs)


def tile_counts(u, v, emitted):
    """Per-merge-tile count of the emitted u-values (u-before-v on ties, as
    the merge path orders them)."""
    pos = np.searchsorted(u, emitted) + np.searchsorted(v, emitted, side="left")
    ntiles = (u.size + v.size + TILE - 1) // TILE
    return np.bincount(pos // TILE, minlength=ntiles)


class Case:
    """A batch of pairs with its oracle results, computed once."""

    def __init__(self, pairs):
        self.u = [p[0] for p in pairs]
        self.v = [p[1] for p in pairs]
        self.want = {
            algo.OP_INTERSECT: [orc.intersect_with(u, v) for u, v in pairs],
            algo.OP_DIFFERENCE: [orc.difference(u, v) for u, v in pairs],
        }
        self._merge = None
        self.du = [to_dev(u) for u in self.u]
        self.dv = [to_dev(v) for v in self.v]

    def want_merge(self):
        if self._merge is None:
            self._merge = [orc.merge_sorted([u, v]) for u, v in zip(self.u, self.v)]
        return self._merge

    def new_outs(self):
        # n+m + 1 fits every op; the +1 keeps empty pairs a real allocation
        return [torch.full((u.size + v.size + 1,), -1, dtype=torch.int64,
                           device="cuda:0") for u, v in zip(self.u, self.v)]

    def check(self, outs, lens, want, what):
        assert [int(x) for x in lens] == [w.size for w in want], what
        for i, w in enumerate(want):
            got = to_np(outs[i][:lens[i]])
            assert np.array_equal(got, w), f"{what}: pair {i} differs"


def sizes_pairs(rng):
    """~300 pairs: the chunk-map edge sizes, each followed by an empty pair,
    spread among small random pairs."""
    edge = [0, 1, 1, TILE, TILE + 1, CHUNK * TILE, CHUNK * TILE + 1,
            2 * CHUNK * TILE + CHUNK * TILE // 2 + 777]
    pairs = []
    for j in range(292):
        nm = int(rng.integers(1, 3000))
        n = int(rng.integers(0, nm + 1))
        pairs.append(rand_pair(rng, n, nm - n, int(rng.integers(0, min(n, nm - n) + 1))))
    flip = False
    for j, nm in enumerate(edge):
        n = nm // 2 if nm != 1 else int(flip)
        flip = not flip
        m = nm - n
        p = rand_pair(rng, n, m, min(n, m) // 100)
        at = 10 + 35 * j
        pairs.insert(at, p)
        pairs.insert(at + 1, rand_pair(rng, 0, 0, 0))
    return pairs


def boundary_pairs(rng):
    sp = [0, 1, 32, 33, STAGE_P, STAGE_P + 1]
    pairs = []
    # intersect emits 0,1,32,33,64,65 per tile; difference emits a = 7
    pairs.append(planted_pair(rng, [(c, 7) for c in sp] + [(10, 10)] * 3, tail=5))
    # difference emits 0,1,32,33,64,65 per tile; intersect emits 0
    pairs.append(planted_pair(rng, [(0, a) for a in sp]))
    # u == v: intersect emits 1024 per tile (the full stride), difference 0
    pairs.append(planted_pair(rng, [(TILE // 2, 0)] * 5))
    # disjoint: difference emits 2048 per tile for u's tiles
    pairs.append(planted_pair(rng, [(0, TILE)] * 4 + [(0, 0)] * 3))
    pairs.append(rand_pair(rng, 0, 0, 0))
    # two chunks and a bit, mixing sparse and dense tiles: chunk 0 is sparse
    # on average with dense tiles inside, chunk 1 dense with sparse inside
    mix = []
    for t in range(CHUNK):
        mix.append((1000, 40) if t % 29 == 0 else (int(t % 7), int(t % 5)))
    for t in range(CHUNK):
        mix.append((2, 1) if t % 9 == 0 else (700 + t % 3, 600))
    mix += [(STAGE_P + 1, 3), (0, 0), (12, 2000)]
    pairs.append(planted_pair(rng, mix, tail=100))
    return pairs


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sizes_case():
    return Case(sizes_pairs(np.random.default_rng(synth.SEED + 71)))


@pytest.fixture(scope="module")
def boundary_case():
    return Case(boundary_pairs(np.random.default_rng(synth.SEED + 72)))


# ---------- the inputs really hit the boundaries (oracle-side check) ----------

def test_planted_tile_counts(boundary_case):
    c = boundary_case
    want = {0, 1, 32, 33, STAGE_P, STAGE_P + 1}
    ti = tile_counts(c.u[0], c.v[0], c.want[algo.OP_INTERSECT][0])
    assert want <= set(ti.tolist())
    td = tile_counts(c.u[1], c.v[1], c.want[algo.OP_DIFFERENCE][1])
    assert want <= set(td.tolist())
    assert set(tile_counts(c.u[2], c.v[2], c.want[algo.OP_INTERSECT][2]).tolist()) == {TILE // 2}
    assert TILE in tile_counts(c.u[3], c.v[3], c.want[algo.OP_DIFFERENCE][3]).tolist()
    tm = tile_counts(c.u[5], c.v[5], c.want[algo.OP_INTERSECT][5])
    # chunk 0 below the dense switch (mean 64 per tile), chunk 1 above it,
    # and each holds tiles of the other kind
    assert tm[:CHUNK].sum() < 64 * CHUNK and tm[:CHUNK].max() > STAGE_P
    assert tm[CHUNK:2 * CHUNK].sum() >= 64 * CHUNK and tm[CHUNK:2 * CHUNK].min() <= 32


def test_sizes_cover_chunk_edges(sizes_case):
    nm = [u.size + v.size for u, v in zip(sizes_case.u, sizes_case.v)]
    for s in (0, 1, TILE, TILE + 1, CHUNK * TILE, CHUNK * TILE + 1):
        assert s in nm
    assert any(2 * CHUNK * TILE < s < 3 * CHUNK * TILE for s in nm)
    assert len(nm) >= 300
    assert sum(nm) < 4_000_000


# ---------- one batch through both API paths ----------

@pytest.mark.parametrize("case_name", ["sizes_case", "boundary_case"])
def test_one_shot_batch(eng, request, case_name):
    c = request.getfixturevalue(case_name)
    outs = c.new_outs()
    _, lens = eng.intersect_pairs(c.du, c.dv, outs)
    c.check(outs, lens, c.want[algo.OP_INTERSECT], "one-shot intersect")
    # WS_POUT is reused: a second call must not see stale lengths
    outs = c.new_outs()
    _, lens = eng.difference_pairs(c.du, c.dv, outs)
    c.check(outs, lens, c.want[algo.OP_DIFFERENCE], "one-shot difference")
    # fewer pairs after more: empty pairs must still read 0
    k = 40
    outs = c.new_outs()[:k]
    _, lens = eng.intersect_pairs(c.du[:k], c.dv[:k], outs)
    c.check(outs, lens, c.want[algo.OP_INTERSECT][:k], "one-shot intersect (prefix)")


@pytest.mark.parametrize("case_name", ["sizes_case", "boundary_case"])
def test_prepared_batch(eng, request, case_name):
    c = request.getfixturevalue(case_name)
    outs = c.new_outs()
    b = eng.make_batch(c.du, c.dv, outs)
    try:
        for op in (algo.OP_INTERSECT, algo.OP_DIFFERENCE):
            lens = b.run(op)
            c.check(outs, lens, c.want[op], f"prepared op {op}")
    finally:
        b.close()


def test_prepared_run_order_and_run_n(eng, boundary_case):
    c = boundary_case
    outs = c.new_outs()
    b = eng.make_batch(c.du, c.dv, outs)
    try:
        order = [algo.OP_INTERSECT, algo.OP_DIFFERENCE, algo.OP_INTERSECT,
                 algo.OP_MERGE, algo.OP_INTERSECT]
        for step, op in enumerate(order):
            lens = b.run(op)
            want = c.want_merge() if op == algo.OP_MERGE else c.want[op]
            c.check(outs, lens, want, f"step {step} op {op}")
        for op in (algo.OP_INTERSECT, algo.OP_DIFFERENCE):
            lens1 = b.run(op)
            got1 = [to_np(o[:n]).copy() for o, n in zip(outs, lens1)]
            for o in outs:
                o.fill_(-1)
            lens3 = b.run_n(op, 3)
            assert lens3 == lens1
            for i, n in enumerate(lens3):
                assert np.array_equal(to_np(outs[i][:n]), got1[i])
            c.check(outs, lens3, c.want[op], f"run_n op {op}")
    finally:
        b.close()


def test_overlapped_run_n(eng, boundary_case, monkeypatch):
    """UA_OVERLAP=1 alternates two buffer sets; set 1 has no primary staging
    region (prim == nullptr), so every tile reads the overflow layout."""
    c = boundary_case
    monkeypatch.setenv("UA_OVERLAP", "1")
    outs = c.new_outs()
    b = eng.make_batch(c.du, c.dv, outs)
    try:
        for op, n in ((algo.OP_INTERSECT, 4), (algo.OP_DIFFERENCE, 3),
                      (algo.OP_INTERSECT, 2)):
            for o in outs:
                o.fill_(-1)
            lens = b.run_n(op, n)  # last pass lands in set (n - 1) & 1
            c.check(outs, lens, c.want[op], f"overlap op {op} x{n}")
    finally:
        b.close()


def test_forced_fallback(eng, sizes_case, monkeypatch):
    """Chunk limit 1 at create: the 2.5-chunk pair puts the batch on the
    scanned tail; results are the same."""
    c = sizes_case
    monkeypatch.setenv("UA_TAIL_MAX_CHUNKS", "1")
    outs = c.new_outs()
    b = eng.make_batch(c.du, c.dv, outs)
    monkeypatch.delenv("UA_TAIL_MAX_CHUNKS")
    try:
        for op in (algo.OP_INTERSECT, algo.OP_DIFFERENCE):
            lens = b.run(op)
            c.check(outs, lens, c.want[op], f"fallback op {op}")
    finally:
        b.close()
    monkeypatch.setenv("UA_TAIL_MAX_CHUNKS", "1")
    outs = c.new_outs()
    _, lens = eng.intersect_pairs(c.du, c.dv, outs)
    c.check(outs, lens, c.want[algo.OP_INTERSECT], "fallback one-shot")


def test_toggle_off_child_process():
    env = dict(os.environ, UA_FUSED_TAIL="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env,
                       cwd=REPO_ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "toggle-off ok" in r.stdout


def _child_main():
    c = Case(boundary_pairs(np.random.default_rng(synth.SEED + 72)))
    e = algo.Engine(0)
    outs = c.new_outs()
    b = e.make_batch(c.du, c.dv, outs)
    for op in (algo.OP_INTERSECT, algo.OP_DIFFERENCE, algo.OP_INTERSECT):
        lens = b.run(op)
        c.check(outs, lens, c.want[op], f"toggle-off op {op}")
    lens = b.run_n(algo.OP_INTERSECT, 3)
    c.check(outs, lens, c.want[algo.OP_INTERSECT], "toggle-off run_n")
    outs = c.new_outs()
    _, lens = e.difference_pairs(c.du, c.dv, outs)
    c.check(outs, lens, c.want[algo.OP_DIFFERENCE], "toggle-off one-shot")
    b.close()
    e.close()
    print("toggle-off ok")


if __name__ == "__main__":
    _child_main()
