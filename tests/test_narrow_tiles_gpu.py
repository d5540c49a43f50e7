"""Narrow tiles of a prepared batch: ahead of its first intersect/difference
run the batch copies the low 32 bits of its inputs tile by tile, and a tile
whose A range, B range and lookahead element all share their high 32 bits is
then filled and walked from that copy with 32-bit unsigned compares; every
other tile keeps the 64-bit path.  Results must be those of the 64-bit path
on every input.

Every case runs a prepared batch and compares each output with numpy set
algebra and with the one-shot call (which never takes the narrow path), and
asserts the batch's narrow-tile count (`Batch.info()`), so a case cannot pass
without its tiles having taken the path it is about.  The expected count comes
from a host model of the partition (`tile_ranges`): merge path with A first
on ties, cut every 2048 path elements.  What a case needs from that model
(which tiles are wide) is asserted in the case itself as well.

Tile = 2048 merge-path elements, 256 threads x 8 path steps.  Lists have a
few thousand elements, batches at most 24 pairs.
"""
import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth

pytestmark = pytest.mark.gpu

TILE = 2048
STAGE_P = 64  # dense primary staging slots per tile; more goes to the overflow
GUARD = 8
OPS = {"intersect": algo.OP_INTERSECT, "merge": algo.OP_MERGE,
       "difference": algo.OP_DIFFERENCE}
U32 = 1 << 32


def arr(x):
    return np.asarray(x, dtype=np.uint64)


def with_hi(hi, lows):
    return (np.uint64(hi) << np.uint64(32)) | arr(lows)


def tile_ranges(u, v):
    """[(a0, a1, b0, b1)] per tile of a sorted pair."""
    n, m = u.size, v.size
    pos_u = np.arange(n) + np.searchsorted(v, u, side="left")  # A first on ties
    out = []
    for d0 in range(0, n + m, TILE):
        d1 = min(d0 + TILE, n + m)
        a0 = int(np.searchsorted(pos_u, d0, side="left"))
        a1 = int(np.searchsorted(pos_u, d1, side="left"))
        out.append((a0, a1, d0 - a0, d1 - a1))
    return out


def narrow_flags(u, v):
    """Per tile: do A range, B range and the lookahead v[b1] share x >> 32?"""
    flags = []
    for a0, a1, b0, b1 in tile_ranges(u, v):
        his = [u[a0:a1] >> np.uint64(32), v[b0:b1] >> np.uint64(32)]
        if b1 < v.size:
            his.append(v[b1:b1 + 1] >> np.uint64(32))
        flags.append(np.unique(np.concatenate(his)).size == 1)
    return flags


class Pair:
    def __init__(self, name, u, v, pu=0, pv=0, valid=True):
        self.name, self.u, self.v, self.pu, self.pv = name, arr(u), arr(v), pu, pv
        if valid:
            for a in (self.u, self.v):
                assert a.size < 2 or np.all(a[1:] > a[:-1]), name
            self.flags = narrow_flags(self.u, self.v)
            self.want = {"intersect": np.intersect1d(self.u, self.v),
                         "difference": np.setdiff1d(self.u, self.v),
                         "merge": np.union1d(self.u, self.v)}
        assert self.u.size + self.v.size <= 12500, name
        self._dev = None
        self.one_shot = {}

    def dev(self):
        """Slices of larger device tensors at the asked u64 parity; the
        elements around the slice would change a result if they were read."""
        if self._dev is None:
            out = []
            for own, par in ((self.u, self.pu), (self.v, self.pv)):
                off = 2 - par
                pad_lo = own[:1] if own.size else arr([7])
                pad_hi = own[-1:] if own.size else arr([7])
                big = np.concatenate([np.repeat(pad_lo, off), own, np.repeat(pad_hi, 2)])
                t = torch.from_numpy(big.view(np.int64)).to("cuda:0")
                s = t[off:off + own.size]
                assert own.size == 0 or (s.data_ptr() >> 3) & 1 == par
                out.append(s)
            self._dev = tuple(out)
        return self._dev


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def new_outs(pairs):
    return [torch.full((p.u.size + p.v.size + GUARD,), -1, dtype=torch.int64, device="cuda:0")
            for p in pairs]


def one_shot(eng, p, key):
    """The 64-bit path's answer, computed once per (pair, op)."""
    if key not in p.one_shot:
        du, dv = p.dev()
        fn = eng.intersect_pairs if key == "intersect" else (
            eng.difference_pairs if key == "difference" else eng.merge_pairs)
        outs, lens = fn([du], [dv])
        p.one_shot[key] = to_np(outs[0][:lens[0]]).copy()
    return p.one_shot[key]


def check(eng, pairs, outs, lens, key, what):
    for p, o, n in zip(pairs, outs, lens):
        w = p.want[key]
        assert int(n) == w.size, f"{what}: {p.name}: length {n} != {w.size}"
        got = to_np(o[:n])
        assert np.array_equal(got, w), f"{what}: {p.name}: differs from numpy"
        assert np.array_equal(got, one_shot(eng, p, key)), \
            f"{what}: {p.name}: differs from the one-shot call"
        cap = p.u.size + p.v.size
        assert bool((o[cap:] == -1).all()), f"{what}: {p.name}: wrote past the capacity"


def expected_info(pairs):
    tiles = sum(len(p.flags) for p in pairs)
    narrow = sum(sum(p.flags) for p in pairs)
    return tiles, narrow


def run_batch(eng, pairs, order):
    """One fresh batch; `order` holds op names, or (op name, n_runs) for
    run_n.  Every run is checked, and so is info() before and after."""
    du = [p.dev()[0] for p in pairs]
    dv = [p.dev()[1] for p in pairs]
    outs = new_outs(pairs)
    tiles, narrow = expected_info(pairs)
    b = eng.make_batch(du, dv, outs)
    try:
        info = b.info()
        assert info == {"tiles": tiles, "narrow_tiles": 0, "narrow_bytes": 0}
        built = False
        for i, step in enumerate(order):
            key, n_runs = step if isinstance(step, tuple) else (step, 0)
            for o in outs:
                o.fill_(-1)
            lens = b.run_n(OPS[key], n_runs) if n_runs else b.run(OPS[key])
            what = f"order {order}, step {i + 1}"
            check(eng, pairs, outs, lens, key, what)
            built = built or key != "merge"
            info = b.info()
            assert info["tiles"] == tiles, what
            if built and tiles:
                assert info["narrow_tiles"] == narrow, f"{what}: {info}, want {narrow}"
                assert info["narrow_bytes"] >= tiles * (TILE + 4) * 4, what
            else:
                assert info["narrow_tiles"] == 0 and info["narrow_bytes"] == 0, what
    finally:
        b.close()


BOTH = (("intersect", "difference"), ("difference", "intersect"))


def lows_pair(rng, n, m, common, lo=0, hi=U32):
    """Sorted distinct low words in [lo, hi): n for u, m for v, `common` shared."""
    pool = np.sort(rng.choice(np.arange(lo, hi, max(1, (hi - lo) // (4 * (n + m))),
                                        dtype=np.uint64), size=n + m - common, replace=False))
    perm = rng.permutation(pool.size)
    c = pool[perm[:common]]
    u = np.sort(np.concatenate([c, pool[perm[common:n]]]))
    v = np.sort(np.concatenate([c, pool[perm[n:]]]))
    return u, v


# ---------------------------------------------------------------- cases

@pytest.mark.parametrize("hi", [5, 0, 0xFFFFFFFF])
def test_constant_high_word(eng, hi):
    rng = np.random.default_rng(synth.SEED + 300 + (hi & 0xff))
    ul, vl = lows_pair(rng, 3000, 3000, 40)
    if hi == 0xFFFFFFFF:  # UINT64_MAX itself, on both sides
        ul[-1] = vl[-1] = U32 - 1
    p = Pair(f"const_hi_{hi:x}", with_hi(hi, ul), with_hi(hi, vl))
    assert p.flags == [True, True, True]
    assert p.want["intersect"].size >= 40
    assert np.all(p.want["intersect"] >> np.uint64(32) == np.uint64(hi))
    if hi == 0xFFFFFFFF:
        assert int(p.want["intersect"][-1]) == (1 << 64) - 1
    for order in BOTH:
        run_batch(eng, [p], order)


def test_low_half_extremes(eng):
    """0, 1, 0xFFFFFFFE, 0xFFFFFFFF present and matching; one tile holds low
    words on both sides of 0x80000000, where a signed compare orders wrongly."""
    rng = np.random.default_rng(synth.SEED + 310)
    ul, vl = lows_pair(rng, 2990, 2990, 30, lo=2, hi=U32 - 2)
    edge = arr([0, 1, 0x7FFFFFFF, 0x80000000, 0x80000001, U32 - 2, U32 - 1])
    ul = np.unique(np.concatenate([ul, edge]))
    vl = np.unique(np.concatenate([vl, edge]))
    p = Pair("low_extremes", with_hi(3, ul), with_hi(3, vl), 1, 0)
    assert all(p.flags) and len(p.flags) == 3
    a0, a1, b0, b1 = tile_ranges(p.u, p.v)[1]
    mid = with_hi(3, [0x80000000])[0]
    assert p.u[a0] < mid < p.u[a1 - 1] and p.v[b0] < mid < p.v[b1 - 1]
    assert set(with_hi(3, edge).tolist()) <= set(p.want["intersect"].tolist())
    for order in BOTH:
        run_batch(eng, [p], order)


def test_same_low_word_other_high_word(eng):
    """u holds x, v holds x + 2^32, in one tile: wide, and nothing matches."""
    lows = np.arange(1000, dtype=np.uint64) * 7 + 3
    p = Pair("same_low_1tile", with_hi(5, lows), with_hi(6, lows))
    assert p.flags == [False] and p.want["intersect"].size == 0
    # three tiles: all-A with a lookahead in v's range (wide), the seam
    # (wide), all-B (narrow)
    lows3 = np.arange(3000, dtype=np.uint64) * 5 + 1
    q = Pair("same_low_3tiles", with_hi(5, lows3), with_hi(6, lows3), 0, 1)
    assert q.flags == [False, False, True] and q.want["intersect"].size == 0
    for order in BOTH:
        run_batch(eng, [p, q], order)


def crossing_pair(name, hi, n_lo, n_hi, pu=0, pv=0, common=25, seed=0):
    """Both lists hold n_lo elements at the top of range hi and n_hi at the
    bottom of range hi + 1."""
    rng = np.random.default_rng(synth.SEED + 320 + seed)
    ul0, vl0 = lows_pair(rng, n_lo, n_lo, common, lo=U32 - (1 << 20), hi=U32)
    ul1, vl1 = lows_pair(rng, n_hi, n_hi, common, lo=0, hi=1 << 20)
    u = np.concatenate([with_hi(hi, ul0), with_hi(hi + 1, ul1)])
    v = np.concatenate([with_hi(hi, vl0), with_hi(hi + 1, vl1)])
    return Pair(name, u, v, pu, pv)


def test_crossing_a_boundary(eng):
    """Both lists cross 2^32 in the middle of tile 2 of 6: exactly that tile
    is wide, and matches on both sides of the seam are found."""
    p = crossing_pair("crossing", 7, 2500, 3500)
    assert p.flags == [True, True, False, True, True, True]
    w = p.want["intersect"] >> np.uint64(32)
    assert np.sum(w == 7) >= 25 and np.sum(w == 8) >= 25
    for order in BOTH:
        run_batch(eng, [p], order)


def test_lookahead_in_another_range(eng):
    """Tile 0 is exactly the 2048 elements of range 5; only its lookahead
    v[b1] lies in range 6."""
    rng = np.random.default_rng(synth.SEED + 330)
    ul, vl = lows_pair(rng, 1024, 1024, 20)
    v = np.concatenate([with_hi(5, vl), with_hi(6, np.arange(1000, dtype=np.uint64) * 3)])
    p = Pair("lookahead_other", with_hi(5, ul), v, 1, 1)
    (a0, a1, b0, b1), _ = tile_ranges(p.u, p.v)
    assert (a1 - a0, b1 - b0) == (1024, 1024) and int(p.v[b1]) >> 32 == 6
    assert p.flags == [False, True]
    for order in BOTH:
        run_batch(eng, [p], order)


def test_match_at_a_tile_seam(eng):
    """The last A element of tile 0 equals B's lookahead: narrow, found once."""
    u = 10 + 2 * np.arange(1500, dtype=np.uint64)
    v = np.concatenate([arr([1]), 11 + 2 * np.arange(1499, dtype=np.uint64)])
    v[1024] = u[1023]
    p = Pair("seam_match", with_hi(9, u), with_hi(9, v))
    a0, a1, b0, b1 = tile_ranges(p.u, p.v)[0]
    assert a1 == 1024 and b1 == 1024 and p.u[a1 - 1] == p.v[b1]
    assert p.flags == [True, True]
    assert p.want["intersect"].tolist() == [int(with_hi(9, [u[1023]])[0])]
    for order in BOTH:
        run_batch(eng, [p], order)


def degenerate_pairs():
    rng = np.random.default_rng(synth.SEED + 340)
    hi = 11
    ps = []
    # tile 0 all A, tile 1 all B (v sits in a gap of u); and swapped
    u = np.concatenate([np.arange(TILE) * 2 + 1, 50_000 + np.arange(300) * 2])
    v = 10_000 + np.arange(TILE + 100) * 3
    ps.append(Pair("all_a_then_all_b", with_hi(hi, u), with_hi(hi, v), 1, 1))
    ps.append(Pair("all_b_then_all_a", with_hi(hi, v), with_hi(hi, u), 0, 1))
    some = with_hi(hi, np.arange(2500) * 5 + 3)
    ps.append(Pair("n0", [], some, 0, 1))
    ps.append(Pair("m0", some, [], 1, 0))
    ps.append(Pair("n0_m0", [], []))
    ps.append(Pair("n1_hit", some[1200:1201], some, 1, 0))
    ps.append(Pair("n1_miss", some[1200:1201] + np.uint64(1), some, 0, 0))
    for path in (2047, 2048, 2049, 4097 + 300):
        ul, vl = lows_pair(rng, path // 2, path - path // 2, min(30, path // 4))
        ps.append(Pair(f"path{path}", with_hi(hi, ul), with_hi(hi, vl), path & 1, 1))
    return ps


def test_degenerate_tiles(eng):
    ps = degenerate_pairs()
    by = {p.name: p for p in ps}
    (a0, a1, b0, b1) = tile_ranges(by["all_a_then_all_b"].u, by["all_a_then_all_b"].v)[0]
    assert (a1 - a0, b1 - b0) == (TILE, 0)
    (a0, a1, b0, b1) = tile_ranges(by["all_b_then_all_a"].u, by["all_b_then_all_a"].v)[0]
    assert (a1 - a0, b1 - b0) == (0, TILE)
    assert [len(by[f"path{x}"].flags) for x in (2047, 2048, 2049, 4397)] == [1, 1, 2, 3]
    assert all(all(p.flags) for p in ps)
    for order in BOTH:
        run_batch(eng, ps, order)
    run_batch(eng, [by["n0_m0"]], ("intersect", "difference"))  # a batch without tiles


def test_odd_alignment(eng):
    """All four pointer parities, one range each."""
    rng = np.random.default_rng(synth.SEED + 350)
    ps = []
    for k in range(4):
        ul, vl = lows_pair(rng, 2300 + 17 * k, 2100 - 5 * k, 33)
        ps.append(Pair(f"parity{k}", with_hi(20 + k, ul), with_hi(20 + k, vl), k & 1, k >> 1))
    assert all(all(p.flags) for p in ps)
    for order in BOTH:
        run_batch(eng, ps, order)


def test_dense_emission(eng):
    """Difference emits nearly all of A, intersect nearly all of it when the
    lists are almost equal: far more than STAGE_P per tile, so the overflow
    staging carries high words too."""
    rng = np.random.default_rng(synth.SEED + 360)
    ul, vl = lows_pair(rng, 3000, 3000, 10)
    sparse = Pair("diff_dense", with_hi(0x1234, ul), with_hi(0x1234, vl), 1, 0)
    assert all(sparse.flags)
    for a0, a1, _, _ in tile_ranges(sparse.u, sparse.v):
        assert a1 - a0 - 10 > STAGE_P
    ul2, vl2 = lows_pair(rng, 3000, 3000, 2950)
    same = Pair("isect_dense", with_hi(0xABCD, ul2), with_hi(0xABCD, vl2), 0, 1)
    assert all(same.flags) and same.want["intersect"].size == 2950
    for order in BOTH:
        run_batch(eng, [sparse, same], order)


def mixed_pairs():
    rng = np.random.default_rng(synth.SEED + 370)
    ps = []
    for k in range(24):
        hi = 100 + 3 * k
        if k % 6 == 2:
            ps.append(Pair(f"mixed{k}_empty", [], []))
        elif k % 6 == 4:
            ps.append(crossing_pair(f"mixed{k}_cross", hi, 900 + 50 * k, 1500 - 20 * k,
                                    k & 1, (k >> 1) & 1, seed=k))
        else:
            n = int(rng.integers(1, 3000))
            m = int(rng.integers(1, 3000))
            ul, vl = lows_pair(rng, n, m, int(rng.integers(0, min(n, m) + 1) // 3))
            ps.append(Pair(f"mixed{k}", with_hi(hi, ul), with_hi(hi, vl), k & 1, (k >> 1) & 1))
    return ps


def test_mixed_batch(eng):
    ps = mixed_pairs()
    tiles, narrow = expected_info(ps)
    assert 0 < tiles - narrow <= 8 and narrow >= 20  # the crossing pairs' seams
    assert {(p.pu, p.pv) for p in ps} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for order in BOTH:
        run_batch(eng, ps, order)


@pytest.mark.parametrize("order", [
    ("merge", "intersect", "difference"),   # no slab until the intersect
    (("intersect", 3),),                    # run_n on a fresh batch
    (("difference", 3),),
    ("intersect", "intersect", ("intersect", 3)),
    ("difference", "merge", ("intersect", 2), "difference"),
], ids=lambda o: "-".join(s if isinstance(s, str) else f"{s[0]}x{s[1]}" for s in o))
def test_order_of_ops(eng, order):
    ps = [crossing_pair("order_cross", 40, 2200, 2400, 1, 0, seed=99)]
    ps += [p for p in degenerate_pairs() if p.name in ("path2049", "n0_m0", "n1_hit")]
    run_batch(eng, ps, order)


def test_opt_out(eng, monkeypatch):
    """UA_NARROW=0 before the batch is made: no narrow tile, same outputs."""
    ps = [crossing_pair("optout_cross", 60, 2100, 2300, 0, 1, seed=7)]
    assert 0 < sum(ps[0].flags) < len(ps[0].flags)
    du, dv = [ps[0].dev()[0]], [ps[0].dev()[1]]
    got = {}
    for mode in ("narrow", "off"):
        if mode == "off":
            monkeypatch.setenv("UA_NARROW", "0")
        outs = new_outs(ps)
        b = eng.make_batch(du, dv, outs)
        try:
            for key in ("intersect", "difference", "intersect"):
                for o in outs:
                    o.fill_(-1)
                lens = b.run(OPS[key])
                check(eng, ps, outs, lens, key, f"{mode}: {key}")
                got[(mode, key)] = to_np(outs[0][:lens[0]]).copy()
            info = b.info()
            if mode == "off":
                assert info["narrow_tiles"] == 0 and info["narrow_bytes"] == 0
            else:
                assert info["narrow_tiles"] == sum(ps[0].flags)
        finally:
            b.close()
    for key in ("intersect", "difference"):
        assert np.array_equal(got[("narrow", key)], got[("off", key)])


@pytest.mark.parametrize("kind", ["duplicates", "unsorted"])
@pytest.mark.parametrize("key", ["intersect", "difference"])
def test_invalid_input(eng, monkeypatch, kind, key):
    """Inputs that break the contract, inside one 2^32 range: the run
    completes, lengths stay within capacity, nothing behind it is written, and
    the outputs equal those of the same batch with UA_NARROW=0, on the run
    that searches the splits and on the run that reads them back."""
    rng = np.random.default_rng(synth.SEED + 380)
    if kind == "duplicates":
        ul = np.repeat(np.arange(900, dtype=np.uint64) * 4 + 2, 3)
        vl = np.repeat(np.arange(900, dtype=np.uint64) * 6, 3)
    else:
        ul = rng.integers(0, 5000, size=2700).astype(np.uint64)
        vl = rng.integers(0, 5000, size=2700).astype(np.uint64)
        ul[:1200].sort()
        vl[900:].sort()
    p = Pair(f"invalid_{kind}", with_hi(77, ul), with_hi(77, vl), 1, 0, valid=False)
    du, dv = p.dev()
    cap = {"intersect": min(p.u.size, p.v.size), "difference": p.u.size}[key]
    got = {}
    for mode in ("narrow", "off"):
        if mode == "off":
            monkeypatch.setenv("UA_NARROW", "0")
        out = torch.full((cap + GUARD,), -1, dtype=torch.int64, device="cuda:0")
        b = eng.make_batch([du], [dv], [out])
        try:
            for run in (1, 2):
                out.fill_(-1)
                lens = b.run(OPS[key])
                assert lens[0] <= cap, f"{mode} run {run}: length {lens[0]} > {cap}"
                assert bool((out[cap:] == -1).all()), f"{mode} run {run}: guard overwritten"
                got[(mode, run)] = to_np(out[:lens[0]]).copy()
            narrow = b.info()["narrow_tiles"]
            assert narrow == 0 if mode == "off" else narrow <= b.info()["tiles"]
        finally:
            b.close()
    for run in (1, 2):
        assert np.array_equal(got[("narrow", run)], got[("off", run)]), f"run {run}"


def test_host_model():
    """tile_ranges against a brute-force merge (host arithmetic only)."""
    rng = np.random.default_rng(synth.SEED + 390)
    ul, vl = lows_pair(rng, 2500, 2200, 300, lo=0, hi=1 << 16)
    u, v = arr(ul), arr(vl)
    tagged = sorted([(int(x), 0) for x in u] + [(int(x), 1) for x in v])
    for t, (a0, a1, b0, b1) in enumerate(tile_ranges(u, v)):
        seg = tagged[t * TILE:(t + 1) * TILE]
        assert sum(1 for _, s in seg if s == 0) == a1 - a0
        assert sum(1 for _, s in seg if s == 1) == b1 - b0
        assert a0 + b0 == t * TILE
