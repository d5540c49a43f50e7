"""The sentinel walk of narrow full tiles.  A prepared batch's 32-bit record
closes the tile's A range with 0xFFFFFFFF and its B range with the lookahead's
low half (0xFFFFFFFF when there is none), and a narrow tile that is full
(c0: alen + blen == 2048), holds no 0xFFFFFFFF low half (c1) and has no A
element above its lookahead (c2) is FAST: it is walked with no range test at
all.  Every other narrow tile keeps the guarded walk on the same record.
Results must not depend on which walk a tile takes.

Every case runs prepared batches of a few pairs and compares intersect and
difference with numpy, with the one-shot call (the 64-bit path) and with a
batch made under UA_NARROW=0, on the run that searches the splits and on the
run that reads them back (both orders of the two ops), and asserts
`Batch.fast_tiles()` against a host model of c0-c2 over the partition
(`tile_flags`), so that a case cannot pass on the guarded walk by accident.
What a case needs from the model is asserted in the case as well.

Tile = 2048 merge-path elements, 256 threads x 2 chains x 4 steps.
"""
import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth

gpu = pytest.mark.gpu

TILE = 2048
GUARD = 8
OPS = {"intersect": algo.OP_INTERSECT, "difference": algo.OP_DIFFERENCE}
U32 = 1 << 32
FF = U32 - 1
BOTH = (("intersect", "difference"), ("difference", "intersect"))


def arr(x):
    return np.asarray(x, dtype=np.uint64)


def with_hi(hi, lows):
    return (np.uint64(hi) << np.uint64(32)) | arr(lows)


def tile_ranges(u, v):
    """[(a0, a1, b0, b1)] per tile of a sorted pair: merge path with A first
    on ties, cut every TILE path elements."""
    n, m = u.size, v.size
    pos_u = np.arange(n) + np.searchsorted(v, u, side="left")
    out = []
    for d0 in range(0, n + m, TILE):
        d1 = min(d0 + TILE, n + m)
        a0 = int(np.searchsorted(pos_u, d0, side="left"))
        a1 = int(np.searchsorted(pos_u, d1, side="left"))
        out.append((a0, a1, d0 - a0, d1 - a1))
    return out


def tile_flags(u, v):
    """Per tile of a sorted pair: (narrow, fast)."""
    sh, low = np.uint64(32), np.uint64(FF)
    out = []
    for a0, a1, b0, b1 in tile_ranges(u, v):
        A, B = u[a0:a1], v[b0:b1]
        his = [A >> sh, B >> sh]
        if b1 < v.size:
            his.append(v[b1:b1 + 1] >> sh)
        narrow = np.unique(np.concatenate(his)).size == 1
        c0 = A.size + B.size == TILE
        c1 = not np.any(A & low == low) and not np.any(B & low == low)
        c2 = b1 >= v.size or A.size == 0 or bool(np.all(A <= v[b1]))
        out.append((narrow, narrow and c0 and c1 and c2))
    return out


class Pair:
    def __init__(self, name, u, v, pu=0, pv=0, valid=True):
        self.name, self.u, self.v, self.pu, self.pv = name, arr(u), arr(v), pu, pv
        self.valid = valid
        if valid:
            for a in (self.u, self.v):
                assert a.size < 2 or np.all(a[1:] > a[:-1]), name
            fl = tile_flags(self.u, self.v)
            self.narrow = [f[0] for f in fl]
            self.fast = [f[1] for f in fl]
            self.want = {"intersect": np.intersect1d(self.u, self.v),
                         "difference": np.setdiff1d(self.u, self.v)}
        assert self.u.size <= 12500 and self.v.size <= 12500, name
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
                out.append(t[off:off + own.size])
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
    return [torch.full((p.u.size + GUARD,), -1, dtype=torch.int64, device="cuda:0")
            for p in pairs]


def one_shot(eng, p, key):
    """The 64-bit path's answer, computed once per (pair, op)."""
    if key not in p.one_shot:
        du, dv = p.dev()
        fn = eng.intersect_pairs if key == "intersect" else eng.difference_pairs
        outs, lens = fn([du], [dv])
        p.one_shot[key] = to_np(outs[0][:lens[0]]).copy()
    return p.one_shot[key]


def run_order(eng, pairs, order, want_fast, want_narrow=None):
    """One fresh batch; `order` holds op names, or (op name, n_runs) for
    run_n.  Returns [per-pair outputs] per step.  Lengths stay within the
    capacity and the guard words intact on every input; fast_tiles() and
    info()'s narrow-tile count are asserted when they are given."""
    du = [p.dev()[0] for p in pairs]
    dv = [p.dev()[1] for p in pairs]
    outs = new_outs(pairs)
    got = []
    b = eng.make_batch(du, dv, outs)
    try:
        assert b.fast_tiles() == 0  # no record before the first staged run
        for i, step in enumerate(order):
            key, n_runs = step if isinstance(step, tuple) else (step, 0)
            for o in outs:
                o.fill_(-1)
            lens = b.run_n(OPS[key], n_runs) if n_runs else b.run(OPS[key])
            what = f"order {order}, step {i + 1}"
            res = []
            for p, o, n in zip(pairs, outs, lens):
                cap = min(p.u.size, p.v.size) if key == "intersect" else p.u.size
                assert int(n) <= cap, f"{what}: {p.name}: length {n} > {cap}"
                assert bool((o[p.u.size:] == -1).all()), f"{what}: {p.name}: guard overwritten"
                res.append(to_np(o[:n]).copy())
            got.append(res)
            if want_fast is not None:
                assert b.fast_tiles() == want_fast, \
                    f"{what}: fast_tiles {b.fast_tiles()}, want {want_fast} of {b.info()}"
            if want_narrow is not None:  # "narrow" has not moved
                assert b.info()["narrow_tiles"] == want_narrow, f"{what}: {b.info()}"
    finally:
        b.close()
    return got


def run_case(eng, monkeypatch, pairs, orders=BOTH):
    """Valid pairs: every run of every order equals numpy, the one-shot call
    and the UA_NARROW=0 batch."""
    want_fast = sum(sum(p.fast) for p in pairs)
    with monkeypatch.context() as mp:
        mp.setenv("UA_NARROW", "0")
        off = dict(zip(BOTH[0], run_order(eng, pairs, BOTH[0], 0)))
    for order in orders:
        got = run_order(eng, pairs, order, want_fast, sum(sum(p.narrow) for p in pairs))
        for i, (step, res) in enumerate(zip(order, got)):
            key = step[0] if isinstance(step, tuple) else step
            for k, (p, g) in enumerate(zip(pairs, res)):
                what = f"order {order}, step {i + 1}: {p.name}"
                assert np.array_equal(g, p.want[key]), f"{what}: differs from numpy"
                assert np.array_equal(g, one_shot(eng, p, key)), f"{what}: differs from one-shot"
                assert np.array_equal(g, off[key][k]), f"{what}: differs from UA_NARROW=0"
    return want_fast


def lows_pair(rng, n, m, common, lo=0, hi=FF):
    """Sorted distinct low words in [lo, hi): n for u, m for v, `common`
    shared.  hi defaults to 0xFFFFFFFF exclusive: none is the sentinel."""
    pool = np.sort(rng.choice(np.arange(lo, hi, max(1, (hi - lo) // (4 * (n + m))),
                                        dtype=np.uint64), size=n + m - common, replace=False))
    perm = rng.permutation(pool.size)
    c = pool[perm[:common]]
    u = np.sort(np.concatenate([c, pool[perm[common:n]]]))
    v = np.sort(np.concatenate([c, pool[perm[n:]]]))
    return u, v


# ---------------------------------------------------------------- cases

@gpu
@pytest.mark.parametrize("hi", [0, 5])
@pytest.mark.parametrize("common", [30, 1536], ids=["1pct", "50pct"])
def test_plain_full_tiles(eng, monkeypatch, hi, common):
    rng = np.random.default_rng(synth.SEED + 500 + hi + common)
    ul, vl = lows_pair(rng, 3072, 3072, common)
    p = Pair(f"plain_{hi}_{common}", with_hi(hi, ul), with_hi(hi, vl), hi & 1, 1)
    assert p.fast == [True, True, True] and p.want["intersect"].size == common
    run_case(eng, monkeypatch, [p])


@gpu
def test_identical_and_disjoint(eng, monkeypatch):
    """Identical lists: every A step emits for intersect, none for
    difference.  Interleaved disjoint lists: difference emits all of A."""
    x = np.arange(TILE, dtype=np.uint64) * 3 + 1
    same = Pair("identical", with_hi(2, x), with_hi(2, x), 1, 0)
    ev = Pair("interleaved", with_hi(3, x * 2), with_hi(3, x * 2 + 1), 0, 1)
    assert same.fast == [True, True] and ev.fast == [True, True]
    assert same.want["intersect"].size == TILE and same.want["difference"].size == 0
    assert ev.want["intersect"].size == 0 and ev.want["difference"].size == TILE
    run_case(eng, monkeypatch, [same, ev])


def tile_end_pairs():
    rng = np.random.default_rng(synth.SEED + 510)
    hi = 11
    ps = []
    # tile 0 = 2048 A and no B, with a lookahead (sa and sb both in the tail);
    # tile 1 = 2048 B and no A; and swapped
    u = np.concatenate([np.arange(TILE) * 2 + 1, 50_000 + np.arange(300) * 2])
    v = 10_000 + np.arange(TILE + 100) * 3
    ps.append(Pair("all_a_then_all_b", with_hi(hi, u), with_hi(hi, v), 1, 1))
    ps.append(Pair("all_b_then_all_a", with_hi(hi, v), with_hi(hi, u), 0, 1))
    # alen = 1 and alen = 2047, in a single full tile without a lookahead
    # and in a first tile with one
    some = np.arange(3000, dtype=np.uint64) * 5 + 3
    ps.append(Pair("alen1_hit", with_hi(hi, some[1000:1001]), with_hi(hi, some[:TILE - 1]), 1, 0))
    ps.append(Pair("alen1_miss", with_hi(hi, some[1000:1001] + 1), with_hi(hi, some), 0, 0))
    ps.append(Pair("alen2047_hit", with_hi(hi, some[:TILE - 1]), with_hi(hi, some[7:8]), 0, 1))
    ps.append(Pair("alen2047_miss",
                   with_hi(hi, np.concatenate([some[:TILE - 1], some[TILE - 1:] + 1])),
                   with_hi(hi, some[2046:2047] + 1), 1, 1))
    # path an exact multiple of the tile; the last tile ends on A, and on B:
    # no lookahead, sb is the sentinel, and the other side runs out mid-tile
    ul, vl = lows_pair(rng, TILE, TILE, 40)
    if ul[-1] < vl[-1]:
        ul, vl = vl, ul
    ps.append(Pair("ends_on_a", with_hi(hi, ul), with_hi(hi, vl), 0, 1))
    ps.append(Pair("ends_on_b", with_hi(hi, vl), with_hi(hi, ul), 1, 0))
    # u runs out in the middle of tile 0 and B goes on for two more tiles
    ul, vl = lows_pair(rng, 1000, 1048, 25, hi=1 << 20)
    vl = np.concatenate([vl, (1 << 21) + np.arange(3000, dtype=np.uint64) * 7])
    ps.append(Pair("u_exhausted", with_hi(hi, ul), with_hi(hi, vl), 1, 1))
    return ps


@gpu
def test_tile_end_shapes(eng, monkeypatch):
    ps = tile_end_pairs()
    by = {p.name: p for p in ps}

    def shape(name, t):
        a0, a1, b0, b1 = tile_ranges(by[name].u, by[name].v)[t]
        return a1 - a0, b1 - b0, b1 < by[name].v.size

    assert shape("all_a_then_all_b", 0) == (TILE, 0, True)
    assert shape("all_a_then_all_b", 1) == (0, TILE, True)
    assert shape("all_b_then_all_a", 0) == (0, TILE, True)
    assert shape("all_b_then_all_a", 1) == (TILE, 0, True)
    assert shape("alen1_hit", 0) == (1, TILE - 1, False)
    assert shape("alen1_miss", 0) == (1, TILE - 1, True)
    assert shape("alen2047_hit", 0) == (TILE - 1, 1, False)
    assert shape("alen2047_miss", 0) == (TILE - 1, 1, False)
    assert by["alen1_hit"].want["intersect"].size == 1
    assert by["alen2047_hit"].want["intersect"].size == 1
    assert by["alen1_miss"].want["intersect"].size == 0
    assert by["alen2047_miss"].want["intersect"].size == 0
    for name in ("ends_on_a", "ends_on_b"):
        assert by[name].fast == [True, True] and not shape(name, 1)[2]
    assert by["ends_on_a"].u[-1] > by["ends_on_a"].v[-1]
    assert shape("u_exhausted", 0) == (1000, 1048, True)
    assert by["u_exhausted"].fast == [True, True, False]
    assert by["all_a_then_all_b"].fast == [True, True, False]
    assert by["alen1_hit"].fast == [True] and by["alen2047_hit"].fast == [True]
    run_case(eng, monkeypatch, ps)


@gpu
@pytest.mark.parametrize("delta", [0, 1, -1], ids=["equal", "a_below", "look_below"])
def test_last_a_against_the_lookahead(eng, monkeypatch, delta):
    """Tile 0 ends on u[1023] and its lookahead is v[1024]: equal (found
    once, in tile 0), one above it, and one below it (then it ends tile 0
    itself and u[1023] opens tile 1)."""
    u = 10 + 4 * np.arange(1500, dtype=np.uint64)
    v = np.concatenate([arr([1]), 12 + 4 * np.arange(1499, dtype=np.uint64)])
    v[1024] = np.uint64(int(u[1023]) + delta)
    p = Pair(f"seam_{delta}", with_hi(9, u), with_hi(9, v), 0, 1)
    a0, a1, b0, b1 = tile_ranges(p.u, p.v)[0]
    if delta >= 0:
        assert (a1, b1) == (1024, 1024) and int(p.v[b1] - p.u[a1 - 1]) == delta
    else:
        assert (a1, b1) == (1023, 1025)
    assert p.fast == [True, False]
    assert p.want["intersect"].size == (1 if delta == 0 else 0)
    run_case(eng, monkeypatch, [p])


def ff_pairs():
    """0xFFFFFFFF as a low half: in A only, in B only, in both (matching),
    and as a full tile's lookahead only."""
    rng = np.random.default_rng(synth.SEED + 520)
    ps = []
    for k, name in enumerate(("ff_in_a", "ff_in_b", "ff_in_both")):
        ul, vl = lows_pair(rng, TILE, TILE, 30)
        if name != "ff_in_b":
            ul[-1] = FF
        if name != "ff_in_a":
            vl[-1] = FF
        ps.append(Pair(name, with_hi(30 + k, ul), with_hi(30 + k, vl), k & 1, 1))
    ul, vl = lows_pair(rng, 1024, 1024, 30)
    ps.append(Pair("ff_lookahead", with_hi(40, ul),
                   with_hi(40, np.concatenate([vl, arr([FF])])), 1, 0))
    return ps


@gpu
def test_sentinel_value_in_the_data(eng, monkeypatch):
    ps = ff_pairs()
    for p in ps[:3]:
        assert p.narrow == [True, True] and p.fast == [True, False], p.name
    both = ps[2]
    assert int(both.want["intersect"][-1]) == (32 << 32) | FF
    assert int(ps[0].want["difference"][-1]) == (30 << 32) | FF
    look = ps[3]
    a0, a1, b0, b1 = tile_ranges(look.u, look.v)[0]
    assert (a1 - a0, b1 - b0) == (1024, 1024) and int(look.v[b1]) & FF == FF
    assert look.narrow == [True, True] and look.fast == [True, False]
    assert run_case(eng, monkeypatch, ps) == 4


@gpu
def test_partial_tile_behind_fast_tiles(eng, monkeypatch):
    rng = np.random.default_rng(synth.SEED + 530)
    ul, vl = lows_pair(rng, 3000, 3000, 33)
    p = Pair("partial_last", with_hi(6, ul), with_hi(6, vl), 1, 0)
    assert p.fast == [True, True, False] and p.narrow == [True] * 3
    run_case(eng, monkeypatch, [p])


def crossing_pair(name, hi, n_lo, n_hi, pu=0, pv=0, common=25, seed=0):
    """Both lists hold n_lo elements at the top of range hi and n_hi at the
    bottom of range hi + 1: the tile on the seam is wide."""
    rng = np.random.default_rng(synth.SEED + 540 + seed)
    ul0, vl0 = lows_pair(rng, n_lo, n_lo, common, lo=U32 - (1 << 20), hi=FF)
    ul1, vl1 = lows_pair(rng, n_hi, n_hi, common, lo=0, hi=1 << 20)
    u = np.concatenate([with_hi(hi, ul0), with_hi(hi + 1, ul1)])
    v = np.concatenate([with_hi(hi, vl0), with_hi(hi + 1, vl1)])
    return Pair(name, u, v, pu, pv)


def mixed_pairs():
    rng = np.random.default_rng(synth.SEED + 550)
    ps = [crossing_pair("mixed_cross", 7, 2500, 3500, 1, 0)]
    ps += ff_pairs()[1:3]
    ps.append(Pair("mixed_empty", [], []))
    for k in range(4):
        n, m = int(rng.integers(1500, 4000)), int(rng.integers(1500, 4000))
        ul, vl = lows_pair(rng, n, m, int(rng.integers(0, 500)))
        ps.append(Pair(f"mixed{k}", with_hi(100 + k, ul), with_hi(100 + k, vl), k & 1, k >> 1))
    return ps


@gpu
def test_mixed_batch(eng, monkeypatch):
    """Wide, narrow-guarded and fast tiles in one grid."""
    ps = mixed_pairs()
    tiles = sum(len(p.fast) for p in ps)
    narrow = sum(sum(p.narrow) for p in ps)
    fast = sum(sum(p.fast) for p in ps)
    assert ps[0].narrow == [True, True, False, True, True, True]
    assert 0 < tiles - narrow and 0 < narrow - fast and fast >= 8
    run_case(eng, monkeypatch, ps)


@gpu
@pytest.mark.parametrize("order", [
    (("intersect", 3),),
    (("difference", 3),),
    ("difference", ("intersect", 2), "difference", "intersect"),
], ids=lambda o: "-".join(s if isinstance(s, str) else f"{s[0]}x{s[1]}" for s in o))
def test_run_n_and_order(eng, monkeypatch, order):
    rng = np.random.default_rng(synth.SEED + 560)
    ul, vl = lows_pair(rng, 2500, 2500, 400)
    ps = [Pair("order", with_hi(8, ul), with_hi(8, vl), 0, 1), tile_end_pairs()[0]]
    run_case(eng, monkeypatch, ps, orders=(order,))


def invalid_pair(kind):
    rng = np.random.default_rng(synth.SEED + 570)
    if kind == "triplicates":  # 4 full tiles and a partial one
        ul = np.repeat(np.arange(1400, dtype=np.uint64) * 4 + 2, 3)
        vl = np.repeat(np.arange(1400, dtype=np.uint64) * 6, 3)
    else:
        # unsorted with sorted stretches: some full tiles hold an A element
        # above their lookahead (c2), and the split searches still end
        ul = rng.integers(0, 9000, size=4500).astype(np.uint64)
        vl = rng.integers(0, 9000, size=4500).astype(np.uint64)
        ul[:2000].sort()
        vl[1500:].sort()
        if kind == "unsorted_ff":
            ul[rng.integers(0, ul.size, size=6)] = FF
            vl[rng.integers(0, vl.size, size=6)] = FF
    return Pair(f"invalid_{kind}", with_hi(77, ul), with_hi(77, vl), 1, 0, valid=False)


@gpu
@pytest.mark.parametrize("kind", ["triplicates", "unsorted", "unsorted_ff"])
def test_invalid_input(eng, monkeypatch, kind):
    """Inputs that break the contract, inside one 2^32 range: every run
    completes, lengths stay within capacity, the guard words stay intact
    (run_order), and the outputs equal those of the same batch under
    UA_NARROW=0 run by run: on the run that searches the splits and on the
    one that reads them back."""
    p = invalid_pair(kind)
    for order in BOTH:
        steps = order + order  # each op on a cached run too
        with monkeypatch.context() as mp:
            mp.setenv("UA_NARROW", "0")
            off = run_order(eng, [p], steps, 0)
        got = run_order(eng, [p], steps, None)
        for i, (g, w) in enumerate(zip(got, off)):
            assert np.array_equal(g[0], w[0]), f"{kind}: order {order}, step {i + 1}"


def test_host_model():
    """tile_ranges and tile_flags against a brute-force merge (host
    arithmetic only): a tile is fast iff it is full, in one 2^32 range with
    its lookahead, and a walk that relies on the sentinels alone would take
    the steps of the guarded walk."""
    rng = np.random.default_rng(synth.SEED + 590)
    ul, vl = lows_pair(rng, 2500, 3644, 300, lo=FF - (1 << 16), hi=FF)
    ul[-1] = FF  # the last tile holds the sentinel's value
    u = np.concatenate([with_hi(1, ul[:1500] - np.uint64(1 << 20)), with_hi(2, ul[1500:])])
    v = np.concatenate([with_hi(1, vl[:1400] - np.uint64(1 << 20)), with_hi(2, vl[1400:])])
    tagged = sorted([(int(x), 0) for x in u] + [(int(x), 1) for x in v])
    flags = tile_flags(u, v)
    assert len(flags) == 3 and len(tagged) == 3 * TILE
    for t, (a0, a1, b0, b1) in enumerate(tile_ranges(u, v)):
        seg = tagged[t * TILE:(t + 1) * TILE]
        A = [x for x, s in seg if s == 0]
        B = [x for x, s in seg if s == 1]
        assert (len(A), len(B)) == (a1 - a0, b1 - b0) and a0 + b0 == t * TILE
        look = [int(v[b1])] if b1 < v.size else []
        narrow = len({x >> 32 for x in A + B + look}) == 1
        assert flags[t][0] == narrow
        # walk the record's logical array with no range test
        L = [x & FF for x in A] + [FF] + [x & FF for x in B] + [look[0] & FF if look else FF]
        in_b = set(B + look)
        i, j, ok = 0, len(A) + 1, len(seg) == TILE
        for x, s in seg:
            if not (ok and i <= len(A) and j <= len(A) + 1 + len(B)):
                ok = False
                break
            take_a, emit = L[i] <= L[j], L[i] == L[j]
            ok = take_a == (s == 0) and emit == (s == 0 and x in in_b)
            i, j = i + take_a, j + (not take_a)
        assert flags[t][1] == (narrow and ok), t
    assert [f[1] for f in flags] == [True, False, False]  # clean; seam; holds 0xFFFFFFFF
