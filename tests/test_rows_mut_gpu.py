"""ua_rows_decode_mut_dev on the GPU: a fan-out of UidPacks with per-row
mutation layers in, a CSR UID matrix out, against the set expression of
tests/rows_mut_ref.py (sorted((P - uids(M)) | sets(M)), then x > after, then
first), which tests/test_rows_mut_ref.py holds to the reference's known
answers.

Packs are uploaded from the bytes of tests/gv_spec.py, never from an engine
encoder.  Output buffers are pre-filled with a sentinel and carry 64 guard
words past their capacity.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import gv_spec as gv
import rows_decode_ref
from dgraph_amd import _lib, algo
from rows_mut_ref import MUT_DEL, MUT_OVR, MUT_SET, flat, want_row, want_rows

pytestmark = pytest.mark.gpu

UA_ERR_INVALID = 3
GUARD = 64
SENT = 0xA5A5A5A5A5A5A5A5
SENT_I64 = SENT - (1 << 64)
DEV = "cuda:0"
I32_MIN, I32_MAX = -2**31, 2**31 - 1
S, D = MUT_SET, MUT_DEL


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def arena(eng, flats):
    """[[(base, num, deltas)]] per row -> uploaded arena with row boundaries."""
    return eng.upload_pack_batch(
        [(*gv.flatten(blocks), sum(nu for _, nu, _ in blocks)) for blocks in flats])


def dev_u64(vals):
    a = gv.u64(vals)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.int64, device=DEV)
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def dev_i32(vals):
    if not len(vals):
        return torch.zeros(1, dtype=torch.int32, device=DEV)
    return torch.tensor(list(vals), dtype=torch.int32, device=DEV)


def dev_u8(vals):
    if not len(vals):
        return torch.zeros(1, dtype=torch.uint8, device=DEV)
    return torch.tensor(list(vals), dtype=torch.uint8, device=DEV)


def u64_list(t):
    return t.cpu().numpy().view(np.uint64).tolist()


class Result:
    pass


def run(eng, dpb, muts=None, afters=None, firsts=None, cap=None, count_only=False,
        raw=None, plain=False):
    """One raw call into sentinel-filled buffers: ua_rows_decode_mut_dev with
    the rows' (uid, op) lists (or raw = (mut_uids, mut_ops, row_mut_base,
    n_mut) as they are; muts None = no arrays at all), or with plain the
    existing ua_rows_decode_dev."""
    n_rows = len(dpb.pbb) - 1
    nb = int(dpb.pbb[n_rows])
    mu, mo, rmb, n_mut = [], [], None, 0
    if raw is not None:
        mu, mo, rmb, n_mut = raw
    elif muts is not None:
        mu, mo, rmb = flat(muts)
        n_mut = len(mu)
    if cap is None:
        cap = int(sum(dpb.pack_totals)) + n_mut
    rbb = dev_u64([int(x) for x in dpb.pbb])
    t_after = dev_u64(afters) if afters is not None else None
    t_first = dev_i32(firsts) if firsts is not None else None
    t_mu, t_mo = dev_u64(mu), dev_u8(mo)
    t_rmb = dev_u64(rmb) if rmb is not None else None
    out = torch.full((cap + GUARD,), SENT_I64, dtype=torch.int64, device=DEV)
    oro = torch.full((n_rows + 1 + GUARD,), SENT_I64, dtype=torch.int64, device=DEV)
    d = _lib.UaDRowPacks() if plain else _lib.UaDRowMut()
    d.bases, d.num_uids = dpb.bases.data_ptr(), dpb.num_uids.data_ptr()
    d.delta_offs, d.deltas = dpb.delta_offs.data_ptr(), dpb.deltas.data_ptr()
    d.n_blocks, d.n_rows = nb, n_rows
    d.row_block_base = rbb.data_ptr() if n_rows else None
    d.after = t_after.data_ptr() if t_after is not None else None
    d.first = t_first.data_ptr() if t_first is not None else None
    if not plain:
        d.mut_uids = t_mu.data_ptr() if rmb is not None else None
        d.mut_ops = t_mo.data_ptr() if rmb is not None else None
        d.row_mut_base = t_rmb.data_ptr() if rmb is not None else None
        d.n_mut = n_mut
    d.out_vals = None if count_only else out.data_ptr()
    d.cap_vals = 0 if count_only else cap
    d.out_row_offs = oro.data_ptr()
    total = C.c_uint64(77)
    res = Result()
    fn = _lib.lib().ua_rows_decode_dev if plain else _lib.lib().ua_rows_decode_mut_dev
    res.rc = fn(eng._ctx, C.byref(d), C.byref(total))
    res.total = total.value
    res.out = u64_list(out)
    res.offs = u64_list(oro)[:n_rows + 1]
    res.guards_ok = (res.out[cap:] == [SENT] * GUARD and
                     u64_list(oro)[n_rows + 1:] == [SENT] * GUARD)
    res.rows = [res.out[res.offs[r]:res.offs[r + 1]] for r in range(n_rows)] \
        if res.offs and res.offs[-1] <= cap else None
    res.cap = cap
    return res


def check(res, want):
    """A successful call: rows, running lengths, total, guards, and nothing
    written between the total and the capacity."""
    assert res.rc == 0
    offs = [0]
    for w in want:
        offs.append(offs[-1] + len(w))
    assert res.offs == offs
    assert res.total == offs[-1]
    assert res.guards_ok
    for r, w in enumerate(want):
        assert res.rows[r] == w, f"row {r}"
    assert res.out[res.total:res.cap] == [SENT] * (res.cap - res.total)


def check_model(eng, flats, muts, afters=None, firsts=None):
    """The call and its count-only form against the model."""
    lists = [gv.decode(f) for f in flats]
    want = want_rows(lists, muts, afters, firsts)
    dpb = arena(eng, flats)
    check(run(eng, dpb, muts, afters, firsts), want)
    cnt = run(eng, dpb, muts, afters, firsts, count_only=True)
    assert (cnt.rc, cnt.total) == (0, sum(len(w) for w in want))
    assert [b - a for a, b in zip(cnt.offs, cnt.offs[1:])] == [len(w) for w in want]
    assert cnt.guards_ok
    return want


# ---------- 1. empty layers ----------

@pytest.fixture(scope="module")
def format_case(eng):
    lists, flats = [], []
    for name in sorted(gv.inputs()):
        for bs in gv.BLOCK_SIZES:
            lists.append(gv.inputs()[name])
            flats.append(gv.encode(lists[-1], bs))
    return lists, flats, arena(eng, flats)


@pytest.mark.parametrize("opts", [False, True])
def test_empty_layers_are_the_plain_decode(eng, format_case, opts):
    lists, flats, dpb = format_case
    n = len(lists)
    afters = [u[len(u) // 3] if r % 2 else 0 for r, u in enumerate(lists)] if opts else None
    firsts = [(0, 5, -7, I32_MIN)[r % 4] for r in range(n)] if opts else None
    ref = run(eng, dpb, afters=afters, firsts=firsts, plain=True)
    check(ref, rows_decode_ref.want_rows(lists, afters, firsts))
    # no arrays at all; n_mut == 0 with a zero row_mut_base; and the new kernels
    # over layers that are all empty (one posting that no row owns)
    for raw in (None, ([], [], [0] * (n + 1), 0), ([5], [S], [0] * (n + 1), 1)):
        got = run(eng, dpb, afters=afters, firsts=firsts, raw=raw, cap=ref.cap)
        assert (got.rc, got.total, got.offs) == (ref.rc, ref.total, ref.offs)
        assert got.out == ref.out and got.guards_ok


def test_empty_layer_stats_equal_the_plain_call(eng, format_case):
    _, _, dpb = format_case
    n = len(dpb.pbb) - 1
    deltas = []
    for kw in ({"plain": True}, {}, {"raw": ([], [], [0] * (n + 1), 0)}):
        eng.stats_reset()
        assert run(eng, dpb, afters=[3] * n, firsts=[-2] * n, **kw).rc == 0
        st = eng.stats()
        deltas.append((st["launches"], st["bytes_algorithmic"]))
    assert deltas[0] == deltas[1] == deltas[2]


# ---------- 2. rows without blocks ----------

def test_rows_without_blocks(eng):
    a = gv.encode([100 + 3 * i for i in range(20)], 9)
    sets = [(5, S), (7, MUT_OVR), (900, S), (gv.U64_MAX, S)]
    dels = [(5, D), (130, D), (gv.U64_MAX, D)]
    mixed = [(1, S), (2, D), (3, S), (4, D), (1 << 40, 0), ((1 << 40) + 1, D)]
    for flats, muts in (([[]], [sets]), ([[]], [dels]), ([[]], [mixed]),
                        ([a, [], a], [[], mixed, []]),
                        ([a, [], a], [[(101, S)], sets, [(100, D)]]),
                        ([[], [], [], []], [sets, dels, [], mixed])):
        check_model(eng, flats, muts)
    assert check_model(eng, [[]], [dels]) == [[]]
    assert check_model(eng, [[], []], [sets, mixed], [5, 2], [-2, 2]) == \
        [[900, gv.U64_MAX], [3, 1 << 40]]


# ---------- 3. where a mutation can sit ----------

@pytest.mark.parametrize("bs", [1, 2, 9, 256])
def test_every_position_of_one_mutation(eng, bs):
    uids = [1000 + 10 * i for i in range(3 * bs)]
    blocks = gv.encode(uids, bs)
    assert [n for _, n, _ in blocks] == [bs] * 3
    pos = {5, uids[-1] + 7, gv.U64_MAX}
    for b in range(3):
        blk = uids[b * bs:(b + 1) * bs]
        pos |= {blk[0], blk[-1], blk[len(blk) // 2], blk[-1] + 3}
    pos = sorted(pos)
    muts = [[(p, op)] for p in pos for op in (S, D)]
    muts.append([(p, S if i % 2 else D) for i, p in enumerate(pos)])   # all at once
    muts.append([(p, D if i % 2 else S) for i, p in enumerate(pos)])
    want = check_model(eng, [blocks] * len(muts), muts)
    for m, w in zip(muts[:-2], want):
        (p, op), = m
        assert len(w) == len(set(w))                      # a set never duplicates
        if op == S:
            assert w == sorted(set(uids) | {p})
        else:
            assert w == [x for x in uids if x != p]       # absent: nothing changes


# ---------- 4. slice lengths ----------

def slice_muts(base, n):
    """n postings from base on, stride 2: sets and dels interleaved, on present
    uids (multiples of 4 from base) and on absent ones."""
    return [(base + 2 * k, S if k % 3 == 0 else D) for k in range(n)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 256, 257, 1000])
def test_slice_lengths(eng, n):
    base = 1 << 33
    uids = [base + 4 * i for i in range(256)]
    blk = gv.encode(uids, 256)
    high = gv.encode([base + 4096 + i for i in range(9)], 9)
    assert len(blk) == 1 and len(high) == 1
    m = slice_muts(base, n)
    # one block owns the slice; one head owns it, without and with blocks after it;
    # and the middle block of three
    flats = [blk, [], high, gv.encode([5, 6], 2) + blk + gv.encode([1 << 35], 1)]
    want = check_model(eng, flats, [m] * 4)
    assert want[1] == [u for u, op in m if op == S]
    check_model(eng, flats, [m] * 4, [base + 2 * (n // 2)] * 4, [0, -3, 70, -70])


def test_dels_hit_every_uid_of_a_full_block(eng):
    uids = gv.full_block()
    sets = [(uids[i] + 1, S) for i in range(0, 256, 5)]
    m = sorted([(u, D) for u in uids] + sets)
    want = check_model(eng, [gv.encode(uids, 256)], [m])
    assert want == [[u for u, _ in sets]]


# ---------- 5. after ----------

@pytest.mark.parametrize("bs", [1, 9, 256])
def test_after(eng, bs):
    uids = [1000 + 10 * i for i in range(3 * bs)]
    blocks = gv.encode(uids, bs)
    mid = uids[bs + bs // 2]                               # inside the middle block
    m = sorted({(7, S), (uids[0], D), (uids[0] + 1, S), (mid - 10 if bs > 2 else mid - 1, D),
                (mid - 5, S), (mid + 5, S), (uids[-1], D), (uids[-1] + 4, S),
                (gv.U64_MAX, S)})
    assert len({u for u, _ in m}) == len(m)
    afters = [0, 1, 7, mid - 5, uids[0], mid, mid + 5, uids[-1], uids[-1] + 4,
              gv.U64_MAX - 1, gv.U64_MAX]
    want = check_model(eng, [blocks] * len(afters), [m] * len(afters), afters)
    assert want[0] == want[1] and want[-1] == [] and want[-2] == [gv.U64_MAX]
    assert 7 in want[1] and 7 not in want[2]               # strict on a set uid
    assert want[5][0] == mid + 5 and want[6][0] > mid + 5


# ---------- 6. first ----------

def test_first(eng):
    uids = [1000 + 10 * i for i in range(27)]
    blocks = gv.encode(uids, 9)
    m = [(3, S), (4, D), (8, S), (1000, S), (1005, S), (1080, D), (1085, S), (1090, S),
         (1095, S), (1180, D), (1260, S), (1300, S)]
    full = want_row(uids, m)
    L = len(full)
    assert full[:4] == [3, 8, 1000, 1005] and 1085 in full and 1080 not in full
    firsts = list(range(-L - 2, L + 3)) + [I32_MIN, I32_MAX]
    for a in (None, 1005, 1089):
        n = len(firsts)
        check_model(eng, [blocks] * n, [m] * n, None if a is None else [a] * n, firsts)
    # heads only, and a head followed by blocks that own nothing
    check_model(eng, [[]] * 6 + [blocks] * 2, [m] * 6 + [m[:3]] * 2, None,
                [1, -1, 4, -4, I32_MIN, I32_MAX, 2, -28])


# ---------- 7. neighbours ----------

def test_neighbouring_rows_keep_their_slices(eng):
    hi = [5000 + 10 * i for i in range(18)]
    lo = [50 + 10 * i for i in range(18)]
    flats = [gv.encode(hi, 9), gv.encode(lo, 9), [], gv.encode(hi, 2), gv.encode(lo, 256)]
    muts = [[(5005, S), (5170, D), (9000, S)],            # the tail of row 0 ...
            [(3, S), (55, S), (60, D), (8000, S)],        # ... and smaller uids after it
            [(1, S), (7000, S)],
            [(4999, S), (5000, D), (5171, S)],
            [(2, D), (49, S), (220, S), (221, D)]]
    check_model(eng, flats, muts)
    check_model(eng, flats, muts, [5005, 55, 1, 0, 49], [0, -2, 1, 3, -1])


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_scan_chunks_and_workgroups(eng, n):
    """2048 counts per scan chunk and four blocks per workgroup: n rows of one
    posting each and no blocks, then one row of n one-uid blocks with a
    posting at every third block, then the blocks seven to a row."""
    uids = gv.long_list(n)
    blocks = gv.encode(uids, 1)
    assert len(blocks) == n
    heads = [[(u, S if r % 5 else D)] for r, u in enumerate(uids)]
    check_model(eng, [[]] * n, heads, None, [1 if r % 2 else -1 for r in range(n)])
    m = [(u + (r % 2), D if r % 2 == 0 else S) for r, u in enumerate(uids) if r % 3 == 0]
    check_model(eng, [blocks], [m], [uids[n // 3]], [-(n // 2)])
    cuts = list(range(0, n, 7)) + [n]
    flats = [blocks[s:e] for s, e in zip(cuts, cuts[1:])]
    muts = [[(uids[s] - 1, S), (uids[s], D), (uids[e - 1], S), (uids[e - 1] + 1, S)]
            if r % 4 == 0 and e - s > 1 else [] for r, (s, e) in enumerate(zip(cuts, cuts[1:]))]
    check_model(eng, flats, muts, None, [(-2 if r % 2 else 3) if r % 5 == 0 else 0
                                          for r in range(len(flats))])


# ---------- 8. seeded differential ----------

@pytest.mark.parametrize("offset", [0, (1 << 63) - 1500])
def test_seeded_differential(eng, offset):
    rng = random.Random(20261021 + (offset & 0xffff))
    universe = range(1, 4000)
    flats, muts, afters, firsts = [], [], [], []
    for r in range(200):
        n = rng.choice([0, 0, rng.randrange(1, 40), rng.randrange(1, 601)])
        uids = sorted(offset + x for x in rng.sample(universe, n))
        flats.append(gv.encode(uids, rng.choice(gv.BLOCK_SIZES)) if uids else [])
        k = rng.choice([0, rng.randrange(1, 8), rng.randrange(1, 301)])
        muts.append([(offset + x, rng.choice([S, S, D, D, MUT_OVR]))
                     for x in sorted(rng.sample(universe, k))])
        afters.append(rng.choice([0, 0, offset + rng.randrange(1, 4000)]))
        firsts.append(rng.choice([0, 0, 1, -1, rng.randrange(-700, 700)]))
    want = check_model(eng, flats, muts, afters, firsts)
    assert sum(len(w) for w in want) > 2000
    check_model(eng, flats, muts)
    check_model(eng, flats, muts, afters)


# ---------- 9. capacity and count-only ----------

def test_capacity_and_count_only(eng):
    uids = [1000 + 10 * i for i in range(40)]
    flats = [gv.encode(uids, 9), [], gv.encode(gv.full_block(), 256), gv.encode(uids, 2)]
    lists = [gv.decode(f) for f in flats]
    muts = [[(5, S), (1010, D), (1015, S), (2000, S)], [(1, S), (2, S), (3, D)],
            [(gv.full_block()[7], D), (gv.full_block()[9] + 1, S)], []]
    afters = [1000, 0, 0, 1100]
    firsts = [0, 1, -100, 20]
    want = want_rows(lists, muts, afters, firsts)
    total = sum(len(w) for w in want)
    offs = list(np.cumsum([0] + [len(w) for w in want]))
    dpb = arena(eng, flats)
    check(run(eng, dpb, muts, afters, firsts, cap=total), want)
    for cap in (total - 1, 0):
        short = run(eng, dpb, muts, afters, firsts, cap=cap)
        assert (short.rc, short.total, short.offs) == (UA_ERR_INVALID, total, offs)
        assert short.guards_ok
    count = run(eng, dpb, muts, afters, firsts, count_only=True)
    assert (count.rc, count.total, count.offs) == (0, total, offs)
    assert count.guards_ok and count.out[:8] == [SENT] * 8
    # List.Length of every key, and the host mirrors (a None pack = no blocks)
    packs = [(*gv.flatten(f), len(u)) if f else None for f, u in zip(flats, lists)]
    assert algo.row_lengths_mut(eng, packs, muts, after=afters).tolist() == \
        [len(w) for w in want_rows(lists, muts, afters)]
    got = algo.uid_matrix_mut(eng, packs, muts, after=afters, first=firsts)
    assert [g.tolist() for g in got] == want
    none = algo.uid_matrix_mut(eng, packs, [[]] * 4, after=afters, first=firsts)
    assert [g.tolist() for g in none] == rows_decode_ref.want_rows(lists, afters, firsts)
    # the tensor-level wrapper sizes its own buffers
    mu, mo, rmb = flat(muts)
    vals, ro = eng.decode_rows_mut(dpb, mu, mo, rmb, afters=afters, firsts=firsts)
    assert u64_list(vals) == [x for w in want for x in w] and u64_list(ro) == offs
    vals, ro = eng.decode_rows_mut(dpb, mu, mo, rmb, afters=afters, count_only=True)
    assert vals.numel() == 0 and np.diff(u64_list(ro)).tolist() == \
        [len(w) for w in want_rows(lists, muts, afters)]
    with pytest.raises(ValueError):
        eng.decode_rows_mut(dpb, mu, mo, rmb,
                            out_vals=torch.empty(8, dtype=torch.int64, device=DEV))


# ---------- 10. one traversal step on the device ----------

def test_decode_mut_union_filter_step(eng):
    long = gv.long_list(3000)
    lists = [long[(41 * r) % 2500:(41 * r) % 2500 + 20 + 7 * r] for r in range(64)]
    lists[9] = []
    muts = [[] for _ in lists]
    for r in range(0, 64, 3):                              # every third key is live
        u = lists[r] or [long[100]]
        muts[r] = sorted({(u[0], D), (u[len(u) // 2] + 1, S), (u[-1] + 2, S)})
    dpb = arena(eng, [gv.encode(u, 256) for u in lists])
    mu, mo, rmb = flat(muts)
    vals, ro = eng.decode_rows_mut(dpb, mu, mo, rmb)
    rows = want_rows(lists, muts)
    assert u64_list(ro) == list(np.cumsum([0] + [len(w) for w in rows]))
    dest = eng.union_rows(vals)
    union = sorted({x for w in rows for x in w})
    assert u64_list(dest) == union
    shared = dest[::3].contiguous()
    out, oro = eng.filter_rows(vals, ro, shared)
    keep = set(union[::3])
    want = [[x for x in w if x in keep] for w in rows]
    offs = u64_list(oro)
    flat_out = u64_list(out)
    assert [flat_out[offs[r]:offs[r + 1]] for r in range(64)] == want


# ---------- 11. stats ----------

@pytest.mark.parametrize("with_blocks", [False, True])
@pytest.mark.parametrize("with_first", [False, True])
@pytest.mark.parametrize("count_only", [False, True])
def test_stats_follow_the_documented_formula(eng, with_blocks, with_first, count_only):
    """Launches: the flags, their scan (2) and the heads, the item scan (2)
    and the rows, with blocks the validation and the two block counts, with first a
    second scan (2) and the offsets; then the head write and, with blocks, the
    two block writes unless count-only.  Bytes: the whole blob + 20 per block + 16
    per row boundary + 9 per posting + 8 per emitted uid."""
    uids = [1000 + 10 * i for i in range(40)]
    blocks = gv.encode(uids, 9) if with_blocks else []
    flats = [blocks, [], blocks]
    muts = [[(5, S), (1010, D), (1015, S)], [(1, S), (3, D)], []]
    afters = [1005, 0, 0]
    firsts = [0, 0, 12] if with_first else None
    dpb = arena(eng, flats)
    want = want_rows([gv.decode(f) for f in flats], muts, afters, firsts)
    kept = sum(len(w) for w in want)
    blob = 2 * sum(len(d) for _, _, d in blocks)
    eng.stats_reset()
    res = run(eng, dpb, muts, afters, firsts, count_only=count_only)
    st = eng.stats()
    assert (res.rc, res.total) == (0, kept)
    assert st["launches"] == 7 + (3 if with_blocks else 0) + (3 if with_first else 0) + \
        (0 if count_only else (3 if with_blocks else 1))
    assert st["bytes_algorithmic"] == blob + 20 * 2 * len(blocks) + 16 * 4 + 9 * 5 + 8 * kept
    assert st["kernel_ms"] > 0


# ---------- 12. malformed but in-bounds metadata ----------

@pytest.mark.parametrize("kind", ["not_monotone", "past_n_mut", "unsorted_slice",
                                  "zero_uid", "first_base_not_zero"])
def test_malformed_layer_stays_in_bounds(eng, kind):
    """As tests/test_engine_robustness_gpu.py: the rows are unspecified, but
    the call succeeds, the guards stand, nothing is written past the total and
    out_row_offs[n_rows] is the total.  Every index is clamped in
    d_row_muts / d_rowmut_locate before it is used."""
    uids = [1000 + 10 * i for i in range(40)]
    flats = [gv.encode(uids, 9), [], gv.encode(uids, 256), gv.encode(uids, 1)]
    mu = [5, 1010, 1015, 2000, 1, 2, 3, 1100, 1200, 1300]
    mo = [S, D, S, S, S, S, D, D, S, S]
    rmb = [0, 4, 7, 7, 10]
    if kind == "not_monotone":
        rmb = [0, 7, 4, 10, 2]
    elif kind == "past_n_mut":
        rmb = [0, 4, 1 << 40, gv.U64_MAX, 11]
    elif kind == "unsorted_slice":
        mu = [2000, 5, 1015, 1010, 3, 3, 1, 1300, 1100, 1300]
    elif kind == "zero_uid":
        mu[0], mu[4] = 0, 0
    else:
        rmb = [3, 4, 7, 7, 10]
    dpb = arena(eng, flats)
    for kw in ({}, {"afters": [1010, 0, 1, 1100], "firsts": [2, -1, 0, -5]}):
        res = run(eng, dpb, raw=(mu, mo, rmb, len(mu)), cap=200, **kw)  # <= 120 + 4 * 10
        assert res.rc == 0 and res.guards_ok
        assert res.offs[-1] == res.total <= res.cap
        assert res.out[res.total:res.cap] == [SENT] * (res.cap - res.total)
    # the engine is unharmed
    check_model(eng, flats, [[(5, S)], [], [(1010, D)], []])
