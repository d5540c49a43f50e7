"""ua_rows_decode_dev on the GPU: a fan-out of UidPacks in, a CSR UID matrix
out, against the format itself.

Packs are uploaded from the bytes of tests/gv_spec.py, never from an engine
encoder.  Expected rows come from tests/rows_decode_ref.py (List.Uids with
Intersect == nil: x > after, 0 keeps all; then first), which
tests/test_rows_decode_ref.py holds to the oracle.  Output buffers are
pre-filled with a sentinel and carry 64 guard words past their capacity.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gv_spec as gv
from dgraph_amd import _lib, algo
from rows_decode_ref import want_row, want_rows

pytestmark = pytest.mark.gpu

UA_ERR_INVALID = 3
GUARD = 64
SENT = 0xA5A5A5A5A5A5A5A5
SENT_I64 = SENT - (1 << 64)
DEV = "cuda:0"
I32_MIN, I32_MAX = -2**31, 2**31 - 1


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


def u64_list(t):
    return t.cpu().numpy().view(np.uint64).tolist()


class Result:
    pass


def run(eng, dpb, afters=None, firsts=None, cap=None, count_only=False):
    """One raw ua_rows_decode_dev call into sentinel-filled buffers."""
    n_rows = len(dpb.pbb) - 1
    nb = int(dpb.pbb[n_rows])
    if cap is None:
        cap = int(sum(dpb.pack_totals))
    rbb = dev_u64([int(x) for x in dpb.pbb])
    t_after = dev_u64(afters) if afters is not None else None
    t_first = dev_i32(firsts) if firsts is not None else None
    out = torch.full((cap + GUARD,), SENT_I64, dtype=torch.int64, device=DEV)
    oro = torch.full((n_rows + 1 + GUARD,), SENT_I64, dtype=torch.int64, device=DEV)
    d = _lib.UaDRowPacks()
    d.bases, d.num_uids = dpb.bases.data_ptr(), dpb.num_uids.data_ptr()
    d.delta_offs, d.deltas = dpb.delta_offs.data_ptr(), dpb.deltas.data_ptr()
    d.n_blocks, d.n_rows = nb, n_rows
    d.row_block_base = rbb.data_ptr() if n_rows else None
    d.after = t_after.data_ptr() if t_after is not None else None
    d.first = t_first.data_ptr() if t_first is not None else None
    d.out_vals = None if count_only else out.data_ptr()
    d.cap_vals = 0 if count_only else cap
    d.out_row_offs = oro.data_ptr()
    total = C.c_uint64(77)
    res = Result()
    res.rc = _lib.lib().ua_rows_decode_dev(eng._ctx, C.byref(d), C.byref(total))
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


# ---------- 1. the format ----------

def test_every_input_at_every_block_size(eng):
    names = sorted(gv.inputs())
    lists, flats = [], []
    for name in names:
        for bs in gv.BLOCK_SIZES:
            lists.append(gv.inputs()[name])
            flats.append(gv.encode(lists[-1], bs))
    assert len(flats) == 66
    assert any(len(d) == gv.MAX_BLOCK_BYTES for f in flats for _, _, d in f)
    tags = {t for f in flats for blk in gv.control_bytes(f) for t in blk}
    assert tags == set(range(256))
    assert any(0 in u and gv.U64_MAX in u for u in lists)
    for f, u in zip(flats, lists):
        assert gv.decode(f) == u
    check(run(eng, arena(eng, flats)), lists)


# ---------- 2. and 8. the after sweep, and the existing decode path ----------

@pytest.fixture(scope="module")
def seek_case(eng):
    uids = gv.seek_pack()
    blocks = gv.encode(uids, 9)
    seeks = gv.seek_list(blocks)
    assert 30 <= len(blocks) <= 40 and 150 <= len(seeks) <= 300
    assert {0, 1, gv.U64_MAX - 1, gv.U64_MAX} <= set(seeks)
    return uids, blocks, seeks


def test_after_sweep(eng, seek_case):
    uids, blocks, seeks = seek_case
    dpb = arena(eng, [blocks] * len(seeks))
    want = want_rows([uids] * len(seeks), seeks)
    assert want[0] == uids and want[-1] == [] and want[-2] == [gv.U64_MAX]
    check(run(eng, dpb, afters=seeks), want)


def test_agrees_with_decode_pack(eng, seek_case):
    """Both paths are held to want_rows, so a disagreement names the one at
    fault.  Decode's seek keeps x >= seek: after a is seek a + 1, after 0 is
    seek 0, and after 2^64 - 1 has no seek (the row is empty)."""
    uids, blocks, seeks = seek_case
    dp = eng.upload_pack(*gv.flatten(blocks), 9)
    res = run(eng, arena(eng, [blocks] * len(seeks)), afters=seeks)
    assert res.rc == 0
    for r, a in enumerate(seeks):
        want = want_row(uids, a)
        if a < gv.U64_MAX:
            old = u64_list(eng.decode_pack(dp, seek=a + 1 if a else 0))
            assert old == want, f"decode_pack after={a:#x}"
        assert res.rows[r] == want, f"decode_rows after={a:#x}"


# ---------- 3. the first sweep ----------

def test_first_sweep(eng, seek_case):
    uids, blocks, _ = seek_case
    n = len(uids)
    firsts = [1, -1, 8, 9, 10, -8, -9, -10, n - 1, n, n + 1, -(n - 1), -n, -(n + 1),
              I32_MAX, I32_MIN]
    mid = gv.decode([blocks[6]])[4]          # inside a block
    afters = [0, mid, uids[-1]]
    assert blocks[6][1] == 9 and mid not in (blocks[6][0], uids[-1])
    fs = [f for f in firsts for _ in afters]
    as_ = [a for _ in firsts for a in afters]
    dpb = arena(eng, [blocks] * len(fs))
    want = want_rows([uids] * len(fs), as_, fs)
    assert [] in want and uids in want and any(len(w) == 9 for w in want)
    check(run(eng, dpb, afters=as_, firsts=fs), want)
    # after = NULL: the same windows over the whole rows
    dpb = arena(eng, [blocks] * len(firsts))
    check(run(eng, dpb, firsts=firsts), want_rows([uids] * len(firsts), None, firsts))
    # first = NULL: the second scan is skipped
    dpb = arena(eng, [blocks] * len(afters))
    check(run(eng, dpb, afters=afters), want_rows([uids] * len(afters), afters))


# ---------- 4. empty rows ----------

def test_empty_rows(eng):
    a = gv.encode(gv.inputs()["ladder_b_low"][:100], 9)
    b = gv.encode(gv.inputs()["edge_values"], 4)
    flats = [[], a, [], b, [], [], [], a, b, []]
    lists = [gv.decode(f) for f in flats]
    check(run(eng, arena(eng, flats)), lists)
    afters = [5, lists[1][50], 0, gv.U64_MAX, 0, 1, 2, 0, lists[8][3], 9]
    firsts = [1, -3, 2, 1, 0, -1, I32_MIN, 7, -2, I32_MAX]
    check(run(eng, arena(eng, flats), afters=afters, firsts=firsts),
          want_rows(lists, afters, firsts))


@pytest.mark.parametrize("n_rows", [0, 5])
@pytest.mark.parametrize("opts", [False, True])
def test_no_blocks_at_all(eng, n_rows, opts):
    dpb = arena(eng, [[]] * n_rows)
    assert int(dpb.pbb[-1]) == 0
    res = run(eng, dpb, afters=[3] * n_rows if opts else None,
              firsts=[-2] * n_rows if opts else None, cap=8)
    check(res, [[]] * n_rows)
    assert res.out[:8] == [SENT] * 8
    res = run(eng, dpb, count_only=True)
    assert (res.rc, res.total, res.offs) == (0, 0, [0] * (n_rows + 1))


# ---------- 5. geometry ----------

@pytest.mark.parametrize("nb", [1, 2, 3, 5, 2047, 2048, 2049, 4097])
def test_one_uid_blocks(eng, nb):
    """Four blocks per workgroup and 2048 counts per scan chunk: rows of
    seven one-uid blocks, every third row with an after inside it and every
    fifth with a first; then the same blocks as one row."""
    uids = gv.long_list(nb)
    blocks = gv.encode(uids, 1)
    assert len(blocks) == nb
    cuts = list(range(0, nb, 7)) + [nb]
    flats = [blocks[s:e] for s, e in zip(cuts, cuts[1:])]
    lists = [uids[s:e] for s, e in zip(cuts, cuts[1:])]
    afters = [u[len(u) // 2] if r % 3 == 0 else 0 for r, u in enumerate(lists)]
    firsts = [(-2 if r % 2 else 3) if r % 5 == 0 else 0 for r in range(len(lists))]
    dpb = arena(eng, flats)
    check(run(eng, dpb), lists)
    check(run(eng, dpb, afters=afters, firsts=firsts), want_rows(lists, afters, firsts))
    one = arena(eng, [blocks])
    check(run(eng, one), [uids])
    a = uids[nb // 3]
    check(run(eng, one, afters=[a], firsts=[-5]), [want_row(uids, a, -5)])
    check(run(eng, one, afters=[a], firsts=[4]), [want_row(uids, a, 4)])


@pytest.mark.parametrize("n_rows", [2047, 2048, 2049])
def test_one_block_per_row_first_1(eng, n_rows):
    """The scan over the rows' window lengths, in chunks of 2048."""
    uids = gv.long_list(3 * n_rows)
    lists = [uids[3 * r:3 * r + 3] for r in range(n_rows)]
    flats = [gv.encode(u, 256) for u in lists]
    lists = [gv.decode(f[:1]) for f in flats]   # a 32-MSB break may split a row
    flats = [f[:1] for f in flats]
    firsts = [1] * n_rows
    firsts[-1] = -1
    check(run(eng, arena(eng, flats), firsts=firsts), want_rows(lists, None, firsts))


# ---------- 6. capacity ----------

def test_capacity_and_count_only(eng, seek_case):
    uids, blocks, seeks = seek_case
    flats = [blocks, [], gv.encode(gv.full_block(), 256), blocks]
    lists = [gv.decode(f) for f in flats]
    afters = [seeks[40], 0, 0, 0]
    firsts = [0, 0, -100, 20]
    want = want_rows(lists, afters, firsts)
    total = sum(len(w) for w in want)
    offs = list(np.cumsum([0] + [len(w) for w in want]))
    dpb = arena(eng, flats)
    exact = run(eng, dpb, afters=afters, firsts=firsts, cap=total)
    check(exact, want)
    short = run(eng, dpb, afters=afters, firsts=firsts, cap=total - 1)
    assert (short.rc, short.total, short.offs) == (UA_ERR_INVALID, total, offs)
    assert short.guards_ok
    count = run(eng, dpb, afters=afters, firsts=firsts, count_only=True)
    assert (count.rc, count.total, count.offs) == (0, total, offs)
    assert count.guards_ok and count.out[:8] == [SENT] * 8
    # List.Length of every key: the host mirror's count-only form
    packs = [(*gv.flatten(f), len(u)) for f, u in zip(flats, lists)]
    assert algo.row_lengths(eng, packs, after=afters).tolist() == \
        [len(w) for w in want_rows(lists, afters)]
    got = algo.uid_matrix(eng, packs, after=afters, first=firsts)
    assert [g.tolist() for g in got] == want
    # the tensor-level wrapper sizes its own buffers
    vals, ro = eng.decode_rows(dpb, afters=afters, firsts=firsts)
    assert u64_list(vals) == [x for w in want for x in w] and u64_list(ro) == offs
    with pytest.raises(ValueError):
        eng.decode_rows(dpb, out_vals=torch.empty(8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        eng.decode_rows(dpb, out_row_offs=torch.empty(4, dtype=torch.int64, device=DEV))


# ---------- 7. the limits: 256 uids, 1092 delta bytes ----------

def malformed(kind):
    """Three blocks whose middle one breaks exactly one documented limit.
    Every byte the offsets span is real, zero-filled memory."""
    if kind == "num_uids_257":
        blocks = gv.encode([1 << 36, (1 << 36) + 1, 2 << 36, (2 << 36) + 5,
                            3 << 36, (3 << 36) + 7], 256)
        bases, nums, offs, blob = gv.flatten(blocks)
        assert nums.tolist() == [2, 2, 2]
        nums[1] = 257
        return bases, nums, offs, blob
    return (gv.u64([1 << 36, 2 << 36, 3 << 36]), np.array([1, 2, 1], dtype=np.uint32),
            gv.u64([0, 5, 5 + 1093, 5 + 1093 + 5]), np.zeros(5 + 1093 + 5, dtype=np.uint8))


@pytest.mark.parametrize("kind", ["num_uids_257", "deltas_1093"])
def test_limit_violation_rejected(eng, kind):
    bases, nums, offs, blob = malformed(kind)
    dpb = eng.upload_pack(bases, nums, offs, blob, 256)
    dpb.pbb = np.array([0, 2, 3], dtype=np.uint64)
    dpb.pack_totals = [int(nums[:2].sum()), int(nums[2])]
    for kw in ({}, {"afters": [1 << 36, 0], "firsts": [1, -1]}, {"count_only": True}):
        res = run(eng, dpb, **kw)
        assert (res.rc, res.total) == (UA_ERR_INVALID, 0), kw
        assert res.guards_ok
    # the engine is unharmed
    uids = gv.full_block()
    check(run(eng, arena(eng, [gv.encode(uids, 256)])), [uids])


def test_full_block_accepted(eng):
    uids = gv.full_block()
    blocks = gv.encode(uids, 256)
    assert [(n, len(d)) for _, n, d in blocks] == [(256, 1085)]
    afters = [0, uids[0], uids[100], uids[254], uids[255]]
    firsts = [0, -256, 100, -1, 1]
    check(run(eng, arena(eng, [blocks] * 5), afters=afters, firsts=firsts),
          want_rows([uids] * 5, afters, firsts))


# ---------- 9. one traversal step on the device ----------

def test_decode_union_filter_step(eng):
    """decode_rows -> union_rows -> filter_rows: UidMatrix, DestUIDs and
    updateUidMatrix with nothing but the three totals crossing to the host."""
    long = gv.long_list(3000)
    lists = [long[(41 * r) % 2500:(41 * r) % 2500 + 20 + 7 * r] for r in range(64)]
    lists[9] = []
    dpb = arena(eng, [gv.encode(u, 256) for u in lists])
    vals, ro = eng.decode_rows(dpb)
    assert u64_list(ro) == list(np.cumsum([0] + [len(u) for u in lists]))
    dest = eng.union_rows(vals)
    union = sorted({x for u in lists for x in u})
    assert u64_list(dest) == union
    shared = dest[::3].contiguous()
    out, oro = eng.filter_rows(vals, ro, shared)
    keep = set(union[::3])
    want = [[x for x in u if x in keep] for u in lists]
    offs = u64_list(oro)
    flat = u64_list(out)
    assert [flat[offs[r]:offs[r + 1]] for r in range(64)] == want


# ---------- 10. stats ----------

@pytest.mark.parametrize("with_first", [False, True])
@pytest.mark.parametrize("count_only", [False, True])
def test_stats_follow_the_documented_formula(eng, seek_case, with_first, count_only):
    """Launches: validation, count, scan (2), rows, then with first a second
    scan (2) and the offsets, then the write unless count-only.  Bytes: the
    whole blob + 20 per block + 8 per row boundary + 8 per kept uid."""
    uids, blocks, seeks = seek_case
    flats = [blocks, [], blocks]
    afters = [seeks[30], 0, 0]
    firsts = [0, 0, 12] if with_first else None
    dpb = arena(eng, flats)
    want = want_rows([uids, [], uids], afters, firsts)
    kept = sum(len(w) for w in want)
    blob = 2 * sum(len(d) for _, _, d in blocks)
    eng.stats_reset()
    res = run(eng, dpb, afters=afters, firsts=firsts, count_only=count_only)
    st = eng.stats()
    assert (res.rc, res.total) == (0, kept)
    assert st["launches"] == 5 + (3 if with_first else 0) + (0 if count_only else 1)
    assert st["bytes_algorithmic"] == blob + 20 * 2 * len(blocks) + 8 * 4 + 8 * kept
    assert st["kernel_ms"] > 0
