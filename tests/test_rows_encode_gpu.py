"""ua_rows_encode_dev on the GPU: a CSR UID matrix in, a fan-out of UidPacks
out, byte for byte against tests/rows_encode_ref.want_arena (the block format
of tests/gv_spec.py per row), which tests/test_rows_encode_ref.py holds to the
oracle's encoder and to literals.

Output buffers are pre-filled with a sentinel and carry guard words past
their capacity.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gv_spec as gv
import rows_isect_ref
import rows_mut_ref
from dgraph_amd import _lib, algo
from rows_encode_ref import TILE, cases, csr, one_run, want_arena

pytestmark = pytest.mark.gpu

UA_ERR_INVALID = 3
GUARD = 64
SENT = 0xA5A5A5A5A5A5A5A5
SENT_I64 = SENT - (1 << 64)
DEV = "cuda:0"
CASES = cases()


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def dev_u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.int64, device=DEV)
    return torch.from_numpy(a.view(np.int64)).to(DEV)


class Result:
    pass


def run(eng, vals, offs, bs, cap_blocks, cap_deltas, count_only=False, total=None, skew=0):
    """One raw call into sentinel-filled buffers with guards past every
    capacity; skew moves the blob off its 16-byte alignment."""
    n_rows = offs.size - 1
    total = vals.size if total is None else total
    t_vals, t_offs = dev_u64(vals), dev_u64(offs)
    full = lambda n, dt: torch.full((n + GUARD,), SENT_I64 if dt == torch.int64 else
                                    (-1 if dt == torch.int32 else -91), dtype=dt, device=DEV)
    bases = full(cap_blocks, torch.int64)
    nums = full(cap_blocks, torch.int32)
    doffs = full(cap_blocks + 1, torch.int64)
    blob_all = full(cap_deltas + skew, torch.int8)
    blob = blob_all[skew:]
    rbb = full(n_rows + 1, torch.int64)
    d = _lib.UaDRowEnc()
    d.vals = t_vals.data_ptr() if total else None
    d.row_offs = t_offs.data_ptr() if n_rows else None
    d.n_rows, d.total, d.block_size = n_rows, total, bs
    if not count_only:
        d.bases, d.num_uids = bases.data_ptr(), nums.data_ptr()
        d.delta_offs, d.deltas = doffs.data_ptr(), blob.data_ptr()
        d.cap_blocks, d.cap_deltas = cap_blocks, cap_deltas
    d.row_block_base = rbb.data_ptr()
    nb, db = C.c_uint64(77), C.c_uint64(77)
    res = Result()
    res.rc = _lib.lib().ua_rows_encode_dev(eng._ctx, C.byref(d), C.byref(nb), C.byref(db))
    res.nb, res.db = nb.value, db.value
    res.bases = bases.cpu().numpy().view(np.uint64)
    res.nums = nums.cpu().numpy().view(np.uint32)
    res.doffs = doffs.cpu().numpy().view(np.uint64)
    res.blob = blob.cpu().numpy().view(np.uint8)
    res.rbb = rbb.cpu().numpy().view(np.uint64)
    res.guards_ok = bool((blob_all[:skew].cpu().numpy().view(np.uint8) == 0xa5).all() and
                         (res.bases[cap_blocks:] == SENT).all() and
                         (res.nums[cap_blocks:] == 0xffffffff).all() and
                         (res.doffs[cap_blocks + 1:] == SENT).all() and
                         (res.blob[cap_deltas:] == 0xa5).all() and
                         (res.rbb[n_rows + 1:] == SENT).all())
    res.untouched = bool((res.bases[:cap_blocks] == SENT).all() and
                         (res.blob[:cap_deltas] == 0xa5).all())
    return res


def check(res, want, cap_blocks, cap_deltas):
    """A successful full call: all five arrays, both sizes, the guards, and
    nothing written between the sizes and the capacities."""
    bases, nums, offs, blob, rbb = want
    nb, db = bases.size, blob.size
    assert (res.rc, res.nb, res.db) == (0, nb, db)
    assert np.array_equal(res.rbb[:rbb.size], rbb)
    assert np.array_equal(res.bases[:nb], bases)
    assert np.array_equal(res.nums[:nb], nums)
    assert np.array_equal(res.doffs[:nb + 1], offs)
    assert np.array_equal(res.blob[:db], blob)
    assert res.guards_ok
    assert (res.bases[nb:cap_blocks] == SENT).all()
    assert (res.nums[nb:cap_blocks] == 0xffffffff).all()
    assert (res.doffs[nb + 1:cap_blocks + 1] == SENT).all()
    assert (res.blob[db:cap_deltas] == 0xa5).all()


def check_rows(eng, rows, bs):
    """The exact-capacity call, a roomy call and the count-only form."""
    want = want_arena(rows, bs)
    vals, offs = csr(rows)
    nb, db = want[0].size, want[3].size
    check(run(eng, vals, offs, bs, nb, db), want, nb, db)
    check(run(eng, vals, offs, bs, nb + 7, db + 37), want, nb + 7, db + 37)
    check(run(eng, vals, offs, bs, nb, db, skew=5), want, nb, db)
    cnt = run(eng, vals, offs, bs, 0, 0, count_only=True)
    assert (cnt.rc, cnt.nb, cnt.db) == (0, nb, db)
    assert np.array_equal(cnt.rbb[:offs.size], want[4])
    assert cnt.guards_ok
    return want


# ---------- 1. bytes ----------

@pytest.mark.parametrize("name", sorted(CASES))
def test_arena_bytes(eng, name):
    rows, sizes = CASES[name]
    for bs in sizes:
        check_rows(eng, rows, bs)


def test_fullest_tile_reaches_the_lds_bound():
    rows, _ = CASES["fullest_tile"]
    _, _, offs, _, _ = want_arena(rows, 256)
    # flat elements [TILE, 2 * TILE) are the two-uid row's second uid and 2047 rows
    # of one uid: blocks TILE - 1 .. 2 * TILE - 2
    assert int(offs[2 * TILE - 1]) - int(offs[TILE - 1]) == 5 * TILE + 3


# ---------- 2. capacities ----------

def test_short_capacities(eng):
    rows = [gv.long_list(3000, (TILE,)), [], gv.tag_ladder("high", "b")[:700]]
    want = want_arena(rows, 9)
    vals, offs = csr(rows)
    nb, db = want[0].size, want[3].size
    for cb, cd in ((nb - 1, db), (nb, db - 1), (nb - 1, db - 1), (1, 1), (0, db), (nb, 0)):
        res = run(eng, vals, offs, 9, cb, cd)
        assert (res.rc, res.nb, res.db) == (UA_ERR_INVALID, nb, db), (cb, cd)
        assert np.array_equal(res.rbb[:offs.size], want[4])
        assert res.guards_ok, (cb, cd)
    # the reported sizes make the retry exact
    check(run(eng, vals, offs, 9, nb, db), want, nb, db)


# ---------- 3. the consumers take the arena as it is ----------

def arena_of(eng, rows, bs):
    vals, offs = csr(rows)
    return eng.encode_rows(dev_u64(vals)[:vals.size], dev_u64(offs), bs)


def test_round_trip_and_intersect(eng):
    rows = [gv.long_list(5000, (TILE - 1, TILE + 1)), [], gv.edge_values(),
            gv.tag_ladder("low"), [7], []]
    vals, offs = csr(rows)
    for bs in (0, 9, 256):
        dp = arena_of(eng, rows, bs)
        want = want_arena(rows, bs)
        assert np.array_equal(dp.pbb, want[4])
        assert dp.pack_totals == [len(r) for r in rows]
        got_vals, got_offs = eng.decode_rows(dp)
        assert np.array_equal(got_vals.cpu().numpy().view(np.uint64), vals)
        assert np.array_equal(got_offs.cpu().numpy().view(np.uint64), offs)
        shared = sorted(set(rows[0][::3] + rows[2][::2] + [7, 8]))
        iv, io = eng.intersect_rows(dp, dev_u64(gv.u64(shared)))
        w_vals, w_offs = csr(rows_isect_ref.want_rows(rows, shared))
        assert np.array_equal(iv.cpu().numpy().view(np.uint64), w_vals)
        assert np.array_equal(io.cpu().numpy().view(np.uint64), w_offs)
        # and with an empty mutation layer through decode_rows_mut
        mv, mo = eng.decode_rows_mut(dp, [], [], [0] * (len(rows) + 1))
        assert np.array_equal(mv.cpu().numpy().view(np.uint64), vals)
        assert np.array_equal(mo.cpu().numpy().view(np.uint64), offs)


def test_engine_encode_rows_forms(eng):
    rows = [one_run(2100), [], [5, 6]]
    vals, offs = csr(rows)
    want = want_arena(rows, 256)
    t_vals, t_offs = dev_u64(vals), dev_u64(offs)
    nb, db, rbb = eng.encode_rows(t_vals, t_offs, 256, count_only=True)
    assert (nb, db) == (want[0].size, want[3].size)
    assert np.array_equal(rbb.cpu().numpy().view(np.uint64), want[4])
    bufs = (torch.empty(nb + 3, dtype=torch.int64, device=DEV),
            torch.empty(nb + 3, dtype=torch.int32, device=DEV),
            torch.empty(nb + 4, dtype=torch.int64, device=DEV),
            torch.empty(db + 5, dtype=torch.int8, device=DEV))
    eng.stats_reset()
    dp = eng.encode_rows(t_vals, t_offs, 256, out=bufs)
    assert eng.stats()["launches"] == 8          # caller-supplied buffers: one call
    assert dp.bases.data_ptr() == bufs[0].data_ptr()
    assert np.array_equal(dp.bases.cpu().numpy().view(np.uint64), want[0])
    assert np.array_equal(dp.num_uids.cpu().numpy().view(np.uint32), want[1])
    assert np.array_equal(dp.delta_offs.cpu().numpy().view(np.uint64), want[2])
    assert np.array_equal(dp.deltas.cpu().numpy().view(np.uint8)[:db], want[3])
    short = (bufs[0][:nb - 1], bufs[1], bufs[2], bufs[3])
    with pytest.raises(ValueError, match=f"required {nb} / {db}"):
        eng.encode_rows(t_vals, t_offs, 256, out=short)
    # an all-empty matrix
    dp0 = eng.encode_rows(torch.empty(0, dtype=torch.int64, device=DEV),
                          dev_u64(np.zeros(3, np.uint64)), 256)
    assert dp0.pbb.tolist() == [0, 0, 0] and dp0.pack_totals == [0, 0]
    v0, o0 = eng.decode_rows(dp0)
    assert v0.numel() == 0 and o0.cpu().tolist() == [0, 0, 0]


# ---------- 4. host forms ----------

def test_host_forms_equal_the_device_form(eng):
    rows = [gv.long_list(2500, (TILE,)), [], gv.edge_values(), [3]]
    for bs in (0, 9, 256):
        want = want_arena(rows, bs)
        got = algo.encode_rows(eng, rows, bs)
        assert len(got) == len(rows)
        for r, (bases, nums, doffs, blob, total) in enumerate(got):
            b0, b1 = int(want[4][r]), int(want[4][r + 1])
            y0, y1 = int(want[2][b0]), int(want[2][b1])
            assert np.array_equal(bases, want[0][b0:b1])
            assert np.array_equal(nums, want[1][b0:b1])
            assert np.array_equal(doffs, want[2][b0:b1 + 1] - np.uint64(y0))
            assert np.array_equal(blob, want[3][y0:y1])
            assert total == len(rows[r])
            # the tuple is encode_flat's
            flat = algo.encode_flat(gv.u64(rows[r]), bs)
            for x, y in zip((bases, nums, doffs, blob), flat[:4]):
                assert np.array_equal(x, y)
            assert total == flat[4]
    assert algo.encode_rows(eng, [], 256) == []
    # a short capacity through ua_rows_encode: sizes and row_block_base still arrive
    vals, offs = csr(rows)
    want = want_arena(rows, 256)
    nb, db = want[0].size, want[3].size
    L = _lib.lib()
    u64p, u32p, u8p = (C.POINTER(t) for t in (C.c_uint64, C.c_uint32, C.c_uint8))
    bases = np.full(nb, SENT, dtype=np.uint64)
    nums = np.zeros(nb, dtype=np.uint32)
    doffs = np.zeros(nb + 1, dtype=np.uint64)
    blob = np.full(db, 0xa5, dtype=np.uint8)
    rbb = np.zeros(len(rows) + 1, dtype=np.uint64)
    n, y = C.c_uint64(77), C.c_uint64(77)
    rc = L.ua_rows_encode(eng._ctx, vals.ctypes.data_as(u64p), offs.ctypes.data_as(u64p),
                          len(rows), 256, bases.ctypes.data_as(u64p),
                          nums.ctypes.data_as(u32p), doffs.ctypes.data_as(u64p), nb - 1,
                          blob.ctypes.data_as(u8p), db, rbb.ctypes.data_as(u64p),
                          C.byref(n), C.byref(y))
    assert (rc, n.value, y.value) == (UA_ERR_INVALID, nb, db)
    assert np.array_equal(rbb, want[4])
    assert bases[nb - 1] == SENT


def test_three_rows_equal_encode_dev_per_row(eng):
    rows = [gv.long_list(2300, (TILE,)), gv.edge_values(), gv.full_block()]
    for bs in (9, 256):
        dp = arena_of(eng, rows, bs)
        bases = dp.bases.cpu().numpy().view(np.uint64)
        nums = dp.num_uids.cpu().numpy().view(np.uint32)
        doffs = dp.delta_offs.cpu().numpy().view(np.uint64)
        blob = dp.deltas.cpu().numpy().view(np.uint8)
        for r, row in enumerate(rows):
            one = eng.encode_dev(dev_u64(gv.u64(row)), bs)
            b0, b1 = int(dp.pbb[r]), int(dp.pbb[r + 1])
            y0, y1 = int(doffs[b0]), int(doffs[b1])
            assert np.array_equal(one.bases.cpu().numpy().view(np.uint64), bases[b0:b1])
            assert np.array_equal(one.num_uids.cpu().numpy().view(np.uint32), nums[b0:b1])
            assert np.array_equal(one.delta_offs.cpu().numpy().view(np.uint64),
                                  doffs[b0:b1 + 1] - np.uint64(y0))
            assert np.array_equal(one.deltas.cpu().numpy().view(np.uint8)[:y1 - y0],
                                  blob[y0:y1])


# ---------- 5. rollup ----------

S, D = rows_mut_ref.MUT_SET, rows_mut_ref.MUT_DEL


def rollup_fixtures():
    a = [100 + 3 * i for i in range(20)]
    sets = [(5, S), (7, rows_mut_ref.MUT_OVR), (900, S), (gv.U64_MAX, S)]
    dels = [(5, D), (130, D), (gv.U64_MAX, D)]
    mixed = [(1, S), (2, D), (3, S), (4, D), (1 << 40, 0), ((1 << 40) + 1, D)]
    full = gv.full_block()
    every = sorted([(u, D) for u in full] + [(full[i] + 1, S) for i in range(0, 256, 5)])
    big = gv.long_list(2300, (TILE,))
    churn = [(big[i] + (i % 2), S if i % 3 else D) for i in range(0, 2300, 7)]
    yield [a, [], a], [[], mixed, []]
    yield [a, [], a], [[(101, S)], sets, [(100, D)]]
    yield [[], [], [], []], [sets, dels, [], mixed]
    yield [full, a, big], [every, dels, sorted(set(churn))]


@pytest.mark.parametrize("bs", [9, 256])
def test_rollup_rows(eng, bs):
    for lists, muts in rollup_fixtures():
        rolled = rows_mut_ref.want_rows(lists, muts)
        want = want_arena(rolled, bs)
        packs = [(*gv.flatten(gv.encode(u, 4)), len(u)) for u in lists]
        dpb = eng.upload_pack_batch(packs)
        mu, mo, rmb = rows_mut_ref.flat(muts)
        dp = eng.rollup_rows(dpb, mu, mo, rmb, bs)
        nb, db = want[0].size, want[3].size
        assert np.array_equal(dp.pbb, want[4])
        assert np.array_equal(dp.bases.cpu().numpy().view(np.uint64), want[0])
        assert np.array_equal(dp.num_uids.cpu().numpy().view(np.uint32), want[1])
        assert np.array_equal(dp.delta_offs.cpu().numpy().view(np.uint64), want[2])
        assert np.array_equal(dp.deltas.cpu().numpy().view(np.uint8)[:db], want[3])
        assert dp.bases.numel() == nb
        host = algo.rollup_rows(eng, packs, muts, bs)
        for r, (bases, nums, doffs, blob, total) in enumerate(host):
            b0, b1 = int(want[4][r]), int(want[4][r + 1])
            y0, y1 = int(want[2][b0]), int(want[2][b1])
            assert np.array_equal(bases, want[0][b0:b1])
            assert np.array_equal(nums, want[1][b0:b1])
            assert np.array_equal(blob, want[3][y0:y1])
            assert total == len(rolled[r])


# ---------- 6. stats ----------

@pytest.mark.parametrize("count_only", [False, True])
def test_stats_follow_the_documented_formula(eng, count_only):
    rows = [one_run(2100), [], [5, 6]]
    vals, offs = csr(rows)
    want = want_arena(rows, 9)
    nb, db = want[0].size, want[3].size
    eng.stats_reset()
    res = run(eng, vals, offs, 9, nb, db, count_only=count_only)
    st = eng.stats()
    assert res.rc == 0
    assert st["launches"] == (7 if count_only else 8)
    assert st["bytes_algorithmic"] == (8 * vals.size + 8 * offs.size) + \
        (db + 20 * nb + 8 * offs.size)
    assert st["kernel_ms"] > 0
    # total == 0: zero offsets and no launch
    eng.stats_reset()
    res = run(eng, np.empty(0, np.uint64), np.zeros(4, np.uint64), 9, 2, 2,
              count_only=count_only)
    assert (res.rc, res.nb, res.db) == (0, 0, 0) and res.rbb[:4].tolist() == [0] * 4
    assert eng.stats()["launches"] == 0
    assert eng.stats()["bytes_algorithmic"] == 16 * 4
    if not count_only:
        assert res.doffs[0] == 0 and res.guards_ok and res.untouched


# ---------- 7. malformed input stays in bounds ----------

def test_malformed_call_stays_in_bounds(eng):
    up = [1000 + 5 * i for i in range(2500)]
    vals = gv.u64(up[::-1] + up[:700])                   # a descending row
    offs = np.array([0, 2500, 9000, 2600, 3200], dtype=np.uint64)  # 9000 > total, not monotone
    # one block per uid and 5 bytes per uid plus 3 per tile bound any input
    cap_blocks, cap_deltas = vals.size, 5 * vals.size + 3 * (vals.size // TILE + 1)
    res = run(eng, vals, offs, 9, cap_blocks, cap_deltas)
    assert res.rc == 0
    assert res.nb <= cap_blocks and res.db <= cap_deltas
    assert res.guards_ok
