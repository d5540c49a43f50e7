"""ua_rows_intersect_packed_dev on the GPU: a fan-out of UidPacks and one
shared sorted list in, a CSR UID matrix out, against the format itself.

Packs are uploaded from the bytes of tests/gv_spec.py, never from an engine
encoder.  Expected rows come from tests/rows_isect_ref.py
(IntersectCompressedWith: x >= after, inclusive, and x in shared; no first),
which tests/test_rows_isect_ref.py holds to the oracle.  Output buffers are
pre-filled with a sentinel and carry 64 guard words past their capacity.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gv_spec as gv
from dgraph_amd import _lib, algo
from rows_isect_ref import want_row, want_rows

pytestmark = pytest.mark.gpu

UA_ERR_INVALID = 3
GUARD = 64
SENT = 0xA5A5A5A5A5A5A5A5
SENT_I64 = SENT - (1 << 64)
DEV = "cuda:0"


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


def u64_list(t):
    return t.cpu().numpy().view(np.uint64).tolist()


class Result:
    pass


def run(eng, dpb, shared, afters=None, cap=None, count_only=False):
    """One raw ua_rows_intersect_packed_dev call into sentinel-filled buffers."""
    n_rows = len(dpb.pbb) - 1
    nb = int(dpb.pbb[n_rows])
    if cap is None:
        cap = int(sum(dpb.pack_totals))
    rbb = dev_u64([int(x) for x in dpb.pbb])
    t_shared = dev_u64(shared)
    t_after = dev_u64(afters) if afters is not None else None
    out = torch.full((cap + GUARD,), SENT_I64, dtype=torch.int64, device=DEV)
    oro = torch.full((n_rows + 1 + GUARD,), SENT_I64, dtype=torch.int64, device=DEV)
    d = _lib.UaDRowIsect()
    d.bases, d.num_uids = dpb.bases.data_ptr(), dpb.num_uids.data_ptr()
    d.delta_offs, d.deltas = dpb.delta_offs.data_ptr(), dpb.deltas.data_ptr()
    d.n_blocks, d.n_rows = nb, n_rows
    d.row_block_base = rbb.data_ptr() if n_rows else None
    d.after = t_after.data_ptr() if t_after is not None else None
    d.shared = t_shared.data_ptr() if len(shared) else None
    d.m = len(shared)
    d.out_vals = None if count_only else out.data_ptr()
    d.cap_vals = 0 if count_only else cap
    d.out_row_offs = oro.data_ptr()
    total = C.c_uint64(77)
    res = Result()
    res.rc = _lib.lib().ua_rows_intersect_packed_dev(eng._ctx, C.byref(d), C.byref(total))
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


def neighbours(uids, step=1):
    """Non-members next to every step-th uid."""
    member = set(uids)
    return {x + d for x in uids[::step] for d in (-1, 1)
            if 0 <= x + d <= gv.U64_MAX and x + d not in member}


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
    shared = {0, gv.U64_MAX}
    for name in names:
        u = gv.inputs()[name]
        shared |= set(u[::2]) | neighbours(u, 3)
    shared = sorted(shared)
    want = want_rows(lists, shared)
    assert all(0 < len(w) < len(u) for w, u in zip(want, lists))
    check(run(eng, arena(eng, flats), shared), want)


# ---------- 2. the after sweep ----------

@pytest.fixture(scope="module")
def seek_case(eng):
    uids = gv.seek_pack()
    blocks = gv.encode(uids, 9)
    seeks = gv.seek_list(blocks)
    assert 30 <= len(blocks) <= 40 and 150 <= len(seeks) <= 300
    assert {0, 1, gv.U64_MAX - 1, gv.U64_MAX} <= set(seeks)
    return uids, blocks, seeks


@pytest.mark.parametrize("every", [1, 3])
def test_after_sweep(eng, seek_case, every):
    uids, blocks, seeks = seek_case
    shared = uids[::every]
    if gv.U64_MAX not in shared:
        shared = shared + [gv.U64_MAX]
    dpb = arena(eng, [blocks] * len(seeks))
    want = want_rows([uids] * len(seeks), shared, seeks)
    kept = [x for x in uids if x in set(shared)]
    assert seeks[0] == 0 and want[0] == kept                      # after = 0
    assert seeks[-1] == gv.U64_MAX and want[-1] == [gv.U64_MAX]   # inclusive at the top
    bases = {b for b, _, _ in blocks}
    inner = [a for a in seeks if a in kept and a not in bases and a < gv.U64_MAX]
    member = inner[len(inner) // 2]
    assert want[seeks.index(member)][0] == member                 # a member is kept
    base = blocks[7][0]
    assert want[seeks.index(base)] == [x for x in kept if x >= base] != []
    check(run(eng, dpb, shared, afters=seeks), want)


# ---------- 3. both match forms, by construction ----------

def test_list_driven_sparse_shared(eng, seek_case):
    """shared = every 3rd uid of the row: a block of num uids spans at most
    num shared values, so R <= UA_RI_RATIO * num for every ratio >= 1."""
    uids, blocks, _ = seek_case
    long = gv.long_list(3000)
    for u, bs in ((long, 256), (long, 9), (uids, 9)):
        f = gv.encode(u, bs)
        shared = u[::3]
        inside = gv.decode([f[len(f) // 2]])
        afters = [0, inside[len(inside) // 2], inside[-1], u[-1]]
        check(run(eng, arena(eng, [f] * 4), shared, afters=afters),
              want_rows([u] * 4, shared, afters))


@pytest.mark.parametrize("bs", [9, 256])
def test_block_driven_dense_shared(eng, bs):
    """Uids 1000 apart against every 7th integer: a block of num uids spans
    about 143 * num shared values, above 16 * num, so R > UA_RI_RATIO * num
    for every ratio <= 16 in every block of at least two uids."""
    lists = [[1000 * i + 7 * r for i in range(1, n)] for r, n in enumerate((700, 300, 10, 2))]
    flats = [gv.encode(u, bs) for u in lists]
    top = max(u[-1] for u in lists)
    shared = list(range(0, top + 50, 7))
    for f in flats:
        for base, num, _ in f[:-1]:
            last = base + 1000 * (num - 1)
            assert num == bs and (last - base) // 7 > 16 * num
    want = want_rows(lists, shared)                                # one match in seven
    assert all(0 < len(w) < len(u) for w, u in zip(want[:2], lists))
    check(run(eng, arena(eng, flats), shared), want)
    check(run(eng, arena(eng, flats), list(range(top + 50))), lists)   # every uid matches
    # an after inside a block, on a member and next to one
    afters = [lists[0][350], lists[1][100] + 1, lists[2][4], lists[3][0] + 1]
    check(run(eng, arena(eng, flats), shared, afters=afters), want_rows(lists, shared, afters))


# ---------- 4. rows are independent ----------

def test_rows_in_descending_order_and_empty_rows(eng):
    """One block per row, every row below the one before it: the bound taken
    from the next block's base must stop at the row boundary."""
    lists = [[((64 - r) << 20) + 3 * i for i in range(5 + r % 4)] for r in range(64)]
    flats = [gv.encode(u, 256) for u in lists]
    assert all(len(f) == 1 for f in flats)
    shared = sorted(x for u in lists for x in u)
    check(run(eng, arena(eng, flats), shared), lists)
    afters = [u[2] for u in lists]
    check(run(eng, arena(eng, flats), shared, afters=afters),
          want_rows(lists, shared, afters))
    # empty rows between the rows, at the front and at the end
    gl, gf = [], []
    for u, f in zip(lists, flats):
        gl += [[], u, []]
        gf += [[], f, []]
    check(run(eng, arena(eng, gf), shared), gl)
    check(run(eng, arena(eng, gf), shared[::2]), want_rows(gl, shared[::2]))


# ---------- 5. blocks dropped from their headers ----------

def test_header_only_drops(eng):
    u = gv.long_list(500)
    f = gv.encode(u, 9)
    lasts = [gv.decode([blk])[-1] for blk in f]
    gaps = [l + 1 for l, nxt in zip(lasts, f[1:]) if l + 1 < nxt[0]]
    assert len(gaps) > 10 and u[0] > 100 and u[-1] < gv.U64_MAX - 100
    dpb = arena(eng, [f, f[:3], [], f[5:]])
    lists = [u, gv.decode(f[:3]), [], gv.decode(f[5:])]
    for shared in (list(range(1, 100)),                       # below every pack
                   list(range(u[-1] + 1, u[-1] + 100)),       # above every pack
                   gaps,                                      # between the blocks
                   [], [u[40]], [u[40] + 1] if u[40] + 1 not in u else [u[40] - 1],
                   [0], [gv.U64_MAX]):
        want = want_rows(lists, shared)
        if shared not in ([u[40]],):
            assert want[0] == []
        check(run(eng, dpb, shared), want)
    # last == 2^64 - 1: the tightening step has no last + 1
    e = gv.edge_values()
    for bs in (4, 256):
        fe = gv.encode(e, bs)
        for shared in ([gv.U64_MAX], [gv.U64_MAX - 2, gv.U64_MAX], e, [0, gv.U64_MAX]):
            for a in (0, gv.U64_MAX - 1, gv.U64_MAX):
                res = run(eng, arena(eng, [fe, fe]), shared, afters=[a, 0])
                check(res, want_rows([e, e], shared, [a, 0]))
                assert res.rows[0][-1] == gv.U64_MAX


# ---------- 6. geometry ----------

@pytest.mark.parametrize("nb", [1, 2, 3, 5, 2047, 2048, 2049, 4097])
def test_one_uid_blocks(eng, nb):
    """Four blocks per workgroup and 2048 counts per scan chunk: rows of
    seven one-uid blocks, every third row with an after inside it; then the
    same blocks as one row."""
    uids = gv.long_list(nb)
    blocks = gv.encode(uids, 1)
    assert len(blocks) == nb
    cuts = list(range(0, nb, 7)) + [nb]
    flats = [blocks[s:e] for s, e in zip(cuts, cuts[1:])]
    lists = [uids[s:e] for s, e in zip(cuts, cuts[1:])]
    afters = [u[len(u) // 2] if r % 3 == 0 else 0 for r, u in enumerate(lists)]
    shared = sorted(set(uids[::2]) | {uids[-1]} | neighbours(uids, 5))
    dpb = arena(eng, flats)
    check(run(eng, dpb, uids), lists)
    check(run(eng, dpb, shared), want_rows(lists, shared))
    check(run(eng, dpb, shared, afters=afters), want_rows(lists, shared, afters))
    one = arena(eng, [blocks])
    check(run(eng, one, shared), [want_row(uids, shared)])
    a = uids[nb // 3]
    check(run(eng, one, shared, afters=[a]), [want_row(uids, shared, a)])


@pytest.mark.parametrize("n_rows", [2047, 2048, 2049])
def test_one_block_per_row(eng, n_rows):
    uids = gv.long_list(3 * n_rows)
    lists = [uids[3 * r:3 * r + 3] for r in range(n_rows)]
    flats = [gv.encode(u, 256)[:1] for u in lists]   # a 32-MSB break may split a row
    lists = [gv.decode(f) for f in flats]
    shared = sorted({x for u in lists for x in u[::2]})
    check(run(eng, arena(eng, flats), shared), want_rows(lists, shared))


@pytest.mark.parametrize("n_rows", [0, 5])
def test_no_blocks_at_all(eng, n_rows):
    dpb = arena(eng, [[]] * n_rows)
    assert int(dpb.pbb[-1]) == 0
    for shared in ([], [1, 2, 3]):
        res = run(eng, dpb, shared, afters=[3] * n_rows if shared else None, cap=8)
        check(res, [[]] * n_rows)
        assert res.out[:8] == [SENT] * 8
        res = run(eng, dpb, shared, count_only=True)
        assert (res.rc, res.total, res.offs) == (0, 0, [0] * (n_rows + 1))


# ---------- 7. capacity ----------

def test_capacity_and_count_only(eng, seek_case):
    uids, blocks, seeks = seek_case
    flats = [blocks, [], gv.encode(gv.full_block(), 256), blocks]
    lists = [gv.decode(f) for f in flats]
    shared = sorted(set(uids[::2]) | set(gv.full_block()[10:200]))
    afters = [seeks[40], 0, gv.full_block()[50], 0]
    want = want_rows(lists, shared, afters)
    total = sum(len(w) for w in want)
    offs = list(np.cumsum([0] + [len(w) for w in want]))
    assert total > 100 and want[2] == gv.full_block()[50:200]
    dpb = arena(eng, flats)
    exact = run(eng, dpb, shared, afters=afters, cap=total)
    check(exact, want)
    short = run(eng, dpb, shared, afters=afters, cap=total - 1)
    assert (short.rc, short.total, short.offs) == (UA_ERR_INVALID, total, offs)
    assert short.guards_ok
    count = run(eng, dpb, shared, afters=afters, count_only=True)
    assert (count.rc, count.total, count.offs) == (0, total, offs)
    assert count.guards_ok and count.out[:8] == [SENT] * 8
    # the host mirror; algo.uid_matrix keeps its own semantics next to it
    packs = [(*gv.flatten(f), len(u)) for f, u in zip(flats, lists)]
    got = algo.uid_matrix_intersect(eng, packs, gv.u64(shared), after=afters)
    assert [g.tolist() for g in got] == want
    got = algo.uid_matrix_intersect(eng, packs, gv.u64([]))
    assert [g.tolist() for g in got] == [[]] * 4
    assert [g.tolist() for g in algo.uid_matrix(eng, packs)] == lists
    # the tensor-level wrapper sizes its own buffers
    t_shared = dev_u64(shared)
    vals, ro = eng.intersect_rows(dpb, t_shared, afters=afters)
    assert u64_list(vals) == [x for w in want for x in w] and u64_list(ro) == offs
    vals, ro = eng.intersect_rows(dpb, t_shared, afters=afters, count_only=True)
    assert vals.numel() == 0 and u64_list(ro) == offs
    vals, ro = eng.intersect_rows(dpb, t_shared, afters=seeks[40])
    assert u64_list(vals) == [x for w in want_rows(lists, shared, [seeks[40]] * 4) for x in w]
    with pytest.raises(ValueError):
        eng.intersect_rows(dpb, t_shared, out_vals=torch.empty(8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        eng.intersect_rows(dpb, t_shared,
                           out_row_offs=torch.empty(4, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        eng.intersect_rows(dpb, t_shared, afters=[1, 2])


# ---------- 8. the limits: 256 uids, 1092 delta bytes ----------

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
    shared = [1 << 36, 2 << 36, (2 << 36) + 5, 3 << 36]
    for kw in ({}, {"afters": [1 << 36, 0]}, {"count_only": True}):
        res = run(eng, dpb, shared, **kw)
        assert (res.rc, res.total) == (UA_ERR_INVALID, 0), kw
        assert res.guards_ok
    # the engine is unharmed
    uids = gv.full_block()
    check(run(eng, arena(eng, [gv.encode(uids, 256)]), uids), [uids])


def test_full_block_accepted(eng):
    uids = gv.full_block()
    blocks = gv.encode(uids, 256)
    assert [(n, len(d)) for _, n, d in blocks] == [(256, 1085)]
    afters = [0, uids[0], uids[100], uids[255], uids[255] + 1]
    for shared in (uids, uids[::3], uids[255:], sorted(set(uids[::64]) | neighbours(uids))):
        check(run(eng, arena(eng, [blocks] * 5), shared, afters=afters),
              want_rows([uids] * 5, shared, afters))


# ---------- 9. agreement with the existing paths ----------

def test_agrees_with_packed_batch_and_decode_filter(eng, seek_case):
    """All three are held to rows_isect_ref, so a disagreement names the path
    at fault.  decode_rows keeps x > after and 0 keeps all: x >= a is after
    a - 1 for a >= 2 and after 0 for a = 0 (a = 1 has no such form)."""
    uids, blocks, seeks = seek_case
    shared = sorted(set(uids[::2]) | neighbours(uids, 4) | {gv.U64_MAX})
    t_shared = dev_u64(shared)
    n = len(seeks)
    dpb = arena(eng, [blocks] * n)
    want = want_rows([uids] * n, shared, seeks)
    vals, ro = eng.intersect_rows(dpb, t_shared, afters=seeks)
    offs = u64_list(ro)
    flat = u64_list(vals)
    new = [flat[offs[r]:offs[r + 1]] for r in range(n)]
    outs, lens = eng.intersect_packed_batch(dpb, [t_shared] * n, afters=seeks)
    old = [u64_list(o[:k]) for o, k in zip(outs, lens)]
    rows = [r for r, a in enumerate(seeks) if a != 1]
    sub = arena(eng, [blocks] * len(rows))
    dv, dro = eng.decode_rows(sub, afters=[max(seeks[r] - 1, 0) for r in rows])
    fv, fro = eng.filter_rows(dv, dro, t_shared)
    foffs, fflat = u64_list(fro), u64_list(fv)
    for r, a in enumerate(seeks):
        assert old[r] == want[r], f"intersect_packed_batch after={a:#x}"
        assert new[r] == want[r], f"intersect_rows after={a:#x}"
    for i, r in enumerate(rows):
        assert fflat[foffs[i]:foffs[i + 1]] == want[r], f"decode+filter after={seeks[r]:#x}"


# ---------- 10. one traversal step on the device ----------

def test_intersect_union_step(eng):
    """intersect_rows -> union_rows: the filtered UidMatrix and its DestUIDs
    with nothing but the two totals crossing to the host."""
    long = gv.long_list(3000)
    lists = [long[(41 * r) % 2500:(41 * r) % 2500 + 20 + 7 * r] for r in range(64)]
    lists[9] = []
    keep = set(long[::3])
    dpb = arena(eng, [gv.encode(u, 256) for u in lists])
    vals, ro = eng.intersect_rows(dpb, dev_u64(sorted(keep)))
    want = [[x for x in u if x in keep] for u in lists]
    offs, flat = u64_list(ro), u64_list(vals)
    assert [flat[offs[r]:offs[r + 1]] for r in range(64)] == want
    dest = eng.union_rows(vals)
    assert u64_list(dest) == sorted({x for w in want for x in w})


# ---------- 11. stats ----------

@pytest.mark.parametrize("count_only", [False, True])
def test_stats_follow_the_documented_formula(eng, seek_case, count_only):
    """Launches: validation, count, scan (2), rows, then the write unless
    count-only.  Bytes: the whole blob + 20 per block + 8 per row boundary +
    8 per shared uid + 8 per kept uid."""
    uids, blocks, seeks = seek_case
    flats = [blocks, [], blocks]
    afters = [seeks[30], 0, 0]
    shared = uids[::2]
    want = want_rows([uids, [], uids], shared, afters)
    kept = sum(len(w) for w in want)
    blob = 2 * sum(len(d) for _, _, d in blocks)
    dpb = arena(eng, flats)
    eng.stats_reset()
    res = run(eng, dpb, shared, afters=afters, count_only=count_only)
    st = eng.stats()
    assert (res.rc, res.total) == (0, kept)
    assert st["launches"] == 5 + (0 if count_only else 1)
    assert st["bytes_algorithmic"] == \
        blob + 20 * 2 * len(blocks) + 8 * 4 + 8 * len(shared) + 8 * kept
    assert st["kernel_ms"] > 0
