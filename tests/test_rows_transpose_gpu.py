"""ua_rows_transpose_dev on the GPU: every case element for element against
tests/rows_transpose_ref.py (keys, group offsets, entries, out_src, *n_groups,
*out_total), which tests/test_rows_transpose_ref.py holds to hand-written
matrices.  The shapes sit on the tile grid's edges (2048 flat elements per
tile), on merge-round counts 0 to 3, on groups cut by tile boundaries of the
sorted run, and on every way an element can be dead."""
import ctypes as C

import numpy as np
import pytest
import torch

import gv_spec as gv
import rows_mut_ref
import rows_transpose_ref as ref
from dgraph_amd import _lib, algo
from oracle import bind as orc
from test_rows_transpose_ref import FWD_ROWS, FWD_UIDS, REVERSE

pytestmark = pytest.mark.gpu

TILE = 2048
U64 = np.uint64
U64MAX = (1 << 64) - 1
POISON = 0x5A5A5A5A5A5A5A5A
PAD = 8


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def dev(a, dtype=np.uint64):
    a = np.ascontiguousarray(a, dtype=dtype)
    if dtype == np.uint64:
        a = a.view(np.int64)
    if a.size == 0:
        return torch.empty(0, dtype=torch.from_numpy(a).dtype, device="cuda:0")
    return torch.from_numpy(a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def offsets(lens):
    o = np.zeros(len(lens) + 1, dtype=np.uint64)
    o[1:] = np.cumsum(np.asarray(lens, dtype=np.uint64))
    return o


def check(eng, vals, offs, row_uids=None, row_keep=None, unique=False):
    """One full call with out_src against the ref; returns the engine's outputs."""
    vals = np.asarray(vals, dtype=U64)
    offs = np.asarray(offs, dtype=U64)
    wk, wo, wv, ws = ref.transpose(vals, offs, len(vals), row_uids, row_keep, unique)
    res = eng.transpose_rows(dev(vals), dev(offs),
                             row_uids=None if row_uids is None else dev(row_uids),
                             row_keep=None if row_keep is None else dev(row_keep, np.uint8),
                             unique=unique, want_src=True)
    gk, go, gv_, gs = (host(t) for t in res)
    assert gk.size == len(wk) and gv_.size == len(wv)       # *n_groups, *out_total
    assert np.array_equal(gk, np.array(wk, dtype=U64))
    assert np.array_equal(go, np.array(wo, dtype=U64))
    assert np.array_equal(gv_, np.array(wv, dtype=U64))
    assert np.array_equal(gs, np.array(ws, dtype=U64))
    return gk, go, gv_, gs


def raw(eng, vals, offs, total=None, row_uids=None, row_keep=None, flags=0, form="full",
        cap_keys=None, cap_vals=None):
    """ua_rows_transpose_dev with explicit capacities over poisoned buffers
    that are PAD words longer.  Returns (rc, n_groups, out_total, keys, offs,
    vals, src) with the four whole buffers as host arrays (None when absent)."""
    vals_t, offs_t = dev(vals), dev(offs)
    total = len(vals) if total is None else total
    keep = [vals_t, offs_t]
    d = _lib.UaDRowTr()
    d.vals = vals_t.data_ptr() if vals_t.numel() else None
    d.row_offs = offs_t.data_ptr()
    d.n_rows = len(offs) - 1
    d.total = total
    if row_uids is not None:
        keep.append(dev(row_uids))
        d.row_uids = keep[-1].data_ptr()
    if row_keep is not None:
        keep.append(dev(row_keep, np.uint8))
        d.row_keep = keep[-1].data_ptr()
    d.flags = flags
    cap_keys = total if cap_keys is None else cap_keys
    cap_vals = total if cap_vals is None else cap_vals

    def poisoned(n):
        return torch.full((n + PAD,), POISON, dtype=torch.int64, device="cuda:0")

    bk = bo = bv = bs = None
    if form != "count":
        bk, bo = poisoned(cap_keys), poisoned(cap_keys + 1)
        d.out_keys, d.out_offs, d.cap_keys = bk.data_ptr(), bo.data_ptr(), cap_keys
        if form == "full":
            bv, bs = poisoned(cap_vals), poisoned(cap_vals)
            d.out_vals, d.out_src, d.cap_vals = bv.data_ptr(), bs.data_ptr(), cap_vals
    ng, nt = C.c_uint64(U64MAX), C.c_uint64(U64MAX)
    rc = _lib.lib().ua_rows_transpose_dev(eng._ctx, C.byref(d), C.byref(ng), C.byref(nt))
    outs = [None if b is None else host(b) for b in (bk, bo, bv, bs)]
    return (rc, ng.value, nt.value, *outs)


def shared_rows(rng, lens, pool, share=0.3):
    """Rows of the given lengths, duplicate-free and sorted: about `share` of
    a row's values come from a small common pool, the rest are its own."""
    rows = []
    for r, n in enumerate(lens):
        k = min(int(round(share * n)), pool.size)
        common = rng.choice(pool, size=k, replace=False)
        own = (np.arange(n - k, dtype=U64) * U64(7919) + U64((r + 1) << 34))
        rows.append(np.unique(np.concatenate([common, own])))
    return rows


def csr(rows):
    rows = [np.asarray(r, dtype=U64) for r in rows]
    vals = np.concatenate(rows) if rows else np.empty(0, U64)
    return vals, offsets([r.size for r in rows])


# ---- tile edges ----

@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097, 10240])
def test_one_row_at_the_tile_edges(eng, n):
    # 10240 is 5 tiles: R = 3 and round 0 copies the group without a partner
    rng = np.random.default_rng(n)
    check(eng, rng.integers(0, 2**64, size=n, dtype=U64), [0, n])
    few = rng.integers(0, 37, size=n).astype(U64)           # long groups
    check(eng, few, [0, n])
    check(eng, few, [0, n], unique=True)                    # one entry per value


# ---- a group cut by tile boundaries of the sorted run ----

def test_groups_cut_by_tile_boundaries(eng):
    rng = np.random.default_rng(11)
    vals = rng.integers(0, 2**64, size=8192, dtype=U64)
    at = rng.choice(8192, size=5000, replace=False)
    vals[at] = U64(1 << 62)                                 # spans three sorted tiles
    lens = [1000, 3000, 0, 4000, 192]
    check(eng, vals, offsets(lens))
    check(eng, vals, offsets(lens), unique=True)
    check(eng, np.full(6000, 12345, dtype=U64), offsets([1500] * 4))
    check(eng, np.full(6000, 12345, dtype=U64), offsets([1500] * 4), unique=True)
    distinct = rng.permutation(7000).astype(U64) * U64(3)
    gk, go, _, _ = check(eng, distinct, offsets([3500, 3500]))
    assert gk.size == 7000 and np.array_equal(go, np.arange(7001, dtype=U64))


# ---- values ----

def test_unsigned_order_of_the_extreme_values(eng):
    rng = np.random.default_rng(5)
    special = np.array([0, 1, (1 << 63) - 1, 1 << 63, U64MAX], dtype=U64)
    vals = rng.integers(0, 2**64, size=5000, dtype=U64)
    vals[rng.choice(5000, size=1500, replace=False)] = rng.choice(special, size=1500)
    gk, _, _, _ = check(eng, vals, offsets([1200, 1300, 2500]))
    assert gk[0] == 0 and gk[1] == 1 and gk[-1] == U64(U64MAX)
    assert np.all(gk[1:] > gk[:-1])
    check(eng, special[::-1].copy(), offsets([2, 3]))


# ---- rows ----

def test_zipf_rows_with_shared_values(eng):
    rng = np.random.default_rng(3)
    lens = np.minimum(rng.zipf(1.3, size=300) - 1, 200)
    lens[[0, 1, 2, 150, 151, 152, 153, 298, 299]] = 0      # empty rows first, in a run, last
    pool = rng.integers(1, 2**40, size=400, dtype=U64)
    vals, offs = csr(shared_rows(rng, lens, pool))
    uids = np.arange(300, dtype=U64) * U64(11) + U64(1 << 33)
    check(eng, vals, offs)
    check(eng, vals, offs, row_uids=uids)
    shuffled = vals.copy()                                  # rows need not be sorted
    for r in range(300):
        rng.shuffle(shuffled[int(offs[r]):int(offs[r + 1])])
    check(eng, shuffled, offs, row_uids=uids)


def test_one_element_per_row(eng):
    # the per-row-key form: rebuildCountIndex with vals = the list lengths
    rng = np.random.default_rng(4096)
    lengths = np.minimum(rng.zipf(1.5, size=4096), 300).astype(U64)
    uids = np.arange(4096, dtype=U64) * U64(5) + U64(1 << 32)
    gk, go, gvals, _ = check(eng, lengths, np.arange(4097, dtype=U64), row_uids=uids)
    assert np.all(np.diff(gvals[int(go[0]):int(go[1])].astype(np.int64)) > 0)
    check(eng, rng.integers(0, 2**64, size=3000, dtype=U64), [0, 3000])    # one row against it


def test_empty_matrices(eng):
    check(eng, [], [0])                                     # n_rows == 0
    check(eng, [], [0, 0, 0, 0])
    rc, ng, nt, bk, bo, bv, bs = raw(eng, [], [0, 0])
    assert (rc, ng, nt) == (0, 0, 0)
    assert bo[0] == 0 and np.all(bo[1:] == U64(POISON))
    assert np.all(bk == U64(POISON)) and np.all(bv == U64(POISON))


# ---- duplicates ----

def test_duplicates_with_and_without_unique(eng):
    rng = np.random.default_rng(9)
    rows = []
    for r in range(120):
        base = rng.integers(0, 500, size=rng.integers(0, 60)).astype(U64)
        twice = base[: base.size // 3]
        thrice = base[: base.size // 5]
        row = np.concatenate([base, twice, thrice, thrice])
        rng.shuffle(row)
        rows.append(row)
    vals, offs = csr(rows)
    uids = np.arange(120, dtype=U64) + U64(1 << 35)
    _, _, mv, _ = check(eng, vals, offs, row_uids=uids)
    _, go, uv, us = check(eng, vals, offs, row_uids=uids, unique=True)
    assert uv.size < mv.size
    for g in range(go.size - 1):                            # a set per group, ascending
        grp = uv[int(go[g]):int(go[g + 1])]
        assert np.all(grp[1:] > grp[:-1])
    # on duplicate-free rows the two agree
    dvals, doffs = csr(shared_rows(rng, [40] * 50, np.arange(1, 90, dtype=U64)))
    a = check(eng, dvals, doffs)
    b = check(eng, dvals, doffs, unique=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_equal_value_and_row_across_a_sorted_tile_boundary(eng):
    # sorted run: 2040 smaller values, then X 20 times at ranks 2040 .. 2059:
    # row 0 holds 6 of them (ranks 2040-2045), row 1 the other 14, which lie on
    # both sides of rank 2048
    X = U64(1 << 50)
    small = (np.arange(2040, dtype=U64) * U64(3))[::-1].copy()
    row0 = np.concatenate([small, np.full(6, X)])
    row1 = np.concatenate([np.full(7, X), np.arange(3000, dtype=U64) + X + U64(1), np.full(7, X)])
    vals, offs = csr([row0, row1])
    gk, go, gvals, gs = check(eng, vals, offs)
    g = int(np.searchsorted(gk, X))
    assert (int(go[g]), int(go[g + 1])) == (2040, 2060)
    gk, go, gvals, gs = check(eng, vals, offs, unique=True)
    g = int(np.searchsorted(gk, X))
    assert gvals[int(go[g]):int(go[g + 1])].tolist() == [0, 1]
    assert gs[int(go[g]):int(go[g + 1])].tolist() == [2040, 2046]    # the lowest flat index


# ---- row_uids, row_keep, the tail ----

def test_row_uids_and_row_keep(eng):
    rng = np.random.default_rng(21)
    lens = rng.integers(0, 90, size=100)
    pool = rng.integers(1, 2**30, size=200, dtype=U64)
    vals, offs = csr(shared_rows(rng, lens, pool, share=0.5))
    uids = np.cumsum(rng.integers(1, 1000, size=100)).astype(U64) + U64(1 << 32)
    first, last = np.ones(100, np.uint8), np.ones(100, np.uint8)
    first[0], last[-1] = 0, 0
    alternate = (np.arange(100) % 2).astype(np.uint8)
    for keep in (None, first, last, alternate, 7 * alternate, np.zeros(100, np.uint8)):
        check(eng, vals, offs, row_keep=keep)
        check(eng, vals, offs, row_uids=uids, row_keep=keep, unique=True)
    gk, _, _, _ = check(eng, vals, offs, row_keep=np.zeros(100, np.uint8))
    assert gk.size == 0


def test_tail_past_the_last_row(eng):
    rng = np.random.default_rng(22)
    vals = rng.integers(0, 300, size=5000).astype(U64)
    offs = offsets([1000, 0, 2000, 500])                    # row_offs[n_rows] = 3500 < total
    wk, wo, wv, ws = ref.transpose(vals, offs, 5000)
    assert max(ws) < 3500
    rc, ng, nt, bk, bo, bv, bs = raw(eng, vals, offs, total=5000)
    assert (rc, ng, nt) == (0, len(wk), 3500)
    assert bk[:ng].tolist() == wk and bo[:ng + 1].tolist() == wo
    assert bv[:nt].tolist() == wv and bs[:nt].tolist() == ws
    # row_offs[n_rows] above total is clamped to it
    offs = np.array([0, 1000, 9000], dtype=U64)
    wk, wo, wv, ws = ref.transpose(vals, offs, 5000)
    rc, ng, nt, bk, bo, bv, bs = raw(eng, vals, offs, total=5000)
    assert (rc, ng, nt) == (0, len(wk), 5000)
    assert bv[:nt].tolist() == wv and bs[:nt].tolist() == ws


# ---- forms and capacities ----

def test_forms_agree_and_short_capacities(eng):
    rng = np.random.default_rng(31)
    vals = rng.integers(0, 900, size=6000).astype(U64)
    offs = offsets([2500, 1500, 2000])
    wk, wo, wv, ws = ref.transpose(vals, offs)
    NG, NT = len(wk), len(wv)
    for flags in (0, 1):
        full = raw(eng, vals, offs, flags=flags)
        grp = raw(eng, vals, offs, flags=flags, form="groups")
        cnt = raw(eng, vals, offs, flags=flags, form="count")
        assert full[:3] == grp[:3] == cnt[:3]
        assert full[0] == 0
        assert np.array_equal(full[3], grp[3]) and np.array_equal(full[4], grp[4])
    rc, ng, nt, bk, bo, bv, bs = raw(eng, vals, offs)
    assert (ng, nt) == (NG, NT)
    assert bk[:NG].tolist() == wk and bo[:NG + 1].tolist() == wo
    assert bv[:NT].tolist() == wv and bs[:NT].tolist() == ws
    # nothing is stored past what a call needs, also under a roomy capacity
    assert np.all(bk[NG:] == U64(POISON)) and np.all(bo[NG + 1:] == U64(POISON))
    assert np.all(bv[NT:] == U64(POISON)) and np.all(bs[NT:] == U64(POISON))
    # exact capacities pass
    assert raw(eng, vals, offs, cap_keys=NG, cap_vals=NT)[:3] == (0, NG, NT)
    for ck, cv in ((NG - 1, NT), (NG, NT - 1), (3, 5), (0, 0), (NG // 2, NT)):
        rc, ng, nt, bk, bo, bv, bs = raw(eng, vals, offs, cap_keys=ck, cap_vals=cv)
        assert (rc, ng, nt) == (ref.UA_ERR_INVALID, NG, NT), (ck, cv)
        assert ref.capacity_rc(NG, NT, ck, cv, True, True) == rc
        ek, eo, ev, es = ref.bounded(wk, wo, wv, ws, ck, cv)
        assert bk[:ck].tolist() == ek and bo[:ck + 1].tolist() == eo
        assert bv[:cv].tolist() == ev and bs[:cv].tolist() == es
        assert np.all(bk[ck:] == U64(POISON)) and np.all(bo[ck + 1:] == U64(POISON))
        assert np.all(bv[cv:] == U64(POISON)) and np.all(bs[cv:] == U64(POISON))
    rc, ng, nt, bk, bo, _, _ = raw(eng, vals, offs, form="groups", cap_keys=NG - 1)
    assert (rc, ng, nt) == (ref.UA_ERR_INVALID, NG, NT)
    assert np.all(bk[NG - 1:] == U64(POISON)) and np.all(bo[NG:] == U64(POISON))
    # the Engine's forms
    assert eng.transpose_rows(dev(vals), dev(offs), count_only=True) == (NG, NT)
    k2, o2 = eng.transpose_rows(dev(vals), dev(offs), groups_only=True)
    assert host(k2).tolist() == wk and host(o2).tolist() == wo


# ---- properties ----

def test_keys_equal_union_rows(eng):
    rng = np.random.default_rng(41)
    vals = rng.integers(0, 2**64, size=9000, dtype=U64)
    vals[rng.choice(9000, size=4000, replace=False)] = rng.integers(0, 50, size=4000).astype(U64)
    keys, _ = eng.transpose_rows(dev(vals), dev(offsets([4000, 5000])), groups_only=True)
    assert torch.equal(keys, eng.union_rows(dev(vals)))


def test_transposing_twice_returns_the_matrix(eng):
    rng = np.random.default_rng(42)
    lens = rng.integers(0, 70, size=150)
    lens[[0, 77, 149]] = 0
    rows = shared_rows(rng, lens, rng.integers(1, 2**36, size=300, dtype=U64), share=0.6)
    vals, offs = csr(rows)
    uids = np.cumsum(rng.integers(1, 50, size=150)).astype(U64) + U64(1 << 33)
    k1, o1, v1 = eng.transpose_rows(dev(vals), dev(offs), row_uids=dev(uids))
    k2, o2, v2 = eng.transpose_rows(v1, o1, row_uids=k1)
    full = [r for r in range(150) if rows[r].size]
    assert host(k2).tolist() == [int(uids[r]) for r in full]
    wvals, woffs = csr([rows[r] for r in full])
    assert np.array_equal(host(o2), woffs) and np.array_equal(host(v2), wvals)


def test_reverse_rows_equals_the_oracle_encoding(eng):
    rng = np.random.default_rng(64)
    S, D = rows_mut_ref.MUT_SET, rows_mut_ref.MUT_DEL
    pool = np.unique(rng.integers(1, 2**34, size=250, dtype=U64))
    lists, muts = [], []
    for r in range(64):
        n = int(rng.integers(0, 120))
        u = sorted(int(x) for x in rng.choice(pool, size=min(n, pool.size), replace=False))
        m = {}
        for x in rng.choice(pool, size=int(rng.integers(0, 12)), replace=False):
            m[int(x)] = S if rng.random() < 0.6 else D
        if r % 16 == 5:
            u, m = [], {}                                   # a forward list without postings
        lists.append(u)
        muts.append(sorted(m.items()))
    fwd = np.arange(64, dtype=U64) * U64(3) + U64(1 << 32)
    rolled = rows_mut_ref.want_rows(lists, muts)
    vals, offs = csr(rolled)
    want = ref.groups_of(vals, offs, row_uids=fwd, unique=True)
    packs = [(*gv.flatten(gv.encode(u, 4)), len(u)) for u in lists]
    dpb = eng.upload_pack_batch(packs)
    mu, mo, rmb = rows_mut_ref.flat(muts)
    for bs in (9, 256):
        keys, arena = eng.reverse_rows(dpb, mu, mo, rmb, row_uids=dev(fwd), block_size=bs)
        assert host(keys).tolist() == [k for k, _ in want]
        bases, nums, blobs, pbb, doffs = [], [], [], [0], [0]
        for _, g in want:
            b, n, o, blob = orc.Pack(np.array(g, dtype=U64), bs).flatten()
            bases.append(b)
            nums.append(n)
            blobs.append(blob)
            at = doffs[-1]
            doffs += [at + int(x) for x in o[1:]]           # arena-wide delta offsets
            pbb.append(pbb[-1] + b.size)
        wb, wn, wblob = np.concatenate(bases), np.concatenate(nums), np.concatenate(blobs)
        assert np.array_equal(arena.pbb, np.array(pbb, dtype=U64))
        assert np.array_equal(arena.bases.cpu().numpy().view(U64), wb)
        assert np.array_equal(arena.num_uids.cpu().numpy().view(np.uint32), wn)
        assert arena.delta_offs.cpu().numpy().view(U64).tolist() == doffs
        assert np.array_equal(arena.deltas.cpu().numpy().view(np.uint8)[:wblob.size], wblob)
        assert arena.pack_totals == [len(g) for _, g in want]


def test_host_mirrors(eng):
    assert algo.group_by_uid(eng, FWD_ROWS, FWD_UIDS) == REVERSE
    assert algo.group_by_uid(eng, FWD_ROWS, FWD_UIDS, keep=[0, 1, 1, 1]) == \
        [(0x20, [0x13]), (0x30, [0x11, 0x13]), (0x40, [0x13])]
    rows = [[7, 4, 7, 7], [4, 7, 7]]
    keys, groups, srcs = algo.transpose_uid_matrix(eng, rows, unique=True, want_src=True)
    assert keys.tolist() == [4, 7]
    assert [g.tolist() for g in groups] == [[0, 1], [0, 1]]
    assert [s.tolist() for s in srcs] == [[1, 4], [0, 5]]
    keys, groups = algo.transpose_uid_matrix(eng, [], None)
    assert keys.size == 0 and groups == []


# ---- broken input ----

def test_broken_row_offs_stays_in_bounds(eng):
    rng = np.random.default_rng(51)
    total = 5000
    vals = rng.integers(0, 100, size=total).astype(U64)
    broken = [
        np.array([0, 3000, 1000, 4000, 2000, 1 << 40], dtype=U64),
        np.array([700, 100, U64MAX, 0, 4999, 5001, 3], dtype=U64),
        rng.integers(0, 2 * total, size=400).astype(U64),
    ]
    for offs in broken:
        for flags in (0, 1):
            rc, ng, nt, bk, bo, bv, bs = raw(eng, vals, offs, total=total, flags=flags)
            assert rc == 0
            assert nt <= total and ng <= nt
            o = bo[:ng + 1].astype(np.int64)
            assert o[0] == 0 and o[-1] == nt and np.all(np.diff(o) >= 1)
            keys = bk[:ng]
            assert np.all(keys[1:] > keys[:-1])
            assert np.all(bv[:nt] < U64(len(offs) - 1)) and np.all(bs[:nt] < U64(total))
            assert np.unique(bs[:nt]).size == nt            # each element at most once
            assert np.array_equal(vals[bs[:nt].astype(np.int64)],
                                  np.repeat(bk[:ng], np.diff(o)))


# ---- stats ----

@pytest.mark.parametrize("total", [0, 1500, 4096, 10240])   # no kernel, R = 0, 1, 3
@pytest.mark.parametrize("form", ["full", "groups", "count"])
def test_stats_follow_the_documented_formula(eng, total, form):
    rng = np.random.default_rng(total)
    vals = rng.integers(0, 64, size=total).astype(U64)
    offs = offsets([total // 2, total - total // 2])
    uids = np.array([9, 10], dtype=U64)
    eng.stats_reset()
    rc, ng, nt, bk, bo, bv, bs = raw(eng, vals, offs, row_uids=uids, form=form)
    st = eng.stats()
    assert rc == 0 and nt == total
    assert st["launches"] == ref.launches(total, form)
    stored = {"count": 0, "groups": 8 * ng + 8 * (ng + 1),
              "full": 8 * ng + 8 * (ng + 1) + 16 * nt}[form]
    assert st["bytes_algorithmic"] == 8 * total + 8 * 3 + 8 * 2 + stored
