"""ua_rows_sort_dev on the GPU: every case element for element against
tests/rows_sort_ref.py (values, offsets, out_src, out_ms_offs, *out_total),
which tests/test_rows_sort_ref.py holds to hand-written rows and to
oracle/sortref.py.  The shapes sit on the tile grid's edges (2048 flat
elements per tile), on every merge-round count up to 6, and on every PageRange
branch."""
import ctypes as C

import numpy as np
import pytest
import torch

import rows_sort_ref as ref
from dgraph_amd import _lib, algo, sortpath
from oracle import sortref
from rows_sort_ref import DESC, DROP_NULLS, MULTI
from test_rows_sort_ref import HAND

pytestmark = pytest.mark.gpu

TILE = 2048
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31
U64 = np.uint64


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


def rounds_of(total):
    ntiles = -(-total // TILE)
    k = 0
    while (1 << k) < ntiles:
        k += 1
    return k


def check(eng, vals, offs, keys=None, has=None, flags=0, count=0, offset=0):
    """One full call with out_src against the ref; returns the engine's outputs."""
    vals = np.asarray(vals, dtype=U64)
    offs = np.asarray(offs, dtype=U64)
    wv, wo, ws, wm = ref.sort_rows(vals, offs, keys, has, flags, count, offset)
    res = eng.sort_rows(dev(vals), dev(offs),
                        keys=None if keys is None else dev(keys),
                        has=None if has is None else dev(has, np.uint8),
                        count=count, offset=offset, desc=bool(flags & DESC),
                        multi=bool(flags & MULTI), drop_nulls=bool(flags & DROP_NULLS),
                        want_src=True)
    gv, go, gs = host(res[0]), host(res[1]), host(res[2])
    assert go.tolist() == wo
    assert gv.size == len(wv)               # *out_total
    assert np.array_equal(gv, np.array(wv, dtype=U64))
    assert np.array_equal(gs, np.array(ws, dtype=U64))
    if flags & MULTI:
        assert host(res[3]).tolist() == wm
    return gv, go, gs


def rand_keys(rng, n):
    return rng.integers(0, 2**64, size=n, dtype=U64)


FLAGSETS = [0, DESC, MULTI, MULTI | DESC, DROP_NULLS, DROP_NULLS | DESC]


# ---- tile edges ----

@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_one_row_at_the_tile_edges(eng, n):
    rng = np.random.default_rng(n)
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    keys = rng.integers(0, 50, size=n).astype(U64)         # long equal runs
    has = (rng.random(n) < 0.8).astype(np.uint8)
    for flags in (0, DESC):
        check(eng, vals, [0, n], keys, has, flags)
    check(eng, vals, [0, n], keys, has, MULTI, count=5, offset=n // 2)
    check(eng, vals, [0, n], rand_keys(rng, n), None, 0, count=7, offset=3)


def test_rows_cut_by_a_tile_boundary(eng):
    rng = np.random.default_rng(7)
    # one element on either side of 2048 and of 4096; a 10-element row
    # straddling flat index 4096 of an 8192-element matrix
    lens = [2047, 2, 2047 - 5, 10, 8192 - 4101]
    assert sum(lens) == 8192 and sum(lens[:3]) == 4091
    offs = offsets(lens)
    vals = rng.integers(0, 2**64, size=8192, dtype=U64)
    keys = rand_keys(rng, 8192)
    has = (rng.random(8192) < 0.5).astype(np.uint8)
    for flags in FLAGSETS:
        check(eng, vals, offs, keys, has, flags)
        check(eng, vals, offs, keys, has, flags, count=3, offset=1)
    lens = [2047, 1, 1, 2047, 1, 1, 100]                    # rows of one at the boundary
    offs = offsets(lens)
    n = int(offs[-1])
    check(eng, vals[:n], offs, keys[:n], has[:n], 0)


def test_three_rounds_with_a_partnerless_group(eng):
    rng = np.random.default_rng(11)
    lens = [1000, 3 * TILE + 5, 300]                        # starts at flat index 1000
    offs = offsets(lens)
    n = int(offs[-1])
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    keys = rng.integers(0, 1000, size=n).astype(U64)
    has = (rng.random(n) < 0.9).astype(np.uint8)
    for flags in (0, DESC, MULTI):
        check(eng, vals, offs, keys, has, flags)
    for nseg_len in (4 * TILE + 1, 5 * TILE, 2 * TILE + 7):  # 5, 5-6 and 3 segments
        lens = [1000, nseg_len, 17]
        offs = offsets(lens)
        n = int(offs[-1])
        vals = rng.integers(0, 2**64, size=n, dtype=U64)
        check(eng, vals, offs, rand_keys(rng, n), None, 0)


def test_one_long_row_beside_many_short_ones(eng):
    rng = np.random.default_rng(13)
    lens = list(rng.integers(0, 21, size=150)) + [66_000] + list(rng.integers(0, 21, size=150))
    offs = offsets(lens)
    n = int(offs[-1])
    assert n <= 71_000
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    keys = rand_keys(rng, n)
    has = (rng.random(n) < 0.7).astype(np.uint8)
    eng.stats_reset()
    check(eng, vals, offs, keys, has, 0)
    assert eng.stats()["launches"] == 7 + rounds_of(n)      # 6 rounds
    assert rounds_of(n) == 6
    check(eng, vals, offs, keys, has, DESC | MULTI, count=10, offset=5)
    check(eng, vals, offs, keys, has, DROP_NULLS, count=-9)


# ---- rows ----

def test_thousands_of_empty_rows_and_rows_of_one(eng):
    rng = np.random.default_rng(17)
    lens = np.zeros(6000, dtype=np.int64)
    lens[rng.choice(6000, size=900, replace=False)] = 1
    lens[rng.choice(6000, size=40, replace=False)] = rng.integers(2, 200, size=40)
    offs = offsets(lens)
    n = int(offs[-1])
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    keys = rand_keys(rng, n)
    has = (rng.random(n) < 0.5).astype(np.uint8)
    for flags in FLAGSETS:
        check(eng, vals, offs, keys, has, flags, count=2, offset=1)
    check(eng, vals, offs)                                   # page only, all
    check(eng, np.arange(500), np.arange(501), rand_keys(rng, 500), None, DESC)


def test_no_rows_and_no_elements(eng):
    check(eng, [], [0])
    check(eng, [], [0], [], None, DESC)
    check(eng, [], [0, 0, 0, 0])
    check(eng, [], [0, 0, 0, 0], [], [], MULTI, count=2, offset=3)   # ms_offs = offset
    check(eng, [], [0, 0], [], [], DROP_NULLS, count=-1)


def raw_call(eng, vals, offs, keys=None, has=None, flags=0, count=0, offset=0, cap=None,
             want_src=False, n_rows=None, count_only=False):
    """The C entry itself: returns (rc, total, out_vals, out_row_offs, out_src)
    with one guard word past the capacity."""
    total = vals.numel()
    n_rows = offs.numel() - 1 if n_rows is None else n_rows
    cap = total if cap is None else cap
    guard = -0x0123456789abcdef
    ov = torch.full((cap + 1,), guard, dtype=torch.int64, device="cuda:0")
    osrc = torch.full((cap + 1,), guard, dtype=torch.int64, device="cuda:0")
    oro = torch.full((n_rows + 1,), guard, dtype=torch.int64, device="cuda:0")
    d = _lib.UaDRowSort()
    d.vals, d.row_offs, d.n_rows, d.total = vals.data_ptr(), offs.data_ptr(), n_rows, total
    d.keys = keys.data_ptr() if keys is not None else None
    d.has = has.data_ptr() if has is not None else None
    d.flags, d.count, d.offset = flags, count, offset
    d.out_vals = None if count_only else ov.data_ptr()
    d.cap_vals = 0 if count_only else cap
    d.out_row_offs = oro.data_ptr()
    d.out_src = osrc.data_ptr() if want_src else None
    need = C.c_uint64(0)
    rc = _lib.lib().ua_rows_sort_dev(eng._ctx, C.byref(d), C.byref(need))
    return rc, need.value, ov, oro, osrc, guard


def test_malformed_row_offs_stays_in_bounds(eng):
    rng = np.random.default_rng(19)
    n = 3 * TILE + 100
    vals = dev(rng.integers(0, 2**64, size=n, dtype=U64))
    keys = dev(rand_keys(rng, n))
    has = dev((rng.random(n) < 0.5).astype(np.uint8), np.uint8)
    bad = [
        [0, 5000, 100, 7000, 3, n],                         # not monotone
        [0, 10, 2**40, 2**63, 50, 2**64 - 1],               # past total
        [n, 0, n, 0, n, 0],
        [4000, 3000, 2000, 1000, 0, 0],
        [0, 100, 200, 300, 400, 500],                       # ends before total
    ]
    for offs in bad:
        for flags in (0, MULTI, DROP_NULLS | DESC):
            rc, need, ov, oro, _, _ = raw_call(eng, vals, dev(np.array(offs, dtype=U64)), keys,
                                               has, flags, count=0, offset=1, want_src=True)
            assert rc == 0
            go = host(oro)
            assert int(go[-1]) == need <= n
            assert np.all(np.diff(go.astype(np.int64)) >= 0)
        rc, need, ov, oro, _, _ = raw_call(eng, vals, dev(np.array(offs, dtype=U64)))
        assert rc == 0 and int(host(oro)[-1]) == need <= n


def test_rows_past_the_last_offset_do_not_disturb_the_last_row(eng):
    rng = np.random.default_rng(23)
    vals = rng.integers(0, 2**64, size=600, dtype=U64)
    keys = rand_keys(rng, 600)
    offs = np.array([0, 100, 400], dtype=U64)               # 200 elements in no row
    wv, wo, ws, _ = ref.sort_rows(vals[:400], offs, keys[:400], None, 0, 0, 0)
    rc, need, ov, oro, osrc, _ = raw_call(eng, dev(vals), dev(offs), dev(keys), want_src=True)
    assert rc == 0 and need == 400
    assert host(ov)[:400].tolist() == wv and host(oro).tolist() == wo
    assert host(osrc)[:400].tolist() == ws


# ---- keys ----

def test_all_keys_equal_across_three_tiles(eng):
    n = 2 * TILE + 700
    vals = np.arange(n, dtype=U64)[::-1].copy()
    keys = np.full(n, 42, dtype=U64)
    for flags in (0, DESC):                                  # position order both ways
        gv, _, gs = check(eng, vals, [0, n], keys, None, flags)
        assert np.array_equal(gs, np.arange(n, dtype=U64))
    gv, go, _ = check(eng, vals, [0, n], keys, None, MULTI, count=1, offset=n // 2)
    assert gv.size == n                                      # MULTI swallows the row
    has = np.ones(n, dtype=np.uint8)
    has[-100:] = 0
    gv, go, _ = check(eng, vals, [0, n], keys, has, MULTI | DESC, count=1, offset=5)
    assert gv.size == n - 100


def test_extreme_keys(eng):
    rng = np.random.default_rng(29)
    n = TILE + 900
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    vals[:4] = [0, 2**64 - 1, 0, 2**64 - 1]                  # ordinary uids too
    offs = offsets([700, n - 700])
    k01 = np.where(rng.random(n) < 0.5, U64(0), U64(2**64 - 1))
    around = (U64(2**63) + rng.integers(-3, 3, size=n).astype(np.int64).view(U64))
    has = (rng.random(n) < 0.5).astype(np.uint8)
    for keys in (k01, around):
        for flags in FLAGSETS:
            check(eng, vals, offs, keys, None, flags)
            check(eng, vals, offs, keys, has, flags, count=4, offset=2)


def test_nulls(eng):
    rng = np.random.default_rng(31)
    n = TILE + 333
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    keys = rng.integers(0, 9, size=n).astype(U64)
    offs = offsets([5, 0, 1200, n - 1205])
    allnull = np.zeros(n, dtype=np.uint8)
    half = (np.arange(n) % 2).astype(np.uint8)               # interleaved, density 1/2
    for has in (None, allnull, half):
        for flags in FLAGSETS:
            check(eng, vals, offs, keys, has, flags)
            check(eng, vals, offs, keys, has, flags, count=6, offset=600)


def test_unsorted_rows_with_duplicate_uids(eng):
    rng = np.random.default_rng(37)
    lens = rng.integers(0, 300, size=40)
    offs = offsets(lens)
    n = int(offs[-1])
    vals = rng.integers(0, 20, size=n).astype(U64)           # many duplicates, no order
    keys = rng.integers(0, 5, size=n).astype(U64)
    has = (rng.random(n) < 0.6).astype(np.uint8)
    for flags in FLAGSETS:
        check(eng, vals, offs, keys, has, flags, count=0, offset=0)
        check(eng, vals, offs, keys, has, flags, count=7, offset=2)


# ---- pages ----

PAGES = [(0, 0), (5, 0), (5, 3), (0, 7), (-4, 0), (-10**6, 0), (3, 10**6), (5, -2),
         (INT32_MAX, INT32_MAX), (INT32_MIN, 0)]


@pytest.fixture(scope="module")
def page_matrix():
    rng = np.random.default_rng(41)
    lens = list(range(0, 41)) + list(rng.integers(0, 41, size=30))
    offs = offsets(lens)
    n = int(offs[-1])
    vals = rng.integers(0, 2**64, size=n, dtype=U64)
    keys = rng.integers(0, 3, size=n).astype(U64)           # equal runs on both page edges
    has = (rng.random(n) < 0.75).astype(np.uint8)
    return vals, offs, keys, has


@pytest.mark.parametrize("flags", FLAGSETS)
def test_pages(eng, page_matrix, flags):
    vals, offs, keys, has = page_matrix
    for count, offset in PAGES:
        check(eng, vals, offs, keys, has, flags, count, offset)
        check(eng, vals, offs, keys, None, flags, count, offset)


def test_hand_cases_through_the_engine(eng):
    for _, vals, offs, keys, has, flags, count, offset, wv, wo, ws, wm in HAND:
        gv, go, gs = check(eng, vals, offs, keys, has, flags, count, offset)
        assert gv.tolist() == wv and go.tolist() == wo and gs.tolist() == ws


# ---- forms ----

def test_page_only_is_page_range_slicing(eng, page_matrix):
    vals, offs, _, _ = page_matrix
    for count, offset in PAGES:
        got_v, got_o = eng.paginate_rows(dev(vals), dev(offs), count, offset)
        want = []
        for r in range(len(offs) - 1):
            a, b = int(offs[r]), int(offs[r + 1])
            s, e = ref.page_range(count, offset, b - a)
            want.append(vals[a + s:a + e])
        assert np.array_equal(host(got_v), np.concatenate(want))
        assert host(got_o).tolist() == [0] + list(np.cumsum([w.size for w in want]))
        check(eng, vals, offs, None, None, 0, count, offset)
    eng.stats_reset()
    eng.paginate_rows(dev(vals), dev(offs), 5, 3)
    assert eng.stats()["launches"] == 5                      # page, two scan kernels, offsets, write


def test_count_only_equals_the_full_call(eng, page_matrix):
    vals, offs, keys, has = page_matrix
    dv, do, dk, dh = dev(vals), dev(offs), dev(keys), dev(has, np.uint8)
    n = vals.size
    for flags in FLAGSETS:
        for count, offset in ((0, 0), (5, 3), (-4, 0)):
            kw = dict(keys=dk, has=dh, count=count, offset=offset, desc=bool(flags & DESC),
                      multi=bool(flags & MULTI), drop_nulls=bool(flags & DROP_NULLS))
            full = eng.sort_rows(dv, do, **kw)
            eng.stats_reset()
            only = eng.sort_rows(dv, do, count_only=True, **kw)
            launches = eng.stats()["launches"]
            assert only[0].numel() == 0
            assert torch.equal(only[1], full[1])
            if flags & MULTI:
                assert torch.equal(only[2], full[2])
            # the order decides the lengths only under MULTI and DROP_NULLS
            needs_sort = bool(flags & (MULTI | DROP_NULLS))
            assert launches == (6 + rounds_of(n) if needs_sort else 4)
    only = eng.sort_rows(dv, do, count=5, offset=3, count_only=True)
    assert torch.equal(only[1], eng.paginate_rows(dv, do, 5, 3)[1])


def test_short_capacity(eng, page_matrix):
    vals, offs, keys, has = page_matrix
    dv, do, dk, dh = dev(vals), dev(offs), dev(keys), dev(has, np.uint8)
    rc, need, ov, oro, osrc, guard = raw_call(eng, dv, do, dk, dh, DESC, count=5, offset=1,
                                              want_src=True)
    assert rc == 0 and 0 < need < vals.size
    assert int(ov[need].item()) == guard                     # exact capacity is enough
    rc2, need2, ov2, oro2, osrc2, _ = raw_call(eng, dv, do, dk, dh, DESC, count=5, offset=1,
                                               cap=need - 1, want_src=True)
    assert rc2 == 3 and need2 == need                        # UA_ERR_INVALID, total complete
    assert torch.equal(oro2, oro)                            # offsets complete
    assert int(ov2[need - 1].item()) == guard                # the word past the capacity
    assert int(osrc2[need - 1].item()) == guard
    assert torch.equal(ov2[:need - 1], ov[:need - 1])
    rc3, need3, ov3, oro3, _, _ = raw_call(eng, dv, do, dk, dh, DESC, count=5, offset=1, cap=need)
    assert rc3 == 0 and need3 == need and torch.equal(ov3[:need], ov[:need])
    with pytest.raises(ValueError):
        eng.sort_rows(dv, do, keys=dk, out_vals=torch.empty(3, dtype=torch.int64, device="cuda:0"))


def test_out_src_absent_and_present_agree(eng, page_matrix):
    vals, offs, keys, has = page_matrix
    dv, do, dk, dh = dev(vals), dev(offs), dev(keys), dev(has, np.uint8)
    a = eng.sort_rows(dv, do, keys=dk, has=dh, count=7, offset=2, desc=True)
    b = eng.sort_rows(dv, do, keys=dk, has=dh, count=7, offset=2, desc=True, want_src=True)
    assert len(a) == 2 and len(b) == 3
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(dv[b[2]], b[0])


def test_host_form_equals_the_device_form(eng, page_matrix):
    vals, offs, keys, has = page_matrix
    rows = [vals[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]
    krows = [[int(k) if h else None for k, h in
              zip(keys[int(offs[r]):int(offs[r + 1])], has[int(offs[r]):int(offs[r + 1])])]
             for r in range(len(offs) - 1)]
    for flags in FLAGSETS:
        gv, go, gs = check(eng, vals, offs, keys, has, flags, count=4, offset=1)
        out, ms, src = algo.sort_uid_matrix(
            eng, rows, krows, count=4, offset=1, desc=bool(flags & DESC),
            multi=bool(flags & MULTI), drop_nulls=bool(flags & DROP_NULLS), want_src=True)
        assert np.array_equal(np.concatenate(out), gv)
        assert np.array_equal(np.concatenate(src), gs)
        assert [o.size for o in out] == np.diff(go.astype(np.int64)).tolist()
        if flags & MULTI:
            assert ms == ref.sort_rows(vals, offs, keys, has, flags, 4, 1)[3]
        else:
            assert ms == []
    paged = algo.paginate_uid_matrix(eng, rows, 3, 2)
    assert [p.tolist() for p in paged] == [r[2:5].tolist() for r in rows]
    assert algo.sort_uid_matrix(eng, [], [])[0] == []


def test_stats_bytes_follow_the_documented_formula(eng, page_matrix):
    vals, offs, keys, has = page_matrix
    dv, do, dk, dh = dev(vals), dev(offs), dev(keys), dev(has, np.uint8)
    n, nro = vals.size, offs.size
    eng.stats_reset()
    out = eng.sort_rows(dv, do, keys=dk, has=dh, count=5, want_src=True)
    st = eng.stats()
    assert st["launches"] == 7 + rounds_of(n)
    assert st["bytes_algorithmic"] == 8 * n + 8 * n + n + 16 * nro + 16 * out[0].numel()
    eng.stats_reset()
    out = eng.paginate_rows(dv, do, 5, 0)
    assert eng.stats()["bytes_algorithmic"] == 8 * n + 16 * nro + 8 * out[0].numel()


# ---- chain ----

def test_sorted_pages_feed_union_rows(eng):
    rng = np.random.default_rng(43)
    lens = rng.integers(0, 500, size=60)
    offs = offsets(lens)
    n = int(offs[-1])
    vals = rng.integers(1, 5000, size=n).astype(U64)
    keys = rand_keys(rng, n)
    ov, oo = eng.sort_rows(dev(vals), dev(offs), keys=dev(keys), count=10, offset=2)
    dest = host(eng.union_rows(ov))
    wv = ref.sort_rows(vals, offs, keys, None, 0, 10, 2)[0]
    assert dest.tolist() == sorted(set(wv))


def test_sortpath_csr_form_against_the_oracle(eng):
    rng = np.random.default_rng(47)
    rows, keymap = [], {}
    for _ in range(40):
        row = np.unique(rng.integers(1, 4000, size=int(rng.integers(0, 120))).astype(U64))
        rows.append(row)
    offs = offsets([r.size for r in rows])
    vals = np.concatenate(rows)
    for multi in (False, True):
        for u in np.unique(vals):
            null = (not multi) and rng.random() < 0.3         # the oracle's agreeing domain
            keymap[int(u)] = None if null else int(rng.integers(0, 6))
        keys = np.array([keymap[int(u)] or 0 for u in vals], dtype=U64)
        has = np.array([keymap[int(u)] is not None for u in vals], dtype=np.uint8)
        for desc in (False, True):
            for count, offset in ((0, 0), (5, 3), (-4, 0), (3, 1)):
                want_rows, want_ms = sortref.sort_without_index(
                    rows, keymap.get, offset, count, desc=desc, multi=multi)
                ov, oo, ms = sortpath.sort_rows_without_index(
                    eng, dev(vals), dev(offs), dev(keys), dev(has, np.uint8), offset, count,
                    desc=desc, multi=multi)
                gv, go = host(ov), host(oo)
                got = [gv[int(go[r]):int(go[r + 1])].tolist() for r in range(len(rows))]
                assert got == [list(map(int, r)) for r in want_rows]
                if multi:
                    assert host(ms).tolist() == want_ms
                else:
                    assert ms is None
