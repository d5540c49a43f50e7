"""GPU parity of the row-wise UID-matrix filter (Engine.filter_rows,
update_uid_matrix): every row of a CSR matrix filtered by membership in one
shared sorted list.  Expected values come from the CPU oracle (and numpy's
isin where the oracle would be slow); every comparison is exact.

The shapes are the smallest that reach each boundary the kernels have: the
64-lane ballot word, the 2048-element tile, the 1024-entry pivot table and a
pivot stride above 1 (m > 1024), including one that is not a power of two.
"""
import numpy as np
import pytest
import torch

from dgraph_amd import algo, synth
from oracle import bind as orc

pytestmark = pytest.mark.gpu

MODES = [algo.ROWS_INTERSECT, algo.ROWS_DIFFERENCE]


def to_dev(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size == 0:
        return torch.empty(0, dtype=torch.int64, device="cuda:0")
    return torch.from_numpy(a.view(np.int64)).to("cuda:0")


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def csr(rows):
    rows = [np.asarray(r, dtype=np.uint64) for r in rows]
    offs = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        offs[1:] = np.cumsum([r.size for r in rows], dtype=np.uint64)
    vals = np.concatenate(rows) if rows else np.empty(0, dtype=np.uint64)
    return vals.astype(np.uint64), offs


def run_rows(eng, rows, shared, mode):
    """filter_rows over a list of host rows -> (list of host rows, offsets)."""
    vals, offs = csr(rows)
    out, out_offs = eng.filter_rows(to_dev(vals), to_dev(offs), to_dev(shared), mode)
    out, out_offs = to_np(out), to_np(out_offs)
    assert out_offs.size == len(rows) + 1
    assert out_offs[0] == 0 and out_offs[-1] == out.size
    assert np.all(np.diff(out_offs.astype(np.int64)) >= 0)
    return [out[int(out_offs[r]):int(out_offs[r + 1])] for r in range(len(rows))], out_offs


def assert_rows_equal(got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, np.asarray(w, dtype=np.uint64)), f"row {r}"


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


# ---------- 1. known answers ----------

KNOWN_ROWS = [[1, 2, 3], [], [2], [0, 5], [3, 5], [1, 2, 3, 4, 5]]
KNOWN_SHARED = [1, 2, 3]
KNOWN_WANT = {
    algo.ROWS_INTERSECT: [[1, 2, 3], [], [2], [], [3], [1, 2, 3]],
    algo.ROWS_DIFFERENCE: [[], [], [], [0, 5], [5], [4, 5]],
}


def check_known(eng):
    for mode in MODES:
        got, _ = run_rows(eng, KNOWN_ROWS, KNOWN_SHARED, mode)
        assert_rows_equal(got, KNOWN_WANT[mode])


def test_known_answers(eng):
    check_known(eng)


@pytest.mark.parametrize("ordered", [False, True])
def test_known_answers_host_path(eng, ordered):
    for mode in MODES:
        got = algo.update_uid_matrix(eng, KNOWN_ROWS, KNOWN_SHARED, ordered=ordered,
                                     mode=mode)
        assert_rows_equal(got, KNOWN_WANT[mode])
    assert algo.update_uid_matrix(eng, [], KNOWN_SHARED) == []


# ---------- 2. parity vs the oracle, sorted duplicate-free rows ----------

ROW_LENS = [0, 1, 63, 64, 65, 0, 0, 2047, 2048, 2049, 5000, 0]


@pytest.mark.parametrize("m", [0, 1, 2, 1023, 1024, 1025, 2048, 2049, 100_000, 1_500_001])
def test_parity_sorted_rows(eng, m):
    """total = 11337: no multiple of 64 or 2048; first and last rows empty."""
    rng = np.random.default_rng(synth.SEED + m)
    limit = max(int(m / 0.3), 16)  # ~30% of a row's values are members
    shared = synth.gen_sorted_unique(rng, m, limit)
    rows = [synth.gen_sorted_unique(rng, n, limit) for n in ROW_LENS]
    got_i, _ = run_rows(eng, rows, shared, algo.ROWS_INTERSECT)
    got_d, _ = run_rows(eng, rows, shared, algo.ROWS_DIFFERENCE)
    assert_rows_equal(got_i, [orc.intersect_with(r, shared) for r in rows])
    assert_rows_equal(got_d, [orc.difference(r, shared) for r in rows])


# ---------- 3. u64 extremes ----------

def test_u64_extremes_small(eng):
    top = (1 << 64) - 1
    b63 = 1 << 63
    shared = np.array([0, 7, b63 - 1, b63, b63 + 9, top - 1, top], dtype=np.uint64)
    rows = [np.array([0, 5, b63, b63 + 7, top], dtype=np.uint64),
            np.array([top, 0, b63 - 1, 1, top - 1], dtype=np.uint64),
            np.array([b63 + 9, b63 + 8, 7, 8], dtype=np.uint64)]
    for mode in MODES:
        got, _ = run_rows(eng, rows, shared, mode)
        want = [r[np.isin(r, shared) == (mode == algo.ROWS_INTERSECT)] for r in rows]
        assert_rows_equal(got, want)
    got, _ = run_rows(eng, rows, shared, algo.ROWS_INTERSECT)
    assert got[0].tolist() == [0, b63, top]
    assert got[1].tolist() == [top, 0, b63 - 1, top - 1]


def test_u64_extremes_strided(eng):
    """m > 1024, so members on both sides of bit 63 are found by the global
    bracket search, and 0 / 2**64-1 are the first and last pivots' ends."""
    rng = np.random.default_rng(synth.SEED + 63)
    low = synth.gen_sorted_unique(rng, 6000, 1 << 20)
    pool = np.unique(np.concatenate([
        low[:3000], low[3000:] | np.uint64(1 << 63),
        np.array([0, (1 << 64) - 1], dtype=np.uint64)]))
    member = rng.random(pool.size) < 0.5
    member[0] = member[-1] = True
    shared = pool[member]
    assert shared.size > 2048 and shared[0] == 0 and shared[-1] == (1 << 64) - 1
    rows = [pool[:2500], pool[2500:], pool[::7], np.array([0, (1 << 64) - 1], dtype=np.uint64)]
    got_i, _ = run_rows(eng, rows, shared, algo.ROWS_INTERSECT)
    got_d, _ = run_rows(eng, rows, shared, algo.ROWS_DIFFERENCE)
    assert_rows_equal(got_i, [orc.intersect_with(r, shared) for r in rows])
    assert_rows_equal(got_d, [orc.difference(r, shared) for r in rows])
    assert got_i[3].tolist() == [0, (1 << 64) - 1]


# ---------- 4. unsorted rows with duplicates (the ordered branch) ----------

@pytest.mark.parametrize("m", [700, 3000])
def test_unsorted_rows_with_duplicates(eng, m):
    rng = np.random.default_rng(synth.SEED + 4 + m)
    limit = 3 * m
    shared = synth.gen_sorted_unique(rng, m, limit)
    rows = [rng.integers(0, limit, size=n, dtype=np.uint64)
            for n in [0, 5, 64, 100, 2048, 3000, 1]]
    rows[3][:50] = rows[3][50:]  # guaranteed repeats
    for mode in MODES:
        got, _ = run_rows(eng, rows, shared, mode)
        want = [orc.apply_filter(r, np.isin(r, shared) == (mode == algo.ROWS_INTERSECT))
                for r in rows]
        assert_rows_equal(got, want)
    got = algo.update_uid_matrix(eng, rows, shared, ordered=True)
    assert_rows_equal(got, [orc.apply_filter(r, np.isin(r, shared)) for r in rows])


# ---------- 5. boundary density and skew ----------

def test_boundary_density_and_skew(eng):
    rng = np.random.default_rng(synth.SEED + 5)
    m, limit = 1_000_000, 3_300_000
    shared = synth.gen_sorted_unique(rng, m, limit)
    small_lens = rng.integers(0, 6, size=20_000)
    lens = np.concatenate([[300_000], np.zeros(5_000, dtype=np.int64), small_lens])
    offs = np.zeros(lens.size + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    big = synth.gen_sorted_unique(rng, 300_000, limit)
    small = rng.permutation(synth.gen_sorted_unique(rng, int(small_lens.sum()), limit))
    row_id = np.repeat(np.arange(small_lens.size), small_lens)
    small = small[np.lexsort((small, row_id))]  # sorted inside each row
    vals = np.concatenate([big, small]).astype(np.uint64)
    member = np.isin(vals, shared)
    dv, do, ds = to_dev(vals), to_dev(offs), to_dev(shared)
    spot = np.concatenate([[0, 1, 5_000, 5_001, lens.size - 1],
                           rng.integers(5_001, lens.size, size=195)])
    for mode in MODES:
        keep = member if mode == algo.ROWS_INTERSECT else ~member
        want_offs = np.concatenate([[0], np.cumsum(keep)])[offs.astype(np.int64)]
        out, out_offs = eng.filter_rows(dv, do, ds, mode)
        out, out_offs = to_np(out), to_np(out_offs)
        assert np.all(np.diff(out_offs.astype(np.int64)) >= 0)
        assert out_offs[-1] == out.size
        assert np.array_equal(out_offs, want_offs.astype(np.uint64))
        assert np.array_equal(out, vals[keep])
        ref = orc.intersect_with if mode == algo.ROWS_INTERSECT else orc.difference
        for r in spot:
            row = vals[int(offs[r]):int(offs[r + 1])]
            got = out[int(out_offs[r]):int(out_offs[r + 1])]
            assert np.array_equal(got, ref(row, shared)), f"row {r}"


# ---------- 6. degenerate and error paths ----------

def test_degenerate_and_errors(eng):
    shared = to_dev(KNOWN_SHARED)
    out, offs = eng.filter_rows(to_dev([]), to_dev([0]), shared)
    assert out.numel() == 0 and to_np(offs).tolist() == [0]

    for mode in MODES:
        out, offs = eng.filter_rows(to_dev([]), to_dev([0] * 8), shared, mode)
        assert out.numel() == 0 and to_np(offs).tolist() == [0] * 8

    vals, row_offs = csr(KNOWN_ROWS)
    dv, do = to_dev(vals), to_dev(row_offs)
    with pytest.raises(RuntimeError, match="uidalgo error 3"):  # UA_ERR_INVALID
        eng.filter_rows(dv, do, shared, out_vals=dv)
    with pytest.raises(RuntimeError, match="uidalgo error 3"):
        eng.filter_rows(dv, do, shared, out_row_offs=do)
    with pytest.raises(RuntimeError, match="uidalgo error 3"):
        eng.filter_rows(dv, do, shared, mode=2)
    with pytest.raises(ValueError):
        eng.filter_rows(dv, do, shared,
                        out_vals=torch.empty(vals.size - 1, dtype=torch.int64,
                                             device="cuda:0"))
    assert to_np(dv).tolist() == vals.tolist()  # rejected calls wrote nothing
    check_known(eng)


# ---------- 7. agreement with the existing pair path ----------

def test_agrees_with_pair_path(eng):
    rng = np.random.default_rng(synth.SEED + 7)
    m, limit = 50_000, 160_000
    shared = synth.gen_sorted_unique(rng, m, limit)
    rows = [synth.gen_sorted_unique(rng, int(n), limit)
            for n in rng.integers(1, 3000, size=64)]
    got, _ = run_rows(eng, rows, shared, algo.ROWS_INTERSECT)
    ds = to_dev(shared)
    outs, lens = eng.intersect_pairs([to_dev(r) for r in rows], [ds] * 64)
    assert_rows_equal(got, [to_np(o[:n]) for o, n in zip(outs, lens)])
