"""tests/rows_sort_ref.py against hand-written rows for every rule of
ua_rows_sort_dev (include/uidalgo.h), and against oracle.sortref's
sort_without_index over the domain where the two agree: uid-sorted rows with
32-bit keys, asc and desc, with and without nulls for multi=False; rows
without nulls for multi=True (the oracle treats two nulls as equal, the call
does not)."""
import numpy as np
import pytest

import rows_sort_ref as ref
from oracle import sortref
from rows_sort_ref import DESC, DROP_NULLS, MULTI

INT32_MAX, INT32_MIN = 2**31 - 1, -2**31

# (name, vals, row_offs, keys, has, flags, count, offset,
#  want_vals, want_offs, want_src, want_ms)
HAND = [
    ("page only keeps input order",
     [9, 3, 7, 3, 1], [0, 5], None, None, 0, 2, 1,
     [3, 7], [0, 2], [1, 2], [0]),
    ("asc, ties by position",
     [10, 11, 12, 13], [0, 4], [5, 2, 5, 2], None, 0, 0, 0,
     [11, 13, 10, 12], [0, 4], [1, 3, 0, 2], [0]),
    ("desc, ties by position ascending too",
     [10, 11, 12, 13], [0, 4], [5, 2, 5, 2], None, DESC, 0, 0,
     [10, 12, 11, 13], [0, 4], [0, 2, 1, 3], [0]),
    ("nulls appended in input order, asc",
     [1, 2, 3, 4, 5], [0, 5], [9, 0, 4, 0, 1], [1, 0, 1, 0, 1], 0, 0, 0,
     [5, 3, 1, 2, 4], [0, 5], [4, 2, 0, 1, 3], [0]),
    ("nulls appended after the valued, desc as well",
     [1, 2, 3, 4, 5], [0, 5], [9, 0, 4, 0, 1], [1, 0, 1, 0, 1], DESC, 0, 0,
     [1, 3, 5, 2, 4], [0, 5], [0, 2, 4, 1, 3], [0]),
    ("0 and UINT64_MAX are ordinary keys, desc",
     [1, 2, 3], [0, 3], [0, ref.U64_MAX, 0], None, DESC, 0, 0,
     [2, 1, 3], [0, 3], [1, 0, 2], [0]),
    ("drop nulls pages over V",
     [1, 2, 3, 4, 5], [0, 5], [9, 0, 4, 0, 1], [1, 0, 1, 0, 1], DROP_NULLS, 2, 1,
     [3, 1], [0, 2], [2, 0], [0]),
    ("drop nulls with an all-null row: the row stays, then pages",
     [7, 5, 6, 1, 2], [0, 3, 5], [1, 1, 1, 8, 3], [0, 0, 0, 1, 1], DROP_NULLS, 2, 0,
     [7, 5, 2, 1], [0, 2, 4], [0, 1, 4, 3], [0, 0]),
    ("count < 0 takes the last, offset ignored",
     [1, 2, 3, 4, 5], [0, 5], None, None, 0, -2, 3,
     [4, 5], [0, 2], [3, 4], [0]),
    ("count < -n clamps to the row",
     [1, 2, 3], [0, 3], None, None, 0, -10, 0,
     [1, 2, 3], [0, 3], [0, 1, 2], [0]),
    ("offset < 0 counts as 0",
     [1, 2, 3], [0, 3], None, None, 0, 2, -5,
     [1, 2], [0, 2], [0, 1], [0]),
    ("offset > len gives an empty page",
     [1, 2, 3], [0, 3], None, None, 0, 2, 4,
     [], [0, 0], [], [4 - 3]),
    ("count == 0 runs to the end",
     [1, 2, 3, 4], [0, 4], None, None, 0, 0, 3,
     [4], [0, 1], [3], [0]),
    ("empty rows between rows",
     [1, 2, 3], [0, 0, 2, 2, 3, 3], None, None, 0, 1, 0,
     [1, 3], [0, 0, 1, 1, 2, 2], [0, 2], [0, 0, 0, 0, 0]),
    ("multi grows both edges over equal keys",
     [1, 2, 3, 4, 5, 6], [0, 6], [1, 2, 2, 2, 2, 3], None, MULTI, 1, 2,
     [2, 3, 4, 5], [0, 4], [1, 2, 3, 4], [1]),
    ("multi: page edge at the valued/null boundary does not enter the nulls",
     [1, 2, 3, 4, 5], [0, 5], [4, 4, 4, 0, 0], [1, 1, 1, 0, 0], MULTI, 2, 1,
     [1, 2, 3], [0, 3], [0, 1, 2], [1]),
    ("multi: a start at the boundary stays (a null equals nothing)",
     [1, 2, 3, 4, 5], [0, 5], [4, 4, 4, 0, 0], [1, 1, 1, 0, 0], MULTI, 1, 3,
     [4], [0, 1], [3], [0]),
    ("multi: both edges inside the null tail stay",
     [1, 2, 3, 4, 5, 6], [0, 6], [4, 4, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], MULTI, 2, 3,
     [4, 5], [0, 2], [3, 4], [0]),
    ("multi: ms_offs is offset - start after the extension",
     [1, 2, 3, 4], [0, 4], [7, 7, 7, 7], None, MULTI, 1, 3,
     [1, 2, 3, 4], [0, 4], [0, 1, 2, 3], [3]),
    ("unsorted row with duplicate uids",
     [5, 5, 2, 5], [0, 4], [3, 1, 2, 1], None, 0, 3, 0,
     [5, 5, 2], [0, 3], [1, 3, 2], [0]),
]


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(case):
    _, vals, offs, keys, has, flags, count, offset, wv, wo, ws, wm = case
    got = ref.sort_rows(vals, offs, keys, has, flags, count, offset)
    assert got[0] == wv
    assert got[1] == wo
    assert got[2] == ws
    assert got[3] == wm


def test_page_range_matches_the_oracle_everywhere():
    vals = (0, 1, 2, 3, 5, 7, -1, -2, -4, -7, 10**6, -10**6, INT32_MAX, INT32_MIN)
    for n in range(0, 8):
        for count in vals:
            for offset in vals:
                assert ref.page_range(count, offset, n) == \
                    sortref.page_range(count, offset, n), (count, offset, n)
                s, e = ref.page_range(count, offset, n)
                assert 0 <= s <= e <= n


def _matrix(rng, n_rows, max_len, null_density):
    rows, keymap = [], {}
    for _ in range(n_rows):
        n = int(rng.integers(0, max_len + 1))
        row = np.unique(rng.integers(1, 500, size=n).astype(np.uint64))
        rows.append(row)
        for u in row:
            u = int(u)
            if u not in keymap:  # few distinct keys: equal runs on the page edges
                keymap[u] = None if rng.random() < null_density else int(rng.integers(0, 4))
    return rows, keymap


PAGES = [(0, 0), (5, 0), (5, 3), (0, 7), (-4, 0), (3, 100), (5, -2), (2, 1)]


def test_agrees_with_the_oracle_on_the_shared_domain():
    rng = np.random.default_rng(20240611)
    checked = skipped = 0
    for trial in range(24):
        for multi in (False, True):
            density = 0.0 if multi else (0.0, 0.3, 1.0)[trial % 3]
            rows, keymap = _matrix(rng, 6, 24, density)
            for desc in (False, True):
                for count, offset in PAGES:
                    if multi and any(v is None for v in keymap.values()):
                        skipped += 1
                        continue
                    want_rows, want_ms = sortref.sort_without_index(
                        rows, keymap.get, offset, count, desc=desc, multi=multi)
                    vals = [int(u) for r in rows for u in r]
                    offs = [0]
                    for r in rows:
                        offs.append(offs[-1] + len(r))
                    keys = [keymap[u] or 0 for u in vals]
                    has = [keymap[u] is not None for u in vals]
                    flags = (DESC if desc else 0) | (MULTI if multi else 0)
                    gv, go, gs, gm = ref.sort_rows(vals, offs, keys, has, flags, count, offset)
                    got_rows = [gv[go[r]:go[r + 1]] for r in range(len(rows))]
                    assert got_rows == [list(map(int, r)) for r in want_rows]
                    assert [vals[s] for s in gs] == gv
                    if multi:
                        assert gm == want_ms
                    checked += 1
    assert skipped == 0  # the generator leaves the shared domain nowhere
    assert checked == 24 * 2 * 2 * len(PAGES)
