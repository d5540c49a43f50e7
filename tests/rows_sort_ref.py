"""Pure-Python restatement of ua_rows_sort_dev's semantics (include/uidalgo.h):
order and pagination of every row of a CSR UID matrix.

Restates x.PageRange (x/x.go:815-844), sortByValue's V-then-N order
(worker/sort.go:775-821, :813), sortAndPaginateUsingVar's dropped nulls with
its empty-V `continue` (query/query.go:2709-2720), paginate's multi-sort
extension (worker/sort.go:748-769) over the valued run only, the permutation
`src` and multiSortOffsets (worker/sort.go:170-178).

Ties among equal keys are ordered by input position ascending, asc and desc
alike.  A null equals nothing, so the multi extension never moves an edge
inside the null tail (oracle/sortref.py treats two nulls as equal there)."""

DESC, MULTI, DROP_NULLS = 1, 2, 4
U64_MAX = (1 << 64) - 1


def page_range(count, offset, n):
    """x.PageRange, word for word."""
    if n == 0:
        return 0, 0
    if count == 0 and offset == 0:
        return 0, n
    if count < 0:
        if count * -1 > n:
            count = -n
        return (((n + count) % n) + n) % n, n
    start = offset
    if start < 0:
        start = 0
    if start > n:
        return n, n
    if count == 0:
        return start, n
    end = start + count
    if end > n:
        end = n
    return start, end


def sort_row(n, keys, has, flags, count, offset):
    """One row of n elements.  keys/has: sequences of n (keys None = page
    only, has None = all valued).  Returns (positions, ms_off): the row-local
    input positions of the output row, in order, and multiSortOffsets."""
    if keys is None:
        s = list(range(n))
        nv = n
        skeys = None
    else:
        hv = [True] * n if has is None else [bool(h) for h in has]
        desc = bool(flags & DESC)
        v = [i for i in range(n) if hv[i]]
        v.sort(key=lambda i: ((U64_MAX - int(keys[i])) if desc else int(keys[i]), i))
        nulls = [i for i in range(n) if not hv[i]]
        nv = len(v)
        if flags & DROP_NULLS:
            s = v if v else list(range(n))
        else:
            s = v + nulls
        skeys = [int(keys[i]) for i in v]
    start, end = page_range(count, offset, len(s))
    if flags & MULTI:
        while 0 < start < nv and skeys[start] == skeys[start - 1]:
            start -= 1
        while 0 < end < nv and skeys[end - 1] == skeys[end]:
            end += 1
    ms = offset - start if start < offset else 0
    return s[start:end], ms


def sort_rows(vals, row_offs, keys=None, has=None, flags=0, count=0, offset=0):
    """The whole call over a well-formed CSR matrix.  Returns (out_vals,
    out_row_offs, out_src, ms_offs) as Python lists; ms_offs holds one entry
    per row whatever the flags (the engine delivers it under MULTI only)."""
    n_rows = len(row_offs) - 1
    out_vals, out_src, out_offs, ms_offs = [], [], [0], []
    for r in range(n_rows):
        a, b = int(row_offs[r]), int(row_offs[r + 1])
        pos, ms = sort_row(b - a, None if keys is None else keys[a:b],
                           None if has is None else has[a:b], flags, count, offset)
        out_vals.extend(int(vals[a + p]) for p in pos)
        out_src.extend(a + p for p in pos)
        out_offs.append(len(out_vals))
        ms_offs.append(ms)
    return out_vals, out_offs, out_src, ms_offs
