"""What ua_rows_intersect_packed_dev must return, in plain Python ints (a
helper, not a test): algo.IntersectCompressedWith(pack, after, shared),
algo/uidlist.go:33, as List.Uids calls it when opts.Intersect != nil
(posting/list.go:1823-1829).

Per row: the uids with x >= after (INCLUSIVE: dec.Seek(afterUID, SeekStart),
codec.go:279-329; 0 keeps everything) that occur in shared.  No first.
tests/test_rows_isect_ref.py holds this to the oracle and to literals.
"""


def want_row(uids, shared, a=0):
    s = shared if isinstance(shared, (set, frozenset)) else set(shared)
    return [x for x in uids if x >= a and x in s]


def want_rows(lists, shared, afters=None):
    n = len(lists)
    afters = [0] * n if afters is None else afters
    assert len(afters) == n
    s = frozenset(shared)
    return [want_row(u, s, a) for u, a in zip(lists, afters)]
