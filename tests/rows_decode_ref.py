"""What ua_rows_decode_dev must return, in plain Python ints (a helper, not a
test): List.Uids with Intersect == nil, posting/list.go:1786-1902.

Per row: the uids strictly above `after` (0 keeps everything, uid 0 included),
then ListOptions.First: the first f of them for f > 0, the last -f for f < 0,
all of them for f == 0.  tests/test_rows_decode_ref.py holds this to the
oracle and to literals.
"""


def want_row(uids, a=0, f=0):
    r = [x for x in uids if a == 0 or x > a]
    if f > 0:
        r = r[:f]
    elif f < 0:
        r = r[f:]
    return r


def want_rows(lists, afters=None, firsts=None):
    n = len(lists)
    afters = [0] * n if afters is None else afters
    firsts = [0] * n if firsts is None else firsts
    assert len(afters) == n and len(firsts) == n
    return [want_row(u, a, f) for u, a, f in zip(lists, afters, firsts)]
