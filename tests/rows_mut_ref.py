"""What ua_rows_decode_mut_dev must return, in plain Python ints (a helper,
not a test): List.Uids on a list with a mutable layer, i.e. List.iterate's
merge (posting/list.go:1135-1251), stated as a set expression and not as a
transcription of the Go loop.

Per row, with P the pack's uids and M the row's (uid, op) slice:
  1. sorted((P - uids(M)) | S), S = the uids of M whose op is not MUT_DEL
  2. then x > after (0 keeps everything)
  3. then ListOptions.First, as rows_decode_ref.want_row
tests/test_rows_mut_ref.py holds this to the reference's own known answers
(tests/golden/mutation_layer.json) and to literals.
"""
import rows_decode_ref

MUT_SET, MUT_DEL, MUT_OVR = 1, 2, 3


def want_row(uids, muts, a=0, f=0):
    touched = {u for u, _ in muts}
    sets = {u for u, op in muts if op != MUT_DEL}
    merged = sorted((set(uids) - touched) | sets)
    return rows_decode_ref.want_row(merged, a, f)


def want_rows(lists, muts, afters=None, firsts=None):
    n = len(lists)
    afters = [0] * n if afters is None else afters
    firsts = [0] * n if firsts is None else firsts
    assert len(muts) == n and len(afters) == n and len(firsts) == n
    return [want_row(u, m, a, f) for u, m, a, f in zip(lists, muts, afters, firsts)]


def flat(muts):
    """Per-row (uid, op) lists -> (mut_uids, mut_ops, row_mut_base) as lists."""
    base = [0]
    for m in muts:
        base.append(base[-1] + len(m))
    return ([u for m in muts for u, _ in m], [op for m in muts for _, op in m], base)
