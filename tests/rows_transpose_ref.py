"""Pure-Python restatement of ua_rows_transpose_dev (include/uidalgo.h): a dict
of lists filled in flat input order, exactly as dedup.addValue
(query/groupby.go:104-128) appends one srcUid per edge, then the keys sorted.

Defined for a non-decreasing row_offs; entries are clamped to total, and
elements at or past min(row_offs[n_rows], total) belong to no row.
"""

UA_OK = 0
UA_ERR_INVALID = 3
MASK = (1 << 64) - 1


def live_elements(row_offs, total, row_keep=None):
    """[(flat index, row)] of the elements that take part, in flat order."""
    n_rows = len(row_offs) - 1
    if n_rows <= 0:
        return []
    offs = [min(int(x), total) for x in row_offs]
    out = []
    for r in range(n_rows):
        if row_keep is not None and not row_keep[r]:
            continue
        for i in range(offs[r], offs[r + 1]):
            out.append((i, r))
    return out


def transpose(vals, row_offs, total=None, row_uids=None, row_keep=None, unique=False):
    """Returns (keys, offs, out_vals, out_src) as lists of ints: keys ascending
    as unsigned 64-bit, offs the CSR offsets of the groups (len(keys) + 1),
    out_vals the payload row_uids[r] (or r) of every entry and out_src its flat
    input index.  unique keeps, of the entries with the same (value, row), the
    one with the lowest flat index."""
    if total is None:
        total = len(vals)
    groups = {}
    seen = set()
    for i, r in live_elements(row_offs, total, row_keep):
        v = int(vals[i]) & MASK
        if unique:
            if (v, r) in seen:
                continue
            seen.add((v, r))
        payload = int(row_uids[r]) & MASK if row_uids is not None else r
        groups.setdefault(v, []).append((payload, i))     # addValue's append
    keys = sorted(groups)
    offs, out_vals, out_src = [0], [], []
    for k in keys:
        for payload, i in groups[k]:
            out_vals.append(payload)
            out_src.append(i)
        offs.append(len(out_vals))
    return keys, offs, out_vals, out_src


def groups_of(vals, row_offs, **kw):
    """[(key, [payload...])...]: the shape formGroups consumes at depth 1."""
    keys, offs, out_vals, _ = transpose(vals, row_offs, **kw)
    return [(k, out_vals[offs[g]:offs[g + 1]]) for g, k in enumerate(keys)]


def capacity_rc(n_groups, n_entries, cap_keys, cap_vals, have_keys, have_vals):
    """The status of a call that passed the argument checks: a short capacity
    of an output that is present is UA_ERR_INVALID."""
    short = (have_keys and n_groups > cap_keys) or (have_vals and n_entries > cap_vals)
    return UA_ERR_INVALID if short else UA_OK


def bounded(keys, offs, out_vals, out_src, cap_keys, cap_vals):
    """What a call stores under the capacities: keys below cap_keys, group
    offsets below cap_keys + 1, entries below cap_vals."""
    return keys[:cap_keys], offs[:cap_keys + 1], out_vals[:cap_vals], out_src[:cap_vals]


def launches(total, form):
    """The header's launch-count formula; form is 'full', 'groups' or 'count'."""
    if total == 0:
        return 0
    ntiles = (total + 2047) // 2048
    rounds = 0
    while (1 << rounds) < ntiles:
        rounds += 1
    return (2 if form == "count" else 5) + rounds
