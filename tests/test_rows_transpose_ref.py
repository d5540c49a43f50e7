"""tests/rows_transpose_ref.py against hand-written matrices: every rule of
ua_rows_transpose_dev's header comment with the expected output written out,
so the GPU test's reference is itself pinned."""
import rows_transpose_ref as ref

U64MAX = (1 << 64) - 1

# rebuildReverseEdges (posting/index.go:1759-1791) over the predicate
# `follows`: uid 0x10 follows 0x20, 0x30; 0x11 follows 0x30; 0x12 follows
# nobody; 0x13 follows 0x20, 0x30, 0x40.  Every forward posting (Entity = src,
# ValueId = dst) becomes one reverse posting (Entity = dst, ValueId = src).
FWD_UIDS = [0x10, 0x11, 0x12, 0x13]
FWD_ROWS = [[0x20, 0x30], [0x30], [], [0x20, 0x30, 0x40]]
REVERSE = [(0x20, [0x10, 0x13]), (0x30, [0x10, 0x11, 0x13]), (0x40, [0x13])]


def flat(rows):
    vals, offs = [], [0]
    for r in rows:
        vals += list(r)
        offs.append(len(vals))
    return vals, offs


def test_reverse_edges_by_hand():
    vals, offs = flat(FWD_ROWS)
    assert ref.groups_of(vals, offs, row_uids=FWD_UIDS, unique=True) == REVERSE
    keys, goffs, out, src = ref.transpose(vals, offs, row_uids=FWD_UIDS)
    assert keys == [0x20, 0x30, 0x40]
    assert goffs == [0, 2, 5, 6]                            # rule 4
    assert out == [0x10, 0x13, 0x10, 0x11, 0x13, 0x13]
    assert src == [0, 3, 1, 2, 4, 5]                        # the forward postings' positions
    # the transpose of the transpose is the matrix without its empty row
    back = ref.groups_of(out, goffs, row_uids=keys)
    assert back == [(0x10, [0x20, 0x30]), (0x11, [0x30]), (0x13, [0x20, 0x30, 0x40])]


def test_count_index_by_hand():
    # rebuildCountIndex (posting/index.go:1595-1640): one element per row, the
    # value is the list's length, the group the uids with that length
    uids = [5, 6, 7, 8, 9]
    lengths = [2, 0, 2, 7, 0]
    assert ref.groups_of(lengths, list(range(6)), row_uids=uids) == \
        [(0, [6, 9]), (2, [5, 7]), (7, [8])]


def test_row_index_payload_and_flat_order():
    # unsorted rows; rule 3: entries by flat index, payload the row index
    vals, offs = flat([[9, 3], [3, 9, 1], [9]])
    keys, goffs, out, src = ref.transpose(vals, offs)
    assert keys == [1, 3, 9]
    assert goffs == [0, 1, 3, 6]
    assert out == [1, 0, 1, 0, 1, 2]
    assert src == [4, 1, 2, 0, 3, 5]


def test_unsigned_order_of_the_keys():
    vals, offs = flat([[1 << 63, 0, U64MAX], [(1 << 63) - 1, 1, U64MAX]])
    keys, goffs, out, _ = ref.transpose(vals, offs)
    assert keys == [0, 1, (1 << 63) - 1, 1 << 63, U64MAX]   # rule 2
    assert goffs == [0, 1, 2, 3, 4, 6]
    assert out == [0, 1, 1, 0, 0, 1]


def test_multiplicity_and_unique():
    # rule 5: 7 three times in row 0 (flat 0, 2, 3) and twice in row 1 (5, 6)
    vals, offs = flat([[7, 4, 7, 7], [4, 7, 7]])
    keys, goffs, out, src = ref.transpose(vals, offs)
    assert (keys, goffs) == ([4, 7], [0, 2, 7])
    assert out == [0, 1, 0, 0, 0, 1, 1]
    assert src == [1, 4, 0, 2, 3, 5, 6]
    keys, goffs, out, src = ref.transpose(vals, offs, unique=True)
    assert (keys, goffs) == ([4, 7], [0, 2, 4])
    assert out == [0, 1, 0, 1]
    assert src == [1, 4, 0, 5]                              # the lowest flat index stays
    # on duplicate-free rows the two agree
    vals, offs = flat(FWD_ROWS)
    assert ref.transpose(vals, offs) == ref.transpose(vals, offs, unique=True)


def test_row_keep():
    vals, offs = flat(FWD_ROWS)
    keep = [0, 1, 1, 1]                                     # 0x10 is not in the parent's list
    assert ref.groups_of(vals, offs, row_uids=FWD_UIDS, row_keep=keep) == \
        [(0x20, [0x13]), (0x30, [0x11, 0x13]), (0x40, [0x13])]
    assert ref.transpose(vals, offs, row_keep=[0, 0, 0, 0]) == ([], [0], [], [])
    # a value that only a dropped row holds is no key
    assert ref.groups_of(vals, offs, row_keep=[1, 1, 1, 0]) == [(0x20, [0]), (0x30, [0, 1])]


def test_tail_past_the_last_row_and_clamping():
    vals = [5, 6, 5, 6, 5]
    # row_offs[n_rows] = 3 < total = 5: flat 3 and 4 belong to no row
    assert ref.groups_of(vals, [0, 2, 3], total=5) == [(5, [0, 1]), (6, [0])]
    # row_offs[n_rows] = 9 > total = 4 is clamped to 4
    keys, goffs, out, src = ref.transpose(vals, [0, 2, 9], total=4)
    assert (keys, goffs, out, src) == ([5, 6], [0, 2, 4], [0, 1, 0, 1], [0, 2, 1, 3])


def test_empty_inputs_and_empty_rows():
    assert ref.transpose([], [0]) == ([], [0], [], [])      # n_rows == 0
    assert ref.transpose([], [0, 0, 0]) == ([], [0], [], [])
    vals, offs = flat([[], [], [3], [], [], [3, 2], []])
    assert ref.groups_of(vals, offs) == [(2, [5]), (3, [2, 5])]


def test_groupby_value_child_one_element_per_row():
    # rule 7: value-node groupby (query/groupby.go:224-234) over u64 keys
    keys_per_row = [40, 17, 40, 40, 17]
    src = [101, 102, 103, 104, 105]
    assert ref.groups_of(keys_per_row, list(range(6)), row_uids=src) == \
        [(17, [102, 105]), (40, [101, 103, 104])]


def test_ascending_row_uids_give_ascending_groups():
    # rule 6
    vals, offs = flat([[8, 2], [2, 8], [8], [2]])
    for _, g in ref.groups_of(vals, offs, row_uids=[1 << 33, (1 << 33) + 5, 1 << 40, U64MAX]):
        assert g == sorted(g) and len(set(g)) == len(g)


def test_capacity_rule():
    keys, goffs, out, src = ref.transpose(*flat(FWD_ROWS))
    ng, nt = len(keys), len(out)
    assert (ng, nt) == (3, 6)
    assert ref.capacity_rc(ng, nt, 3, 6, True, True) == ref.UA_OK
    assert ref.capacity_rc(ng, nt, 2, 6, True, True) == ref.UA_ERR_INVALID
    assert ref.capacity_rc(ng, nt, 3, 5, True, True) == ref.UA_ERR_INVALID
    assert ref.capacity_rc(ng, nt, 3, 0, True, False) == ref.UA_OK       # groups only
    assert ref.capacity_rc(ng, nt, 0, 0, False, False) == ref.UA_OK      # count only
    assert ref.bounded(keys, goffs, out, src, 2, 4) == \
        ([0x20, 0x30], [0, 2, 5], [0, 3, 0, 1], [0, 3, 1, 2])


def test_launch_formula():
    assert ref.launches(0, "full") == 0
    assert ref.launches(2048, "count") == 2 and ref.launches(2048, "full") == 5
    assert ref.launches(2049, "groups") == 6
    assert ref.launches(10240, "count") == 5 and ref.launches(10240, "full") == 8
