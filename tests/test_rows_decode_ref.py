"""The expected-value helper of the fan-out decode tests, held to the oracle
and to hand-written literals (CPU only).

want_rows is List.Uids with Intersect == nil: x > after (0 keeps all), then
first.  The oracle's Decode(pack, seek) keeps x >= seek, so x > a is
decode(a + 1) for 0 < a < 2^64 - 1, and a == 0 is decode(0).
"""
import gv_spec as gv
from oracle import bind as orc
from rows_decode_ref import want_row, want_rows


def test_after_matches_oracle_seek():
    uids = gv.seek_pack()
    blocks = gv.encode(uids, 9)
    opack = orc.Pack(gv.u64(uids), 9)
    seeks = gv.seek_list(blocks)
    checked = 0
    for a in seeks:
        if 0 < a < gv.U64_MAX:
            assert want_rows([uids], [a])[0] == opack.decode(a + 1).tolist(), hex(a)
            checked += 1
    assert checked >= len(seeks) - 2 and checked > 100
    assert want_rows([uids], [0])[0] == opack.decode(0).tolist() == uids
    assert uids[0] == 0  # after == 0 keeps uid 0
    assert want_row(uids, gv.U64_MAX) == []
    assert want_row(uids, gv.U64_MAX - 1) == [gv.U64_MAX]
    assert want_row(uids, 1)[0] > 1 and 1 in uids


def test_first_slicing_literals():
    u = [3, 5, 8, 13, 21]
    assert want_row(u) == [3, 5, 8, 13, 21]
    assert want_row(u, 0, 2) == [3, 5]
    assert want_row(u, 0, -2) == [13, 21]
    assert want_row(u, 0, 5) == u and want_row(u, 0, 6) == u
    assert want_row(u, 0, -5) == u and want_row(u, 0, -6) == u
    assert want_row(u, 0, 2**31 - 1) == u and want_row(u, 0, -2**31) == u
    # after first, then first: strictly greater
    assert want_row(u, 5) == [8, 13, 21]
    assert want_row(u, 5, 1) == [8]
    assert want_row(u, 5, -1) == [21]
    assert want_row(u, 4, 2) == [5, 8]
    assert want_row(u, 21, 1) == [] and want_row(u, 21, -1) == []
    assert want_row([0, 1, 2], 0, 1) == [0]
    assert want_row([], 0, 3) == []
    assert want_rows([u, [], [0, 7]], [5, 0, 0], [-2, 1, -1]) == [[13, 21], [], [7]]
    assert want_rows([u, [1]]) == [u, [1]]


def test_shared_inputs_reach_every_delta_offset_residue():
    """The byte fill of a block starts at delta_offs[b]: the shared inputs,
    flattened at block sizes 4, 9 and 256, put blocks on all 16 residues mod
    16 (what a granule-wise fill would have to get right)."""
    seen = set()
    for uids in gv.inputs().values():
        for bs in (4, 9, 256):
            _, _, offs, _ = gv.flatten(gv.encode(uids, bs))
            seen |= {int(o) % 16 for o in offs[:-1]}
    assert seen == set(range(16))
