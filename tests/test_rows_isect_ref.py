"""The expected-value helper of the fan-out intersect tests, held to the oracle
and to hand-written literals (CPU only).

want_row is algo.IntersectCompressedWith(pack, after, shared): x >= after
(inclusive) and x in shared.  On sorted duplicate-free shared lists the
oracle's result must be that set arithmetic for every seek of the seek sweep
and at every block size.
"""
import gv_spec as gv
import rows_decode_ref
from oracle import bind as orc
from rows_isect_ref import want_row, want_rows


def shared_lists(uids):
    """Every k-th uid plus non-member neighbours plus both ends of the uid
    space; then tiny and empty lists."""
    member = set(uids)
    near = {x + d for x in uids[::5] for d in (-1, 1)
            if 0 <= x + d <= gv.U64_MAX and x + d not in member}
    assert near
    out = []
    for k in (1, 2, 3, 7, 50):
        out.append(sorted(set(uids[::k]) | near | {0, gv.U64_MAX}))
    return out


def tiny_lists(uids):
    return [[], [uids[0]], [uids[-1]], [uids[len(uids) // 2]],
            [uids[3] + 1] if uids[3] + 1 not in uids else [uids[3]],
            [uids[0], uids[-1]]]


def test_matches_oracle_on_the_seek_sweep():
    uids = gv.seek_pack()
    seeks = gv.seek_list(gv.encode(uids, 9))
    assert 150 <= len(seeks) <= 300
    big, tiny = shared_lists(uids), tiny_lists(uids)
    checked = 0
    for bs in (1, 9, 256):
        opack = orc.Pack(gv.u64(uids), bs)
        for a in seeks:
            for sh in big + tiny:
                got = orc.intersect_compressed_with(opack, a, gv.u64(sh)).tolist()
                assert got == want_row(uids, sh, a), (bs, hex(a), len(sh))
                checked += 1
    assert checked == 3 * len(seeks) * (len(big) + len(tiny)) and checked > 3000


def test_inclusive_after_literals():
    u = [3, 5, 8, 13, 21]
    every = range(0, 30)
    assert want_row(u, every) == u
    assert want_row(u, [5, 8, 9, 21]) == [5, 8, 21]
    assert want_row(u, [4, 6, 7]) == [] and want_row(u, []) == [] and want_row([], every) == []
    # after equal to a member keeps it here and drops it in List.Uids' x > after
    assert want_row(u, every, 5) == [5, 8, 13, 21]
    assert rows_decode_ref.want_row(u, 5) == [8, 13, 21]
    assert want_row(u, every, 6) == [8, 13, 21] and want_row(u, every, 22) == []
    assert want_row(u, [5, 13], 5) == [5, 13] and want_row(u, [5, 13], 6) == [13]
    # after = 2^64 - 1 keeps 2^64 - 1 if both hold it; x > after keeps nothing
    top = [0, 7, gv.U64_MAX]
    assert want_row(top, top, gv.U64_MAX) == [gv.U64_MAX]
    assert want_row(top, [0, 7], gv.U64_MAX) == []
    assert rows_decode_ref.want_row(top, gv.U64_MAX) == []
    # 0 is an ordinary value on both sides
    assert want_row(top, top, 0) == top and want_row(top, [0], 0) == [0]
    assert want_row(top, top, 1) == [7, gv.U64_MAX]
    assert want_rows([u, [], top], [0, 5, 13, gv.U64_MAX], [6, 0, 7]) == \
        [[13], [], [gv.U64_MAX]]
    assert want_rows([u, [1]], [1, 3]) == [[3], [1]]
