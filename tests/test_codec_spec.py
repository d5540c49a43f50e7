"""CPU checks of the UidPack byte format: tests/gv_spec.py (a plain Python
restatement) is anchored on literals derived by hand from the published
group-varint format, and the oracle encoder and the host encoder
(ua_encode) are held to it byte for byte on inputs that reach every control
byte, every delta-length boundary and the longest legal block.

The GPU encoder and decoder are checked against the same module in
tests/test_codec_tags_gpu.py.
"""
import ctypes as C

import numpy as np
import pytest

import gv_spec as gv
from dgraph_amd import _lib, algo
from oracle import bind as orc

INPUTS = gv.inputs()
B = 5 << 32


# ---------- gv_spec against hand-derived bytes ----------

def test_group_literals():
    # lengths 1, 2, 3, 4 -> bit pairs 00 01 10 11 from the low end: 0b11100100
    assert gv.encode_group([1, 0x100, 0x10000, 0x1000000]) == bytes.fromhex(
        "e4" "01" "0001" "000001" "00000001")
    assert gv.encode_group([0xff, 0xffff, 0xffffff, 0xffffffff]) == bytes.fromhex(
        "e4" "ff" "ffff" "ffffff" "ffffffff")
    assert gv.encode_group([0, 0, 0, 0]) == bytes.fromhex("0000000000")
    # lengths 4, 1, 1, 2 -> 0b01000011; the order of the pairs matters
    assert gv.encode_group([0x01020304, 0, 0xff, 0x100]) == bytes.fromhex(
        "43" "04030201" "00" "ff" "0001")
    # each threshold from both sides
    assert gv.encode_group([0xff, 0x100, 0xffff, 0x10000]) == bytes.fromhex(
        "94" "ff" "0001" "ffff" "000001")
    assert gv.encode_group([0xffffff, 0x1000000, 0, 0]) == bytes.fromhex(
        "0e" "ffffff" "00000001" "00" "00")


def test_block_literals():
    # six uids: deltas 3, 0x100, 0x20000, 5 | 0x01020304 and three pad zeros
    uids = [B, B + 3, B + 0x103, B + 0x20103, B + 0x20108, B + 0x20108 + 0x01020304]
    want = bytes.fromhex("24" "03" "0001" "000002" "05"
                         "03" "04030201" "00" "00" "00")
    assert gv.encode(uids, 256) == [(B, 6, want)]
    assert gv.control_bytes(gv.encode(uids, 256)) == [[0x24, 0x03]]
    assert gv.decode([(B, 6, want)]) == uids
    # one uid: the pad-only group
    assert gv.encode([42], 256) == [(42, 1, bytes(5))]
    assert gv.decode([(42, 1, bytes(5))]) == [42]
    assert gv.encode([], 256) == []


def test_split_literals():
    one = bytes.fromhex("0001000000")
    # block_size closes a block; 0 means one uid per block
    assert gv.encode([1, 2, 3], 2) == [(1, 2, one), (3, 1, bytes(5))]
    assert gv.encode([1, 2], 0) == [(1, 1, bytes(5)), (2, 1, bytes(5))]
    assert gv.encode([1, 2], 1) == gv.encode([1, 2], 0)
    # a change in the upper 32 bits starts a block, and the count restarts
    assert gv.encode([0xfffffffe, 0xffffffff, 1 << 32, (1 << 32) + 1, (1 << 32) + 2], 3) \
        == [(0xfffffffe, 2, one), (1 << 32, 3, bytes.fromhex("000101" "0000"))]
    bases, nums, offs, blob = gv.flatten(gv.encode([1, 2, 3], 2))
    assert (bases.tolist(), nums.tolist(), offs.tolist()) == ([1, 3], [2, 1], [0, 5, 10])
    assert blob.tobytes() == one + bytes(5)
    assert (bases.dtype, nums.dtype, offs.dtype, blob.dtype) == \
        (np.uint64, np.uint32, np.uint64, np.uint8)


# ---------- the inputs cover the format (conditions on gv_spec alone) ----------

def test_input_coverage():
    packs = {k: gv.encode(u, 256) for k, u in INPUTS.items()}
    blocks = [b for p in packs.values() for b in p]
    tags = {t for p in packs.values() for blk in gv.control_bytes(p) for t in blk}
    assert tags == set(range(256))
    # ladder a alone reaches every control byte, one group per run
    for w in ("ladder_a_low", "ladder_a_high"):
        assert [t for blk in gv.control_bytes(packs[w]) for t in blk] == list(range(256))
        assert len(INPUTS[w]) == 1280
    # unequal groups at every group position of a block
    odd = set()
    for base, num, deltas in blocks:
        for g, t in enumerate(gv.control_bytes([(base, num, deltas)])[0]):
            if 5 + sum((t >> s) & 3 for s in (0, 2, 4, 6)) != 5:
                odd.add(g)
    assert odd == set(range(64))
    # and not only through the all-17-byte block: ladder b spreads them too
    odd_b = {g for w in ("ladder_b_low", "ladder_b_high")
             for blk in gv.control_bytes(packs[w]) for g, t in enumerate(blk) if t}
    assert odd_b == set(range(64))
    sizes = [len(d) for _, _, d in blocks]
    assert max(sizes) == gv.MAX_BLOCK_BYTES == 63 * 17 + 14
    assert packs["full_block"] == [(5 << 32, 256, packs["full_block"][0][2])]
    assert any(n == 1 for _, n, _ in blocks)
    assert any(gv.decode([b])[-1] == gv.U64_MAX for b in blocks)
    # the low ladder sums to 0x101010100: two 32-MSB runs
    assert len({u >> 32 for u in INPUTS["ladder_b_low"]}) == 2
    # each delta-length boundary, from both sides, in every lane of a group
    seen = set()
    for p in packs.values():
        for base, num, deltas in p:
            for _, vals in gv._groups(num, deltas):
                seen |= {(lane, d) for lane, d in enumerate(vals)}
    for d in (0xff, 0x100, 0xffff, 0x10000, 0xffffff, 0x1000000):
        assert all((lane, d) in seen for lane in range(4)), hex(d)
    assert any(d == 0xffffffff for _, d in seen)
    # the edge values the issue names
    e = INPUTS["edge_values"]
    assert {0, (1 << 63) - 1, 1 << 63, gv.U64_MAX - 2, gv.U64_MAX} <= set(e)
    # small by construction, sorted and duplicate-free
    for u in list(INPUTS.values()) + [gv.seek_pack(), gv.long_list(4097, {2048, 4096})]:
        assert len(u) <= 5000 and all(a < b for a, b in zip(u, u[1:]))
    assert len(gv.encode(gv.seek_pack(), 9)) <= 40
    for n in (2047, 2049, 4097):
        u = gv.long_list(n, {2048, n - 1})
        assert len(u) == n and u[n - 1] >> 32 != u[n - 2] >> 32
        assert n <= 2048 or u[2048] >> 32 != u[2047] >> 32


# ---------- oracle and host encoder against gv_spec ----------

def _same_flat(got, want, who):
    for g, w, name in zip(got, want, ("bases", "num_uids", "delta_offs", "deltas")):
        assert g.tolist() == w.tolist(), f"{who}: {name}"


@pytest.mark.parametrize("bs", gv.BLOCK_SIZES)
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_encoders_match_spec_bytes(name, bs):
    uids = INPUTS[name]
    blocks = gv.encode(uids, bs)
    assert gv.decode(blocks) == uids
    want = gv.flatten(blocks)
    arr = gv.u64(uids)

    opack = orc.Pack(arr, bs)
    _same_flat(opack.flatten(), want, "oracle")
    assert opack.decode(0).tolist() == uids
    assert opack.exact_len() == len(uids)
    assert opack.approx_len() == len(blocks) * bs

    bases, nums, offs, blob, total = algo.encode_flat(arr, bs)
    _same_flat((bases, nums, offs, blob), want, "ua_encode")
    assert total == len(uids)


@pytest.mark.parametrize("bs", [0, 1, 5, 256])
def test_host_pack_lengths(bs):
    """ua_pack_exact_len / ua_pack_approx_len (codec.ExactLen: the sum of
    num_uids; codec.ApproxLen: blocks times block_size) on the host pack."""
    L = _lib.lib()
    for name, uids in sorted(INPUTS.items()):
        arr = gv.u64(uids)
        h = C.c_void_p()
        _lib.check(L.ua_encode(arr.ctypes.data_as(C.POINTER(C.c_uint64)), arr.size, bs,
                               C.byref(h)))
        try:
            view = L.ua_owned_pack_view(h)
            blocks = gv.encode(uids, bs)
            assert view.contents.n_blocks == len(blocks), name
            assert L.ua_pack_exact_len(view) == len(uids), name
            assert L.ua_pack_approx_len(view) == len(blocks) * bs, name
            for i, (base, num, deltas) in enumerate(blocks):
                b = view.contents.blocks[i]
                assert (b.base, b.num_uids, b.deltas_len) == (base, num, len(deltas))
        finally:
            L.ua_owned_pack_free(h)


@pytest.mark.parametrize("bs", [1, 4, 5])
def test_oracle_linear_seek_to_uint64_max(bs):
    """UINT64_MAX in v on the LinearSeek path: the reference's loop
    (seek >= PeekNextBase(), which is MaxUint64 after the last block) never
    ends there; the oracle stops on the last block and finds the uid."""
    uids = INPUTS["edge_values"]
    opack = orc.Pack(gv.u64(uids), bs)
    lasts = [gv.decode([b])[-1] for b in gv.encode(uids, bs)]
    for v in (uids, lasts, [gv.U64_MAX - 1, gv.U64_MAX], [gv.U64_MAX]):
        got = orc.intersect_compressed_with(opack, 0, gv.u64(v)).tolist()
        assert got == [x for x in v if x in set(uids)]


def test_oracle_seek_matches_set_arithmetic():
    """codec.Decode(pack, seek) keeps x >= seek and IntersectCompressedWith
    keeps the x of v that are in the pack and >= after (Decoder.Seek with
    SeekStart): the oracle against that arithmetic on the seek-sweep pack."""
    uids = gv.seek_pack()
    blocks = gv.encode(uids, 9)
    opack = orc.Pack(gv.u64(uids), 9)
    have = set(uids)
    near = sorted({y for x in uids for y in (x - 1, x, x + 1) if 0 <= y <= gv.U64_MAX})
    for s in gv.seek_list(blocks):
        assert opack.decode(s).tolist() == [x for x in uids if x >= s], hex(s)
        got = orc.intersect_compressed_with(opack, s, gv.u64(near)).tolist()
        assert got == [x for x in near if x in have and x >= s], hex(s)
