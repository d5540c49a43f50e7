"""The expected-value helper of the fan-out encode tests, held to the oracle's
encoder and to hand-written byte literals (CPU only).
"""
import numpy as np

import gv_spec as gv
from oracle import bind as orc
from rows_encode_ref import cases, csr, want_arena


def arena_lists(rows, bs):
    bases, nums, offs, blob, rbb = want_arena(rows, bs)
    return (bases.tolist(), nums.tolist(), offs.tolist(), bytes(blob.tobytes()),
            rbb.tolist())


def test_helper_matches_the_oracle_row_by_row():
    checked = 0
    for name, (rows, sizes) in cases().items():
        for bs in sizes:
            bases, nums, offs, blob, rbb = want_arena(rows, bs)
            assert rbb[0] == 0 and rbb[-1] == bases.size == nums.size == offs.size - 1
            assert offs[-1] == blob.size
            for r, row in enumerate(rows):
                b0, b1 = int(rbb[r]), int(rbb[r + 1])
                if not row:
                    assert b0 == b1, (name, bs, r)
                    continue
                ob, on, oo, od = orc.Pack(gv.u64(row), bs).flatten()
                y0, y1 = int(offs[b0]), int(offs[b1])
                assert np.array_equal(bases[b0:b1], ob), (name, bs, r)
                assert np.array_equal(nums[b0:b1], on), (name, bs, r)
                assert np.array_equal(offs[b0:b1 + 1] - np.uint64(y0), oo), (name, bs, r)
                assert bytes(blob[y0:y1].tobytes()) == bytes(od[:y1 - y0].tobytes()), \
                    (name, bs, r)
                checked += 1
    assert checked > 10000


def test_byte_literals():
    z5 = bytes(5)
    assert arena_lists([[7]], 256) == ([7], [1], [0, 5], z5, [0, 1])
    # a 4-byte delta: control byte 0b11 for value 0, three one-byte zero pads
    assert arena_lists([[1, 1 + 0x01020304]], 256) == (
        [1], [2], [0, 8], bytes([0x03, 0x04, 0x03, 0x02, 0x01, 0, 0, 0]), [0, 1])
    # the upper 32 bits change inside the row: two blocks
    row = [0xfffffffe, 0xffffffff, 1 << 32, (1 << 32) + 5]
    assert arena_lists([row], 256) == (
        [0xfffffffe, 1 << 32], [2, 2], [0, 5, 10],
        bytes([0, 1, 0, 0, 0]) + bytes([0, 5, 0, 0, 0]), [0, 2])
    # an empty row between two rows owns no block
    assert arena_lists([[3], [], [4, 6]], 256) == (
        [3, 4], [1, 2], [0, 5, 10], z5 + bytes([0, 2, 0, 0, 0]), [0, 1, 1, 2])
    # block_size 0 packs one uid per block, as 1 does
    assert arena_lists([[4, 6]], 0) == arena_lists([[4, 6]], 1) == (
        [4, 6], [1, 1], [0, 5, 10], z5 + z5, [0, 2])
    # five uids: one full group; six: a second group with three pads
    assert arena_lists([[10, 11, 0x10b, 0x1010b, 0x101010b]], 256)[3] == bytes(
        [0b11100100, 1, 0, 1, 0, 0, 1, 0, 0, 0, 1])
    assert arena_lists([[1, 2, 3, 4, 5, 0x105]], 256)[3] == bytes(
        [0, 1, 1, 1, 1]) + bytes([0b01, 0, 1, 0, 0, 0])


def test_csr_helper():
    vals, offs = csr([[3], [], [4, 6]])
    assert vals.tolist() == [3, 4, 6] and offs.tolist() == [0, 1, 1, 3]
    vals, offs = csr([])
    assert vals.size == 0 and offs.tolist() == [0]
