"""What ua_rows_encode_dev must return, in plain Python (a helper, not a
test): one codec.Encoder{BlockSize} per row (codec.go:57-136), the rows'
blocks laid out one after another in one flat arena.

want_arena concatenates tests/gv_spec.encode of every row: bases, num_uids,
delta_offs (arena-wide, n_blocks + 1 entries), the blob, and row_block_base
(n_rows + 1 entries; an empty row owns no block).
tests/test_rows_encode_ref.py holds this to the oracle and to literals.
"""
import numpy as np

import gv_spec as gv


def want_arena(rows, block_size):
    blocks, rbb = [], [0]
    for row in rows:
        blocks += gv.encode(row, block_size)
        rbb.append(len(blocks))
    bases, nums, offs, blob = gv.flatten(blocks)
    return bases, nums, offs, blob, np.array(rbb, dtype=np.uint64)


TILE = 2048  # flat elements per workgroup of the encoder's kernels


def one_run(n=2 * TILE + 300):
    """n uids of ONE 32-MSB run with deltas of 1 to 4 bytes."""
    small = [1, 0x100, 5, 0x10000, 0xff, 2, 0xffff, 9]
    uids = [3 << 32]
    for i in range(n - 1):
        uids.append(uids[-1] + (0x1000000 if i % 32 == 31 else small[i % 8]))
    assert uids[-1] >> 32 == 3
    return uids


def lead_row(n):
    return [10 + 3 * i for i in range(n)]


LEADS = [0, 1, 2, 3] + list(range(TILE - 3, TILE + 4))
RUN_SIZES = [9, 255, 256]


def cases():
    """name -> (rows, block sizes): every input of the encoder tests."""
    all_bs = gv.BLOCK_SIZES
    out = {}
    for name, uids in gv.inputs().items():
        out[name] = ([uids], all_bs)
    out["inputs_as_rows"] = ([gv.inputs()[k] for k in sorted(gv.inputs())], all_bs)
    run = one_run()
    out["one_run"] = ([run], RUN_SIZES)
    for n in LEADS:
        out[f"run_behind_{n}"] = ([lead_row(n), run], RUN_SIZES)
    out["one_uid_rows"] = ([[(1 << 33) + 3 * i] for i in range(5000)], [0, 1, 256])
    # the most bytes a tile can hold: its first element ends a two-uid block
    # with a 4-byte delta (8 bytes), the other 2047 are one-uid blocks
    base = 1 << 34
    fat = [[base + 2 * i] for i in range(TILE - 1)]
    fat.append([base + 2 * TILE, base + 2 * TILE + 0x1000000])
    fat += [[base + (1 << 30) + 2 * i] for i in range(TILE + 10)]
    out["fullest_tile"] = (fat, [2, 256])
    a, b, c = [5, 6, 7], [1 << 32, (1 << 32) + 1], [9]
    out["empty_rows"] = ([[], []] + [a] + [[]] * 3000 + [b] + [[]] + [c] + [[]] * 3,
                         [1, 2, 256])
    out["no_rows"] = ([], [256])
    out["one_empty_row"] = ([[]], [256])
    out["two_empty_rows"] = ([[], []], [0, 256])
    for n in (1, TILE, TILE + 1):
        out[f"total_{n}"] = ([lead_row(n)], [0, 7, 256])
        out[f"total_{n}_split"] = ([lead_row(n - n // 2), [1 << 40] * 0,
                                    [(1 << 35) + 2 * i for i in range(n // 2)]], [7, 256])
    for br in ((TILE - 1,), (TILE,), (TILE + 1,), (TILE - 1, TILE, TILE + 1)):
        out["long_list_" + "_".join(map(str, br))] = ([gv.long_list(6000, br)], [4, 9, 256])
    return out


def csr(rows):
    """Rows -> (vals u64, row_offs u64[n_rows + 1])."""
    offs = [0]
    for row in rows:
        offs.append(offs[-1] + len(row))
    return gv.u64([x for row in rows for x in row]), np.array(offs, dtype=np.uint64)
