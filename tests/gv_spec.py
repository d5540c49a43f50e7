"""The UidPack block format, restated in plain Python for the tests.

A pack is a list of blocks (base, num_uids, deltas).  A new block starts where
the upper 32 bits of the uid change, and a block closes once it holds
block_size uids (block_size 0 behaves like 1).  A block stores its first uid as
base and the num_uids - 1 differences between neighbours as group-varint
groups of four, the last group padded with zeros; a one-uid block carries one
all-zero group.  A group is one control byte, then its four values, each
little-endian in 1..4 bytes; bit pair 2i of the control byte is value i's
length minus one.

Everything here is Python int and bytes arithmetic, so nothing can wrap.
The second half holds the inputs that the codec tests share.
"""
import numpy as np

U64_MAX = (1 << 64) - 1
BLOCK_SIZES = [0, 1, 2, 3, 4, 5, 6, 7, 9, 255, 256]
MAX_BLOCK_BYTES = 1085  # 256 uids, 255 four-byte deltas: 63 * 17 + 14


def _nbytes(d):
    assert 0 <= d < 1 << 32
    return 1 if d < 1 << 8 else 2 if d < 1 << 16 else 3 if d < 1 << 24 else 4


def encode_group(vals):
    """Four values below 2^32 -> control byte + payload."""
    assert len(vals) == 4
    tag, body = 0, b""
    for i, d in enumerate(vals):
        k = _nbytes(d)
        tag |= (k - 1) << (2 * i)
        body += d.to_bytes(k, "little")
    return bytes([tag]) + body


def encode(uids, block_size):
    """Sorted duplicate-free uids -> [(base, num_uids, deltas)]."""
    uids = [int(x) for x in uids]
    cap = max(int(block_size), 1)
    runs = []
    for u in uids:
        if runs and runs[-1][-1] >> 32 == u >> 32 and len(runs[-1]) < cap:
            assert u > runs[-1][-1]
            runs[-1].append(u)
        else:
            runs.append([u])
    blocks = []
    for r in runs:
        ds = [b - a for a, b in zip(r, r[1:])] or [0]
        ds += [0] * (-len(ds) % 4)
        blob = b"".join(encode_group(ds[i:i + 4]) for i in range(0, len(ds), 4))
        blocks.append((r[0], len(r), blob))
    return blocks


def _groups(num_uids, deltas):
    """Yield (control byte, [four values]) for each group of one block."""
    pos = 0
    for _ in range(max((num_uids - 1 + 3) // 4, 1)):
        tag, pos, vals = deltas[pos], pos + 1, []
        for i in range(4):
            k = ((tag >> (2 * i)) & 3) + 1
            vals.append(int.from_bytes(deltas[pos:pos + k], "little"))
            pos += k
        yield tag, vals
    assert pos == len(deltas)


def decode(blocks):
    out = []
    for base, num, deltas in blocks:
        vals = [d for _, g in _groups(num, deltas) for d in g][:num - 1]
        out.append(base)
        for d in vals:
            out.append(out[-1] + d)
    return out


def control_bytes(blocks):
    return [[tag for tag, _ in _groups(num, deltas)] for _, num, deltas in blocks]


def flatten(blocks):
    """Blocks -> (bases u64, num_uids u32, delta_offs u64[nb + 1], blob u8)."""
    offs = [0]
    for _, _, d in blocks:
        offs.append(offs[-1] + len(d))
    return (np.array([b for b, _, _ in blocks], dtype=np.uint64),
            np.array([n for _, n, _ in blocks], dtype=np.uint32),
            np.array(offs, dtype=np.uint64),
            np.frombuffer(b"".join(d for _, _, d in blocks), dtype=np.uint8).copy())


def u64(uids):
    return np.array([int(x) for x in uids], dtype=np.uint64)


# ---- shared inputs ----

LOW = [1, 0x100, 0x10000, 0x1000000]          # smallest value of each length
HIGH = [0xff, 0xffff, 0xffffff, 0x3fffffff]   # largest; four still fit one run
TAG_ORDER = [(167 * i + 13) % 256 for i in range(256)]  # a fixed shuffle


def tag_group(t, which):
    """The four deltas whose group has control byte t."""
    vals = LOW if which == "low" else HIGH
    return [vals[(t >> (2 * i)) & 3] for i in range(4)]


def from_deltas(deltas, breaks=()):
    """A first uid, then one uid per delta.  A new 32-MSB run (an extra uid
    with low word 0) starts only where the sum would pass 2^32, or where the
    next uid's index is in breaks."""
    run, uids = 1, [1 << 36]
    for d in deltas:
        if len(uids) in breaks or (uids[-1] & 0xffffffff) + d >= 1 << 32:
            run += 1
            uids.append(run << 36)
        uids.append(uids[-1] + d)
    return uids


def tag_ladder(which, version="a"):
    """One group per control byte 0..255.  Version a: every group in a
    32-MSB run of its own, 256 runs of 5 uids.  Version b: the groups in
    TAG_ORDER, concatenated into runs as long as 32 bits allow."""
    if version == "b":
        return from_deltas([d for t in TAG_ORDER for d in tag_group(t, which)])
    uids = []
    for t in range(256):
        uids.append((t + 1) << 36)
        for d in tag_group(t, which):
            uids.append(uids[-1] + d)
    return uids


def long_list(n, breaks=()):
    """n uids whose deltas cycle through both shuffled ladders."""
    ds = [d for w in ("low", "high") for t in TAG_ORDER for d in tag_group(t, w)]
    return from_deltas([ds[i % len(ds)] for i in range(n)], breaks)[:n]


def full_block():
    """256 uids, 255 four-byte deltas: the longest legal block."""
    return [(5 << 32) + 0x1000000 * i for i in range(256)]


def edge_values():
    return ([0, 1, 0x100, 0xffffffff]
            + [7 << 32, (7 << 32) + 0xffffffff]          # a maximum delta
            + [(1 << 63) - 1, 1 << 63, (1 << 63) + 2]   # 2^63 - 1 is a block alone
            + [U64_MAX - 0x1000, U64_MAX - 2, U64_MAX])


def inputs():
    """Every named input of the codec tests."""
    return {"ladder_a_low": tag_ladder("low"), "ladder_a_high": tag_ladder("high"),
            "ladder_b_low": tag_ladder("low", "b"),
            "ladder_b_high": tag_ladder("high", "b"),
            "full_block": full_block(), "edge_values": edge_values()}


def seek_pack():
    """The pack of the seek sweeps: the start of ladder b high and the edge
    values, at block_size 9."""
    return sorted(set(tag_ladder("high", "b")[:200] + edge_values()))


def seek_list(blocks):
    """Seeks around every block: base - 1, base, base + 1, last, last + 1,
    and the ends of the uid space."""
    s = {0, 1, U64_MAX - 1, U64_MAX}
    for blk in blocks:
        last = decode([blk])[-1]
        s |= {blk[0] - 1, blk[0], blk[0] + 1, last, last + 1}
    return sorted(x for x in s if 0 <= x <= U64_MAX)
