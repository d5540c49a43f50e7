"""CPU-side checks of the fan-out decode's C-ABI surface (no GPU compute): the
library exports both entry points, the header declares them with the
reference's call sites, the ctypes layer binds them, and every argument check
that needs no device rejects its bad call.

ua_rows_decode_dev checks its arguments before it touches the context, so the
stand-in context below is never read by a call that is rejected, and a
rejected call writes nothing: out_total keeps its sentinel.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3
NAMES = ("ua_rows_decode_dev", "ua_rows_decode")
SENTINEL = 77


def test_library_exports_rows_decode():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"


def test_header_declares_rows_decode():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    for cite in ("list.go:1786", "task.go:834-971", "list.go:1345"):
        assert cite in txt, cite
    assert "ua_drowpacks" in txt
    # the semantics are stated against the two calls they differ from
    doc = txt[:txt.index("} ua_drowpacks;")]
    doc = doc[doc.rindex("worker/task.go:834-971"):]
    for word in ("ua_ptask.after_uid", "x > after[r]", "INT32_MIN", "cap_vals"):
        assert word in doc, word


def test_lib_binds_rows_decode():
    L = _lib.lib()
    assert L.ua_version() >= 14
    assert len(L.ua_rows_decode_dev.argtypes) == 3
    assert len(L.ua_rows_decode.argtypes) == 9
    assert L.ua_rows_decode.argtypes[4] == C.POINTER(C.c_int32)
    assert C.sizeof(_lib.UaDRowPacks) == 96  # 12 pointers and u64 counts
    assert _lib.UaDRowPacks.n_blocks.offset == 32
    assert _lib.UaDRowPacks.cap_vals.offset == 80
    for fn in (algo.Engine.decode_rows, algo.uid_matrix, algo.row_lengths):
        assert callable(fn)


class Arena:
    """Host memory standing in for device arrays: a rejected call never
    dereferences any of it."""

    def __init__(self):
        self.buf = (C.c_uint64 * 1024)()
        self.base = C.addressof(self.buf)

    def at(self, word):
        return self.base + 8 * word

    def desc(self, **over):
        # a well-formed call over 4 blocks and 3 rows, all ranges disjoint
        d = _lib.UaDRowPacks()
        d.bases = self.at(0)
        d.num_uids = self.at(8)
        d.delta_offs = self.at(16)
        d.deltas = self.at(32)
        d.n_blocks = 4
        d.row_block_base = self.at(64)
        d.n_rows = 3
        d.after = self.at(72)
        d.first = self.at(80)
        d.out_vals = self.at(128)
        d.cap_vals = 64
        d.out_row_offs = self.at(96)
        for k, v in over.items():
            setattr(d, k, v)
        return d


def rejected(d, ctx=True, total=True):
    L = _lib.lib()
    n = C.c_uint64(SENTINEL)
    stand_in = C.create_string_buffer(4096)
    rc = L.ua_rows_decode_dev(C.cast(stand_in, C.c_void_p) if ctx else None,
                              C.byref(d) if d is not None else None,
                              C.byref(n) if total else None)
    assert bytes(stand_in) == b"\0" * 4096, "a rejected call touched the context"
    assert n.value == SENTINEL, "a rejected call wrote out_total"
    return rc == UA_ERR_INVALID


def test_null_arguments_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(), ctx=False)
    assert rejected(None)
    assert rejected(a.desc(), total=False)
    assert rejected(a.desc(out_row_offs=None))
    for field in ("bases", "num_uids", "delta_offs", "deltas"):
        assert rejected(a.desc(**{field: None})), field
    assert rejected(a.desc(row_block_base=None))
    assert rejected(a.desc(out_vals=None))               # cap_vals > 0
    assert bytes(a.buf) == b"\0" * 8192


def test_shape_bounds_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(n_rows=0))                    # blocks without rows
    assert rejected(a.desc(n_rows=0, row_block_base=None))
    assert rejected(a.desc(n_blocks=1 << 24))            # 2^24 - 1 is the most
    assert rejected(a.desc(n_blocks=(1 << 64) - 1))


def test_overlaps_rejected_without_a_device():
    a = Arena()
    # out_row_offs (4 words) against row_block_base (4 words at 64)
    for w in (61, 64, 67):
        assert rejected(a.desc(out_row_offs=a.at(w))), w
    # out_vals (64 words at 128) against every input and out_row_offs
    ins = {"bases": 4, "num_uids": 2, "delta_offs": 5, "deltas": 1, "row_block_base": 4,
           "after": 3, "first": 2, "out_row_offs": 4}
    for field, words in ins.items():
        for w in (128, 160, 191):                        # first, middle, last word
            assert rejected(a.desc(**{field: a.at(w)})), (field, w)
        assert rejected(a.desc(**{field: a.at(129 - words)})), field  # tail inside
    # the other way round: out_vals laid over the inputs
    assert rejected(a.desc(out_vals=a.at(0)))
    assert rejected(a.desc(out_vals=a.at(90)))
    assert bytes(a.buf) == b"\0" * 8192


def test_host_form_rejects_nulls_without_a_device():
    L = _lib.lib()
    n = C.c_uint64(SENTINEL)
    buf = (C.c_uint64 * 16)()
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    packs = (C.POINTER(_lib.UaPack) * 2)()
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    ok = (packs, 2, None, None, hp, 8, hp, C.byref(n))
    assert L.ua_rows_decode(None, *ok) == UA_ERR_INVALID
    assert L.ua_rows_decode(cp, None, 2, None, None, hp, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_decode(cp, packs, 2, None, None, None, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_decode(cp, packs, 2, None, None, hp, 8, None, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_decode(cp, packs, 2, None, None, hp, 8, hp, None) == UA_ERR_INVALID
    assert n.value == SENTINEL
    assert bytes(ctx) == b"\0" * 4096
