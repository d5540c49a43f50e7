"""CPU-side checks of the fan-out intersect's C-ABI surface (no GPU compute):
the library exports both entry points, the header declares them with the
reference's call sites and pins the semantics, the ctypes layer binds them,
and every argument check that needs no device rejects its bad call.

ua_rows_intersect_packed_dev checks its arguments before it touches the
context, so the stand-in context below is never read by a call that is
rejected, and a rejected call writes nothing: out_total keeps its sentinel.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3
NAMES = ("ua_rows_intersect_packed_dev", "ua_rows_intersect_packed")
SENTINEL = 77


def test_library_exports_rows_intersect():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"


def test_header_declares_rows_intersect():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    assert "ua_drowisect" in txt
    # the semantics are stated next to the struct, against the call they differ from
    doc = txt[:txt.index("} ua_drowisect;")]
    doc = doc[doc.rindex("ua_rows_decode_dev(ua_ctx *"):]
    for cite in ("uidlist.go:33", "list.go:1823", "codec.go:279", "list.go:1892"):
        assert cite in doc, cite
    for word in ("x >= after[r]", "ua_rows_decode_dev", "cap_vals", "(since v16)",
                 "ua_ptask.after_uid", "duplicate-free", "NO first"):
        assert word in doc, word
    host = txt[txt.index("} ua_drowisect;"):]
    assert "(since v16)" in host[:host.index("int ua_rows_intersect_packed(")]


def test_lib_binds_rows_intersect():
    L = _lib.lib()
    assert L.ua_version() >= 16
    assert len(L.ua_rows_intersect_packed_dev.argtypes) == 3
    assert len(L.ua_rows_intersect_packed.argtypes) == 10
    assert C.sizeof(_lib.UaDRowIsect) == 112  # 14 pointers and u64 counts
    assert _lib.UaDRowIsect.n_blocks.offset == 32
    assert _lib.UaDRowIsect.m.offset == 80
    assert _lib.UaDRowIsect.cap_vals.offset == 96
    # up to after, the layout is ua_drowpacks'
    for f in ("bases", "num_uids", "delta_offs", "deltas", "n_blocks", "row_block_base",
              "n_rows", "after"):
        assert getattr(_lib.UaDRowIsect, f).offset == getattr(_lib.UaDRowPacks, f).offset
    for fn in (algo.Engine.intersect_rows, algo.uid_matrix_intersect, algo.uid_matrix):
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
        # a well-formed call over 4 blocks, 3 rows and 6 shared uids, all
        # ranges disjoint
        d = _lib.UaDRowIsect()
        d.bases = self.at(0)
        d.num_uids = self.at(8)
        d.delta_offs = self.at(16)
        d.deltas = self.at(32)
        d.n_blocks = 4
        d.row_block_base = self.at(64)
        d.n_rows = 3
        d.after = self.at(72)
        d.shared = self.at(80)
        d.m = 6
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
    rc = L.ua_rows_intersect_packed_dev(C.cast(stand_in, C.c_void_p) if ctx else None,
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
    assert rejected(a.desc(shared=None))                 # m > 0
    assert rejected(a.desc(out_vals=None))               # cap_vals > 0
    assert rejected(a.desc(reserved=a.at(200)))          # there is no first
    assert bytes(a.buf) == b"\0" * 8192


def test_shape_bounds_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(n_rows=0))                    # blocks without rows
    assert rejected(a.desc(n_rows=0, row_block_base=None))
    assert rejected(a.desc(n_blocks=1 << 24))            # 2^24 - 1 is the most
    assert rejected(a.desc(n_blocks=(1 << 64) - 1))
    assert rejected(a.desc(m=1 << 61))                   # 8 * m is a byte count
    assert rejected(a.desc(m=(1 << 64) - 1))


def test_overlaps_rejected_without_a_device():
    a = Arena()
    ins = {"bases": 4, "num_uids": 2, "delta_offs": 5, "deltas": 1, "row_block_base": 4,
           "after": 3, "shared": 6}
    # out_row_offs (4 words at 96) against every input
    for field, words in ins.items():
        for w in (96, 99):
            assert rejected(a.desc(**{field: a.at(w)})), (field, w)
        assert rejected(a.desc(**{field: a.at(97 - words)})), field   # tail inside
    for w in (61, 64, 67, 70, 72, 74, 77, 80, 85):       # laid over rbb, after, shared
        assert rejected(a.desc(out_row_offs=a.at(w))), w
    # out_vals (64 words at 128) against every input and out_row_offs
    ins["out_row_offs"] = 4
    for field, words in ins.items():
        for w in (128, 160, 191):                        # first, middle, last word
            assert rejected(a.desc(**{field: a.at(w)})), (field, w)
        assert rejected(a.desc(**{field: a.at(129 - words)})), field  # tail inside
    # the other way round: out_vals laid over the inputs
    for w in (0, 20, 70, 82, 90):
        assert rejected(a.desc(out_vals=a.at(w))), w
    assert bytes(a.buf) == b"\0" * 8192


def test_host_form_rejects_nulls_without_a_device():
    L = _lib.lib()
    n = C.c_uint64(SENTINEL)
    buf = (C.c_uint64 * 16)()
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    packs = (C.POINTER(_lib.UaPack) * 2)()
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    f = L.ua_rows_intersect_packed
    assert f(None, packs, 2, None, hp, 4, hp, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, None, 2, None, hp, 4, hp, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, packs, 2, None, None, 4, hp, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, packs, 2, None, hp, 4, None, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, packs, 2, None, hp, 4, hp, 8, None, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, packs, 2, None, hp, 4, hp, 8, hp, None) == UA_ERR_INVALID
    assert f(cp, packs, 2, None, hp, 1 << 61, hp, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert n.value == SENTINEL
    assert bytes(ctx) == b"\0" * 4096
