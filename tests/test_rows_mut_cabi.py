"""CPU-side checks of the mutation-layer decode's C-ABI surface (no GPU
compute): the library exports both entry points, the header states the
semantics against List.iterate and List.Uids, the ctypes layer binds them, and
every argument check that needs no device rejects its bad call.

ua_rows_decode_mut_dev checks its arguments before it touches the context, so
the stand-in context below is never read by a call that is rejected, and a
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
NAMES = ("ua_rows_decode_mut_dev", "ua_rows_decode_mut")
SENTINEL = 77


def test_library_exports_rows_decode_mut():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"
    assert dll.ua_version() >= 17


def test_header_states_the_semantics():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    assert re.search(r"UA_MUT_SET\s*=\s*1\s*,\s*UA_MUT_DEL\s*=\s*2", txt)
    doc = txt[:txt.index("} ua_drowmut;")]
    doc = doc[doc.rindex("ua_rows_intersect_packed_dev(ua_ctx"):]
    for cite in ("list.go:1135-1251", "list.go:1099-1133", "list.go:1786-1902",
                 "list.go:1345-1363", "list.go:1146", "list.go:1892-1900", "list.go:1868",
                 "list.go:580-584", "list.go:49-53"):
        assert cite in doc, cite
    for phrase in ("List.iterate", "List.Uids", "pickPostings", "(P - uids(M)) | S",
                   "emits it once", "does nothing", "STRICTLY", "both sides of the merge",
                   "Ovr = 3 is a set", "after == NULL means all 0", "INT32_MIN",
                   "prevUid", "deleteBelowTs", "REF postings", "iterator exhausted",
                   "n_mut == 0 IS ua_rows_decode_dev", "2^32 - 2", "clamped",
                   "negative First", "cap_vals"):
        assert phrase in doc, phrase


def test_lib_binds_rows_decode_mut():
    L = _lib.lib()
    assert L.ua_version() >= 17
    assert len(L.ua_rows_decode_mut_dev.argtypes) == 3
    assert len(L.ua_rows_decode_mut.argtypes) == 12
    assert L.ua_rows_decode_mut.argtypes[7] == C.POINTER(C.c_int32)
    assert C.sizeof(_lib.UaDRowMut) == 128  # 16 pointers and u64 counts
    assert _lib.UaDRowMut.n_mut.offset == 96
    assert _lib.UaDRowMut.cap_vals.offset == 112
    # slots 0-8 are ua_drowpacks'
    for (a, _), (b, _) in zip(_lib.UaDRowMut._fields_[:9], _lib.UaDRowPacks._fields_[:9]):
        assert a == b and getattr(_lib.UaDRowMut, a).offset == getattr(_lib.UaDRowPacks,
                                                                       b).offset
    for fn in (algo.Engine.decode_rows_mut, algo.uid_matrix_mut, algo.row_lengths_mut):
        assert callable(fn)
    assert (algo.MUT_SET, algo.MUT_DEL) == (1, 2)


class Arena:
    """Host memory standing in for device arrays: a rejected call never
    dereferences any of it."""

    def __init__(self):
        self.buf = (C.c_uint64 * 1024)()
        self.base = C.addressof(self.buf)

    def at(self, word):
        return self.base + 8 * word

    def desc(self, **over):
        # a well-formed call over 4 blocks, 3 rows and 6 mutations, all ranges disjoint
        d = _lib.UaDRowMut()
        d.bases = self.at(0)
        d.num_uids = self.at(8)
        d.delta_offs = self.at(16)
        d.deltas = self.at(32)
        d.n_blocks = 4
        d.row_block_base = self.at(64)
        d.n_rows = 3
        d.after = self.at(72)
        d.first = self.at(80)
        d.mut_uids = self.at(200)
        d.mut_ops = self.at(216)
        d.row_mut_base = self.at(224)
        d.n_mut = 6
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
    rc = L.ua_rows_decode_mut_dev(C.cast(stand_in, C.c_void_p) if ctx else None,
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
    for field in ("bases", "num_uids", "delta_offs", "deltas", "row_block_base",
                  "mut_uids", "mut_ops", "row_mut_base"):
        assert rejected(a.desc(**{field: None})), field
    assert rejected(a.desc(out_vals=None))               # cap_vals > 0
    # the plain call's rejections hold with an empty layer too
    for field in ("bases", "row_block_base", "out_row_offs"):
        assert rejected(a.desc(n_mut=0, **{field: None})), field
    assert bytes(a.buf) == b"\0" * 8192


def test_shape_bounds_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(n_rows=0))                    # blocks and mutations without rows
    assert rejected(a.desc(n_rows=0, n_blocks=0))        # mutations without rows
    assert rejected(a.desc(n_rows=0, n_blocks=0, row_block_base=None, row_mut_base=None))
    assert rejected(a.desc(n_blocks=1 << 24))            # 2^24 - 1 is the most
    assert rejected(a.desc(n_blocks=1 << 24, n_mut=0))
    # 256 * n_blocks + n_mut stays below 2^32 - 1: 4 blocks leave 2^32 - 2 - 1024
    assert rejected(a.desc(n_mut=(1 << 32) - 1 - 1024))
    assert rejected(a.desc(n_mut=(1 << 32) - 1, n_blocks=0))
    assert rejected(a.desc(n_mut=1 << 32, n_blocks=0))
    assert rejected(a.desc(n_mut=(1 << 64) - 1))
    assert rejected(a.desc(n_blocks=(1 << 24) - 1, n_mut=255))


def test_overlaps_rejected_without_a_device():
    a = Arena()
    # out_row_offs (4 words at 96) against the three new inputs and row_block_base
    news = {"mut_uids": 6, "mut_ops": 1, "row_mut_base": 4, "row_block_base": 4}
    for field, words in news.items():
        for w in (96, 99, 97 - words):
            assert rejected(a.desc(**{field: a.at(w)})), (field, w)
    # out_vals (64 words at 128) against them
    for field, words in news.items():
        for w in (128, 160, 191, 129 - words):
            assert rejected(a.desc(**{field: a.at(w)})), (field, w)
    # ... and against the plain call's inputs
    for field in ("bases", "num_uids", "delta_offs", "deltas", "after", "first",
                  "out_row_offs"):
        assert rejected(a.desc(**{field: a.at(150)})), field
    # the other way round: the outputs laid over the new inputs
    assert rejected(a.desc(out_vals=a.at(190)))          # reaches mut_uids at 200
    assert rejected(a.desc(out_row_offs=a.at(222)))      # reaches row_mut_base at 224
    assert rejected(a.desc(out_row_offs=a.at(216)))      # mut_ops' 6 bytes
    assert bytes(a.buf) == b"\0" * 8192


def test_host_form_rejects_nulls_without_a_device():
    L = _lib.lib()
    n = C.c_uint64(SENTINEL)
    buf = (C.c_uint64 * 16)()
    buf[2] = 3                                            # row_mut_base[n_rows] = n_mut
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    bp = C.cast(buf, C.POINTER(C.c_uint8))
    packs = (C.POINTER(_lib.UaPack) * 2)()
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    f = L.ua_rows_decode_mut
    tail = (None, None, hp, 8, hp, C.byref(n))
    assert f(None, packs, 2, hp, bp, hp, *tail) == UA_ERR_INVALID
    assert f(cp, None, 2, hp, bp, hp, *tail) == UA_ERR_INVALID
    assert f(cp, packs, 2, None, bp, hp, *tail) == UA_ERR_INVALID
    assert f(cp, packs, 2, hp, None, hp, *tail) == UA_ERR_INVALID
    assert f(cp, packs, 2, hp, bp, hp, None, None, None, 8, hp, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, packs, 2, hp, bp, hp, None, None, hp, 8, None, C.byref(n)) == UA_ERR_INVALID
    assert f(cp, packs, 2, hp, bp, hp, None, None, hp, 8, hp, None) == UA_ERR_INVALID
    buf[2] = 1 << 32                                      # n_mut past the bound
    assert f(cp, packs, 2, hp, bp, hp, *tail) == UA_ERR_INVALID
    assert n.value == SENTINEL
    assert bytes(ctx) == b"\0" * 4096
