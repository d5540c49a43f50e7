"""CPU-side checks of the fan-out encode's C-ABI surface (no GPU compute): the
library exports both entry points, the header declares them with the
reference's call sites, the ctypes layer binds them, and every argument check
rejects its bad call.

ua_rows_encode_dev checks its arguments before it touches the context, so the
stand-in context below is never read by a call that is rejected, and a
rejected call writes nothing: n_blocks and deltas_bytes keep their sentinels.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3
NAMES = ("ua_rows_encode_dev", "ua_rows_encode")
SENTINEL = 77


def test_library_exports_rows_encode():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"


def test_header_declares_rows_encode():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    assert "ua_drowenc" in txt
    doc = txt[:txt.index("} ua_drowenc;")]
    doc = doc[doc.rindex("ua_rows_decode_mut_dev(ua_ctx"):]
    for cite in ("codec.go:57-136", "codec.go:393", "list.go:1609-1664",
                 "reduce.go:811-861", "count_index.go:133-154"):
        assert cite in doc, cite
    for word in ("Splits", "2^24 - 1", "cap_blocks", "cap_deltas", "bytes_algorithmic",
                 "launches", "clamped"):
        assert word in doc, word


def test_lib_binds_rows_encode():
    L = _lib.lib()
    assert L.ua_version() >= 18
    assert len(L.ua_rows_encode_dev.argtypes) == 4
    assert len(L.ua_rows_encode.argtypes) == 14
    E = _lib.UaDRowEnc
    assert C.sizeof(E) == 96  # 12 pointers and u64 counts
    want = ["vals", "row_offs", "n_rows", "total", "block_size", "bases", "num_uids",
            "delta_offs", "cap_blocks", "deltas", "cap_deltas", "row_block_base"]
    assert [f[0] for f in E._fields_] == want
    for i, name in enumerate(want):
        assert getattr(E, name).offset == 8 * i, name
    for fn in (algo.Engine.encode_rows, algo.Engine.rollup_rows, algo.encode_rows,
               algo.rollup_rows):
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
        # a well-formed call over 3 rows of 40 uids, all ranges disjoint:
        # vals 40 words, row_offs 4, bases 48, num_uids 24, delta_offs 49,
        # deltas 32 (256 bytes), row_block_base 4
        d = _lib.UaDRowEnc()
        d.vals = self.at(0)
        d.row_offs = self.at(64)
        d.n_rows = 3
        d.total = 40
        d.block_size = 256
        d.bases = self.at(128)
        d.num_uids = self.at(192)
        d.delta_offs = self.at(256)
        d.cap_blocks = 48
        d.deltas = self.at(320)
        d.cap_deltas = 256
        d.row_block_base = self.at(384)
        for k, v in over.items():
            setattr(d, k, v)
        return d


WORDS = {"vals": 40, "row_offs": 4, "bases": 48, "num_uids": 24, "delta_offs": 49,
         "deltas": 32, "row_block_base": 4}
START = {"vals": 0, "row_offs": 64, "bases": 128, "num_uids": 192, "delta_offs": 256,
         "deltas": 320, "row_block_base": 384}


def rejected(d, ctx=True, nb=True, db=True):
    L = _lib.lib()
    n, y = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    stand_in = C.create_string_buffer(4096)
    rc = L.ua_rows_encode_dev(C.cast(stand_in, C.c_void_p) if ctx else None,
                              C.byref(d) if d is not None else None,
                              C.byref(n) if nb else None, C.byref(y) if db else None)
    assert bytes(stand_in) == b"\0" * 4096, "a rejected call touched the context"
    assert n.value == SENTINEL and y.value == SENTINEL, "a rejected call wrote a size"
    return rc == UA_ERR_INVALID


def test_null_arguments_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(), ctx=False)
    assert rejected(None)
    assert rejected(a.desc(), nb=False)
    assert rejected(a.desc(), db=False)
    assert rejected(a.desc(row_block_base=None))
    assert rejected(a.desc(vals=None))                      # total > 0
    assert rejected(a.desc(row_offs=None))                  # n_rows > 0
    assert bytes(a.buf) == b"\0" * 8192


def test_shape_bounds_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(n_rows=0))                       # uids without rows
    assert rejected(a.desc(n_rows=0, row_offs=None))
    assert rejected(a.desc(block_size=257))
    assert rejected(a.desc(block_size=1 << 32))
    assert rejected(a.desc(block_size=(1 << 64) - 1))
    assert rejected(a.desc(total=1 << 42))                  # 2^42 - 1 is the most
    assert rejected(a.desc(total=(1 << 64) - 1))
    assert rejected(a.desc(n_rows=1 << 39))
    assert rejected(a.desc(cap_blocks=1 << 60))
    assert bytes(a.buf) == b"\0" * 8192


def test_partial_outputs_rejected_without_a_device():
    a = Arena()
    outs = ("bases", "num_uids", "delta_offs", "deltas")
    for field in outs:                                      # one NULL, three NULL
        assert rejected(a.desc(**{field: None})), field
        others = {f: None for f in outs if f != field}
        assert rejected(a.desc(**others)), field
    assert rejected(a.desc(bases=None, deltas=None))
    none = {f: None for f in outs}
    assert rejected(a.desc(cap_deltas=0, **none))           # NULL with a capacity
    assert rejected(a.desc(cap_blocks=0, **none))
    assert bytes(a.buf) == b"\0" * 8192


def test_overlaps_rejected_without_a_device():
    a = Arena()
    outs = ("bases", "num_uids", "delta_offs", "deltas", "row_block_base")
    for out in outs:
        for other in WORDS:
            if other == out:
                continue
            s, w = START[other], WORDS[other]
            # laid over the other range's first word, over its last, and with
            # only its own last word inside
            for at in (s, s + w - 1, s - WORDS[out] + 1):
                if at < 0:
                    continue
                assert rejected(a.desc(**{out: a.at(at)})), (out, other, at)
    # an input laid over an output
    assert rejected(a.desc(vals=a.at(128)))
    assert rejected(a.desc(row_offs=a.at(386)))
    assert bytes(a.buf) == b"\0" * 8192


def test_host_form_rejects_without_a_device():
    L = _lib.lib()
    n, y = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    buf = (C.c_uint64 * 64)()
    buf[2] = 5                                              # row_offs[n_rows] of 2 rows
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    h32 = C.cast(buf, C.POINTER(C.c_uint32))
    h8 = C.cast(buf, C.POINTER(C.c_uint8))
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    nn, yy = C.byref(n), C.byref(y)

    def call(c=cp, vals=hp, ro=hp, bs=256, bases=hp, nums=h32, offs=hp, cb=8, blob=h8,
             cd=64, rbb=hp, pn=nn, py=yy):
        return L.ua_rows_encode(c, vals, ro, 2, bs, bases, nums, offs, cb, blob, cd, rbb,
                                pn, py)

    assert call(c=None) == UA_ERR_INVALID
    assert call(vals=None) == UA_ERR_INVALID
    assert call(ro=None) == UA_ERR_INVALID
    assert call(bs=257) == UA_ERR_INVALID
    assert call(rbb=None) == UA_ERR_INVALID
    assert call(pn=None) == UA_ERR_INVALID
    assert call(py=None) == UA_ERR_INVALID
    assert call(bases=None) == UA_ERR_INVALID
    assert call(blob=None) == UA_ERR_INVALID
    assert call(bases=None, nums=None, offs=None, blob=None) == UA_ERR_INVALID  # caps > 0
    assert n.value == SENTINEL and y.value == SENTINEL
    assert bytes(ctx) == b"\0" * 4096
