"""CPU-side checks of the row sort's C-ABI surface (no GPU compute): the library
exports both entry points, the header declares them with the reference's call
sites, the ctypes layer binds them, and every argument check rejects its bad
call.

ua_rows_sort_dev checks its arguments before it touches the context, so the
stand-in context below is never read by a call that is rejected, and a
rejected call writes nothing: out_total keeps its sentinel.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo, sortpath

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3
NAMES = ("ua_rows_sort_dev", "ua_rows_sort")
SENTINEL = 77
DESC, MULTI, DROP = 1, 2, 4


def test_library_exports_rows_sort():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"


def test_header_declares_rows_sort():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    assert re.search(r"enum\s*\{\s*UA_SORT_DESC = 1, UA_SORT_MULTI = 2, "
                     r"UA_SORT_DROP_NULLS = 4\s*\}", txt)
    doc = txt[:txt.index("} ua_drowsort;")]
    doc = doc[doc.rindex("ua_rows_encode_dev(ua_ctx"):]
    for cite in ("query/query.go:2493-2507", "query/query.go:2511-2578",
                 "worker/sort.go:139-187", "worker/sort.go:775-821",
                 "worker/sort.go:740-772", "query/query.go:2697-2738",
                 "query/query.go:1483-1487, 3006-3010", "x/x.go:815-844",
                 "sort.go:813", "query.go:2709-2716", "query.go:2718-2720",
                 "sort.go:748-769", "query.go:2561-2569", "sort.go:170-178"):
        assert cite in doc, cite
    for word in ("oracle/sortref.py", "types.Equal", "cap_vals", "bytes_algorithmic",
                 "launches", "clamped", "24 bytes per element", "2^31"):
        assert word in doc, word


def test_lib_binds_rows_sort():
    L = _lib.lib()
    assert L.ua_version() >= 19
    assert len(L.ua_rows_sort_dev.argtypes) == 3
    assert len(L.ua_rows_sort.argtypes) == 15
    S = _lib.UaDRowSort
    assert C.sizeof(S) == 104  # 13 eight-byte slots
    want = ["vals", "row_offs", "n_rows", "total", "keys", "has", "flags", "count", "offset",
            "out_vals", "cap_vals", "out_row_offs", "out_src", "out_ms_offs"]
    assert [f[0] for f in S._fields_] == want
    offs = [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 72, 80, 88, 96]
    for name, off in zip(want, offs):
        assert getattr(S, name).offset == off, name
    assert (_lib.UA_SORT_DESC, _lib.UA_SORT_MULTI, _lib.UA_SORT_DROP_NULLS) == (1, 2, 4)
    for fn in (algo.Engine.sort_rows, algo.Engine.paginate_rows, algo.sort_uid_matrix,
               algo.paginate_uid_matrix, sortpath.sort_rows_without_index):
        assert callable(fn)


# a well-formed call over 3 rows of 40 elements, all ranges disjoint (words)
WORDS = {"vals": 40, "row_offs": 4, "keys": 40, "has": 5, "out_vals": 40, "out_row_offs": 4,
         "out_src": 40, "out_ms_offs": 2}
START = {"vals": 0, "row_offs": 64, "keys": 128, "has": 192, "out_vals": 256,
         "out_row_offs": 320, "out_src": 384, "out_ms_offs": 448}


class Arena:
    """Host memory standing in for device arrays: a rejected call never
    dereferences any of it."""

    def __init__(self):
        self.buf = (C.c_uint64 * 1024)()
        self.base = C.addressof(self.buf)

    def at(self, word):
        return self.base + 8 * word

    def desc(self, **over):
        d = _lib.UaDRowSort()
        for name, start in START.items():
            setattr(d, name, self.at(start))
        d.n_rows = 3
        d.total = 40
        d.flags = MULTI
        d.count = 5
        d.offset = 1
        d.cap_vals = 40
        for k, v in over.items():
            setattr(d, k, v)
        return d


def call(d, ctx=True, tot=True):
    L = _lib.lib()
    n = C.c_uint64(SENTINEL)
    stand_in = C.create_string_buffer(4096)
    rc = L.ua_rows_sort_dev(C.cast(stand_in, C.c_void_p) if ctx else None,
                            C.byref(d) if d is not None else None,
                            C.byref(n) if tot else None)
    assert bytes(stand_in) == b"\0" * 4096, "a rejected call touched the context"
    assert n.value == SENTINEL, "a rejected call wrote out_total"
    return rc


def rejected(d, **kw):
    return call(d, **kw) == UA_ERR_INVALID


def test_null_arguments_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(), ctx=False)
    assert rejected(None)
    assert rejected(a.desc(), tot=False)
    assert rejected(a.desc(out_row_offs=None))
    assert rejected(a.desc(vals=None))                      # total > 0
    assert rejected(a.desc(row_offs=None))                  # n_rows > 0
    assert bytes(a.buf) == b"\0" * 8192


def test_shape_bounds_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(n_rows=0))                       # elements without rows
    assert rejected(a.desc(n_rows=0, row_offs=None, out_ms_offs=None))
    assert rejected(a.desc(total=1 << 31))                  # 2^31 - 1 is the most
    assert rejected(a.desc(total=(1 << 64) - 1))
    assert rejected(a.desc(n_rows=1 << 31, out_ms_offs=None, flags=0))
    assert rejected(a.desc(n_rows=(1 << 64) - 1, out_ms_offs=None, flags=0))
    assert rejected(a.desc(cap_vals=1 << 60))
    assert bytes(a.buf) == b"\0" * 8192


def test_flag_rules_rejected_without_a_device():
    a = Arena()
    nokeys = dict(keys=None, has=None, flags=0, out_ms_offs=None)
    for flags in (DESC, MULTI, DROP):                       # flags need keys
        over = dict(nokeys, flags=flags)
        if flags == MULTI:
            over["out_ms_offs"] = a.at(START["out_ms_offs"])
        assert rejected(a.desc(**over)), flags
    assert rejected(a.desc(**dict(nokeys, has=a.at(START["has"]))))  # has needs keys
    for flags in (8, 16, 1 << 32, 1 << 63, MULTI | 8):      # unknown bits
        assert rejected(a.desc(flags=flags)), flags
    assert rejected(a.desc(flags=MULTI | DROP))
    assert rejected(a.desc(flags=MULTI | DROP | DESC))
    assert rejected(a.desc(flags=0))                        # out_ms_offs without MULTI
    assert rejected(a.desc(flags=DESC))
    assert rejected(a.desc(flags=DROP))
    assert rejected(a.desc(out_vals=None, cap_vals=0))      # out_src without out_vals
    assert rejected(a.desc(out_vals=None, out_src=None))    # NULL out_vals with a capacity
    assert bytes(a.buf) == b"\0" * 8192


def test_overlaps_rejected_without_a_device():
    a = Arena()
    outs = ("out_vals", "out_row_offs", "out_src", "out_ms_offs")
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
    assert rejected(a.desc(vals=a.at(256)))
    assert rejected(a.desc(keys=a.at(384 + 39)))
    assert rejected(a.desc(has=a.at(321)))
    assert rejected(a.desc(row_offs=a.at(448)))
    assert bytes(a.buf) == b"\0" * 8192


def test_host_form_rejects_without_a_device():
    L = _lib.lib()
    n = C.c_uint64(SENTINEL)
    buf = (C.c_uint64 * 64)()
    buf[2] = 5                                              # row_offs[n_rows] of 2 rows
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    h32 = C.cast(buf, C.POINTER(C.c_int32))
    h8 = C.cast(buf, C.POINTER(C.c_uint8))
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    nn = C.byref(n)

    def call(c=cp, vals=hp, ro=hp, keys=hp, has=h8, flags=MULTI, ov=hp, cap=8, oro=hp,
             osrc=hp, oms=h32, pn=nn):
        return L.ua_rows_sort(c, vals, ro, 2, keys, has, flags, 5, 1, ov, cap, oro, osrc, oms,
                              pn)

    assert call(c=None) == UA_ERR_INVALID
    assert call(vals=None) == UA_ERR_INVALID
    assert call(ro=None) == UA_ERR_INVALID
    assert call(oro=None) == UA_ERR_INVALID
    assert call(pn=None) == UA_ERR_INVALID
    assert call(keys=None) == UA_ERR_INVALID                # has and flags without keys
    assert call(keys=None, has=None, flags=DESC, oms=None) == UA_ERR_INVALID
    assert call(flags=8) == UA_ERR_INVALID
    assert call(flags=MULTI | DROP) == UA_ERR_INVALID
    assert call(flags=0) == UA_ERR_INVALID                  # out_ms_offs without MULTI
    assert call(ov=None, cap=0) == UA_ERR_INVALID           # out_src without out_vals
    assert call(ov=None, osrc=None) == UA_ERR_INVALID       # NULL out_vals with a capacity
    assert call(cap=1 << 60) == UA_ERR_INVALID
    buf[2] = 1 << 31
    assert call() == UA_ERR_INVALID                         # total >= 2^31
    assert n.value == SENTINEL
    assert bytes(ctx) == b"\0" * 4096
