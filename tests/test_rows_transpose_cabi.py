"""CPU-side checks of the row transpose's C-ABI surface (no GPU compute): the
library exports both entry points, the header declares them with the
reference's call sites, the ctypes layer binds them, and every argument check
rejects its bad call.

ua_rows_transpose_dev checks its arguments before it touches the context, so
the stand-in context below is never read by a call that is rejected, and a
rejected call writes nothing: n_groups and out_total keep their sentinels and
the poisoned arena stays as it was.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3
NAMES = ("ua_rows_transpose_dev", "ua_rows_transpose")
SENTINEL = 77
POISON = 0xA5A5A5A5A5A5A5A5
UNIQUE = 1


def test_library_exports_rows_transpose():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"
    assert dll.ua_version() == 20


def test_header_declares_rows_transpose():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    assert re.search(r"enum\s*\{\s*UA_TR_UNIQUE = 1\s*\}", txt)
    doc = txt[:txt.index("} ua_drowtr;")]
    doc = doc[doc.rindex("ua_rows_sort_dev(ua_ctx"):]
    for cite in ("query/groupby.go:195-260", "query/groupby.go:265-361",
                 "query/groupby.go:104-128", ":210-221", ":292-298", ":224-234", ":302-312",
                 "posting/index.go:1759-1791", "posting/index.go:276-298",
                 "posting/index.go:1595-1640", "dgraph/cmd/bulk/mapper.go:398-432",
                 "index.go:1775"):
        assert cite in doc, cite
    for word in ("ua_index_of_batch_dev", "ua_rows_union_dev", "addValue", "UA_TR_UNIQUE",
                 "cap_keys", "cap_vals", "bytes_algorithmic", "launches", "clamped",
                 "28 bytes per element", "2^31", "2^60", "workgroup-uniform",
                 "rebuildCountIndex"):
        assert word in doc, word
    # the struct has 13 eight-byte slots
    body = doc[doc.rindex("typedef struct {"):]
    slots = 0
    for line in body.splitlines()[1:]:
        decl = line.split("/*")[0].strip()
        if decl.endswith(";"):
            slots += decl.count(",") + 1
    assert slots == 13
    assert "13 slots, 104 bytes" in txt[txt.index("} ua_drowtr;"):][:80]


def test_lib_binds_rows_transpose():
    L = _lib.lib()
    assert L.ua_version() == 20
    assert len(L.ua_rows_transpose_dev.argtypes) == 4
    assert len(L.ua_rows_transpose.argtypes) == 15
    S = _lib.UaDRowTr
    assert C.sizeof(S) == 104  # 13 eight-byte slots
    want = ["vals", "row_offs", "n_rows", "total", "row_uids", "row_keep", "flags",
            "out_keys", "out_offs", "cap_keys", "out_vals", "out_src", "cap_vals"]
    assert [f[0] for f in S._fields_] == want
    for k, name in enumerate(want):
        assert getattr(S, name).offset == 8 * k, name
    assert _lib.UA_TR_UNIQUE == 1
    for fn in (algo.Engine.transpose_rows, algo.Engine.reverse_rows,
               algo.transpose_uid_matrix, algo.group_by_uid):
        assert callable(fn)


# a well-formed call over 3 rows of 40 elements, all ranges disjoint (words)
WORDS = {"vals": 40, "row_offs": 4, "row_uids": 3, "row_keep": 1, "out_keys": 40,
         "out_offs": 41, "out_vals": 40, "out_src": 40}
START = {"vals": 0, "row_offs": 64, "row_uids": 128, "row_keep": 192, "out_keys": 256,
         "out_offs": 320, "out_vals": 384, "out_src": 448}
OUTS = ("out_keys", "out_offs", "out_vals", "out_src")


class Arena:
    """Host memory standing in for device arrays: a rejected call never
    dereferences or writes any of it."""

    def __init__(self):
        self.buf = (C.c_uint64 * 1024)(*([POISON] * 1024))
        self.base = C.addressof(self.buf)

    def at(self, word):
        return self.base + 8 * word

    def desc(self, **over):
        d = _lib.UaDRowTr()
        for name, start in START.items():
            setattr(d, name, self.at(start))
        d.n_rows = 3
        d.total = 40
        d.flags = UNIQUE
        d.cap_keys = 40
        d.cap_vals = 40
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def untouched(self):
        return all(x == POISON for x in self.buf)


def call(d, ctx=True, ng=True, tot=True):
    L = _lib.lib()
    g, n = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    stand_in = C.create_string_buffer(4096)
    rc = L.ua_rows_transpose_dev(C.cast(stand_in, C.c_void_p) if ctx else None,
                                 C.byref(d) if d is not None else None,
                                 C.byref(g) if ng else None, C.byref(n) if tot else None)
    assert bytes(stand_in) == b"\0" * 4096, "a rejected call touched the context"
    assert g.value == SENTINEL and n.value == SENTINEL, "a rejected call wrote a size"
    return rc


def rejected(d, **kw):
    return call(d, **kw) == UA_ERR_INVALID


def test_null_arguments_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(), ctx=False)
    assert rejected(None)
    assert rejected(a.desc(), ng=False)
    assert rejected(a.desc(), tot=False)
    assert rejected(a.desc(vals=None))                      # total > 0
    assert rejected(a.desc(row_offs=None))                  # n_rows > 0
    assert a.untouched()


def test_shape_bounds_rejected_without_a_device():
    a = Arena()
    assert rejected(a.desc(n_rows=0))                       # elements without rows
    assert rejected(a.desc(n_rows=0, row_offs=None, row_uids=None, row_keep=None))
    assert rejected(a.desc(total=1 << 31))                  # 2^31 - 1 is the most
    assert rejected(a.desc(total=(1 << 64) - 1))
    assert rejected(a.desc(n_rows=1 << 31, row_uids=None, row_keep=None))
    assert rejected(a.desc(n_rows=(1 << 64) - 1, row_uids=None, row_keep=None))
    assert rejected(a.desc(cap_keys=1 << 60))
    assert rejected(a.desc(cap_vals=1 << 60))
    assert rejected(a.desc(cap_keys=(1 << 64) - 1))
    assert a.untouched()


def test_flag_and_form_rules_rejected_without_a_device():
    a = Arena()
    for flags in (2, 4, 1 << 32, 1 << 63, UNIQUE | 2):      # unknown bits
        assert rejected(a.desc(flags=flags)), flags
    none = dict(out_vals=None, out_src=None, cap_vals=0)    # the groups-only form
    assert rejected(a.desc(out_keys=None, **none))          # out_offs without out_keys
    assert rejected(a.desc(out_offs=None, **none))          # out_keys without out_offs
    assert rejected(a.desc(out_keys=None, out_offs=None, **none))   # NULL with cap_keys > 0
    assert rejected(a.desc(out_vals=None, out_src=None))    # NULL out_vals with cap_vals > 0
    assert rejected(a.desc(out_vals=None, cap_vals=0))      # out_src without out_vals
    assert rejected(a.desc(out_keys=None, out_offs=None, cap_keys=0))   # out_vals without keys
    assert rejected(a.desc(out_keys=None, out_offs=None, cap_keys=0, out_src=None))
    assert a.untouched()


def test_overlaps_rejected_without_a_device():
    a = Arena()
    for out in OUTS:
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
    assert rejected(a.desc(row_offs=a.at(320 + 40)))        # out_offs has cap_keys + 1 words
    assert rejected(a.desc(row_uids=a.at(384 + 39)))
    assert rejected(a.desc(row_keep=a.at(448)))
    assert a.untouched()


def test_host_form_rejects_without_a_device():
    L = _lib.lib()
    g, n = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    buf = (C.c_uint64 * 64)()
    buf[2] = 5                                              # row_offs[n_rows] of 2 rows
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    h8 = C.cast(buf, C.POINTER(C.c_uint8))
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    gg, nn = C.byref(g), C.byref(n)

    def call(c=cp, vals=hp, ro=hp, ru=hp, keep=h8, flags=UNIQUE, ok=hp, oo=hp, ck=8, ov=hp,
             osrc=hp, cv=8, pg=gg, pn=nn):
        return L.ua_rows_transpose(c, vals, ro, 2, ru, keep, flags, ok, oo, ck, ov, osrc, cv,
                                   pg, pn)

    assert call(c=None) == UA_ERR_INVALID
    assert call(vals=None) == UA_ERR_INVALID
    assert call(ro=None) == UA_ERR_INVALID
    assert call(pg=None) == UA_ERR_INVALID
    assert call(pn=None) == UA_ERR_INVALID
    assert call(flags=2) == UA_ERR_INVALID
    assert call(ok=None) == UA_ERR_INVALID
    assert call(oo=None) == UA_ERR_INVALID
    assert call(ok=None, oo=None, ov=None, osrc=None, cv=0) == UA_ERR_INVALID   # cap_keys > 0
    assert call(ov=None, osrc=None) == UA_ERR_INVALID       # NULL out_vals with a capacity
    assert call(ov=None, cv=0) == UA_ERR_INVALID            # out_src without out_vals
    assert call(ok=None, oo=None, ck=0) == UA_ERR_INVALID   # out_vals without out_keys
    assert call(ck=1 << 60) == UA_ERR_INVALID
    assert call(cv=1 << 60) == UA_ERR_INVALID
    buf[2] = 1 << 31
    assert call() == UA_ERR_INVALID                         # total >= 2^31
    assert g.value == SENTINEL and n.value == SENTINEL
    assert bytes(ctx) == b"\0" * 4096
