"""CPU-side checks of the flat sort-unique DestUIDs path's C-ABI surface (no
GPU compute): the library exports both entry points, the header declares them
with the reference's call sites, the ctypes layer binds them, and the
argument checks that need no device reject bad calls.

ua_rows_union_dev checks its arguments before it touches the context, so the
overlap rule can be exercised without a device: the stand-in context below is
never read by a call that is rejected.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3
NAMES = ("ua_rows_union_dev", "ua_rows_union")


def test_library_exports_rows_union():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in NAMES:
        assert hasattr(dll, name), f"missing C-ABI export {name}"


def test_header_declares_rows_union():
    txt = open(HDR).read()
    for name in NAMES:
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    # the call sites this replaces, and the contract's fine print
    for cite in ("query.go:1874", "2290", "2505", "recurse.go:134", "task.go:1629",
                 "trigram.go:87", "match.go:100", "2594-2609"):
        assert cite in txt, cite
    decl = txt[txt.index("int ua_rows_union_dev"):]
    decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
    assert "row_offs" not in decl and decl.count(",") == 4


def test_lib_binds_rows_union():
    L = _lib.lib()
    assert len(L.ua_rows_union_dev.argtypes) == 5
    assert len(L.ua_rows_union.argtypes) == 5
    assert L.ua_rows_union_dev.argtypes[2] == C.c_uint64
    assert L.ua_rows_union.argtypes[2] == C.c_uint64
    assert L.ua_version() >= 12
    for fn in (algo.Engine.union_rows, algo.dest_uids, algo.update_dest_uids):
        assert callable(fn)


def test_null_arguments_rejected_without_a_device():
    L = _lib.lib()
    n = C.c_uint64(77)
    buf = (C.c_uint64 * 16)()
    p = C.cast(buf, C.c_void_p)
    hp = C.cast(buf, C.POINTER(C.c_uint64))
    # null ctx
    assert L.ua_rows_union_dev(None, p, 16, p, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union(None, hp, 16, hp, C.byref(n)) == UA_ERR_INVALID
    # total == 0 with a null ctx: like ua_rows_filter_dev, a null ctx is invalid
    # whatever the sizes
    assert L.ua_rows_union_dev(None, None, 0, None, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union(None, None, 0, None, C.byref(n)) == UA_ERR_INVALID
    assert n.value == 77  # rejected calls write nothing

    ctx = C.create_string_buffer(4096)  # stand-in: a rejected call never reads it
    cp = C.cast(ctx, C.c_void_p)
    assert L.ua_rows_union_dev(cp, p, 16, p, None) == UA_ERR_INVALID      # null out_n
    assert L.ua_rows_union_dev(cp, None, 16, p, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union_dev(cp, p, 16, None, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union(cp, hp, 16, hp, None) == UA_ERR_INVALID
    assert L.ua_rows_union(cp, None, 16, hp, C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union(cp, hp, 16, None, C.byref(n)) == UA_ERR_INVALID
    assert n.value == 77


def test_overlap_and_size_bound_rejected_without_a_device():
    L = _lib.lib()
    n = C.c_uint64(77)
    buf = (C.c_uint64 * 64)()
    base = C.addressof(buf)
    ctx = C.create_string_buffer(4096)
    cp = C.cast(ctx, C.c_void_p)
    # out shifted into vals by 8 elements, either way round; out == vals is the
    # one allowed overlap and therefore needs a real context (GPU tests)
    assert L.ua_rows_union_dev(cp, C.c_void_p(base), 32, C.c_void_p(base + 64),
                               C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union_dev(cp, C.c_void_p(base + 64), 32, C.c_void_p(base),
                               C.byref(n)) == UA_ERR_INVALID
    assert L.ua_rows_union_dev(cp, C.c_void_p(base), 32, C.c_void_p(base + 8 * 31),
                               C.byref(n)) == UA_ERR_INVALID
    # more tiles than the tree's int counts hold: total > (2^31 - 1) * 2048
    assert L.ua_rows_union_dev(cp, C.c_void_p(base), ((1 << 31) - 1) * 2048 + 1,
                               C.c_void_p(base), C.byref(n)) == UA_ERR_INVALID
    assert n.value == 77
    assert bytes(ctx) == b"\0" * 4096
