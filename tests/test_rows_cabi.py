"""CPU-side checks of the row-wise UID-matrix filter's C-ABI surface (no GPU
compute): the library exports both entry points, the header declares them,
the ctypes layer binds them with a ua_drows mirror of the right layout, and
the argument checks that need no device reject bad calls.
"""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")
UA_ERR_INVALID = 3


def test_library_exports_rows_filter():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    for name in ("ua_rows_filter_dev", "ua_rows_filter"):
        assert hasattr(dll, name), f"missing C-ABI export {name}"


def test_header_declares_rows_filter():
    txt = open(HDR).read()
    for name in ("ua_rows_filter_dev", "ua_rows_filter"):
        assert re.search(rf"^\s*int\s+{name}\s*\(", txt, re.M), name
    assert "UA_ROWS_INTERSECT = 0" in txt and "UA_ROWS_DIFFERENCE = 1" in txt
    assert "ua_drows" in txt


def test_lib_binds_rows_filter():
    L = _lib.lib()
    assert L.ua_rows_filter_dev.argtypes[1] == C.POINTER(_lib.UaDRows)
    assert len(L.ua_rows_filter_dev.argtypes) == 4
    assert len(L.ua_rows_filter.argtypes) == 10
    # ua_drows: 5 pointers + 3 u64, no padding
    assert C.sizeof(_lib.UaDRows) == 64
    assert [f[0] for f in _lib.UaDRows._fields_] == [
        "vals", "row_offs", "n_rows", "total", "shared", "m", "out_vals", "out_row_offs"]
    assert (algo.ROWS_INTERSECT, algo.ROWS_DIFFERENCE) == (0, 1)
    assert callable(algo.Engine.filter_rows) and callable(algo.update_uid_matrix)


def test_null_arguments_rejected_without_a_device():
    L = _lib.lib()
    kept = C.c_uint64()
    d = _lib.UaDRows()
    assert L.ua_rows_filter_dev(None, C.byref(d), 0, C.byref(kept)) == UA_ERR_INVALID
