"""CPU-side checks of the fast-tile observable's C-ABI surface (no GPU
compute): the library exports ua_batch_fast_tiles at version 15, the header
declares it, and the ctypes layer binds it."""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")


def test_library_exports_fast_tiles():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    assert hasattr(dll, "ua_batch_fast_tiles")
    assert dll.ua_version() >= 15


def test_header_declares_fast_tiles():
    txt = open(HDR).read()
    assert re.search(r"^\s*int\s+ua_batch_fast_tiles\s*\(", txt, re.M)
    decl = txt[txt.index("int ua_batch_fast_tiles"):]
    decl = decl[:decl.index(";")]
    assert decl.count("uint64_t *") == 1 and "ua_batch *" in decl
    assert "(since v15)" in txt


def test_lib_binds_fast_tiles():
    L = _lib.lib()
    assert len(L.ua_batch_fast_tiles.argtypes) == 3
    assert callable(algo.Batch.fast_tiles)
