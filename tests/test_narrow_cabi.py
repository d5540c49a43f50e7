"""CPU-side checks of the narrow-tile observable's C-ABI surface (no GPU
compute): the library exports ua_batch_info, the header declares it and names
the prepared batch's third cache, and the ctypes layer binds it."""
import ctypes as C
import os
import re

from dgraph_amd import _lib
from dgraph_amd import algo

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   "include", "uidalgo.h")


def test_library_exports_batch_info():
    dll = C.CDLL(os.path.join(os.path.dirname(_lib.__file__), "libuidalgo.so"))
    assert hasattr(dll, "ua_batch_info")
    assert dll.ua_version() >= 13


def test_header_declares_batch_info_and_the_third_cache():
    txt = open(HDR).read()
    assert re.search(r"^\s*int\s+ua_batch_info\s*\(", txt, re.M)
    decl = txt[txt.index("int ua_batch_info"):]
    decl = decl[:decl.index(";")]
    assert decl.count("uint64_t *") == 3
    for words in ("THIRD", "4 B per input element", "UA_NARROW=0", "All three caches"):
        assert words in txt, words


def test_lib_binds_batch_info():
    L = _lib.lib()
    assert len(L.ua_batch_info.argtypes) == 5
    assert callable(algo.Batch.info)
