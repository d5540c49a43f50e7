"""ctypes loader for libuidalgo.so (the product C-ABI, include/uidalgo.h).

Fails loudly if the extension is missing — the product path has no CPU
fallback by design (the Go caller keeps its own fallback).
"""
import ctypes as C
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
# UA_LIB_PATH overrides the library for perf-bisection builds (tools/ubench.py)
_LIB_PATH = os.environ.get("UA_LIB_PATH", os.path.join(_DIR, "libuidalgo.so"))

UA_OK = 0

_u64 = C.c_uint64
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_i64p = C.POINTER(C.c_int64)
_voidpp = C.POINTER(C.c_void_p)


class UaDPair(C.Structure):
    _fields_ = [
        ("u", C.c_void_p),
        ("n", _u64),
        ("v", C.c_void_p),
        ("m", _u64),
        ("out", C.c_void_p),
    ]


class UaDPack(C.Structure):
    _fields_ = [
        ("block_size", C.c_uint32),
        ("n_blocks", _u64),
        ("bases", C.c_void_p),
        ("num_uids", C.c_void_p),
        ("delta_offs", C.c_void_p),
        ("deltas", C.c_void_p),
        ("total_uids", _u64),
    ]


class UaDFilter(C.Structure):
    _fields_ = [
        ("u", C.c_void_p),
        ("n", _u64),
        ("mask", C.c_void_p),
        ("out", C.c_void_p),
    ]


class UaDSeg(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("n", _u64),
        ("tmp", C.c_void_p),
    ]


class UaDRows(C.Structure):
    _fields_ = [
        ("vals", C.c_void_p),
        ("row_offs", C.c_void_p),
        ("n_rows", _u64),
        ("total", _u64),
        ("shared", C.c_void_p),
        ("m", _u64),
        ("out_vals", C.c_void_p),
        ("out_row_offs", C.c_void_p),
    ]


# the three pack fan-out -> CSR descriptors share their first nine slots (the
# block arena, the row boundaries, after, first) and their last three
_ROW_ARENA = [
    ("bases", C.c_void_p),
    ("num_uids", C.c_void_p),
    ("delta_offs", C.c_void_p),
    ("deltas", C.c_void_p),
    ("n_blocks", _u64),
    ("row_block_base", C.c_void_p),
    ("n_rows", _u64),
    ("after", C.c_void_p),
]
_ROW_PREFIX = _ROW_ARENA + [("first", C.c_void_p)]
_ROW_OUT = [
    ("out_vals", C.c_void_p),
    ("cap_vals", _u64),
    ("out_row_offs", C.c_void_p),
]


class UaDRowPacks(C.Structure):
    _fields_ = _ROW_PREFIX + _ROW_OUT


class UaDRowIsect(C.Structure):  # slot 8 must stay NULL: this call has no first
    _fields_ = _ROW_ARENA + [("reserved", C.c_void_p), ("shared", C.c_void_p),
                             ("m", _u64)] + _ROW_OUT


class UaDRowMut(C.Structure):
    _fields_ = _ROW_PREFIX + [("mut_uids", C.c_void_p), ("mut_ops", C.c_void_p),
                              ("row_mut_base", C.c_void_p), ("n_mut", _u64)] + _ROW_OUT


class UaDRowEnc(C.Structure):
    _fields_ = [
        ("vals", C.c_void_p),
        ("row_offs", C.c_void_p),
        ("n_rows", _u64),
        ("total", _u64),
        ("block_size", _u64),
        ("bases", C.c_void_p),
        ("num_uids", C.c_void_p),
        ("delta_offs", C.c_void_p),
        ("cap_blocks", _u64),
        ("deltas", C.c_void_p),
        ("cap_deltas", _u64),
        ("row_block_base", C.c_void_p),
    ]


UA_SORT_DESC = 1
UA_SORT_MULTI = 2
UA_SORT_DROP_NULLS = 4


class UaDRowSort(C.Structure):
    _fields_ = [
        ("vals", C.c_void_p),
        ("row_offs", C.c_void_p),
        ("n_rows", _u64),
        ("total", _u64),
        ("keys", C.c_void_p),
        ("has", C.c_void_p),
        ("flags", _u64),
        ("count", C.c_int32),
        ("offset", C.c_int32),
        ("out_vals", C.c_void_p),
        ("cap_vals", _u64),
        ("out_row_offs", C.c_void_p),
        ("out_src", C.c_void_p),
        ("out_ms_offs", C.c_void_p),
    ]


UA_TR_UNIQUE = 1


class UaDRowTr(C.Structure):
    _fields_ = [
        ("vals", C.c_void_p),
        ("row_offs", C.c_void_p),
        ("n_rows", _u64),
        ("total", _u64),
        ("row_uids", C.c_void_p),
        ("row_keep", C.c_void_p),
        ("flags", _u64),
        ("out_keys", C.c_void_p),
        ("out_offs", C.c_void_p),
        ("cap_keys", _u64),
        ("out_vals", C.c_void_p),
        ("out_src", C.c_void_p),
        ("cap_vals", _u64),
    ]


class UaPTask(C.Structure):
    _fields_ = [
        ("v", C.c_void_p),
        ("m", _u64),
        ("out", C.c_void_p),
        ("after_uid", _u64),
    ]


class UaBlock(C.Structure):
    _fields_ = [
        ("base", _u64),
        ("num_uids", C.c_uint32),
        ("deltas_len", C.c_uint32),
        ("deltas", _u8p),
    ]


class UaPack(C.Structure):
    _fields_ = [
        ("block_size", C.c_uint32),
        ("n_blocks", _u64),
        ("blocks", C.POINTER(UaBlock)),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"libuidalgo.so not found at {_LIB_PATH}: the HIP extension is "
                "mandatory — run __graft_entry__.build() (hipcc "
                "--offload-arch=gfx950).")
        L = C.CDLL(_LIB_PATH)
        L.ua_strerror.restype = C.c_char_p
        L.ua_strerror.argtypes = [C.c_int]
        L.ua_version.restype = C.c_int
        L.ua_ctx_create.argtypes = [_voidpp, C.c_int]
        L.ua_ctx_destroy.argtypes = [C.c_void_p]
        L.ua_dev_alloc.argtypes = [C.c_void_p, _u64, _voidpp]
        L.ua_dev_free.argtypes = [C.c_void_p, C.c_void_p]
        L.ua_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _u64]
        L.ua_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, _u64]
        L.ua_sync.argtypes = [C.c_void_p]
        L.ua_stats_reset.argtypes = [C.c_void_p]
        L.ua_stats_get.argtypes = [C.c_void_p, _u64p, C.POINTER(C.c_double), _u64p]
        L.ua_intersect_batch_dev.argtypes = [C.c_void_p, C.POINTER(UaDPair), C.c_int, _u64p]
        L.ua_batch_create.argtypes = [C.c_void_p, C.POINTER(UaDPair), C.c_int, _voidpp]
        L.ua_batch_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, _u64p]
        L.ua_batch_run_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, _u64p]
        L.ua_batch_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.ua_batch_destroy.restype = None
        if L.ua_version() >= 13:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_batch_info.argtypes = [C.c_void_p, C.c_void_p, _u64p, _u64p, _u64p]
        if L.ua_version() >= 15:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_batch_fast_tiles.argtypes = [C.c_void_p, C.c_void_p, _u64p]
        L.ua_merge_batch_dev.argtypes = [C.c_void_p, C.POINTER(UaDPair), C.c_int, _u64p]
        L.ua_difference_batch_dev.argtypes = [C.c_void_p, C.POINTER(UaDPair), C.c_int, _u64p]
        L.ua_merge_all_batch_dev.argtypes = [C.c_void_p, C.POINTER(UaDPair), C.c_int, _u64p]
        L.ua_sort_segments_dev.argtypes = [C.c_void_p, C.POINTER(UaDSeg), C.c_int]
        L.ua_index_of_batch_dev.argtypes = [C.c_void_p, C.c_void_p, _u64, C.c_void_p, _u64,
                                            C.c_void_p]
        L.ua_apply_filter_batch_dev.argtypes = [C.c_void_p, C.POINTER(UaDFilter),
                                                C.c_int, _u64p]
        L.ua_apply_filter.argtypes = [C.c_void_p, _u64p, _u64, _u8p, _u64p]
        L.ua_rows_filter_dev.argtypes = [C.c_void_p, C.POINTER(UaDRows), C.c_int, _u64p]
        L.ua_rows_filter.argtypes = [C.c_void_p, _u64p, _u64p, _u64, _u64p, _u64, C.c_int,
                                     _u64p, _u64p, _u64p]
        L.ua_rows_union_dev.argtypes = [C.c_void_p, C.c_void_p, _u64, C.c_void_p, _u64p]
        L.ua_rows_union.argtypes = [C.c_void_p, _u64p, _u64, _u64p, _u64p]
        if L.ua_version() >= 14:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_rows_decode_dev.argtypes = [C.c_void_p, C.POINTER(UaDRowPacks), _u64p]
            L.ua_rows_decode.argtypes = [C.c_void_p, C.POINTER(C.POINTER(UaPack)), _u64,
                                         _u64p, C.POINTER(C.c_int32), _u64p, _u64, _u64p,
                                         _u64p]
        if L.ua_version() >= 16:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_rows_intersect_packed_dev.argtypes = [C.c_void_p, C.POINTER(UaDRowIsect),
                                                       _u64p]
            L.ua_rows_intersect_packed.argtypes = [
                C.c_void_p, C.POINTER(C.POINTER(UaPack)), _u64, _u64p, _u64p, _u64, _u64p,
                _u64, _u64p, _u64p]
        if L.ua_version() >= 17:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_rows_decode_mut_dev.argtypes = [C.c_void_p, C.POINTER(UaDRowMut), _u64p]
            L.ua_rows_decode_mut.argtypes = [
                C.c_void_p, C.POINTER(C.POINTER(UaPack)), _u64, _u64p, _u8p, _u64p, _u64p,
                C.POINTER(C.c_int32), _u64p, _u64, _u64p, _u64p]
        if L.ua_version() >= 18:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_rows_encode_dev.argtypes = [C.c_void_p, C.POINTER(UaDRowEnc), _u64p, _u64p]
            L.ua_rows_encode.argtypes = [
                C.c_void_p, _u64p, _u64p, _u64, _u64, _u64p, _u32p, _u64p, _u64, _u8p, _u64,
                _u64p, _u64p, _u64p]
        if L.ua_version() >= 19:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_rows_sort_dev.argtypes = [C.c_void_p, C.POINTER(UaDRowSort), _u64p]
            L.ua_rows_sort.argtypes = [
                C.c_void_p, _u64p, _u64p, _u64, _u64p, _u8p, _u64, C.c_int32, C.c_int32,
                _u64p, _u64, _u64p, _u64p, C.POINTER(C.c_int32), _u64p]
        if L.ua_version() >= 20:  # an older library via UA_LIB_PATH (A/B runs)
            L.ua_rows_transpose_dev.argtypes = [C.c_void_p, C.POINTER(UaDRowTr), _u64p, _u64p]
            L.ua_rows_transpose.argtypes = [
                C.c_void_p, _u64p, _u64p, _u64, _u64p, _u8p, _u64, _u64p, _u64p, _u64,
                _u64p, _u64p, _u64, _u64p, _u64p]
        L.ua_intersect_k_dev.argtypes = [C.c_void_p, _voidpp, _u64p, C.c_int, C.c_void_p, _u64p]
        L.ua_merge_k_dev.argtypes = [C.c_void_p, _voidpp, _u64p, C.c_int, C.c_void_p, _u64p]
        L.ua_intersect_packed_dev.argtypes = [C.c_void_p, C.POINTER(UaDPack), _u64, C.c_void_p,
                                              _u64, C.c_void_p, _u64p]
        L.ua_intersect_packed_batch_dev.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            _u64p, C.c_int, C.POINTER(UaPTask), _u64p]
        L.ua_pbatch_create.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
            _u64p, C.c_int, C.POINTER(UaPTask), _voidpp]
        L.ua_pbatch_run.argtypes = [C.c_void_p, C.c_void_p, _u64p]
        L.ua_pbatch_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.ua_pbatch_destroy.restype = None
        L.ua_decode_dev.argtypes = [C.c_void_p, C.POINTER(UaDPack), _u64, C.c_void_p, _u64p]
        L.ua_encode.argtypes = [_u64p, _u64, C.c_uint32, _voidpp]
        L.ua_encode_dev.argtypes = [C.c_void_p, C.c_void_p, _u64, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    _u64p, _u64p]
        L.ua_owned_pack_view.restype = C.POINTER(UaPack)
        L.ua_owned_pack_view.argtypes = [C.c_void_p]
        L.ua_owned_pack_free.argtypes = [C.c_void_p]
        L.ua_pack_exact_len.restype = _u64
        L.ua_pack_exact_len.argtypes = [C.POINTER(UaPack)]
        L.ua_pack_approx_len.restype = _u64
        L.ua_pack_approx_len.argtypes = [C.POINTER(UaPack)]
        L.ua_pack_flat_sizes.argtypes = [C.POINTER(UaPack), _u64p, _u64p, _u64p]
        L.ua_pack_flatten.argtypes = [C.POINTER(UaPack), _u64p, _u32p, _u64p, _u8p]
        L.ua_intersect.argtypes = [C.c_void_p, _u64p, _u64, _u64p, _u64, _u64p, _u64p]
        L.ua_intersect_k.argtypes = [C.c_void_p, C.POINTER(_u64p), _u64p, C.c_int, _u64p, _u64p]
        L.ua_merge_k.argtypes = [C.c_void_p, C.POINTER(_u64p), _u64p, C.c_int, _u64p, _u64p]
        L.ua_difference.argtypes = [C.c_void_p, _u64p, _u64, _u64p, _u64, _u64p, _u64p]
        L.ua_index_of.restype = C.c_int64
        L.ua_index_of.argtypes = [_u64p, _u64, _u64]
        L.ua_intersect_packed.argtypes = [C.c_void_p, C.POINTER(UaPack), _u64, _u64p, _u64,
                                          _u64p, _u64p]
        _lib = L
    return _lib


def check(rc):
    if rc != UA_OK:
        msg = lib().ua_strerror(rc).decode()
        raise RuntimeError(f"uidalgo error {rc}: {msg}")
