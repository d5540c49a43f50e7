"""CPU-side check of the overlap rules of the three pack fan-out -> CSR device
entries (no GPU compute).  ua_rows_decode_dev, ua_rows_intersect_packed_dev and
ua_rows_decode_mut_dev share one argument check that a per-call table drives;
the header states a different rule for each call, and the one table below pins
all three: which input may not overlap which output.

Only rejection can be observed without a device.  A pair the header allows
(out_row_offs over the pack arrays, after or first in the two decode calls)
passes the argument check, and what follows locks the context and enqueues
work, so there is no later, unrelated rejection to assert it through: the
allowed pairs are listed in the table and not called.
"""
import ctypes as C

import pytest

from dgraph_amd import _lib

UA_ERR_INVALID = 3
SENTINEL = 77
OUTPUTS = {"out_row_offs": 96, "out_vals": 128}     # 4 and 64 words
VALS, BOTH = ("out_vals",), ("out_vals", "out_row_offs")

# per call: entry, descriptor, its own slots on top of the shared layout, and
# for every input the outputs it must not overlap (the header's "rejected
# with UA_ERR_INVALID" paragraphs)
CALLS = {
    "decode": ("ua_rows_decode_dev", _lib.UaDRowPacks, {"first": 80},
               {"bases": VALS, "num_uids": VALS, "delta_offs": VALS, "deltas": VALS,
                "row_block_base": BOTH, "after": VALS, "first": VALS}),
    "intersect": ("ua_rows_intersect_packed_dev", _lib.UaDRowIsect, {"shared": 80, "m": 6},
                  {"bases": BOTH, "num_uids": BOTH, "delta_offs": BOTH, "deltas": BOTH,
                   "row_block_base": BOTH, "after": BOTH, "shared": BOTH}),
    "decode_mut": ("ua_rows_decode_mut_dev", _lib.UaDRowMut,
                   {"first": 80, "mut_uids": 200, "mut_ops": 216, "row_mut_base": 224,
                    "n_mut": 6},
                   {"bases": VALS, "num_uids": VALS, "delta_offs": VALS, "deltas": VALS,
                    "row_block_base": BOTH, "after": VALS, "first": VALS,
                    "mut_uids": BOTH, "mut_ops": BOTH, "row_mut_base": BOTH}),
}


class Arena:
    """Host memory standing in for device arrays: a rejected call never
    dereferences any of it."""

    def __init__(self):
        self.buf = (C.c_uint64 * 1024)()
        self.base = C.addressof(self.buf)

    def at(self, word):
        return self.base + 8 * word

    def desc(self, cls, own, **over):
        # the well-formed call of the per-call cabi tests: 4 blocks, 3 rows,
        # all ranges disjoint
        d = cls()
        d.bases = self.at(0)
        d.num_uids = self.at(8)
        d.delta_offs = self.at(16)
        d.deltas = self.at(32)
        d.n_blocks = 4
        d.row_block_base = self.at(64)
        d.n_rows = 3
        d.after = self.at(72)
        d.out_vals = self.at(OUTPUTS["out_vals"])
        d.cap_vals = 64
        d.out_row_offs = self.at(OUTPUTS["out_row_offs"])
        for k, v in own.items():
            setattr(d, k, v if k in ("m", "n_mut") else self.at(v))
        for k, v in over.items():
            setattr(d, k, v)
        return d


def rejected(entry, d):
    n = C.c_uint64(SENTINEL)
    stand_in = C.create_string_buffer(4096)
    rc = getattr(_lib.lib(), entry)(C.cast(stand_in, C.c_void_p), C.byref(d), C.byref(n))
    assert bytes(stand_in) == b"\0" * 4096, "a rejected call touched the context"
    assert n.value == SENTINEL, "a rejected call wrote out_total"
    return rc == UA_ERR_INVALID


@pytest.mark.parametrize("call", sorted(CALLS))
def test_the_table_names_every_input_of_the_descriptor(call):
    _, cls, own, rule = CALLS[call]
    counts = {"n_blocks", "n_rows", "m", "n_mut", "cap_vals", "reserved"}
    inputs = [f for f, _ in cls._fields_ if f not in counts and f not in OUTPUTS]
    assert sorted(inputs) == sorted(rule)


@pytest.mark.parametrize("call", sorted(CALLS))
def test_each_input_is_rejected_over_the_outputs_its_call_names(call):
    entry, cls, own, rule = CALLS[call]
    a = Arena()
    for field, outs in rule.items():
        for out in outs:
            # the input laid on the output's first word, and the output on the input's
            assert rejected(entry, a.desc(cls, own, **{field: a.at(OUTPUTS[out])})), (field, out)
            where = getattr(a.desc(cls, own), field)
            assert rejected(entry, a.desc(cls, own, **{out: where})), (out, field)
    # the two outputs over each other, in every call
    assert rejected(entry, a.desc(cls, own, out_row_offs=a.at(OUTPUTS["out_vals"] + 63)))
    assert bytes(a.buf) == b"\0" * 8192
