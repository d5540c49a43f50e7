"""GPU codec kernels against the format itself: the fused group-varint
decode / decode+intersect kernel, the GPU encoder and the pack fan-out, on
inputs that reach all 256 control bytes, every delta-length boundary, the
1085-byte block, 0 and UINT64_MAX, empty packs and the 2048-entry scan chunk.

Packs are uploaded from the bytes of tests/gv_spec.py (anchored on
hand-derived literals in tests/test_codec_spec.py), never from an engine
encoder, so a decoder failure cannot come from an encoder and the other way
round.  Expected values are plain set arithmetic on Python integers:
  decode with a seek:  [x for x in uids if x >= seek]
  intersect:           [x for x in v if x in uids and x >= after]
(Decoder.Seek with SeekStart, codec.go:279).  The oracle is asserted against
the same arithmetic, so a disagreement names the culprit.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gv_spec as gv
from dgraph_amd import _lib, algo
from dgraph_amd._lib import UaPTask
from oracle import bind as orc

pytestmark = pytest.mark.gpu

UA_ERR_INVALID = 3
INPUTS = gv.inputs()
NAMES = sorted(INPUTS)


@pytest.fixture(scope="module")
def eng():
    e = algo.Engine(0)
    yield e
    e.close()


def to_dev(vals):
    """Python ints -> device int64 holding the u64 bits (never empty, so the
    pointer is always real) and the true length."""
    a = gv.u64(vals)
    if a.size == 0:
        return torch.zeros(1, dtype=torch.int64, device="cuda:0"), 0
    return torch.from_numpy(a.view(np.int64)).to("cuda:0"), a.size


def to_list(t, n=None):
    return t.cpu().numpy().view(np.uint64)[:n].tolist()


def upload(eng, blocks, bs):
    return eng.upload_pack(*gv.flatten(blocks), bs)


def decode_dev(eng, dp, seek, cap=None):
    """ua_decode_dev -> (status, uids)."""
    out = torch.empty(max(cap or dp.total_uids, 1), dtype=torch.int64, device="cuda:0")
    out_n = C.c_uint64(77)
    pk = dp.struct()
    rc = _lib.lib().ua_decode_dev(eng._ctx, C.byref(pk), seek, C.c_void_p(out.data_ptr()),
                                  C.byref(out_n))
    return rc, to_list(out, out_n.value), out_n.value


def intersect_dev(eng, dp, after, dv, m):
    """ua_intersect_packed_dev -> (status, uids)."""
    out = torch.empty(max(min(dp.total_uids, m), 1), dtype=torch.int64, device="cuda:0")
    out_n = C.c_uint64(77)
    pk = dp.struct()
    rc = _lib.lib().ua_intersect_packed_dev(
        eng._ctx, C.byref(pk), after, C.c_void_p(dv.data_ptr()), m,
        C.c_void_p(out.data_ptr()), C.byref(out_n))
    return rc, to_list(out, out_n.value), out_n.value


def want_decode(uids, seek):
    return [x for x in uids if x >= seek]


def want_intersect(uids, v, after):
    have = set(uids)
    return [x for x in v if x in have and x >= after]


def v_lists(uids, blocks):
    """The v shapes of the issue, as {name: sorted Python ints}."""
    near = sorted({y for x in uids for y in (x - 1, x + 1) if 0 <= y <= gv.U64_MAX})
    out = {"all": list(uids), "near": near, "third": list(uids[::3]),
           "bases": [b for b, _, _ in blocks],
           "lasts": [gv.decode([b])[-1] for b in blocks], "none": []}
    if uids[0] >= 3:
        out["below"] = [uids[0] - 3, uids[0] - 1]
    if uids[-1] <= gv.U64_MAX - 3:
        out["above"] = [uids[-1] + 1, uids[-1] + 3]
    return out


# ---------- encoder: ua_encode_dev against gv_spec bytes ----------

FILL = 0xA5


def encode_dev_checked(eng, uids, bs):
    """Run ua_encode_dev into buffers of exactly the documented capacity,
    pre-filled with 0xA5, and hold every output to gv_spec."""
    n = len(uids)
    du, _ = to_dev(uids)
    caps = (8 * n, 4 * n, 8 * (n + 1), 6 * n + 24)
    bufs = [torch.full((c,), FILL, dtype=torch.uint8, device="cuda:0") for c in caps]
    nb, db = C.c_uint64(77), C.c_uint64(77)
    rc = _lib.lib().ua_encode_dev(
        eng._ctx, C.c_void_p(du.data_ptr()), n, bs, *[C.c_void_p(b.data_ptr()) for b in bufs],
        C.byref(nb), C.byref(db))
    assert rc == 0
    blocks = gv.encode(uids, bs)
    wb, wn, wo, wd = gv.flatten(blocks)
    assert nb.value == len(blocks)
    assert db.value == wd.size
    raw = [b.cpu().numpy() for b in bufs]
    k = nb.value
    assert raw[0][:8 * k].view(np.uint64).tolist() == wb.tolist()
    assert raw[1][:4 * k].view(np.uint32).tolist() == wn.tolist()
    assert raw[2][:8 * (k + 1)].view(np.uint64).tolist() == wo.tolist()
    assert raw[3][:db.value].tobytes() == wd.tobytes()
    for r, used, name in zip(raw, (8 * k, 4 * k, 8 * (k + 1), db.value),
                             ("bases", "num_uids", "delta_offs", "deltas")):
        assert (r[used:] == FILL).all(), f"{name}: write past the used prefix"


@pytest.mark.parametrize("bs", gv.BLOCK_SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_encode_dev_matches_spec_bytes(eng, name, bs):
    encode_dev_checked(eng, INPUTS[name], bs)


@pytest.mark.parametrize("bs", [1, 256])
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4095, 4096, 4097])
def test_encode_dev_scan_chunk_boundary(eng, n, bs):
    """The encoder's scans run over n + 1 flags in chunks of 2048: a 32-MSB
    run boundary at index 2048 and another at n - 1."""
    encode_dev_checked(eng, gv.long_list(n, {2048, n - 1}), bs)


@pytest.mark.parametrize("which", ["low", "high"])
def test_encode_decode_round_trip(eng, which):
    uids = gv.tag_ladder(which, "b")
    du, _ = to_dev(uids)
    for bs in (0, 5, 256):
        dp = eng.encode_dev(du, bs)
        assert to_list(eng.decode_pack(dp)) == uids, bs


# ---------- decoder and fused intersect, packs from gv_spec bytes ----------

@pytest.mark.parametrize("name", NAMES)
def test_decode_and_intersect_every_input(eng, name):
    uids = INPUTS[name]
    for bs in (1, 4, 5, 256):
        blocks = gv.encode(uids, bs)
        dp = upload(eng, blocks, bs)
        opack = orc.Pack(gv.u64(uids), bs)
        assert opack.decode(0).tolist() == uids
        rc, got, _ = decode_dev(eng, dp, 0)
        assert (rc, got) == (0, uids), f"decode bs={bs}"
        for vname, v in v_lists(uids, blocks).items():
            want = want_intersect(uids, v, 0)
            assert orc.intersect_compressed_with(opack, 0, gv.u64(v)).tolist() == want
            dv, m = to_dev(v)
            rc, got, _ = intersect_dev(eng, dp, 0, dv, m)
            assert (rc, got) == (0, want), f"intersect bs={bs} v={vname}"


@pytest.fixture(scope="module")
def seek_case(eng):
    uids = gv.seek_pack()
    blocks = gv.encode(uids, 9)
    assert len(blocks) <= 40 and 0 in uids and gv.U64_MAX in uids
    return uids, blocks, upload(eng, blocks, 9), orc.Pack(gv.u64(uids), 9)


def test_decode_seek_sweep(eng, seek_case):
    """A seek at, just before and just after every block's base and last uid,
    in the gaps between blocks, and at 0, 1, UINT64_MAX - 1, UINT64_MAX."""
    uids, blocks, dp, opack = seek_case
    seeks = gv.seek_list(blocks)
    assert len(seeks) <= 300 and {0, 1, gv.U64_MAX - 1, gv.U64_MAX} <= set(seeks)
    for s in seeks:
        want = want_decode(uids, s)
        assert opack.decode(s).tolist() == want, f"oracle seek={s:#x}"
        rc, got, _ = decode_dev(eng, dp, s)
        assert (rc, got) == (0, want), f"seek={s:#x}"
    assert want_decode(uids, gv.U64_MAX) == [gv.U64_MAX]


def test_intersect_after_sweep(eng, seek_case):
    uids, blocks, dp, opack = seek_case
    seeks = gv.seek_list(blocks)
    afters = sorted(set(seeks[::max(len(seeks) // 16, 1)]) |
                    {0, 1, gv.U64_MAX - 1, gv.U64_MAX, blocks[3][0], blocks[3][0] + 1})
    assert len(afters) <= 26
    for vname, v in v_lists(uids, blocks).items():
        dv, m = to_dev(v)
        ov = gv.u64(v)
        for a in afters:
            want = want_intersect(uids, v, a)
            assert orc.intersect_compressed_with(opack, a, ov).tolist() == want, \
                f"oracle v={vname} after={a:#x}"
            rc, got, _ = intersect_dev(eng, dp, a, dv, m)
            assert (rc, got) == (0, want), f"v={vname} after={a:#x}"
    # the two ends of the uid space, present in pack and v alike
    assert want_intersect(uids, uids, gv.U64_MAX) == [gv.U64_MAX]
    assert want_intersect(uids, uids, 0)[0] == 0


@pytest.mark.parametrize("nb", [2046, 2047, 2048, 2049, 4095, 4096])
def test_packed_scan_chunk_boundary(eng, nb):
    """One-uid blocks: the count scan runs over nb + 1 entries in chunks of
    2048.  v hits every 64th block and the last one."""
    uids = gv.long_list(nb)
    blocks = gv.encode(uids, 1)
    assert len(blocks) == nb
    dp = upload(eng, blocks, 1)
    opack = orc.Pack(gv.u64(uids), 1)
    mid = uids[nb // 2]
    for s in (0, mid, uids[-1]):
        want = want_decode(uids, s)
        assert opack.decode(s).tolist() == want
        rc, got, _ = decode_dev(eng, dp, s)
        assert (rc, got) == (0, want), f"seek={s:#x}"
    v = sorted(set(uids[::64]) | {uids[-1]} | {x + 1 for x in uids[32::64]})
    dv, m = to_dev(v)
    for a in (0, mid + 1):
        want = want_intersect(uids, v, a)
        assert orc.intersect_compressed_with(opack, a, gv.u64(v)).tolist() == want
        rc, got, _ = intersect_dev(eng, dp, a, dv, m)
        assert (rc, got) == (0, want), f"after={a:#x}"


# ---------- fan-out: one-shot and prepared ----------

def trim(uids, bs, max_blocks=64):
    blocks = gv.encode(uids, bs)
    return gv.decode(blocks[:max_blocks])


def fan_packs():
    """(uids, block_size) per pack: cuts of the shared inputs at mixed block
    sizes, at most 64 blocks each; empty packs first, last, singly in the
    middle and three in a row; one-block packs."""
    I = INPUTS
    E = ([], 256)
    cuts = [
        E,
        (I["full_block"], 256),                # one block of 1085 bytes
        (I["edge_values"], 256),
        (I["ladder_a_low"][:320], 256),
        E,
        (I["ladder_a_high"][640:900], 4),
        (I["ladder_b_low"][:500], 9),
        (I["ladder_b_high"][100:400], 7),
        E, E, E,
        ([gv.U64_MAX], 0),                     # one block, one uid
        ([0], 1),
        (I["ladder_b_high"][:256], 256),
        (I["ladder_b_low"][300:556], 255),
        (I["ladder_a_high"][1000:1150], 5),
        (I["ladder_a_low"][7:107], 3),
        (I["edge_values"], 0),
        (I["ladder_b_low"][513:700], 6),
        (I["ladder_b_high"][700:900], 2),
        (I["full_block"][3:200], 5),
        (I["ladder_b_low"][:64], 1),
        (I["ladder_a_high"][:64], 0),
        E,
    ]
    return [(trim(u, bs), bs) for u, bs in cuts]


class Fan:
    """A fan-out's host-side arguments over an uploaded arena."""

    def __init__(self, eng, flats, vs, afters):
        self.eng = eng
        self.n = len(flats)
        self.dpb = eng.upload_pack_batch(
            [(*gv.flatten(blocks), sum(nu for _, nu, _ in blocks)) for blocks in flats])
        self.pbb = (C.c_uint64 * (self.n + 1))(*[int(x) for x in self.dpb.pbb])
        self.dvs = {id(v): to_dev(v) for v in vs}  # a shared v uploads once
        self.vs, self.afters = vs, afters

    def tasks(self):
        outs = []
        tasks = (UaPTask * self.n)()
        for i, v in enumerate(self.vs):
            dv, m = self.dvs[id(v)]
            outs.append(torch.full((max(min(self.dpb.pack_totals[i], m), 1),), -1,
                                   dtype=torch.int64, device="cuda:0"))
            tasks[i].v, tasks[i].m = dv.data_ptr(), m
            tasks[i].out, tasks[i].after_uid = outs[i].data_ptr(), self.afters[i]
        return tasks, outs

    def arena(self):
        d = self.dpb
        return (self.eng._ctx, C.c_void_p(d.bases.data_ptr()),
                C.c_void_p(d.num_uids.data_ptr()), C.c_void_p(d.delta_offs.data_ptr()),
                C.c_void_p(d.deltas.data_ptr()), self.pbb, self.n)

    def one_shot(self):
        tasks, outs = self.tasks()
        lens = (C.c_uint64 * self.n)(*([77] * self.n))
        rc = _lib.lib().ua_intersect_packed_batch_dev(*self.arena(), tasks, lens)
        return rc, [to_list(outs[i], lens[i]) for i in range(self.n)], list(lens)

    def prepared(self, runs=2):
        """(status of create, per-run results)."""
        tasks, outs = self.tasks()
        h = C.c_void_p()
        rc = _lib.lib().ua_pbatch_create(*self.arena(), tasks, C.byref(h))
        if rc:
            return rc, h.value
        res = []
        try:
            for _ in range(runs):
                lens = (C.c_uint64 * self.n)(*([77] * self.n))
                assert _lib.lib().ua_pbatch_run(self.eng._ctx, h, lens) == 0
                res.append([to_list(outs[i], lens[i]) for i in range(self.n)])
                for o in outs:
                    o.fill_(-1)
        finally:
            _lib.lib().ua_pbatch_destroy(self.eng._ctx, h)
        return 0, res


def test_fanout_mixed_packs(eng):
    packs = fan_packs()
    assert len(packs) == 24
    flats = [gv.encode(u, bs) for u, bs in packs]
    assert all(len(b) <= 64 for b in flats)
    empties = [i for i, b in enumerate(flats) if not b]
    assert empties == [0, 4, 8, 9, 10, 23]
    assert sum(len(b) == 1 for b in flats) >= 3
    assert len(flats[1][0][2]) == gv.MAX_BLOCK_BYTES

    union = sorted({x for u, _ in packs for x in u})
    shared = sorted(set(union[::3]) | {x + 1 for x in union[1::3] if x < gv.U64_MAX} |
                    {0, gv.U64_MAX})
    vs, afters = [], []
    for i, (u, bs) in enumerate(packs):
        if i % 2 == 0:
            vs.append(shared)                               # half share one v
        elif i % 4 == 3:
            vs.append([])                                   # m = 0
        else:
            vs.append(sorted({y for x in u for y in (x - 1, x, x + 1)
                              if 0 <= y <= gv.U64_MAX}))
        sl = gv.seek_list(flats[i])
        afters.append(sl[(7 * i) % len(sl)])
    afters[2] = gv.U64_MAX      # edge values against the shared v: [UINT64_MAX]
    afters[12] = 0              # the pack [0], 0 in the shared v
    assert any(flats[i] and not vs[i] for i in range(24))

    want = [want_intersect(u, vs[i], afters[i]) for i, (u, _) in enumerate(packs)]
    assert want[2] == [gv.U64_MAX] and want[12] == [0]
    assert sum(bool(w) for w in want) >= 10
    for i, (u, bs) in enumerate(packs):
        if u:
            got = orc.intersect_compressed_with(orc.Pack(gv.u64(u), bs), afters[i],
                                                gv.u64(vs[i])).tolist()
            assert got == want[i], f"oracle pack {i}"

    fan = Fan(eng, flats, vs, afters)
    rc, got, lens = fan.one_shot()
    assert rc == 0
    assert lens == [len(w) for w in want]
    for i in range(24):
        assert got[i] == want[i], f"pack {i} bs={packs[i][1]} after={afters[i]:#x}"
    rc, runs = fan.prepared(runs=2)
    assert rc == 0
    for r, res in enumerate(runs):
        for i in range(24):
            assert res[i] == got[i], f"prepared run {r} pack {i}"


def test_fanout_all_packs_empty(eng):
    v = [1, 5, gv.U64_MAX]
    fan = Fan(eng, [[], [], []], [v, [], v], [0, 0, 7])
    rc, got, lens = fan.one_shot()
    assert (rc, got, lens) == (0, [[], [], []], [0, 0, 0])
    rc, runs = fan.prepared(runs=2)
    assert (rc, runs) == (0, [[[], [], []]] * 2)


# ---------- the limits: 256 uids, 1092 delta bytes ----------

def test_full_block_accepted(eng):
    """256 uids and 1085 delta bytes, the longest legal block, through
    decode, intersect, both fan-outs and the encoder."""
    uids = gv.full_block()
    blocks = gv.encode(uids, 256)
    assert [(n, len(d)) for _, n, d in blocks] == [(256, 1085)]
    dp = upload(eng, blocks, 256)
    for s in (0, uids[1], uids[255], uids[255] + 1):
        rc, got, _ = decode_dev(eng, dp, s)
        assert (rc, got) == (0, want_decode(uids, s))
    v = sorted(set(uids[::3]) | {uids[255], uids[7] + 1})
    dv, m = to_dev(v)
    for a in (0, uids[200]):
        rc, got, _ = intersect_dev(eng, dp, a, dv, m)
        assert (rc, got) == (0, want_intersect(uids, v, a))
    fan = Fan(eng, [blocks, blocks], [v, uids], [uids[200], 0])
    want = [want_intersect(uids, v, uids[200]), uids]
    rc, got, _ = fan.one_shot()
    assert (rc, got) == (0, want)
    assert fan.prepared(runs=1) == (0, [want])
    encode_dev_checked(eng, uids, 256)


def malformed(kind):
    """Three blocks whose middle one breaks exactly one documented limit.
    Every byte the offsets span is real, zero-filled memory."""
    if kind == "num_uids_257":
        blocks = gv.encode([1 << 36, (1 << 36) + 1, 2 << 36, (2 << 36) + 5,
                            3 << 36, (3 << 36) + 7], 256)
        bases, nums, offs, blob = gv.flatten(blocks)
        assert nums.tolist() == [2, 2, 2]
        nums[1] = 257
        return bases, nums, offs, blob
    return (gv.u64([1 << 36, 2 << 36, 3 << 36]), np.array([1, 2, 1], dtype=np.uint32),
            gv.u64([0, 5, 5 + 1093, 5 + 1093 + 5]), np.zeros(5 + 1093 + 5, dtype=np.uint8))


@pytest.mark.parametrize("kind", ["num_uids_257", "deltas_1093"])
def test_limit_violation_rejected(eng, kind, seek_case):
    bases, nums, offs, blob = malformed(kind)
    dp = eng.upload_pack(bases, nums, offs, blob, 256)
    cap = int(nums.sum())
    rc, _, n = decode_dev(eng, dp, 0, cap=cap)
    assert (rc, n) == (UA_ERR_INVALID, 0)
    v = [int(b) for b in bases]
    dv, m = to_dev(v)
    rc, _, n = intersect_dev(eng, dp, 0, dv, m)
    assert (rc, n) == (UA_ERR_INVALID, 0)

    fan = Fan.__new__(Fan)  # the arena is the malformed pack, cut in two
    fan.eng, fan.n, fan.dpb = eng, 2, dp
    dp.pack_totals = [int(nums[:2].sum()), int(nums[2])]
    fan.pbb = (C.c_uint64 * 3)(0, 2, 3)
    fan.vs, fan.afters, fan.dvs = [v, v], [0, 0], {id(v): (dv, m)}
    rc, _, lens = fan.one_shot()
    assert (rc, lens) == (UA_ERR_INVALID, [0, 0])
    assert fan.prepared() == (UA_ERR_INVALID, None)

    # the engine is unharmed: a valid pack still decodes
    uids, _, good, _ = seek_case
    assert decode_dev(eng, good, 0)[:2] == (0, uids)
