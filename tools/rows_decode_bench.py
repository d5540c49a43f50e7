#!/usr/bin/env python3
"""The UID matrix of a pack fan-out: Engine.decode_rows (ua_rows_decode_dev,
count -> scan -> write, one call and one sync for all rows) against what a
caller had to write before it, a loop of Engine.decode_pack over per-row views
of the same device arena (one call and one sync per row), and, for the device
rate, ua_decode_dev on ONE pack holding as many uids as the whole fan-out.

Shapes (4096 packs each, block size 256):

  a  sizes synth.zipf_sizes clamped to [1, 100 000]; uids from
     synth.getuids_geometric (one-byte deltas)
  b  the same sizes; deltas cycle through all four byte lengths, smallest and
     largest value of each (the mixed ladders of the codec tests)
  c  sizes uniform in [1, 64], uids as in a
  d  shape a with first = 10 on every row (the loop decodes each row whole
     and keeps its first 10, as List.Uids does)

All paths run in one process, alternating, `reps` timed repetitions each
after one warm-up call per path.  Reported per path: median and max-min of
the host-clock call time (every call ends in a stream sync) and the median of
the engine's event time (decode_rows: count + write kernels; the others:
k_packed).  The outputs are compared for equality before anything is timed.

usage: rows_decode_bench.py [shapes=a,b,c,d] [reps=7]
Prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dgraph_amd import algo, synth  # noqa: E402
from dgraph_amd.algo import DPack  # noqa: E402

N_PACKS = 4096
LOW = [1, 0x100, 0x10000, 0x1000000]
HIGH = [0xff, 0xffff, 0xffffff, 0x3fffffff]


def mixed_deltas():
    """One group of four deltas per control byte 0..255, smallest values then
    largest: 2048 deltas of every byte-length mix."""
    order = [(167 * i + 13) % 256 for i in range(256)]
    return np.array([vals[(t >> (2 * i)) & 3] for vals in (LOW, HIGH) for t in order
                     for i in range(4)], dtype=np.uint64)


def gen_lists(rng, shape):
    if shape in ("a", "b", "d"):
        lens = np.clip(synth.zipf_sizes(rng, N_PACKS, lo=1, hi=100_000), 1, 100_000)
    elif shape == "c":
        lens = rng.integers(1, 65, size=N_PACKS)
    else:
        raise SystemExit(f"unknown shape {shape!r}")
    lists = []
    pat = mixed_deltas()
    for n in lens:
        n = int(n)
        if shape == "b":
            ds = np.resize(np.roll(pat, -int(rng.integers(0, pat.size))), n)
            lists.append(np.uint64(1 << 36) + np.cumsum(ds, dtype=np.uint64))
        else:
            ds = rng.integers(1, 33, size=n, dtype=np.uint64)
            lists.append(np.cumsum(ds, dtype=np.uint64))
    return lists


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def summarize(ts):
    return {"median_ms": round(float(np.median(ts)), 3),
            "spread_ms": round(float(max(ts) - min(ts)), 3)}


def main():
    shapes = sys.argv[1].split(",") if len(sys.argv) > 1 else ["a", "b", "c", "d"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    eng = algo.Engine(0)
    res = {"workload": "rows_decode", "reps": reps, "n_packs": N_PACKS, "configs": []}
    for shape in shapes:
        rng = np.random.default_rng(synth.SEED + 14)
        lists = gen_lists(rng, shape)
        first = 10 if shape == "d" else 0
        packs = [algo.encode_flat(u, 256) for u in lists]
        dpb = eng.upload_pack_batch(packs)
        total = int(sum(dpb.pack_totals))
        pbb = [int(x) for x in dpb.pbb]
        views = [DPack(dpb.bases[pbb[r]:pbb[r + 1]], dpb.num_uids[pbb[r]:pbb[r + 1]],
                       dpb.delta_offs[pbb[r]:pbb[r + 1] + 1], dpb.deltas, 256,
                       dpb.pack_totals[r]) for r in range(N_PACKS)]
        offs = np.zeros(N_PACKS + 1, dtype=np.int64)
        offs[1:] = np.cumsum(dpb.pack_totals)
        o = [int(x) for x in offs]
        out_new = torch.empty(total, dtype=torch.int64, device=dev)
        ro_new = torch.empty(N_PACKS + 1, dtype=torch.int64, device=dev)
        out_old = torch.empty(total, dtype=torch.int64, device=dev)
        firsts = torch.full((N_PACKS,), first, dtype=torch.int32, device=dev) if first else None
        # one pack of as many uids, for the device rate of the existing kernel
        one = eng.upload_pack(*algo.encode_flat(
            np.cumsum(rng.integers(1, 33, size=total, dtype=np.uint64), dtype=np.uint64),
            256)[:4], 256)
        out_one = torch.empty(total, dtype=torch.int64, device=dev)
        del lists, packs

        def new():
            return eng.decode_rows(dpb, firsts=firsts, out_vals=out_new, out_row_offs=ro_new)

        def old():
            for r in range(N_PACKS):
                eng.decode_pack(views[r], 0, out_old[o[r]:o[r + 1]])

        def single():
            return eng.decode_pack(one, 0, out_one)

        vals, ro = new()
        old()
        if first:
            keep = np.minimum(np.diff(offs), first)
            want_ro = np.zeros(N_PACKS + 1, dtype=np.int64)
            want_ro[1:] = np.cumsum(keep)
            idx = torch.from_numpy(np.concatenate(
                [np.arange(o[r], o[r] + keep[r]) for r in range(N_PACKS)])).to(dev)
            want = out_old[idx]
        else:
            want_ro, want = offs, out_old
        if not torch.equal(ro.cpu(), torch.from_numpy(want_ro)) or not torch.equal(vals, want):
            raise SystemExit(f"decode_rows differs from the decode_pack loop: shape {shape}")
        kept = int(vals.numel())
        single()

        t_new, t_old, t_one, k_new, k_old, k_one = [], [], [], [], [], []
        for _ in range(reps):
            for fn, ts, ks in ((new, t_new, k_new), (old, t_old, k_old),
                               (single, t_one, k_one)):
                eng.stats_reset()
                t, _ = timed(fn)
                ts.append(t)
                ks.append(eng.stats()["kernel_ms"])
        sn, so, s1 = summarize(t_new), summarize(t_old), summarize(t_one)
        kn, ko, k1 = (float(np.median(k)) for k in (k_new, k_old, k_one))
        print(f"shape {shape}: decode_rows {sn} loop {so} one pack {s1}", file=sys.stderr)
        res["configs"].append({
            "shape": shape, "total_uids": total, "kept_uids": kept,
            "blocks": pbb[-1], "deltas_bytes": int(dpb.deltas.numel()),
            "decode_rows": sn, "decode_pack_loop": so, "decode_pack_one_pack": s1,
            "loop_over_decode_rows": round(so["median_ms"] / sn["median_ms"], 2),
            "beats_loop_by_more_than_twice_its_spread":
                bool(so["median_ms"] - sn["median_ms"] > 2 * so["spread_ms"]),
            "decode_rows_event_ms": round(kn, 4),
            "decode_pack_loop_event_ms": round(ko, 4),
            "one_pack_event_ms": round(k1, 4),
            "decode_rows_event_Guids_s": round(total / kn / 1e6, 2) if kn else None,
            "one_pack_event_Guids_s": round(total / k1 / 1e6, 2) if k1 else None,
        })
        del dpb, views, out_new, out_old, out_one, one
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
