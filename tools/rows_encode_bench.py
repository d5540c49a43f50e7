#!/usr/bin/env python3
"""A CSR UID matrix into a fan-out of UidPacks: Engine.encode_rows
(ua_rows_encode_dev, row bits -> count -> scans -> row bases -> write, one
call and one sync for all rows) against what a caller had to write before it,
a loop of Engine.encode_dev over the rows (one call and two syncs per row),
and, for the device rate, ua_encode_dev on ONE list holding as many uids as
the whole matrix.

Shapes (4096 rows each, block size 256):

  a  sizes synth.zipf_sizes clamped to [1, 100 000]; one-byte deltas
  b  the same sizes; deltas cycle through all four byte lengths, smallest and
     largest value of each (the mixed ladders of the codec tests)
  c  sizes uniform in [1, 64], uids as in a

Paths: encode_rows (full call into preallocated buffers), encode_rows incl.
the count-only call that sizes them, the encode_dev loop, and one list.  All
run in one process, alternating, `reps` timed repetitions each after one
warm-up call per path.  Reported per path: median and max-min of the
host-clock call time (every call ends in a stream sync) and the median of the
engine's event time (encode_rows: count + write kernels; encode_dev:
k_encode_blocks).  The new arena's bytes are compared with the loop's before
anything is timed.

usage: rows_encode_bench.py [shapes=a,b,c] [reps=7]
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

N_ROWS = 4096
LOW = [1, 0x100, 0x10000, 0x1000000]
HIGH = [0xff, 0xffff, 0xffffff, 0x3fffffff]


def mixed_deltas():
    """One group of four deltas per control byte 0..255, smallest values then
    largest: 2048 deltas of every byte-length mix."""
    order = [(167 * i + 13) % 256 for i in range(256)]
    return np.array([vals[(t >> (2 * i)) & 3] for vals in (LOW, HIGH) for t in order
                     for i in range(4)], dtype=np.uint64)


def gen_list(rng, shape, n, pat):
    if shape == "b":
        ds = np.resize(np.roll(pat, -int(rng.integers(0, pat.size))), n)
        return np.uint64(1 << 36) + np.cumsum(ds, dtype=np.uint64)
    return np.cumsum(rng.integers(1, 33, size=n, dtype=np.uint64), dtype=np.uint64)


def gen_lists(rng, shape):
    if shape in ("a", "b"):
        lens = np.clip(synth.zipf_sizes(rng, N_ROWS, lo=1, hi=100_000), 1, 100_000)
    elif shape == "c":
        lens = rng.integers(1, 65, size=N_ROWS)
    else:
        raise SystemExit(f"unknown shape {shape!r}")
    pat = mixed_deltas()
    return [gen_list(rng, shape, int(n), pat) for n in lens]


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
    shapes = sys.argv[1].split(",") if len(sys.argv) > 1 else ["a", "b", "c"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    eng = algo.Engine(0)
    res = {"workload": "rows_encode", "reps": reps, "n_rows": N_ROWS, "configs": []}
    for shape in shapes:
        rng = np.random.default_rng(synth.SEED + 18)
        lists = gen_lists(rng, shape)
        offs = np.zeros(N_ROWS + 1, dtype=np.int64)
        offs[1:] = np.cumsum([u.size for u in lists])
        total = int(offs[-1])
        o = [int(x) for x in offs]
        vals = torch.from_numpy(np.concatenate(lists).view(np.int64)).to(dev)
        row_offs = torch.from_numpy(offs).to(dev)
        rows = [vals[o[r]:o[r + 1]] for r in range(N_ROWS)]
        one = torch.from_numpy(gen_list(rng, shape, total, mixed_deltas()).view(np.int64)).to(dev)
        del lists

        nb, db, _ = eng.encode_rows(vals, row_offs, 256, count_only=True)
        bufs = (torch.empty(max(nb, 1), dtype=torch.int64, device=dev),
                torch.empty(max(nb, 1), dtype=torch.int32, device=dev),
                torch.empty(nb + 1, dtype=torch.int64, device=dev),
                torch.empty(max(db, 1), dtype=torch.int8, device=dev))
        rbb = torch.empty(N_ROWS + 1, dtype=torch.int64, device=dev)

        def new():
            return eng.encode_rows(vals, row_offs, 256, out=bufs, row_block_base=rbb)

        def new_counted():
            return eng.encode_rows(vals, row_offs, 256)

        def old():
            return [eng.encode_dev(rows[r], 256) for r in range(N_ROWS)]

        def single():
            return eng.encode_dev(one, 256)

        arena = new()
        counted = new_counted()
        packs = old()
        # the loop's packs, concatenated, are the arena
        nbs = torch.tensor([p.bases.numel() for p in packs], dtype=torch.int64)
        pbb = torch.zeros(N_ROWS + 1, dtype=torch.int64)
        pbb[1:] = torch.cumsum(nbs, 0)
        ends = torch.stack([p.delta_offs[-1] for p in packs]).cpu()
        ybase = torch.zeros(N_ROWS + 1, dtype=torch.int64)
        ybase[1:] = torch.cumsum(ends, 0)
        same = (torch.equal(arena._pbb_dev.cpu(), pbb) and
                torch.equal(arena.bases, torch.cat([p.bases for p in packs])) and
                torch.equal(arena.num_uids, torch.cat([p.num_uids for p in packs])) and
                torch.equal(arena.delta_offs[:-1], torch.cat(
                    [p.delta_offs[:-1] + int(ybase[r]) for r, p in enumerate(packs)])) and
                int(arena.delta_offs[-1]) == int(ybase[-1]) == db and
                torch.equal(arena.deltas[:db], torch.cat(
                    [p.deltas[:int(ends[r])] for r, p in enumerate(packs)])) and
                torch.equal(counted.deltas[:db], arena.deltas[:db]) and
                torch.equal(counted.bases, arena.bases))
        if not same:
            raise SystemExit(f"encode_rows differs from the encode_dev loop: shape {shape}")
        del packs, counted
        one_pack = single()
        one_blocks = int(one_pack.bases.numel())
        del one_pack

        paths = (("encode_rows", new), ("encode_rows_with_count", new_counted),
                 ("encode_dev_loop", old), ("encode_dev_one_list", single))
        ts = {k: [] for k, _ in paths}
        ks = {k: [] for k, _ in paths}
        for _ in range(reps):
            for name, fn in paths:
                eng.stats_reset()
                t, _ = timed(fn)
                ts[name].append(t)
                ks[name].append(eng.stats()["kernel_ms"])
        cfg = {"shape": shape, "total_uids": total, "blocks": nb, "deltas_bytes": db,
               "one_list_blocks": one_blocks}
        for name, _ in paths:
            cfg[name] = summarize(ts[name])
            cfg[name + "_event_ms"] = round(float(np.median(ks[name])), 4)
        sn, so = cfg["encode_rows"], cfg["encode_dev_loop"]
        cfg["loop_over_encode_rows"] = round(so["median_ms"] / sn["median_ms"], 2)
        cfg["beats_loop_by_more_than_twice_its_spread"] = \
            bool(so["median_ms"] - sn["median_ms"] > 2 * so["spread_ms"])
        kn = cfg["encode_rows_event_ms"]
        cfg["encode_rows_event_Guids_s"] = round(total / kn / 1e6, 2) if kn else None
        print(f"shape {shape}: " + " ".join(f"{n} {cfg[n]}" for n, _ in paths),
              file=sys.stderr)
        res["configs"].append(cfg)
        del vals, rows, one, bufs, arena
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
