#!/usr/bin/env python3
"""Order and pagination of a CSR UID matrix: Engine.sort_rows
(ua_rows_sort_dev: row bits -> tile sort -> merge rounds -> page -> scan ->
offsets -> write, one call and one sync, a CSR matrix out) against the device
part of what a caller had before it, Engine.sort_segments' engine call
(ua_sort_segments_dev) over per-row tensors of (key32 << 32 | position), with
the descriptors and merge buffers that Engine.sort_segments builds per call
prepared beforehand as well.  Neither the key lookup nor the packing is charged to the
old path, nor is what it still needs afterwards: downloading the sorted rows
and paginating and gathering the uids on the host, which is timed on its own
(host_gather).

Shapes:

  a  4096 rows, sizes synth.zipf_sizes clamped to [1, 100 000]
  b  4096 rows of 1 to 64
  c  one row of 4 M (recorded, not gated: the old path's best case, and it
     moves half the bytes per element)

Keys are random 32-bit values widened to u64, every element has one; the page
is count=10, offset=0.  Both paths run in one process, alternating, `reps`
timed repetitions each after one warm-up call per path; the old path's rows
are restored to their unsorted state outside the timed region.  Reported per
path: median and max-min of the host-clock call time (every call ends in a
stream sync) and the median of the engine's event time.  The new call's rows
are compared with the old path's paginated rows before anything is timed.

usage: rows_sort_bench.py [shapes=a,b,c] [reps=7]
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
from dgraph_amd._lib import UaDSeg, check, lib  # noqa: E402

COUNT, OFFSET = 10, 0


def gen_lens(rng, shape):
    if shape == "a":
        return np.clip(synth.zipf_sizes(rng, 4096, lo=1, hi=100_000), 1, 100_000)
    if shape == "b":
        return rng.integers(1, 65, size=4096)
    if shape == "c":
        return np.array([4 << 20])
    raise SystemExit(f"unknown shape {shape!r}")


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
    res = {"workload": "rows_sort", "reps": reps, "count": COUNT, "offset": OFFSET,
           "configs": []}
    for shape in shapes:
        rng = np.random.default_rng(synth.SEED + 19)
        lens = np.asarray(gen_lens(rng, shape), dtype=np.int64)
        n_rows = lens.size
        offs = np.zeros(n_rows + 1, dtype=np.int64)
        offs[1:] = np.cumsum(lens)
        total = int(offs[-1])
        o = [int(x) for x in offs]
        h_vals = rng.integers(1, 1 << 40, size=total, dtype=np.uint64)
        h_keys = rng.integers(0, 1 << 32, size=total, dtype=np.uint64)
        pos = np.arange(total, dtype=np.uint64) - np.repeat(offs[:-1], lens).astype(np.uint64)
        h_packed = (h_keys << np.uint64(32)) | pos

        vals = torch.from_numpy(h_vals.view(np.int64)).to(dev)
        keys = torch.from_numpy(h_keys.view(np.int64)).to(dev)
        row_offs = torch.from_numpy(offs).to(dev)
        master = torch.from_numpy(h_packed.view(np.int64)).to(dev)
        packed = master.clone()
        segs = [packed[o[r]:o[r + 1]] for r in range(n_rows)]
        out_vals = torch.empty(total, dtype=torch.int64, device=dev)
        out_offs = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)

        def new():
            return eng.sort_rows(vals, row_offs, keys=keys, count=COUNT, offset=OFFSET,
                                 out_vals=out_vals, out_row_offs=out_offs)

        # Engine.sort_segments' call with its descriptors and merge buffers
        # prepared beforehand too: only ua_sort_segments_dev is timed
        tmp = torch.empty(total, dtype=torch.int64, device=dev)
        dsegs = (UaDSeg * n_rows)()
        for r in range(n_rows):
            dsegs[r].data = segs[r].data_ptr()
            dsegs[r].n = segs[r].numel()
            dsegs[r].tmp = tmp[o[r]:o[r + 1]].data_ptr()

        def old():
            check(lib().ua_sort_segments_dev(eng._ctx, dsegs, n_rows))

        def host_gather():
            p = packed.cpu().numpy().view(np.uint64)
            rows = []
            for r in range(n_rows):
                a, b = o[r], o[r + 1]
                idx = (p[a:min(b, a + COUNT)] & np.uint64(0xFFFFFFFF)).astype(np.int64)
                rows.append(h_vals[a + idx])
            return rows

        # outputs compared before timing (also the warm-up call of each path)
        got_v, got_o = new()
        got_v, got_o = got_v.cpu().numpy().view(np.uint64), got_o.cpu().numpy()
        old()
        want = host_gather()
        if not (np.array_equal(got_v, np.concatenate(want)) and
                np.array_equal(np.diff(got_o), [w.size for w in want])):
            raise SystemExit(f"sort_rows differs from the sort_segments path: shape {shape}")

        ts = {"sort_rows": [], "sort_segments": []}
        ks = {"sort_rows": [], "sort_segments": []}
        for _ in range(reps):
            for name, fn in (("sort_rows", new), ("sort_segments", old)):
                if name == "sort_segments":
                    packed.copy_(master)  # unsorted again, outside the timed region
                eng.stats_reset()
                t, _ = timed(fn)
                ts[name].append(t)
                ks[name].append(eng.stats()["kernel_ms"])
        tg = []
        for _ in range(3):
            t0 = time.perf_counter()
            host_gather()
            tg.append((time.perf_counter() - t0) * 1e3)
        cfg = {"shape": shape, "n_rows": n_rows, "total": total,
               "out_total": int(got_v.size)}
        for name in ts:
            cfg[name] = summarize(ts[name])
            cfg[name + "_event_ms"] = round(float(np.median(ks[name])), 4)
        cfg["host_gather_after_sort_segments_ms"] = round(float(np.median(tg)), 3)
        sn, so = cfg["sort_rows"], cfg["sort_segments"]
        cfg["sort_segments_over_sort_rows"] = round(so["median_ms"] / sn["median_ms"], 2)
        cfg["ahead_by_more_than_twice_the_old_spread"] = \
            bool(so["median_ms"] - sn["median_ms"] > 2 * so["spread_ms"])
        print(f"shape {shape}: total {total} sort_rows {sn} sort_segments {so}",
              file=sys.stderr)
        res["configs"].append(cfg)
        del vals, keys, master, packed, segs, tmp, dsegs, out_vals, out_offs
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
