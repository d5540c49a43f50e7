#!/usr/bin/env python3
"""The transpose of a CSR UID matrix: Engine.transpose_rows
(ua_rows_transpose_dev: tile sort -> merge rounds -> flags -> scan -> write,
one call and one sync, keys + group offsets + entries + out_src out) against

  (a) the parent's only device route to the same sort: Engine.sort_rows
      (ua_rows_sort_dev) over ONE row [0, total] with keys = vals and out_src.
      That is its sort alone: no group heads, no group offsets, no row of an
      element.
  (b) the route a caller takes today, the torch composition on the same
      device: stable torch.sort of the values (all below 2^63),
      unique_consecutive with counts, searchsorted of the permutation in
      row_offs for the rows, a gather of the rows' uids and a cumsum for the
      group offsets.

Shapes (those of tools/rows_sort_bench.py):

  a  4096 rows, sizes synth.zipf_sizes clamped to [1, 100 000]
  b  4096 rows of 1 to 64
  c  one row of 4 M

Values are uniform in [1, total / 4], so a group holds four entries on average;
row uids are ascending above 2^32.  The three paths run in one process,
alternating, `reps` timed repetitions each after one warm-up call per path.
Reported per path: median and max-min of the host-clock call time (every call
ends in a device sync) and, for the two engine calls, the median of the
engine's event time.  The new call's keys, offsets, entries and out_src are
compared with path (b)'s before anything is timed.

usage: rows_transpose_bench.py [shapes=a,b,c] [reps=7]
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
    res = {"workload": "rows_transpose", "reps": reps, "configs": []}
    for shape in shapes:
        rng = np.random.default_rng(synth.SEED + 20)
        lens = np.asarray(gen_lens(rng, shape), dtype=np.int64)
        n_rows = lens.size
        offs = np.zeros(n_rows + 1, dtype=np.int64)
        offs[1:] = np.cumsum(lens)
        total = int(offs[-1])
        h_vals = rng.integers(1, max(total // 4, 2) + 1, size=total, dtype=np.int64)
        h_uids = np.arange(n_rows, dtype=np.int64) * 3 + (1 << 32)

        vals = torch.from_numpy(h_vals).to(dev)
        row_offs = torch.from_numpy(offs).to(dev)
        row_uids = torch.from_numpy(h_uids).to(dev)
        one_row = torch.tensor([0, total], dtype=torch.int64, device=dev)

        def new():
            return eng.transpose_rows(vals, row_offs, row_uids=row_uids, want_src=True)

        def sort_one_row():
            return eng.sort_rows(vals, one_row, keys=vals, want_src=True)

        def torch_path():
            s, perm = torch.sort(vals, stable=True)
            keys, counts = torch.unique_consecutive(s, return_counts=True)
            rows = torch.searchsorted(row_offs, perm, right=True) - 1
            goffs = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=dev)
            torch.cumsum(counts, 0, out=goffs[1:])
            return keys, goffs, row_uids[rows], perm

        # outputs compared before timing (also the warm-up call of each path)
        got = new()
        want = torch_path()
        for g, w, what in zip(got, want, ("keys", "offs", "vals", "src")):
            if not torch.equal(g, w):
                raise SystemExit(f"transpose_rows differs from the torch path: {what}, "
                                 f"shape {shape}")
        sv, _, ss = sort_one_row()
        if not (torch.equal(ss, got[3]) and torch.equal(sv, vals[got[3]])):
            raise SystemExit(f"transpose_rows differs from sort_rows' order: shape {shape}")

        paths = (("transpose_rows", new), ("sort_rows_one_row", sort_one_row),
                 ("torch", torch_path))
        ts = {name: [] for name, _ in paths}
        ks = {name: [] for name, _ in paths}
        for _ in range(reps):
            for name, fn in paths:
                eng.stats_reset()
                t, _ = timed(fn)
                ts[name].append(t)
                ks[name].append(eng.stats()["kernel_ms"])
        cfg = {"shape": shape, "n_rows": n_rows, "total": total,
               "n_groups": int(got[0].numel())}
        for name in ts:
            cfg[name] = summarize(ts[name])
            if name != "torch":
                cfg[name + "_event_ms"] = round(float(np.median(ks[name])), 4)
        tn, sa, tb = cfg["transpose_rows"], cfg["sort_rows_one_row"], cfg["torch"]
        cfg["behind_sort_rows_ms"] = round(tn["median_ms"] - sa["median_ms"], 3)
        cfg["behind_by_more_than_twice_its_spread"] = \
            bool(tn["median_ms"] - sa["median_ms"] > 2 * sa["spread_ms"])
        cfg["torch_over_transpose_rows"] = round(tb["median_ms"] / tn["median_ms"], 2)
        print(f"shape {shape}: total {total} transpose_rows {tn} sort_rows {sa} torch {tb}",
              file=sys.stderr)
        res["configs"].append(cfg)
        del vals, row_offs, row_uids, got, want
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
