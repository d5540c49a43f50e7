#!/usr/bin/env python3
"""Row-wise UID-matrix filter (Engine.filter_rows) against the only ways the
engine could express the shape before it:

  sorted rows   Engine.intersect_pairs / difference_pairs(rows, [shared] * N)
  ordered rows  Engine.index_of_batch + a byte mask + Engine.apply_filter_batch

Workload: N sorted rows, lengths synth.zipf_sizes clamped to [1, hi], one
shared sorted list of m uids, both modes; the ordered case shuffles every row.
Both paths run in one process, alternating, `reps` timed repetitions each
after warm-up; reported are median and max-min of the host-clock call time
(every call ends in a stream sync), the traffic each path's model derives from
the shapes, and the probe kernel's event time as a share of the new call.
Both paths' outputs are compared once per configuration with a membership
computed by torch.searchsorted: filter_rows must match it exactly, the
baseline's agreement is reported as `baseline_status`; a baseline that
fails or answers wrongly at a size is not timed.

usage: rows_bench.py [n_rows=4096] [reps=7] [m,m,...=10000,1000000,10000000] [hi=100000]
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

TILE = 2048      # UA_RTILE
PIVOTS = 1024    # UA_ROWS_P


def gen_rows(rng, lens, limit):
    """Flat sorted duplicate-free rows: per-row cumsum of deltas >= 1 scaled so
    a row of n values spans about [0, limit)."""
    total = int(lens.sum())
    scale = np.repeat(np.maximum(limit / lens, 1.0), lens)
    deltas = 1 + np.floor(rng.random(total) * (2 * scale - 1)).astype(np.int64)
    cs = np.cumsum(deltas)
    offs = np.zeros(lens.size + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    start = np.repeat(cs[offs[:-1]] - deltas[offs[:-1]], lens)
    return (cs - start).astype(np.uint64), offs.astype(np.uint64)


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
    n_rows = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    ms = [int(x) for x in sys.argv[3].split(",")] if len(sys.argv) > 3 else \
        [10_000, 1_000_000, 10_000_000]
    hi = int(sys.argv[4]) if len(sys.argv) > 4 else 100_000
    dev = "cuda:0"
    eng = algo.Engine(0)
    rng = np.random.default_rng(synth.SEED + 9)
    lens = np.clip(synth.zipf_sizes(rng, n_rows, lo=1, hi=hi), 1, hi)
    total = int(lens.sum())
    res = {"workload": "rows_filter", "n_rows": n_rows, "reps": reps, "total": total,
           "row_len_median": float(np.median(lens)), "row_len_max": int(lens.max()),
           "configs": []}
    row_id = torch.repeat_interleave(torch.arange(n_rows, device=dev),
                                     torch.from_numpy(lens).to(dev))
    for m in ms:
        limit = max(int(m / 0.3), 4 * hi)
        shared = synth.gen_sorted_unique(rng, m, limit)
        vals, offs = gen_rows(rng, lens, limit)
        d_shared = torch.from_numpy(shared.view(np.int64)).to(dev)
        d_sorted = torch.from_numpy(vals.view(np.int64)).to(dev)
        d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
        g = torch.Generator(device=dev).manual_seed(synth.SEED)
        key = (row_id << 32) | torch.randint(0, 1 << 31, (total,), device=dev, generator=g)
        d_shuf = d_sorted[torch.argsort(key)]
        del key
        o = [int(x) for x in offs]
        out_vals = torch.empty(total, dtype=torch.int64, device=dev)
        out_offs = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        pair_outs = [torch.empty(o[r + 1] - o[r], dtype=torch.int64, device=dev)
                     for r in range(n_rows)]
        filt_out = torch.empty(total, dtype=torch.int64, device=dev)
        ntiles = (total + TILE - 1) // TILE

        for case, d_vals in [("sorted", d_sorted), ("ordered", d_shuf)]:
            rows = [d_vals[o[r]:o[r + 1]] for r in range(n_rows)]
            f_outs = [filt_out[o[r]:o[r + 1]] for r in range(n_rows)]
            # independent membership (values < 2^63: signed order == unsigned)
            idx = torch.searchsorted(d_shared, d_vals).clamp_(max=m - 1)
            member = d_shared[idx] == d_vals
            del idx
            for mode, mname in [(algo.ROWS_INTERSECT, "intersect"),
                                (algo.ROWS_DIFFERENCE, "difference")]:
                def new():
                    return eng.filter_rows(d_vals, d_offs, d_shared, mode, out_vals, out_offs)

                if case == "sorted":
                    pair_fn = eng.intersect_pairs if mode == algo.ROWS_INTERSECT else \
                        eng.difference_pairs

                    def old():
                        return pair_fn(rows, [d_shared] * n_rows, pair_outs)
                else:
                    def old():
                        pos = eng.index_of_batch(d_shared, d_vals)
                        mask = (pos >= 0) if mode == algo.ROWS_INTERSECT else (pos < 0)
                        masks = [mask[o[r]:o[r + 1]] for r in range(n_rows)]
                        return eng.apply_filter_batch(rows, masks, f_outs)

                # warm-up, and both paths checked once against torch.searchsorted
                keep = member if mode == algo.ROWS_INTERSECT else ~member
                want = d_vals[keep]
                want_offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                       torch.cumsum(keep, 0)])[d_offs]
                got, got_offs = new()
                if not (torch.equal(got, want) and torch.equal(got_offs, want_offs)):
                    k = min(got.numel(), want.numel())
                    bad = torch.nonzero(got[:k] != want[:k])[:4].flatten().tolist()
                    raise SystemExit(f"filter_rows differs from searchsorted: m={m} {case} "
                                     f"{mname}: kept {got.numel()} want {want.numel()}, "
                                     f"first differing ranks {bad}")
                # a baseline that fails or answers wrongly at this size is
                # reported as such and not timed
                try:
                    outs, out_lens = old()
                    base = "exact" if (
                        out_lens == (want_offs[1:] - want_offs[:-1]).tolist() and
                        torch.equal(torch.cat([outs[r][:out_lens[r]] for r in range(n_rows)]),
                                    want)) else "wrong result"
                    del outs
                except RuntimeError as e:
                    base = f"failed: {e}"
                kept = int(got.numel())
                del want, keep
                new()
                if base == "exact":
                    old()

                t_new, t_old, k_new, k_old = [], [], [], []
                for _ in range(reps):
                    eng.stats_reset()
                    t, _ = timed(new)
                    t_new.append(t)
                    k_new.append(eng.stats()["kernel_ms"])
                    if base != "exact":
                        continue
                    eng.stats_reset()
                    t, _ = timed(old)
                    t_old.append(t)
                    k_old.append(eng.stats()["kernel_ms"])
                rows_bytes = 8 * (2 * total + kept) + total // 4 + ntiles * 8 * min(m, PIVOTS)
                if case == "sorted":
                    old_bytes = 8 * (total + n_rows * m)
                else:  # index_of: keys + positions; mask write; filter: vals + mask + out
                    old_bytes = 8 * total + 8 * total + total + 9 * total + 8 * kept
                sn = summarize(t_new)
                so = summarize(t_old) if t_old else None
                print(f"m={m} {case} {mname}: rows {sn} baseline {so or base}", file=sys.stderr)
                res["configs"].append({
                    "m": m, "case": case, "mode": mname, "kept": kept,
                    "baseline_status": base,
                    "rows": sn, "baseline": so,
                    "speedup_median": round(so["median_ms"] / sn["median_ms"], 2) if so else None,
                    "rows_probe_kernel_ms": round(float(np.median(k_new)), 3),
                    "rows_probe_share": round(float(sum(k_new) / sum(t_new)), 3),
                    "baseline_kernel_ms": round(float(np.median(k_old)), 3) if so else None,
                    "rows_model_MB": round(rows_bytes / 1e6, 1),
                    "baseline_model_MB": round(old_bytes / 1e6, 1),
                })
        del d_shared, d_sorted, d_shuf, pair_outs, filt_out, out_vals
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
