#!/usr/bin/env python3
"""DestUIDs of a CSR UID matrix: Engine.union_rows (flat sort-unique leaves +
union tree, one call on the flat array) against the only way the engine had
before it, Engine.merge_sorted over per-row views of the same device buffer
(one tree leaf per row).

Shapes (values uniform over [0, total / 3), sorted and duplicate-free inside
each row, so the union is a fraction of the total):

  a  4096 short rows, lengths uniform in [1, 64]
  b  4096 rows, lengths synth.zipf_sizes clamped to [1, 100 000] (rows_bench's)
  c  256 rows of 30 000 (query_bench's matrix)
  uN 4096 rows of N each (to place the crossover, e.g. u1024,u2048,u4096)

Both paths run in one process, alternating, `reps` timed repetitions each
after two warm-up calls per path; reported are median and max-min of the
host-clock call time (every call ends in a stream sync; the baseline's time
includes building its 4096 pointer/length arrays from the prepared views,
which is what a caller of ua_merge_k_dev pays), the engine's event time
(leaf kernel + tree for union_rows, tree for merge_sorted) and its share of
the call.  Both outputs are compared once per shape with
torch.unique(sorted=True); union_rows must match, a baseline that fails or
answers wrongly is recorded and not timed.

usage: rows_union_bench.py [shapes=a,b,c] [reps=7]
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

LEAF = 2048  # UA_SORT_N


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
    return (cs - start).astype(np.uint64), offs


def shape_lens(rng, shape):
    if shape == "a":
        return rng.integers(1, 65, size=4096)
    if shape == "b":
        return np.clip(synth.zipf_sizes(rng, 4096, lo=1, hi=100_000), 1, 100_000)
    if shape == "c":
        return np.full(256, 30_000, dtype=np.int64)
    if shape[0] == "u" and shape[1:].isdigit():
        return np.full(4096, int(shape[1:]), dtype=np.int64)
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


def rounds(k):
    r = 0
    while k > 1:
        k = (k + 1) // 2
        r += 1
    return r


def main():
    shapes = sys.argv[1].split(",") if len(sys.argv) > 1 else ["a", "b", "c"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    eng = algo.Engine(0)
    res = {"workload": "rows_union", "reps": reps, "configs": []}
    for shape in shapes:
        rng = np.random.default_rng(synth.SEED + 11)
        lens = shape_lens(rng, shape)
        n_rows, total = int(lens.size), int(lens.sum())
        vals, offs = gen_rows(rng, lens, max(total // 3, 4 * int(lens.max())))
        d_vals = torch.from_numpy(vals.view(np.int64)).to(dev)
        o = [int(x) for x in offs]
        rows = [d_vals[o[r]:o[r + 1]] for r in range(n_rows)]
        out = torch.empty(total, dtype=torch.int64, device=dev)
        want = torch.unique(d_vals, sorted=True)  # values < 2^63: signed == unsigned
        del vals

        def new():
            return eng.union_rows(d_vals, out)

        def old():
            return eng.merge_sorted(rows)

        got = new()
        if not torch.equal(got, want):
            raise SystemExit(f"union_rows differs from torch.unique: shape {shape}: "
                             f"{got.numel()} values, want {want.numel()}")
        try:
            base = "exact" if torch.equal(old(), want) else "wrong result"
        except RuntimeError as e:
            base = f"failed: {e}"
        union = int(want.numel())
        del want, got
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
        sn = summarize(t_new)
        so = summarize(t_old) if t_old else None
        n_leaf = (total + LEAF - 1) // LEAF
        print(f"shape {shape}: union_rows {sn} merge_sorted {so or base}", file=sys.stderr)
        res["configs"].append({
            "shape": shape, "n_rows": n_rows, "total": total, "union": union,
            "row_len_median": float(np.median(lens)), "row_len_max": int(lens.max()),
            "leaves": n_leaf, "rounds_union_rows": rounds(n_leaf),
            "rounds_merge_sorted": rounds(n_rows),
            "baseline_status": base,
            "union_rows": sn, "merge_sorted": so,
            "merge_sorted_over_union_rows":
                round(so["median_ms"] / sn["median_ms"], 2) if so else None,
            "union_rows_event_ms": round(float(np.median(k_new)), 3),
            "union_rows_event_share": round(float(sum(k_new) / sum(t_new)), 3),
            "merge_sorted_event_ms": round(float(np.median(k_old)), 3) if so else None,
            # leaf pass 16 B/element + count and write passes of every round
            "union_rows_model_MB": round((16 + 24 * rounds(n_leaf)) * total / 1e6, 1),
            "merge_sorted_model_MB": round(24 * rounds(n_rows) * total / 1e6, 1),
        })
        del d_vals, rows, out
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
