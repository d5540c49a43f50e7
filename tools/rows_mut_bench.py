#!/usr/bin/env python3
"""The UID matrix of a pack fan-out over live lists: Engine.decode_rows_mut
(ua_rows_decode_mut_dev) against its floor, Engine.decode_rows
(ua_rows_decode_dev, the parent's kernels) on the same arena.

Shapes a, b, c of tools/rows_decode_bench.py (4096 packs each, block size
256), and per shape three cases:

  plain   decode_rows: no layer, the floor
  sparse  decode_rows_mut with about 1% of the rows mutated, 4 postings each
          (two deletes of present uids, two sets)
  dense   decode_rows_mut with every row mutated by a slice as long as its
          pack: every second uid deleted, and a set next to each of the others

All cases run in one process, alternating, `reps` timed repetitions each after
one warm-up call per case.  Reported per case: median and max-min of the
engine's event time (count + write kernels; for the mutation call the flags,
their scan and the heads count with the count pass) and of the host-clock call
time.  Every row of every case is compared with numpy's set algebra before
anything is timed.

usage: rows_mut_bench.py [shapes=a,b,c] [reps=7]
Prints one JSON line.
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dgraph_amd import algo, synth  # noqa: E402
from rows_decode_bench import N_PACKS, gen_lists, summarize, timed  # noqa: E402


def layer(rng, lists, case):
    """Per-row (uids, ops) of the case's mutation layer."""
    empty = (np.empty(0, np.uint64), np.empty(0, np.uint8))
    rows = [empty] * len(lists)
    if case == "sparse":
        for r in rng.choice(len(lists), size=max(len(lists) // 100, 1), replace=False):
            u = lists[r]
            dels = np.unique(u[rng.integers(0, u.size, size=2)])
            sets = np.array([u[0] + np.uint64(1), u[-1] + np.uint64(7)], dtype=np.uint64)
            rows[r] = merge(dels, sets)
    elif case == "dense":
        for r, u in enumerate(lists):
            rows[r] = merge(u[::2], u[1::2] + np.uint64(1))
    return rows


def merge(dels, sets):
    uids = np.union1d(dels, sets)
    ops = np.where(np.isin(uids, sets), algo.MUT_SET, algo.MUT_DEL).astype(np.uint8)
    return uids, ops


def model(u, m):
    uids, ops = m
    if uids.size == 0:
        return u
    return np.union1d(np.setdiff1d(u, uids, assume_unique=True), uids[ops != algo.MUT_DEL])


def main():
    shapes = sys.argv[1].split(",") if len(sys.argv) > 1 else ["a", "b", "c"]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    eng = algo.Engine(0)
    res = {"workload": "rows_mut", "reps": reps, "n_packs": N_PACKS, "configs": []}
    for shape in shapes:
        rng = np.random.default_rng(synth.SEED + 14)
        lists = gen_lists(rng, shape)
        dpb = eng.upload_pack_batch([algo.encode_flat(u, 256) for u in lists])
        total = int(sum(dpb.pack_totals))
        ro = torch.empty(N_PACKS + 1, dtype=torch.int64, device=dev)
        calls, info = {}, {}
        for case in ("plain", "sparse", "dense"):
            rows = layer(rng, lists, case)
            n_mut = int(sum(u.size for u, _ in rows))
            base = np.zeros(N_PACKS + 1, dtype=np.int64)
            base[1:] = np.cumsum([u.size for u, _ in rows])
            t_mu = torch.from_numpy(np.concatenate([u for u, _ in rows]).view(np.int64)).to(dev)
            t_mo = torch.from_numpy(np.concatenate([o for _, o in rows])).to(dev)
            t_rmb = torch.from_numpy(base).to(dev)
            out = torch.empty(total + n_mut, dtype=torch.int64, device=dev)
            if case == "plain":
                fn = lambda out=out: eng.decode_rows(dpb, out_vals=out, out_row_offs=ro)
            else:
                fn = lambda out=out, a=(t_mu, t_mo, t_rmb): eng.decode_rows_mut(
                    dpb, *a, out_vals=out, out_row_offs=ro)
            vals, offs = fn()
            got = vals.cpu().numpy().view(np.uint64)
            o = offs.cpu().numpy()
            for r, u in enumerate(lists):
                if not np.array_equal(got[o[r]:o[r + 1]], model(u, rows[r])):
                    raise SystemExit(f"shape {shape} case {case}: row {r} differs")
            calls[case] = fn
            info[case] = {"n_mut": n_mut, "rows_mutated": int(sum(u.size > 0 for u, _ in rows)),
                          "out_uids": int(vals.numel())}
        ts = {c: [] for c in calls}
        ks = {c: [] for c in calls}
        for _ in range(reps):
            for case, fn in calls.items():
                eng.stats_reset()
                t, _ = timed(fn)
                ts[case].append(t)
                ks[case].append(eng.stats()["kernel_ms"])
        cfg = {"shape": shape, "total_uids": total, "blocks": int(dpb.pbb[-1])}
        for case in calls:
            ev = summarize(ks[case])
            cfg[case] = dict(info[case], event=ev, call=summarize(ts[case]))
            cfg[case]["event_over_plain"] = round(
                ev["median_ms"] / max(summarize(ks["plain"])["median_ms"], 1e-9), 2)
        print(f"shape {shape}: " + " ".join(
            f"{c} {cfg[c]['event']}" for c in calls), file=sys.stderr)
        res["configs"].append(cfg)
        del dpb, calls
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
