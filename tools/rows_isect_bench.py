#!/usr/bin/env python3
"""A pack fan-out against one shared filter list into a CSR matrix:
Engine.intersect_rows (ua_rows_intersect_packed_dev, count -> scan -> write,
blocks bounded from their headers) against the two ways a caller had before:

  batch    Engine.intersect_packed_batch(dpb, [shared] * n_packs): one grid,
           every block decoded, a host task and an output buffer per pack
  dec+flt  Engine.decode_rows -> Engine.filter_rows: the unfiltered matrix is
           written and read back

Shapes (4096 packs each, block size 256, after = 0):

  a10k  sizes synth.zipf_sizes clamped to [1, 100 000], one-byte deltas;
        shared: m = 10 000
  a1m   the same packs; m = 1 000 000
  b     the same sizes; deltas cycle through all four byte lengths; m = 1 000 000
  c     1..64 uids per pack, drawn over the whole low 32 bits (one block per
        pack, spanning most of shared); m = 1 000 000

shared is half a sample of the packs' own uids and half uniform draws from
their value range, sorted and duplicate-free.

All paths run in one process, alternating, `reps` timed repetitions each after
one warm-up call per path.  Reported per path: median and max-min of the
host-clock call time (every call ends in a stream sync) and the median of the
engine's event time.  The outputs are compared for equality before anything is
timed.  The gate: on a10k and c the new call leads each alternative by more
than twice that alternative's own max-min.

Extra builds of the library (other UA_RI_RATIO values) given as
ratio=PATH arguments are called raw on the same device buffers, in the same
alternation, and their results compared with the default build's.

usage: rows_isect_bench.py [shapes=a10k,a1m,b,c] [reps=7] [LABEL=libpath ...]
Prints one JSON line.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dgraph_amd import _lib, algo, synth  # noqa: E402

N_PACKS = 4096
LOW = [1, 0x100, 0x10000, 0x1000000]
HIGH = [0xff, 0xffff, 0xffffff, 0x3fffffff]
SHAPES = {"a10k": ("a", 10_000), "a1m": ("a", 1_000_000), "b": ("b", 1_000_000),
          "c": ("c", 1_000_000)}


def mixed_deltas():
    order = [(167 * i + 13) % 256 for i in range(256)]
    return np.array([vals[(t >> (2 * i)) & 3] for vals in (LOW, HIGH) for t in order
                     for i in range(4)], dtype=np.uint64)


def gen_lists(rng, kind):
    if kind == "c":
        lens = rng.integers(1, 65, size=N_PACKS)
        return [np.unique(rng.integers(1, 1 << 32, size=int(n), dtype=np.uint64))
                for n in lens]
    lens = np.clip(synth.zipf_sizes(rng, N_PACKS, lo=1, hi=100_000), 1, 100_000)
    lists = []
    pat = mixed_deltas()
    for n in lens:
        n = int(n)
        if kind == "b":
            ds = np.resize(np.roll(pat, -int(rng.integers(0, pat.size))), n)
            lists.append(np.uint64(1 << 36) + np.cumsum(ds, dtype=np.uint64))
        else:
            lists.append(np.cumsum(rng.integers(1, 33, size=n, dtype=np.uint64),
                                   dtype=np.uint64))
    return lists


def gen_shared(rng, lists, m):
    """m sorted duplicate-free uids: members of the packs and values between."""
    lo = min(int(u[0]) for u in lists)
    hi = max(int(u[-1]) for u in lists)
    every = np.concatenate(lists)
    take = every[rng.integers(0, every.size, size=m // 2)]
    rand = rng.integers(lo, hi + 1, size=2 * m, dtype=np.uint64)
    s = np.unique(take)
    extra = np.setdiff1d(np.unique(rand), s)
    rng.shuffle(extra)
    return np.sort(np.concatenate([s, extra[:max(m - s.size, 0)]]))[:m]


class RawLib:
    """Another build of the library, called on the same device buffers."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.ua_ctx_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
        self.L.ua_ctx_destroy.argtypes = [C.c_void_p]
        self.L.ua_stats_reset.argtypes = [C.c_void_p]
        self.L.ua_stats_get.argtypes = [C.c_void_p, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        self.L.ua_rows_intersect_packed_dev.argtypes = [
            C.c_void_p, C.POINTER(_lib.UaDRowIsect), C.POINTER(C.c_uint64)]
        self.ctx = C.c_void_p()
        if self.L.ua_ctx_create(C.byref(self.ctx), 0) != 0:
            raise SystemExit(f"cannot create a context from {path}")

    def call(self, d):
        total = C.c_uint64()
        rc = self.L.ua_rows_intersect_packed_dev(self.ctx, C.byref(d), C.byref(total))
        if rc != 0:
            raise SystemExit(f"ua_rows_intersect_packed_dev: {rc}")
        return total.value

    def stats_reset(self):
        self.L.ua_stats_reset(self.ctx)

    def kernel_ms(self):
        n, ms, b = C.c_uint64(), C.c_double(), C.c_uint64()
        self.L.ua_stats_get(self.ctx, C.byref(n), C.byref(ms), C.byref(b))
        return ms.value

    def close(self):
        self.L.ua_ctx_destroy(self.ctx)


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
    args = sys.argv[1:]
    extra = dict(a.split("=", 1) for a in args if "=" in a)
    args = [a for a in args if "=" not in a]
    shapes = args[0].split(",") if args else list(SHAPES)
    reps = int(args[1]) if len(args) > 1 else 7
    dev = "cuda:0"
    eng = algo.Engine(0)
    raws = {label: RawLib(path) for label, path in extra.items()}
    res = {"workload": "rows_isect", "reps": reps, "n_packs": N_PACKS, "configs": []}
    cache = {}
    for shape in shapes:
        if shape not in SHAPES:
            raise SystemExit(f"unknown shape {shape!r}")
        kind, m = SHAPES[shape]
        if kind not in cache:
            cache.clear()
            rng = np.random.default_rng(synth.SEED + 16)
            lists = gen_lists(rng, kind)
            dpb = eng.upload_pack_batch([algo.encode_flat(u, 256) for u in lists])
            cache[kind] = (lists, dpb)
        lists, dpb = cache[kind]
        rng = np.random.default_rng(synth.SEED + 17)
        shared_h = gen_shared(rng, lists, m)
        m = int(shared_h.size)
        shared = torch.from_numpy(shared_h.view(np.int64)).to(dev)
        total = int(sum(dpb.pack_totals))
        caps = [min(int(t), m) for t in dpb.pack_totals]
        o = np.zeros(N_PACKS + 1, dtype=np.int64)
        o[1:] = np.cumsum(caps)
        out_new = torch.empty(max(int(o[-1]), 1), dtype=torch.int64, device=dev)
        ro_new = torch.empty(N_PACKS + 1, dtype=torch.int64, device=dev)
        out_raw = torch.empty_like(out_new)
        ro_raw = torch.empty_like(ro_new)
        out_old = torch.empty_like(out_new)
        outs_old = [out_old[int(o[r]):int(o[r + 1])] if caps[r] else out_old[:1]
                    for r in range(N_PACKS)]
        vs = [shared] * N_PACKS
        dec_vals = torch.empty(total, dtype=torch.int64, device=dev)
        dec_ro = torch.empty(N_PACKS + 1, dtype=torch.int64, device=dev)
        flt_vals = torch.empty(total, dtype=torch.int64, device=dev)
        flt_ro = torch.empty(N_PACKS + 1, dtype=torch.int64, device=dev)

        def new():
            return eng.intersect_rows(dpb, shared, out_vals=out_new, out_row_offs=ro_new)

        def batch():
            return eng.intersect_packed_batch(dpb, vs, outs=outs_old)

        def decflt():
            v, ro = eng.decode_rows(dpb, out_vals=dec_vals, out_row_offs=dec_ro)
            return eng.filter_rows(v, ro, shared, out_vals=flt_vals, out_row_offs=flt_ro)

        vals, ro = new()
        kept = int(vals.numel())
        _, lens = batch()
        fv, fro = decflt()
        want_ro = np.zeros(N_PACKS + 1, dtype=np.int64)
        want_ro[1:] = np.cumsum(lens)
        cat = torch.cat([outs_old[r][:lens[r]] for r in range(N_PACKS)]) if kept else vals
        if not torch.equal(ro.cpu(), torch.from_numpy(want_ro)) or not torch.equal(vals, cat):
            raise SystemExit(f"intersect_rows differs from intersect_packed_batch: {shape}")
        if not torch.equal(ro, fro) or not torch.equal(vals, fv):
            raise SystemExit(f"intersect_rows differs from decode_rows+filter_rows: {shape}")

        d = _lib.UaDRowIsect()
        d.bases, d.num_uids = dpb.bases.data_ptr(), dpb.num_uids.data_ptr()
        d.delta_offs, d.deltas = dpb.delta_offs.data_ptr(), dpb.deltas.data_ptr()
        d.n_blocks, d.n_rows = int(dpb.pbb[-1]), N_PACKS
        d.row_block_base = dpb._pbb_dev.data_ptr()
        d.shared, d.m = shared.data_ptr(), m
        d.out_vals, d.cap_vals = out_raw.data_ptr(), out_raw.numel()
        d.out_row_offs = ro_raw.data_ptr()
        for label, raw in raws.items():
            if raw.call(d) != kept or not torch.equal(out_raw[:kept], vals) or \
                    not torch.equal(ro_raw, ro):
                raise SystemExit(f"build {label} differs from the default build: {shape}")

        paths = [("intersect_rows", new, eng), ("packed_batch", batch, eng),
                 ("decode_filter", decflt, eng)]
        paths += [(f"intersect_rows[{label}]", (lambda raw=raw: raw.call(d)), raw)
                  for label, raw in raws.items()]
        ts = {name: [] for name, _, _ in paths}
        ks = {name: [] for name, _, _ in paths}
        for _ in range(reps):
            for name, fn, owner in paths:
                owner.stats_reset()
                t, _r = timed(fn)
                ts[name].append(t)
                ks[name].append(owner.stats()["kernel_ms"] if owner is eng
                                else owner.kernel_ms())
        cfg = {"shape": shape, "total_uids": total, "kept_uids": kept, "m": m,
               "blocks": int(dpb.pbb[-1]), "deltas_bytes": int(dpb.deltas.numel())}
        for name, _, _ in paths:
            cfg[name] = summarize(ts[name])
            cfg[name]["event_ms"] = round(float(np.median(ks[name])), 4)
        sn = cfg["intersect_rows"]
        for alt in ("packed_batch", "decode_filter"):
            sa = cfg[alt]
            cfg[f"leads_{alt}_by_more_than_twice_its_spread"] = \
                bool(sa["median_ms"] - sn["median_ms"] > 2 * sa["spread_ms"])
        print(f"shape {shape}: " + " ".join(f"{n} {cfg[n]}" for n, _, _ in paths),
              file=sys.stderr)
        res["configs"].append(cfg)
        del out_new, out_raw, out_old, outs_old, dec_vals, flt_vals, shared, vs
    for raw in raws.values():
        raw.close()
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
