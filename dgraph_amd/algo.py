"""Host-side mirror of dgraph's `algo` package over the uidalgo C-ABI.

Function-for-function surface of /root/reference/algo/uidlist.go (same names'
semantics, same argument meaning, status-code errors), plus the batched
device-resident engine the reference's per-key fan-out maps onto
(worker/task.go:834-971 -> one grid).

UID lists are sorted uint64.  torch has no uint64 CUDA dtype, so device
buffers are int64 tensors REINTERPRETED as u64 by the kernels; numpy uint64
arrays cross the host boundary bit-for-bit via .view(int64).

No CPU fallback: every op goes through libuidalgo.so and raises without it.
"""
import ctypes as C
import sys

import numpy as np

from dgraph_amd._lib import (UaDPack, UaDPair, check, lib, _u64p)

_u64 = C.c_uint64


def _np_u64(x):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.uint64))
    return a


_KEEP = np.empty(1, dtype=np.uint64)


def _hptr(a):
    if a.size == 0:
        return _KEEP.ctypes.data_as(_u64p)
    return a.ctypes.data_as(_u64p)


class Engine:
    """One GPU + one HIP stream (wraps ua_ctx)."""

    def __init__(self, device=0):
        self._ctx = C.c_void_p()
        rc = lib().ua_ctx_create(C.byref(self._ctx), device)
        if rc != 0:
            raise RuntimeError(
                f"uidalgo: cannot create GPU context on device {device}: "
                f"{lib().ua_strerror(rc).decode()} — the HIP engine is "
                "mandatory, there is no CPU fallback.")
        self.device = device

    def close(self):
        if self._ctx:
            lib().ua_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            if sys.is_finalizing():
                return  # HIP runtime may already be torn down at interpreter exit
            self.close()
        except Exception:
            pass

    # ---- stats (dominant-kernel HIP-event time) ----
    def stats_reset(self):
        check(lib().ua_stats_reset(self._ctx))

    def stats(self):
        n = _u64()
        ms = C.c_double()
        b = _u64()
        check(lib().ua_stats_get(self._ctx, C.byref(n), C.byref(ms), C.byref(b)))
        return {"launches": n.value, "kernel_ms": ms.value, "bytes_algorithmic": b.value}

    # ---- batched device-resident ops (torch CUDA int64 tensors) ----
    def _run_pairs(self, fn, us, vs, outs):
        np_ = len(us)
        pairs = (UaDPair * np_)()
        for i in range(np_):
            pairs[i].u = us[i].data_ptr()
            pairs[i].n = us[i].numel()
            pairs[i].v = vs[i].data_ptr()
            pairs[i].m = vs[i].numel()
            pairs[i].out = outs[i].data_ptr()
        lens = (_u64 * np_)()
        check(fn(self._ctx, pairs, np_, lens))
        return [int(lens[i]) for i in range(np_)]

    def intersect_pairs(self, us, vs, outs=None):
        """Batched algo.IntersectWith.  us/vs: lists of CUDA int64 tensors
        (u64 bits).  Returns (outs, lens); outs[i][:lens[i]] is the result."""
        import torch
        if outs is None:
            outs = [torch.empty(min(u.numel(), v.numel()), dtype=torch.int64,
                                device=u.device) for u, v in zip(us, vs)]
        lens = self._run_pairs(lib().ua_intersect_batch_dev, us, vs, outs)
        return outs, lens

    def merge_pairs(self, us, vs, outs=None):
        import torch
        if outs is None:
            outs = [torch.empty(u.numel() + v.numel(), dtype=torch.int64,
                                device=u.device) for u, v in zip(us, vs)]
        lens = self._run_pairs(lib().ua_merge_batch_dev, us, vs, outs)
        return outs, lens

    def difference_pairs(self, us, vs, outs=None):
        import torch
        if outs is None:
            outs = [torch.empty(max(u.numel(), 1), dtype=torch.int64, device=u.device)
                    for u in us]
        lens = self._run_pairs(lib().ua_difference_batch_dev, us, vs, outs)
        return outs, lens

    def make_batch(self, us, vs, outs):
        """Prepared batch: descriptor upload + merge-path partition done once
        (ua_batch_create); run ops repeatedly with Batch.run().  The input
        tensors' contents must stay unchanged while the batch lives."""
        np_ = len(us)
        pairs = (UaDPair * np_)()
        for i in range(np_):
            pairs[i].u = us[i].data_ptr()
            pairs[i].n = us[i].numel()
            pairs[i].v = vs[i].data_ptr()
            pairs[i].m = vs[i].numel()
            pairs[i].out = outs[i].data_ptr()
        h = C.c_void_p()
        check(lib().ua_batch_create(self._ctx, pairs, np_, C.byref(h)))
        b = Batch(self, h, np_, (us, vs, outs))
        b._caps = [(us[i].numel(), vs[i].numel(), outs[i].numel())
                   for i in range(np_)]
        return b

    def intersect_sorted(self, lists):
        """algo.IntersectSorted (uidlist.go:297): k-way fold, smallest first."""
        import torch
        k = len(lists)
        if k == 0:
            return torch.empty(0, dtype=torch.int64)
        ptrs = (C.c_void_p * k)(*[int(t.data_ptr()) for t in lists])
        lens = (_u64 * k)(*[t.numel() for t in lists])
        cap = min(t.numel() for t in lists)
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=lists[0].device)
        out_n = _u64()
        check(lib().ua_intersect_k_dev(self._ctx, C.cast(ptrs, C.POINTER(C.c_void_p)),
                                       lens, k, C.c_void_p(out.data_ptr()),
                                       C.byref(out_n)))
        return out[:out_n.value]

    def merge_sorted(self, lists):
        """algo.MergeSorted (uidlist.go:448): dedup'd k-way union."""
        import torch
        k = len(lists)
        if k == 0:
            return torch.empty(0, dtype=torch.int64)
        ptrs = (C.c_void_p * k)(*[int(t.data_ptr()) for t in lists])
        lens = (_u64 * k)(*[t.numel() for t in lists])
        cap = sum(t.numel() for t in lists)
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=lists[0].device)
        out_n = _u64()
        check(lib().ua_merge_k_dev(self._ctx, C.cast(ptrs, C.POINTER(C.c_void_p)),
                                   lens, k, C.c_void_p(out.data_ptr()), C.byref(out_n)))
        return out[:out_n.value]

    def merge_all_pairs(self, us, vs, outs=None):
        """Batched duplicate-KEEPING merge of sorted runs (no dedup)."""
        import torch
        if outs is None:
            outs = [torch.empty(max(u.numel() + v.numel(), 1), dtype=torch.int64,
                                device=u.device) for u, v in zip(us, vs)]
        lens = self._run_pairs(lib().ua_merge_all_batch_dev, us, vs, outs)
        return outs, lens

    def sort_segments(self, tensors):
        """Batched segmented sort in place (u64 ascending, duplicates kept):
        the sort-path primitive (worker/sort.go UidMatrix shapes, SURVEY
        §8f row 3)."""
        import torch
        from dgraph_amd._lib import UaDSeg
        k = len(tensors)
        if k == 0:
            return tensors
        tmps = [torch.empty(max(t.numel(), 1), dtype=torch.int64, device=t.device)
                for t in tensors]
        segs = (UaDSeg * k)()
        for i, t in enumerate(tensors):
            segs[i].data = t.data_ptr()
            segs[i].n = t.numel()
            segs[i].tmp = tmps[i].data_ptr()
        check(lib().ua_sort_segments_dev(self._ctx, segs, k))
        return tensors

    def apply_filter_batch(self, us, masks, outs=None):
        """Batched algo.ApplyFilter (uidlist.go:21): order-preserving mask
        compaction on device.  us: CUDA int64 tensors; masks: CUDA uint8/bool
        tensors (nonzero = keep).  outs may be the us themselves (in-place,
        the reference's shape).  Returns (outs, lens)."""
        import torch
        from dgraph_amd._lib import UaDFilter
        k = len(us)
        if outs is None:
            outs = us  # in-place like the reference
        tasks = (UaDFilter * max(k, 1))()
        for i in range(k):
            m = masks[i]
            if m.dtype == torch.bool:
                m = m.view(torch.uint8)
            assert m.dtype == torch.uint8 and m.numel() == us[i].numel()
            tasks[i].u = us[i].data_ptr()
            tasks[i].n = us[i].numel()
            tasks[i].mask = m.data_ptr()
            tasks[i].out = outs[i].data_ptr()
        lens = (_u64 * max(k, 1))()
        check(lib().ua_apply_filter_batch_dev(self._ctx, tasks, k, lens))
        return outs, [int(lens[i]) for i in range(k)]

    def index_of_batch(self, u, queries):
        """Batched algo.IndexOf: u, queries CUDA int64; returns int64 tensor
        of positions (-1 = absent)."""
        import torch
        out = torch.empty(queries.numel(), dtype=torch.int64, device=u.device)
        check(lib().ua_index_of_batch_dev(
            self._ctx, C.c_void_p(u.data_ptr()), u.numel(),
            C.c_void_p(queries.data_ptr()), queries.numel(),
            C.c_void_p(out.data_ptr())))
        return out

    def filter_rows(self, vals, row_offs, shared, mode=0, out_vals=None,
                    out_row_offs=None):
        """Row-wise UID-matrix filter against one shared sorted list
        (ua_rows_filter_dev): updateUidMatrix, query/query.go:1425-1437, and
        the worker/task.go:1352,1617,1692,1778 per-row IntersectWith loops as
        ONE grid over the flat element array.  vals (rows concatenated),
        row_offs (n_rows+1) and shared are CUDA int64 tensors holding u64
        bits; rows need not be sorted.  mode is ROWS_INTERSECT or
        ROWS_DIFFERENCE.  Returns (out_vals[:kept], out_row_offs); the
        outputs must not alias the inputs."""
        import torch
        from dgraph_amd._lib import UaDRows
        total = vals.numel()
        n_rows = row_offs.numel() - 1
        if n_rows < 0:
            raise ValueError("row_offs needs n_rows + 1 entries")
        if out_vals is None:
            out_vals = torch.empty(max(total, 1), dtype=torch.int64, device=vals.device)
        if out_row_offs is None:
            out_row_offs = torch.empty(n_rows + 1, dtype=torch.int64, device=vals.device)
        if out_vals.numel() < total:
            raise ValueError(f"out_vals capacity {out_vals.numel()} < required {total}")
        if out_row_offs.numel() < n_rows + 1:
            raise ValueError(f"out_row_offs capacity {out_row_offs.numel()} < "
                             f"required {n_rows + 1}")
        d = UaDRows()
        d.vals = vals.data_ptr()
        d.row_offs = row_offs.data_ptr()
        d.n_rows = n_rows
        d.total = total
        d.shared = shared.data_ptr()
        d.m = shared.numel()
        d.out_vals = out_vals.data_ptr()
        d.out_row_offs = out_row_offs.data_ptr()
        kept = _u64()
        check(lib().ua_rows_filter_dev(self._ctx, C.byref(d), int(mode), C.byref(kept)))
        return out_vals[:kept.value], out_row_offs[:n_rows + 1]

    def union_rows(self, vals, out=None):
        """DestUIDs of a CSR UID matrix (ua_rows_union_dev): the ascending
        duplicate-free set of vals, the rows concatenated — what
        algo.MergeSorted(UidMatrix) gives at query/query.go:1874,2290,2505,
        and also defined when the rows are not uid-sorted.  Row offsets are
        not needed.  vals: CUDA int64 tensor holding u64 bits; out, if given,
        needs capacity vals.numel() and may be vals itself (no other
        overlap).  Returns out[:n]."""
        import torch
        total = vals.numel()
        if out is None:
            out = torch.empty(max(total, 1), dtype=torch.int64, device=vals.device)
        if out.numel() < total:
            raise ValueError(f"out capacity {out.numel()} < required {total}")
        n = _u64()
        check(lib().ua_rows_union_dev(self._ctx, C.c_void_p(vals.data_ptr()), total,
                                      C.c_void_p(out.data_ptr()), C.byref(n)))
        return out[:n.value]

    def sort_rows(self, vals, row_offs, keys=None, has=None, count=0, offset=0, desc=False,
                  multi=False, drop_nulls=False, count_only=False, want_src=False,
                  out_vals=None, out_row_offs=None):
        """Order and pagination of every row of a CSR UID matrix in ONE call
        (ua_rows_sort_dev): sortWithoutIndex (worker/sort.go:139-187),
        sortAndPaginateUsingVar (query/query.go:2697-2738, drop_nulls) and,
        with keys=None, applyPagination (query/query.go:2493-2507).  vals,
        row_offs and keys (parallel to vals, order-preserving u64) are CUDA
        int64 tensors holding u64 bits; has is a CUDA uint8/bool tensor
        (nonzero = the element has a key) or None.  Per row: valued elements
        by key (ties by input position), then the nulls, then
        x.PageRange(count, offset), grown over equal keys with multi.
        Returns (out_vals[:total], out_row_offs[, out_src][, ms_offs]):
        out_src (want_src) is each output element's flat input index, ms_offs
        (multi) the int32 multiSortOffsets.  With count_only out_vals is
        empty.  The default capacity is vals.numel(); the outputs must not
        alias the inputs."""
        import torch
        from dgraph_amd._lib import (UA_SORT_DESC, UA_SORT_DROP_NULLS, UA_SORT_MULTI,
                                     UaDRowSort)
        dev = vals.device
        total = vals.numel()
        n_rows = row_offs.numel() - 1
        if n_rows < 0:
            raise ValueError("row_offs needs n_rows + 1 entries")
        if keys is not None and keys.numel() != total:
            raise ValueError("keys must be parallel to vals")
        if has is not None:
            if has.numel() != total:
                raise ValueError("has must be parallel to vals")
            if has.dtype == torch.bool:
                has = has.view(torch.uint8)
            if has.dtype != torch.uint8:
                raise ValueError("has must be a uint8 or bool tensor")
        if want_src and count_only:
            raise ValueError("count_only delivers no out_src")
        if out_row_offs is None:
            out_row_offs = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        if out_row_offs.numel() < n_rows + 1:
            raise ValueError(f"out_row_offs capacity {out_row_offs.numel()} < "
                             f"required {n_rows + 1}")
        cap = 0
        if not count_only:
            if out_vals is None:
                out_vals = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            cap = out_vals.numel()
        out_src = torch.empty(max(cap, 1), dtype=torch.int64, device=dev) if want_src else None
        ms = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev) if multi else None
        if total == 0:  # an empty tensor has no address; "keys given" needs one
            spare = torch.zeros(1, dtype=torch.int64, device=dev)
            keys = spare if keys is not None else None
            has = spare if has is not None else None
        d = UaDRowSort()
        d.vals = vals.data_ptr()
        d.row_offs = row_offs.data_ptr()
        d.n_rows = n_rows
        d.total = total
        d.keys = keys.data_ptr() if keys is not None else None
        d.has = has.data_ptr() if has is not None else None
        d.flags = ((UA_SORT_DESC if desc else 0) | (UA_SORT_MULTI if multi else 0) |
                   (UA_SORT_DROP_NULLS if drop_nulls else 0))
        d.count = int(count)
        d.offset = int(offset)
        d.out_vals = None if count_only else out_vals.data_ptr()
        d.cap_vals = cap
        d.out_row_offs = out_row_offs.data_ptr()
        d.out_src = out_src.data_ptr() if want_src else None
        d.out_ms_offs = ms.data_ptr() if multi else None
        need = _u64()
        rc = lib().ua_rows_sort_dev(self._ctx, C.byref(d), C.byref(need))
        if rc == 3 and not count_only and need.value > cap:
            raise ValueError(f"out_vals capacity {cap} < required {need.value}")
        check(rc)
        if count_only:
            res = [torch.empty(0, dtype=torch.int64, device=dev), out_row_offs[:n_rows + 1]]
        else:
            res = [out_vals[:need.value], out_row_offs[:n_rows + 1]]
        if want_src:
            res.append(out_src[:need.value])
        if multi:
            res.append(ms[:n_rows])
        return tuple(res)

    def paginate_rows(self, vals, row_offs, count, offset):
        """applyPagination (query/query.go:2493-2507) and the cascade
        paginations (query/query.go:1483-1487, 3006-3010): x.PageRange(count,
        offset) of every row as one call — sort_rows with keys=None."""
        return self.sort_rows(vals, row_offs, count=count, offset=offset)

    def transpose_rows(self, vals, row_offs, row_uids=None, row_keep=None, unique=False,
                       want_src=False, groups_only=False, count_only=False):
        """The transpose of a CSR UID matrix in ONE call
        (ua_rows_transpose_dev): src -> [dst...] into dst -> [src...], the
        grouping dedup.addValue builds per edge (query/groupby.go:104-128,
        formResult :195-260) and the postings rebuildReverseEdges adds one by
        one (posting/index.go:1759-1791).  vals, row_offs and row_uids (the
        rows' uids; None = the row index) are CUDA int64 tensors holding u64
        bits, row_keep a CUDA uint8/bool tensor per row (nonzero = the row takes
        part) or None.  Returns (keys, offs, vals[, src]): the distinct values
        ascending, the CSR offsets of their groups, and per group the uids of
        the rows holding the value in input order; src (want_src) is each
        entry's flat input index.  unique keeps one entry per (value, row).
        groups_only returns (keys, offs), count_only (n_groups, n_entries)."""
        import torch
        from dgraph_amd._lib import UA_TR_UNIQUE, UaDRowTr
        dev = vals.device
        total = vals.numel()
        n_rows = row_offs.numel() - 1
        if n_rows < 0:
            raise ValueError("row_offs needs n_rows + 1 entries")
        if row_uids is not None and row_uids.numel() != n_rows:
            raise ValueError("row_uids needs one entry per row")
        if row_keep is not None:
            if row_keep.numel() != n_rows:
                raise ValueError("row_keep needs one entry per row")
            if row_keep.dtype == torch.bool:
                row_keep = row_keep.view(torch.uint8)
            if row_keep.dtype != torch.uint8:
                raise ValueError("row_keep must be a uint8 or bool tensor")
        if want_src and (groups_only or count_only):
            raise ValueError("out_src comes with the full form only")
        d = UaDRowTr()
        d.vals = vals.data_ptr() if total else None
        d.row_offs = row_offs.data_ptr()
        d.n_rows = n_rows
        d.total = total
        d.row_uids = row_uids.data_ptr() if row_uids is not None and n_rows else None
        d.row_keep = row_keep.data_ptr() if row_keep is not None and n_rows else None
        d.flags = UA_TR_UNIQUE if unique else 0
        keys = offs = out = src = None
        if not count_only:  # both requirements are at most total
            keys = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
            offs = torch.empty(total + 1, dtype=torch.int64, device=dev)
            d.out_keys, d.out_offs, d.cap_keys = keys.data_ptr(), offs.data_ptr(), total
            if not groups_only:
                out = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
                d.out_vals, d.cap_vals = out.data_ptr(), total
                if want_src:
                    src = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
                    d.out_src = src.data_ptr()
        ng, nt = _u64(), _u64()
        check(lib().ua_rows_transpose_dev(self._ctx, C.byref(d), C.byref(ng), C.byref(nt)))
        if count_only:
            return ng.value, nt.value
        res = [keys[:ng.value], offs[:ng.value + 1]]
        if not groups_only:
            res.append(out[:nt.value])
            if want_src:
                res.append(src[:nt.value])
        return tuple(res)

    def reverse_rows(self, dpb, mut_uids, mut_ops, row_mut_base, row_uids=None,
                     block_size=256):
        """A batched rebuildReverseEdges (posting/index.go:1759-1791) on the
        device: decode_rows_mut with after = first = 0, transpose_rows with
        unique=True, then encode_rows.  Takes decode_rows_mut's arguments and
        the forward lists' uids (ascending; None = the row index).  Returns
        (keys, arena): the uids that own a reverse list, ascending, and
        encode_rows' arena with one pack per key."""
        vals, row_offs = self.decode_rows_mut(dpb, mut_uids, mut_ops, row_mut_base)
        keys, offs, rev = self.transpose_rows(vals, row_offs, row_uids=row_uids, unique=True)
        return keys, self.encode_rows(rev, offs, block_size)

    # ---- packed (codec) path ----
    def upload_pack(self, bases, num_uids, delta_offs, deltas_blob, block_size):
        """Upload flat pack arrays (from encode_flat) -> DPack on this GPU."""
        import torch
        dev = f"cuda:{self.device}"
        t_bases = torch.from_numpy(_np_u64(bases).view(np.int64)).to(dev)
        t_nums = torch.from_numpy(np.ascontiguousarray(num_uids, dtype=np.uint32)
                                  .view(np.int32)).to(dev)
        t_offs = torch.from_numpy(_np_u64(delta_offs).view(np.int64)).to(dev)
        blob = np.ascontiguousarray(deltas_blob, dtype=np.uint8)
        t_blob = torch.from_numpy(blob.view(np.int8)).to(dev) if blob.size else \
            torch.zeros(1, dtype=torch.int8, device=dev)
        total = int(np.asarray(num_uids, dtype=np.uint64).sum())
        return DPack(t_bases, t_nums, t_offs, t_blob, int(block_size), total)

    def upload_pack_batch(self, packs):
        """Concatenate many flat packs (tuples from encode_flat) into one
        device arena + pack boundaries — the collected form of a
        handleUidPostings fan-out (worker/task.go:834-971)."""
        import torch
        dev = f"cuda:{self.device}"
        pbb = np.zeros(len(packs) + 1, dtype=np.uint64)
        blob_base = 0
        all_bases, all_nums, all_offs, all_blobs, totals = [], [], [], [], []
        for i, (bases, nums, offs, blob, total) in enumerate(packs):
            pbb[i + 1] = pbb[i] + bases.size
            all_bases.append(bases)
            all_nums.append(nums)
            all_offs.append(np.asarray(offs[:-1], dtype=np.uint64) + np.uint64(blob_base))
            all_blobs.append(blob)
            totals.append(total)
            blob_base += blob.size
        cat = lambda xs, dt: np.ascontiguousarray(
            np.concatenate(xs) if xs else np.empty(0, dtype=dt), dtype=dt)
        bases = cat(all_bases, np.uint64)
        nums = cat(all_nums, np.uint32)
        offs = np.concatenate([cat(all_offs, np.uint64),
                               np.array([blob_base], dtype=np.uint64)])
        blob = cat(all_blobs, np.uint8)
        dp = self.upload_pack(bases, nums, offs, blob, 0)
        dp.pbb = pbb
        dp.pack_totals = totals
        return dp

    def decode_rows(self, dpb, afters=None, firsts=None, out_vals=None,
                    out_row_offs=None, count_only=False):
        """The UID matrix of a whole fan-out in ONE call (ua_rows_decode_dev):
        handleUidPostings' per-key pl.Uids(opts) with opts.Intersect == nil
        (worker/task.go:834-971, posting/list.go:1786-1902).  dpb is an
        upload_pack_batch arena; row r is pack r's uids restricted to
        x > afters[r] (0 keeps all), then cut by firsts[r] (> 0 the first
        that many, < 0 the last, 0 all).  afters/firsts: None, one int for
        every row, a sequence, or a CUDA tensor (int64 u64 bits / int32).
        Returns (vals[:total], row_offs), the CSR form filter_rows and
        union_rows take; with count_only vals is empty and row_offs holds
        every key's List.Length (list.go:1345)."""
        from dgraph_amd._lib import UaDRowPacks
        full = 0 if count_only else int(sum(dpb.pack_totals))
        # without afters and firsts every row is whole: a short buffer is known now
        if afters is None and firsts is None and out_vals is not None and not count_only \
                and out_vals.numel() < full:
            raise ValueError(f"out_vals capacity {out_vals.numel()} < required {full}")
        return self._rows_call(lib().ua_rows_decode_dev, UaDRowPacks(), dpb, afters, firsts,
                               out_vals, out_row_offs, count_only, lambda: full)

    def _rows_arena(self, dpb):
        """(device, n_rows, n_blocks) of an upload_pack_batch arena; its row
        boundaries go to the device once and stay with it (_pbb_dev)."""
        import torch
        dev = dpb.bases.device
        n_rows = len(dpb.pbb) - 1
        if getattr(dpb, "_pbb_dev", None) is None:
            dpb._pbb_dev = torch.from_numpy(_np_u64(dpb.pbb).view(np.int64)).to(dev)
        return dev, n_rows, int(dpb.pbb[n_rows])

    def _rows_call(self, fn, d, dpb, afters, firsts, out_vals, out_row_offs, count_only, full):
        """The one path of decode_rows, intersect_rows and decode_rows_mut: a
        pack fan-out in, a CSR matrix out.  d is the call's descriptor with
        its own slots filled, fn its device entry, full() the capacity a
        missing out_vals gets.  firsts is None for a call without first."""
        import torch
        dev, n_rows, nb = self._rows_arena(dpb)
        t_after = _per_row_dev(afters, n_rows, np.uint64, dev)
        t_first = _per_row_dev(firsts, n_rows, np.int32, dev)
        if out_row_offs is None:
            out_row_offs = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        if out_row_offs.numel() < n_rows + 1:
            raise ValueError(f"out_row_offs capacity {out_row_offs.numel()} < "
                             f"required {n_rows + 1}")
        cap = 0
        if not count_only:
            if out_vals is None:
                out_vals = torch.empty(max(full(), 1), dtype=torch.int64, device=dev)
            cap = out_vals.numel()
        d.bases = dpb.bases.data_ptr()
        d.num_uids = dpb.num_uids.data_ptr()
        d.delta_offs = dpb.delta_offs.data_ptr()
        d.deltas = dpb.deltas.data_ptr()
        d.n_blocks = nb
        d.row_block_base = dpb._pbb_dev.data_ptr()
        d.n_rows = n_rows
        d.after = t_after.data_ptr() if t_after is not None else None
        if t_first is not None:
            d.first = t_first.data_ptr()
        d.out_vals = None if count_only else out_vals.data_ptr()
        d.cap_vals = cap
        d.out_row_offs = out_row_offs.data_ptr()
        total = _u64()
        rc = fn(self._ctx, C.byref(d), C.byref(total))
        if rc == 3 and not count_only and total.value > cap:
            raise ValueError(f"out_vals capacity {cap} < required {total.value}")
        check(rc)
        if count_only:
            return torch.empty(0, dtype=torch.int64, device=dev), out_row_offs[:n_rows + 1]
        return out_vals[:total.value], out_row_offs[:n_rows + 1]

    def decode_rows_mut(self, dpb, mut_uids, mut_ops, row_mut_base, afters=None,
                        firsts=None, out_vals=None, out_row_offs=None, count_only=False):
        """The UID matrix of a whole fan-out over LIVE lists in ONE call
        (ua_rows_decode_mut_dev): handleUidPostings' per-key pl.Uids(opts) on
        lists with a mutable layer, i.e. List.iterate's merge of the pack with
        the picked postings (posting/list.go:1135-1251).  dpb is an
        upload_pack_batch arena (an empty pack = a row without blocks); row r
        owns mut_uids/mut_ops[row_mut_base[r]:row_mut_base[r+1]], strictly
        ascending uids with op MUT_DEL deleting and any other op setting.
        Row r = sorted((pack r - uids(M)) | sets(M)), then x > afters[r]
        (0 keeps all), then firsts[r], as in decode_rows.  mut_uids (u64),
        mut_ops (u8) and row_mut_base (u64, n_rows + 1) are host sequences or
        CUDA tensors (int64 bits / uint8 / int64).  Returns (vals[:total],
        row_offs); with count_only vals is empty and row_offs holds every
        key's List.Length (list.go:1345).  The default capacity is
        sum(pack_totals) + n_mut."""
        import torch
        from dgraph_amd._lib import UaDRowMut
        dev, n_rows, _ = self._rows_arena(dpb)

        def dev_arr(x, n, np_dt, t_dt, what):
            if isinstance(x, torch.Tensor):
                if x.dtype != t_dt or x.numel() < n:
                    raise ValueError(f"{what} needs {n} x {t_dt}")
                return x
            a = np.ascontiguousarray(np.asarray(x, dtype=np_dt).ravel())
            if a.size != n:
                raise ValueError(f"{what} needs {n} entries, got {a.size}")
            return _to_dev(a, dev) if n else None

        n_mut = mut_uids.numel() if isinstance(mut_uids, torch.Tensor) else len(mut_uids)
        keep = [dev_arr(mut_uids, n_mut, np.uint64, torch.int64, "mut_uids"),
                dev_arr(mut_ops, n_mut, np.uint8, torch.uint8, "mut_ops")]
        d = UaDRowMut()
        d.n_mut = n_mut
        if n_mut:  # without a layer the three arrays stay NULL: the plain call
            keep.append(dev_arr(row_mut_base, n_rows + 1, np.uint64, torch.int64,
                                "row_mut_base"))
            d.mut_uids, d.mut_ops, d.row_mut_base = (t.data_ptr() for t in keep)
        return self._rows_call(lib().ua_rows_decode_mut_dev, d, dpb, afters, firsts, out_vals,
                               out_row_offs, count_only,
                               lambda: int(sum(dpb.pack_totals)) + n_mut)

    def intersect_rows(self, dpb, shared, afters=None, out_vals=None, out_row_offs=None,
                       count_only=False):
        """The UID matrix of a whole fan-out under one filter list in ONE call
        (ua_rows_intersect_packed_dev): handleUidPostings' per-key
        pl.Uids(opts) with opts.Intersect != nil, i.e. one
        algo.IntersectCompressedWith(pack, after, q.UidList) per key
        (posting/list.go:1823-1829, uidlist.go:33).  dpb is an
        upload_pack_batch arena; shared a CUDA int64 tensor of u64 bits,
        sorted ascending and duplicate-free.  Row r is pack r's uids with
        x >= afters[r] (INCLUSIVE, unlike decode_rows) and x in shared; there
        is no first on this branch.  afters: None, one int for every row, a
        sequence, or a CUDA int64 tensor.  Returns (vals[:total], row_offs),
        the CSR form filter_rows and union_rows take; with count_only vals is
        empty and row_offs holds every key's count under the filter."""
        import torch
        from dgraph_amd._lib import UaDRowIsect
        m = shared.numel()
        if shared.dtype != torch.int64:
            raise ValueError("shared needs int64 (u64 bits)")
        d = UaDRowIsect()
        d.shared = shared.data_ptr() if m else None
        d.m = m
        return self._rows_call(lib().ua_rows_intersect_packed_dev, d, dpb, afters, None,
                               out_vals, out_row_offs, count_only,
                               lambda: int(sum(min(int(t), m) for t in dpb.pack_totals)))

    def intersect_packed_batch(self, dpb, vs, outs=None, afters=None):
        """Batched algo.IntersectCompressedWith: every pack of the fan-out in
        ONE grid.  vs: per-pack CUDA int64 tensors (may repeat one shared
        tensor — the q.UidList shape).  Returns (outs, lens)."""
        import torch
        from dgraph_amd._lib import UaPTask
        n = len(dpb.pbb) - 1
        assert len(vs) == n
        if afters is None:
            afters = [0] * n
        if outs is None:
            outs = [torch.empty(max(min(dpb.pack_totals[i], vs[i].numel()), 1),
                                dtype=torch.int64, device=vs[i].device)
                    for i in range(n)]
        tasks = (UaPTask * n)()
        for i in range(n):
            tasks[i].v = vs[i].data_ptr()
            tasks[i].m = vs[i].numel()
            tasks[i].out = outs[i].data_ptr()
            tasks[i].after_uid = afters[i]
        pbb = (C.c_uint64 * (n + 1))(*[int(x) for x in dpb.pbb])
        lens = (C.c_uint64 * n)()
        check(lib().ua_intersect_packed_batch_dev(
            self._ctx, C.c_void_p(dpb.bases.data_ptr()),
            C.c_void_p(dpb.num_uids.data_ptr()), C.c_void_p(dpb.delta_offs.data_ptr()),
            C.c_void_p(dpb.deltas.data_ptr()), pbb, n, tasks, lens))
        return outs, [int(lens[i]) for i in range(n)]

    def make_pack_batch(self, dpb, vs, outs=None, afters=None):
        """Prepared pack fan-out (ua_pbatch): a standing query plan — tasks
        and boundaries upload once, each run() is launches only.  vs may
        repeat one shared tensor (the q.UidList shape)."""
        import torch
        from dgraph_amd._lib import UaPTask
        n = len(dpb.pbb) - 1
        assert len(vs) == n
        if afters is None:
            afters = [0] * n
        if outs is None:
            outs = [torch.empty(max(min(dpb.pack_totals[i], vs[i].numel()), 1),
                                dtype=torch.int64, device=vs[i].device)
                    for i in range(n)]
        tasks = (UaPTask * n)()
        for i in range(n):
            tasks[i].v = vs[i].data_ptr()
            tasks[i].m = vs[i].numel()
            tasks[i].out = outs[i].data_ptr()
            tasks[i].after_uid = afters[i]
        pbb = (C.c_uint64 * (n + 1))(*[int(x) for x in dpb.pbb])
        h = C.c_void_p()
        check(lib().ua_pbatch_create(
            self._ctx, C.c_void_p(dpb.bases.data_ptr()),
            C.c_void_p(dpb.num_uids.data_ptr()), C.c_void_p(dpb.delta_offs.data_ptr()),
            C.c_void_p(dpb.deltas.data_ptr()), pbb, n, tasks, C.byref(h)))
        return PackBatch(self, h, n, (dpb, vs, outs))

    def intersect_packed(self, dpack, after, v, out=None):
        """algo.IntersectCompressedWith (uidlist.go:33): fused decode+intersect."""
        import torch
        if out is None:
            out = torch.empty(max(min(dpack.total_uids, v.numel()), 1),
                              dtype=torch.int64, device=v.device)
        out_n = _u64()
        pk = dpack.struct()
        check(lib().ua_intersect_packed_dev(
            self._ctx, C.byref(pk), _u64(after), C.c_void_p(v.data_ptr()),
            v.numel(), C.c_void_p(out.data_ptr()), C.byref(out_n)))
        return out[:out_n.value]

    def encode_dev(self, uids, block_size=256):
        """codec.Encode on the GPU (codec.go:393): sorted device int64 (u64
        bits) -> DPack resident in HBM.  Byte-identical to the reference
        group-varint block format."""
        import torch
        n = uids.numel()
        dev = uids.device
        mb = max(n, 1)
        bases = torch.empty(mb, dtype=torch.int64, device=dev)
        nums = torch.empty(mb, dtype=torch.int32, device=dev)
        offs = torch.empty(mb + 1, dtype=torch.int64, device=dev)
        blob = torch.empty(6 * mb + 24, dtype=torch.int8, device=dev)
        nb = _u64()
        db = _u64()
        check(lib().ua_encode_dev(
            self._ctx, C.c_void_p(uids.data_ptr()), n, block_size,
            C.c_void_p(bases.data_ptr()), C.c_void_p(nums.data_ptr()),
            C.c_void_p(offs.data_ptr()), C.c_void_p(blob.data_ptr()),
            C.byref(nb), C.byref(db)))
        k = nb.value
        return DPack(bases[:max(k, 1)], nums[:max(k, 1)], offs[:k + 1],
                     blob[:max(db.value, 1)], int(block_size), n) if k else \
            DPack(bases[:0], nums[:0], offs[:1], blob[:1], int(block_size), 0)

    def encode_rows(self, vals, row_offs, block_size=256, count_only=False, out=None,
                    row_block_base=None):
        """A CSR UID matrix into a fan-out of UidPacks in ONE call
        (ua_rows_encode_dev): one codec.Encoder{BlockSize} per row
        (codec.go:57-136), as List.encode (posting/list.go:1609-1664) and the
        bulk reducer (dgraph/cmd/bulk/reduce.go:811-861) run it per key.  vals
        (rows concatenated, each strictly ascending) and row_offs (n_rows + 1)
        are CUDA int64 tensors holding u64 bits.  Makes a count-only call, an
        exact allocation and a full call; out = (bases int64, num_uids int32,
        delta_offs int64, deltas int8) skips the first (short buffers raise
        ValueError with the required sizes).  Returns the arena decode_rows,
        intersect_rows and decode_rows_mut take (a DPack with pbb, _pbb_dev
        and pack_totals); with count_only (n_blocks, deltas_bytes,
        row_block_base) and nothing encoded."""
        import torch
        from dgraph_amd._lib import UaDRowEnc
        dev = vals.device
        total = vals.numel()
        n_rows = row_offs.numel() - 1
        if n_rows < 0:
            raise ValueError("row_offs needs n_rows + 1 entries")
        if row_block_base is None:
            row_block_base = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        if row_block_base.numel() < n_rows + 1:
            raise ValueError(f"row_block_base capacity {row_block_base.numel()} < "
                             f"required {n_rows + 1}")
        d = UaDRowEnc()
        d.vals = vals.data_ptr() if total else None
        d.row_offs = row_offs.data_ptr()
        d.n_rows = n_rows
        d.total = total
        d.block_size = block_size
        d.row_block_base = row_block_base.data_ptr()
        nb, db = _u64(), _u64()

        def call(bufs):
            if bufs is None:
                d.bases = d.num_uids = d.delta_offs = d.deltas = None
                d.cap_blocks = d.cap_deltas = 0
            else:
                bases, nums, offs, blob = bufs
                if offs.numel() < 1 or not bases.numel() or not nums.numel() or \
                        not blob.numel():
                    raise ValueError("every pack buffer needs at least one element")
                d.bases, d.num_uids = bases.data_ptr(), nums.data_ptr()
                d.delta_offs, d.deltas = offs.data_ptr(), blob.data_ptr()
                d.cap_blocks = min(bases.numel(), nums.numel(), offs.numel() - 1)
                d.cap_deltas = blob.numel()
            rc = lib().ua_rows_encode_dev(self._ctx, C.byref(d), C.byref(nb), C.byref(db))
            if rc == 3 and bufs is not None and (nb.value > d.cap_blocks or
                                                 db.value > d.cap_deltas):
                raise ValueError(f"pack buffers hold {d.cap_blocks} blocks / {d.cap_deltas} "
                                 f"bytes < required {nb.value} / {db.value}")
            check(rc)

        if count_only or out is None:
            call(None)
            if count_only:
                return nb.value, db.value, row_block_base[:n_rows + 1]
            k, nbytes = nb.value, db.value
            out = (torch.empty(max(k, 1), dtype=torch.int64, device=dev),
                   torch.empty(max(k, 1), dtype=torch.int32, device=dev),
                   torch.empty(k + 1, dtype=torch.int64, device=dev),
                   torch.empty(max(nbytes, 1), dtype=torch.int8, device=dev))
        call(out)
        k = nb.value
        bases, nums, offs, blob = out
        return RowArena(bases[:k], nums[:k], offs[:k + 1], blob[:max(db.value, 1)],
                        int(block_size), total, row_block_base[:n_rows + 1],
                        row_offs[:n_rows + 1])

    def rollup_rows(self, dpb, mut_uids, mut_ops, row_mut_base, block_size=256):
        """A batched rollup of REF-only lists: List.encode over List.iterate
        (posting/list.go:1609-1664) for every row of an arena, i.e.
        decode_rows_mut with after = first = 0, then encode_rows.  Takes
        decode_rows_mut's arguments and returns encode_rows' arena."""
        vals, row_offs = self.decode_rows_mut(dpb, mut_uids, mut_ops, row_mut_base)
        return self.encode_rows(vals, row_offs, block_size)

    # ---- packed compositions (algo/packed.go) ----
    def merge_sorted_packed(self, lists, block_size=256):
        """algo.MergeSortedPacked (packed.go:222): dedup k-way union, packed
        on-device."""
        return self.encode_dev(self.merge_sorted(lists), block_size)

    def intersect_sorted_packed(self, dpacks):
        """algo.IntersectSortedPacked (packed.go:100): decode each pack,
        fold-intersect smallest-first, re-pack (block size of the first
        list, like the reference)."""
        bs = dpacks[0].block_size if dpacks else 10
        lists = [self.decode_pack(dp) for dp in dpacks]
        return self.encode_dev(self.intersect_sorted(lists), bs)

    def apply_filter_packed(self, dpack, mask_fn):
        """algo.ApplyFilterPacked (packed.go:16): decode, boolean-mask
        compaction, re-pack."""
        dec = self.decode_pack(dpack)
        return self.encode_dev(dec[mask_fn(dec)], dpack.block_size)

    def decode_pack(self, dpack, seek=0, out=None):
        """codec.Decode(pack, seek) on the GPU (codec.go:444)."""
        import torch
        if out is None:
            out = torch.empty(max(dpack.total_uids, 1), dtype=torch.int64,
                              device=dpack.bases.device)
        out_n = _u64()
        pk = dpack.struct()
        check(lib().ua_decode_dev(self._ctx, C.byref(pk), _u64(seek),
                                  C.c_void_p(out.data_ptr()), C.byref(out_n)))
        return out[:out_n.value]


OP_INTERSECT = 0
OP_MERGE = 1
OP_DIFFERENCE = 2

ROWS_INTERSECT = 0
ROWS_DIFFERENCE = 1


class Batch:
    """Prepared pair batch (ua_batch): run() executes one op over all pairs
    as one grid, returning per-pair output lengths."""

    def __init__(self, engine, handle, n_pairs, keepalive):
        self._eng = engine
        self._h = handle
        self.n_pairs = n_pairs
        self._keep = keepalive  # input/output tensors must outlive the batch

    def _check_caps(self, op):
        """Per-pair output capacity contract (uidalgo.h: intersect needs
        min(n,m), difference n, union n+m).  The C ABI sees raw pointers;
        this layer knows the tensor sizes, so an undersized output becomes a
        clean error instead of OOB device writes."""
        caps = getattr(self, "_caps", None)
        if caps is None:
            return
        for i, (n, m, o) in enumerate(caps):
            need = min(n, m) if op == OP_INTERSECT else (
                n if op == OP_DIFFERENCE else n + m)
            if o < need:
                raise ValueError(
                    f"pair {i}: out capacity {o} < required {need} for op {op}")

    def run(self, op=OP_INTERSECT):
        self._check_caps(op)
        lens = (C.c_uint64 * self.n_pairs)()
        check(lib().ua_batch_run(self._eng._ctx, self._h, op, lens))
        return [int(lens[i]) for i in range(self.n_pairs)]

    def run_n(self, op, n_runs):
        """n_runs passes enqueued back-to-back, ONE sync at the end (the
        repeated-query serving shape — no host round-trip between runs)."""
        self._check_caps(op)
        lens = (C.c_uint64 * self.n_pairs)()
        check(lib().ua_batch_run_n(self._eng._ctx, self._h, op, n_runs, lens))
        return [int(lens[i]) for i in range(self.n_pairs)]

    def info(self):
        """ua_batch_info: tile count, tiles that run from the 32-bit copy of
        the inputs, and that cache's device bytes (0 before the first
        intersect/difference run, and without the cache)."""
        t, nt, nb = _u64(), _u64(), _u64()
        check(lib().ua_batch_info(self._eng._ctx, self._h, C.byref(t), C.byref(nt),
                                  C.byref(nb)))
        return {"tiles": t.value, "narrow_tiles": nt.value, "narrow_bytes": nb.value}

    def fast_tiles(self):
        """ua_batch_fast_tiles: how many narrow tiles take the sentinel walk
        (0 before the first intersect/difference run, and without the cache)."""
        n = _u64()
        check(lib().ua_batch_fast_tiles(self._eng._ctx, self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            lib().ua_batch_destroy(self._eng._ctx, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass


class PackBatch:
    """Prepared pack fan-out (ua_pbatch)."""

    def __init__(self, engine, handle, n_packs, keepalive):
        self._eng = engine
        self._h = handle
        self.n_packs = n_packs
        self.outs = keepalive[2]
        self._keep = keepalive

    def run(self):
        lens = (C.c_uint64 * self.n_packs)()
        check(lib().ua_pbatch_run(self._eng._ctx, self._h, lens))
        return [int(lens[i]) for i in range(self.n_packs)]

    def close(self):
        if self._h:
            lib().ua_pbatch_destroy(self._eng._ctx, self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass


class DPack:
    """Flattened pb.UidPack resident in HBM (engine-native layout)."""

    def __init__(self, bases, num_uids, delta_offs, deltas, block_size, total_uids):
        self.bases = bases
        self.num_uids = num_uids
        self.delta_offs = delta_offs
        self.deltas = deltas
        self.block_size = block_size
        self.total_uids = total_uids

    def struct(self):
        pk = UaDPack()
        pk.block_size = self.block_size
        pk.n_blocks = self.bases.numel()
        pk.bases = self.bases.data_ptr()
        pk.num_uids = self.num_uids.data_ptr()
        pk.delta_offs = self.delta_offs.data_ptr()
        pk.deltas = self.deltas.data_ptr()
        pk.total_uids = self.total_uids
        return pk


class RowArena(DPack):
    """Engine.encode_rows' result: the flat block arena of a fan-out, as
    upload_pack_batch builds it from host packs.  The row boundaries stay on
    the device (_pbb_dev); their host copies pbb and pack_totals, which the
    row decoders size their outputs from, are fetched on first use."""

    def __init__(self, bases, num_uids, delta_offs, deltas, block_size, total_uids,
                 pbb_dev, row_offs):
        super().__init__(bases, num_uids, delta_offs, deltas, block_size, total_uids)
        self._pbb_dev = pbb_dev
        self._row_offs = row_offs
        self._pbb = self._totals = None

    @property
    def pbb(self):
        if self._pbb is None:
            self._pbb = self._pbb_dev.cpu().numpy().view(np.uint64)
        return self._pbb

    @property
    def pack_totals(self):
        if self._totals is None:
            self._totals = np.diff(self._row_offs.cpu().numpy().view(np.uint64)).tolist()
        return self._totals


# ---- host-side codec (product encoder; codec.Encode restated in C++) ----

def encode_flat(uids, block_size=256):
    """codec.Encode(uids, blockSize) -> flat arrays
    (bases u64[nb], num_uids u32[nb], delta_offs u64[nb+1], deltas u8[...])."""
    uids = _np_u64(uids)
    h = C.c_void_p()
    check(lib().ua_encode(_hptr(uids), uids.size, block_size, C.byref(h)))
    try:
        view = lib().ua_owned_pack_view(h)
        nb = _u64()
        db = _u64()
        tu = _u64()
        check(lib().ua_pack_flat_sizes(view, C.byref(nb), C.byref(db), C.byref(tu)))
        bases = np.empty(nb.value, dtype=np.uint64)
        nums = np.empty(nb.value, dtype=np.uint32)
        offs = np.empty(nb.value + 1, dtype=np.uint64)
        blob = np.empty(max(db.value, 1), dtype=np.uint8)
        check(lib().ua_pack_flatten(
            view, _hptr(bases), nums.ctypes.data_as(C.POINTER(C.c_uint32)),
            _hptr(offs), blob.ctypes.data_as(C.POINTER(C.c_uint8))))
        return bases, nums, offs, blob[:db.value], tu.value
    finally:
        lib().ua_owned_pack_free(h)


# ---- host-pointer convenience mirror (the cgo drop-in surface) ----
# These run on the GPU via upload/compute/download; they exist so the cgo shim
# maps 1:1 onto algo's signatures.

def intersect_with(engine, u, v):
    u, v = _np_u64(u), _np_u64(v)
    out = np.empty(max(min(u.size, v.size), 1), dtype=np.uint64)
    n = _u64()
    check(lib().ua_intersect(engine._ctx, _hptr(u), u.size, _hptr(v), v.size,
                             _hptr(out), C.byref(n)))
    return out[:n.value]


def difference(engine, u, v):
    u, v = _np_u64(u), _np_u64(v)
    out = np.empty(max(u.size, 1), dtype=np.uint64)
    n = _u64()
    check(lib().ua_difference(engine._ctx, _hptr(u), u.size, _hptr(v), v.size,
                              _hptr(out), C.byref(n)))
    return out[:n.value]


def update_uid_matrix(engine, rows, dest_uids, ordered=False, mode=ROWS_INTERSECT):
    """updateUidMatrix (query/query.go:1425-1437) and the worker/task.go:1352,
    1617,1692,1778 loops as ONE call (ua_rows_filter): every row filtered by
    membership in the sorted dest_uids.  rows: list of host uint64 arrays;
    returns a list of host arrays.  `ordered` only names the reference branch
    the caller is on (IntersectWith per row, or ApplyFilter+IndexOf when the
    rows are not uid-sorted): the computation is the same."""
    arrs = [_np_u64(r) for r in rows]
    n_rows = len(arrs)
    row_offs = np.zeros(n_rows + 1, dtype=np.uint64)
    if n_rows:
        row_offs[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
    vals = np.ascontiguousarray(np.concatenate(arrs), dtype=np.uint64) if n_rows else \
        np.empty(0, dtype=np.uint64)
    shared = _np_u64(dest_uids)
    out_vals = np.empty(max(vals.size, 1), dtype=np.uint64)
    out_offs = np.empty(n_rows + 1, dtype=np.uint64)
    kept = _u64()
    check(lib().ua_rows_filter(engine._ctx, _hptr(vals), _hptr(row_offs), n_rows,
                               _hptr(shared), shared.size, int(mode), _hptr(out_vals),
                               _hptr(out_offs), C.byref(kept)))
    return [out_vals[int(out_offs[r]):int(out_offs[r + 1])] for r in range(n_rows)]


def dest_uids(engine, rows):
    """DestUIDs = MergeSorted(UidMatrix) (query/query.go:1874,2290,2505,
    recurse.go:134, worker/task.go:1629,1706) as ONE call (ua_rows_union)
    over the rows' concatenation: the ascending duplicate-free set of every
    uid in the matrix.  rows: list of host uint64 arrays, sorted or not, with
    or without duplicates; returns a host array.  The counterpart of
    update_uid_matrix."""
    arrs = [_np_u64(r).ravel() for r in rows]
    vals = np.ascontiguousarray(np.concatenate(arrs), dtype=np.uint64) if arrs else \
        np.empty(0, dtype=np.uint64)
    out = np.empty(max(vals.size, 1), dtype=np.uint64)
    n = _u64()
    check(lib().ua_rows_union(engine._ctx, _hptr(vals), vals.size, _hptr(out), C.byref(n)))
    return out[:n.value]


def _host_packs(packs):
    """encode_flat tuples -> (ua_pack* array, keepalive)."""
    from dgraph_amd._lib import UaBlock, UaPack
    n = len(packs)
    structs = (UaPack * max(n, 1))()
    ptrs = (C.POINTER(UaPack) * max(n, 1))()
    keep = []
    for r, (bases, nums, offs, blob, _total) in enumerate(packs):
        nb = len(bases)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        blocks = (UaBlock * max(nb, 1))()
        for i in range(nb):
            blocks[i].base = int(bases[i])
            blocks[i].num_uids = int(nums[i])
            blocks[i].deltas_len = int(offs[i + 1]) - int(offs[i])
            blocks[i].deltas = C.cast(C.c_void_p(blob.ctypes.data + int(offs[i])),
                                      C.POINTER(C.c_uint8))
        structs[r].block_size = 0
        structs[r].n_blocks = nb
        structs[r].blocks = blocks
        ptrs[r] = C.pointer(structs[r])
        keep.append((blocks, blob))
    return ptrs, (structs, keep)


def _per_row(x, n, dtype):
    a = np.asarray(x, dtype=dtype)
    a = np.full(n, a, dtype=dtype) if a.ndim == 0 else np.ascontiguousarray(a)
    if a.size != n:
        raise ValueError(f"per-row argument needs {n} entries, got {a.size}")
    return a if n else np.zeros(1, dtype=dtype)


def _to_dev(a, dev):
    """A host array as a device tensor; u64 crosses as its int64 bits."""
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


def _per_row_dev(x, n, dtype, dev):
    """A per-row argument of an Engine call as a device tensor: None stays
    None (= all 0), one value or a sequence goes through _per_row, a CUDA
    tensor of at least n entries (int64 for u64 bits) passes as it is."""
    import torch
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        t_dt = torch.int64 if dtype is np.uint64 else torch.int32
        if x.dtype != t_dt or x.numel() < n:
            raise ValueError(f"per-row tensor needs {n} x {t_dt}")
        return x
    a = _per_row(x, n, dtype)
    return _to_dev(a, dev) if n else None


def _rows_out(n, cap):
    """Host buffers of a CSR result: cap values (one at least) and n + 1 offsets."""
    return np.empty(max(cap, 1), dtype=np.uint64), np.empty(n + 1, dtype=np.uint64)


def _split_rows(vals, offs):
    return [vals[int(offs[r]):int(offs[r + 1])] for r in range(len(offs) - 1)]


def _rows_decode_host(engine, packs, after, first, count_only):
    n = len(packs)
    ptrs, keep = _host_packs(packs)
    a = _per_row(after, n, np.uint64)
    f = _per_row(first, n, np.int32)
    cap = 0 if count_only else sum(int(p[4]) for p in packs)
    out_vals, out_offs = _rows_out(n, cap)
    total = _u64()
    check(lib().ua_rows_decode(engine._ctx, ptrs, n, _hptr(a),
                               f.ctypes.data_as(C.POINTER(C.c_int32)),
                               None if count_only else _hptr(out_vals), cap,
                               _hptr(out_offs), C.byref(total)))
    del keep
    return out_vals, out_offs


def uid_matrix(engine, packs, after=0, first=0):
    """The UidMatrix of a handleUidPostings fan-out (worker/task.go:834-971)
    on the opts.Intersect == nil branch as ONE call (ua_rows_decode): row r is
    pl.Uids of pack r (posting/list.go:1786-1902), its uids > after (0 keeps
    all), then the first `first` of them (or the last -first; 0 all).  packs:
    tuples from encode_flat; after/first: one value or one per row.  Returns
    a list of host uint64 arrays."""
    return _split_rows(*_rows_decode_host(engine, packs, after, first, False))


def row_lengths(engine, packs, after=0):
    """List.Length(readTs, afterUid) of every key (posting/list.go:1345-1363),
    what count(uid) asks for: the count-only form of uid_matrix.  Returns a
    host uint64 array of len(packs) lengths."""
    _, offs = _rows_decode_host(engine, packs, after, 0, True)
    return np.diff(offs)


MUT_SET, MUT_DEL = 1, 2  # UA_MUT_SET / UA_MUT_DEL (posting/list.go:49-53)
_EMPTY_PACK = (np.empty(0, np.uint64), np.empty(0, np.uint32), np.zeros(1, np.uint64),
               np.empty(0, np.uint8), 0)


def flatten_mutations(muts):
    """Per-row lists of (uid, op) -> (mut_uids u64, mut_ops u8, row_mut_base
    u64[n_rows + 1]), the flat form ua_rows_decode_mut takes."""
    base = np.zeros(len(muts) + 1, dtype=np.uint64)
    base[1:] = np.cumsum([len(m) for m in muts], dtype=np.uint64)
    flat = [p for m in muts for p in m]
    uids = np.array([int(u) for u, _ in flat], dtype=np.uint64)
    ops = np.array([int(o) for _, o in flat], dtype=np.uint8)
    return uids, ops, base


def _rows_decode_mut_host(engine, packs, muts, after, first, count_only):
    n = len(packs)
    if len(muts) != n:
        raise ValueError(f"muts needs {n} rows, got {len(muts)}")
    packs = [_EMPTY_PACK if p is None else p for p in packs]
    ptrs, keep = _host_packs(packs)
    uids, ops, base = flatten_mutations(muts)
    a = _per_row(after, n, np.uint64)
    f = _per_row(first, n, np.int32)
    cap = 0 if count_only else sum(int(p[4]) for p in packs) + uids.size
    out_vals, out_offs = _rows_out(n, cap)
    total = _u64()
    check(lib().ua_rows_decode_mut(
        engine._ctx, ptrs, n, _hptr(uids) if uids.size else None,
        ops.ctypes.data_as(C.POINTER(C.c_uint8)) if uids.size else None, _hptr(base),
        _hptr(a), f.ctypes.data_as(C.POINTER(C.c_int32)),
        None if count_only else _hptr(out_vals), cap, _hptr(out_offs), C.byref(total)))
    del keep
    return out_vals, out_offs


def uid_matrix_mut(engine, packs, muts, after=0, first=0):
    """uid_matrix over LIVE lists (ua_rows_decode_mut): row r is pl.Uids of a
    list with a mutable layer, List.iterate's merge (posting/list.go:1135-1251)
    of pack r (a tuple from encode_flat, or None for a list without blocks)
    with muts[r], a list of (uid, op) strictly ascending by uid: MUT_DEL
    removes the uid, any other op sets it.  Then uids > after (0 keeps all),
    then first, as in uid_matrix.  Returns a list of host uint64 arrays."""
    return _split_rows(*_rows_decode_mut_host(engine, packs, muts, after, first, False))


def row_lengths_mut(engine, packs, muts, after=0):
    """List.Length(readTs, afterUid) of every key on lists with a mutable
    layer (posting/list.go:1345-1363): the count-only form of uid_matrix_mut.
    Returns a host uint64 array of len(packs) lengths."""
    _, offs = _rows_decode_mut_host(engine, packs, muts, after, 0, True)
    return np.diff(offs)


def encode_rows(engine, rows, block_size=256):
    """codec.Encode of every list of a population as ONE call (ua_rows_encode):
    the per-key encoders of List.encode (posting/list.go:1609-1664) and of the
    bulk reducer (dgraph/cmd/bulk/reduce.go:811-861).  rows: sequences of
    strictly ascending uids.  Returns one encode_flat-shaped tuple per row."""
    n = len(rows)
    rows = [_np_u64(r).ravel() for r in rows]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([r.size for r in rows], dtype=np.uint64)
    vals = np.ascontiguousarray(np.concatenate(rows)) if n else np.empty(0, np.uint64)
    rbb = np.empty(n + 1, dtype=np.uint64)
    nb, db = _u64(), _u64()
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    check(lib().ua_rows_encode(engine._ctx, _hptr(vals), _hptr(offs), n, block_size, None,
                               None, None, 0, None, 0, _hptr(rbb), C.byref(nb), C.byref(db)))
    k = nb.value
    bases = np.empty(max(k, 1), dtype=np.uint64)
    nums = np.empty(max(k, 1), dtype=np.uint32)
    doffs = np.empty(k + 1, dtype=np.uint64)
    blob = np.empty(max(db.value, 1), dtype=np.uint8)
    check(lib().ua_rows_encode(engine._ctx, _hptr(vals), _hptr(offs), n, block_size,
                               _hptr(bases), nums.ctypes.data_as(u32p), _hptr(doffs), k,
                               blob.ctypes.data_as(u8p), db.value, _hptr(rbb), C.byref(nb),
                               C.byref(db)))
    out = []
    for r in range(n):
        b0, b1 = int(rbb[r]), int(rbb[r + 1])
        y0, y1 = int(doffs[b0]), int(doffs[b1])
        out.append((bases[b0:b1], nums[b0:b1], doffs[b0:b1 + 1] - np.uint64(y0),
                    blob[y0:y1], int(rows[r].size)))
    return out


def sort_uid_matrix(engine, rows, keys, count=0, offset=0, desc=False, multi=False,
                    drop_nulls=False, want_src=False):
    """sortWithoutIndex (worker/sort.go:139-187) or, with drop_nulls,
    sortAndPaginateUsingVar (query/query.go:2697-2738) over a whole UID matrix
    as ONE call (ua_rows_sort).  rows: sequences of uids; keys: one parallel
    sequence per row of order-preserving u64 keys, a None entry meaning the
    uid has no value.  Returns (rows, ms_offs): the ordered, paginated rows and
    the multiSortOffsets ([] unless multi); with want_src also each row's flat
    input indices, as a third item."""
    from dgraph_amd._lib import UA_SORT_DESC, UA_SORT_DROP_NULLS, UA_SORT_MULTI
    n = len(rows)
    rows = [_np_u64(r).ravel() for r in rows]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([r.size for r in rows], dtype=np.uint64)
    total = int(offs[n])
    vals = np.ascontiguousarray(np.concatenate(rows)) if n else np.empty(0, np.uint64)
    kk = has = None
    if keys is not None:
        if len(keys) != n or any(len(k) != r.size for k, r in zip(keys, rows)):
            raise ValueError("keys must be parallel to rows")
        flat = [x for k in keys for x in k]
        has = np.array([x is not None for x in flat], dtype=np.uint8)
        kk = np.array([0 if x is None else int(x) for x in flat], dtype=np.uint64)
    flags = ((UA_SORT_DESC if desc else 0) | (UA_SORT_MULTI if multi else 0) |
             (UA_SORT_DROP_NULLS if drop_nulls else 0))
    out = np.empty(max(total, 1), dtype=np.uint64)
    src = np.empty(max(total, 1), dtype=np.uint64) if want_src else None
    ooffs = np.empty(n + 1, dtype=np.uint64)
    ms = np.zeros(max(n, 1), dtype=np.int32) if multi else None
    need = _u64()
    check(lib().ua_rows_sort(
        engine._ctx, _hptr(vals), _hptr(offs), n,
        _hptr(kk) if kk is not None else None,
        (has if has.size else np.zeros(1, np.uint8)).ctypes.data_as(C.POINTER(C.c_uint8))
        if has is not None else None,
        flags, int(count), int(offset), _hptr(out), total, _hptr(ooffs),
        _hptr(src) if want_src else None,
        ms.ctypes.data_as(C.POINTER(C.c_int32)) if multi else None, C.byref(need)))
    res = (_split_rows(out, ooffs), [int(x) for x in ms[:n]] if multi else [])
    if want_src:
        res += (_split_rows(src, ooffs),)
    return res


def paginate_uid_matrix(engine, rows, count, offset):
    """applyPagination (query/query.go:2493-2507): x.PageRange(count, offset)
    of every row as ONE call (ua_rows_sort without keys).  Returns the rows."""
    return sort_uid_matrix(engine, rows, None, count=count, offset=offset)[0]


def transpose_uid_matrix(engine, rows, src_uids=None, keep=None, unique=False,
                         want_src=False):
    """The transpose of a UID matrix as ONE call (ua_rows_transpose): what
    dedup.addValue (query/groupby.go:104-128) collects per edge and
    rebuildReverseEdges (posting/index.go:1759-1791) adds per posting.  rows:
    sequences of uids; src_uids: the rows' uids (None = the row index); keep:
    one truth value per row (None = all).  Returns (keys, groups): the distinct
    values ascending and, per key, the uids of the rows that hold it in input
    order (one per (value, row) with unique); with want_src also each group's
    flat input indices, as a third item."""
    from dgraph_amd._lib import UA_TR_UNIQUE
    n = len(rows)
    rows = [_np_u64(r).ravel() for r in rows]
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([r.size for r in rows], dtype=np.uint64)
    total = int(offs[n])
    vals = np.ascontiguousarray(np.concatenate(rows)) if n else np.empty(0, np.uint64)
    ru = kp = None
    if src_uids is not None:
        ru = _np_u64(src_uids).ravel()
        if ru.size != n:
            raise ValueError("src_uids needs one uid per row")
    if keep is not None:
        kp = np.ascontiguousarray(np.asarray(keep, dtype=bool).ravel().astype(np.uint8))
        if kp.size != n:
            raise ValueError("keep needs one entry per row")
    keys = np.empty(max(total, 1), dtype=np.uint64)
    goffs = np.empty(total + 1, dtype=np.uint64)
    out = np.empty(max(total, 1), dtype=np.uint64)
    src = np.empty(max(total, 1), dtype=np.uint64) if want_src else None
    ng, nt = _u64(), _u64()
    check(lib().ua_rows_transpose(
        engine._ctx, _hptr(vals), _hptr(offs), n,
        _hptr(ru) if ru is not None and n else None,
        kp.ctypes.data_as(C.POINTER(C.c_uint8)) if kp is not None and n else None,
        UA_TR_UNIQUE if unique else 0, _hptr(keys), _hptr(goffs), total, _hptr(out),
        _hptr(src) if want_src else None, total, C.byref(ng), C.byref(nt)))
    k = ng.value
    res = (keys[:k].copy(), _split_rows(out, goffs[:k + 1]))
    if want_src:
        res += (_split_rows(src, goffs[:k + 1]),)
    return res


def group_by_uid(engine, rows, src_uids, keep=None):
    """groupby over one uid predicate (formResult, query/groupby.go:195-260):
    rows[i] is the child's UidMatrix row of src_uids[i], keep[i] whether
    src_uids[i] is in the parent's list (the `IndexOf(ul, srcUid) < 0`
    test).  Returns [(dst, [src...])...] with dst ascending, the groups
    formGroups consumes at depth 1; count(uid) of a group is its length."""
    keys, groups = transpose_uid_matrix(engine, rows, src_uids, keep)
    return [(int(k), [int(x) for x in g]) for k, g in zip(keys, groups)]


def rollup_rows(engine, packs, muts, block_size=256):
    """A batched rollup of REF-only lists: List.encode over List.iterate
    (posting/list.go:1609-1664) per list, i.e. uid_matrix_mut with after =
    first = 0, then encode_rows.  Returns one encode_flat-shaped tuple per
    row."""
    return encode_rows(engine, uid_matrix_mut(engine, packs, muts), block_size)


def uid_matrix_intersect(engine, packs, shared, after=0):
    """The UidMatrix of a handleUidPostings fan-out on the opts.Intersect !=
    nil branch as ONE call (ua_rows_intersect_packed): row r is
    algo.IntersectCompressedWith(pack r, after, shared) (posting/list.go:
    1823-1829, uidlist.go:33), the pack's uids with x >= after (inclusive)
    that occur in shared; no first is applied on this branch.  packs: tuples
    from encode_flat; shared: sorted duplicate-free host uint64 array; after:
    one value or one per row.  Returns a list of host uint64 arrays."""
    n = len(packs)
    ptrs, keep = _host_packs(packs)
    a = _per_row(after, n, np.uint64)
    sh = np.ascontiguousarray(_np_u64(shared).ravel())
    cap = sum(min(int(p[4]), sh.size) for p in packs)
    out_vals, offs = _rows_out(n, cap)
    total = _u64()
    check(lib().ua_rows_intersect_packed(engine._ctx, ptrs, n, _hptr(a),
                                         _hptr(sh), sh.size,
                                         _hptr(out_vals), cap, _hptr(offs),
                                         C.byref(total)))
    del keep
    return _split_rows(out_vals, offs)


def update_dest_uids(engine, rows, dest):
    """updateDestUids (query/query.go:2594-2609), the ordered-query fallback
    for rows that are not uid-sorted ("Can't use merge sort if the UIDs are
    not sorted", recurse.go:131): keep the uids of dest that occur anywhere in
    the matrix, in dest's order.  The reference marks IndexOf(dest, uid) per
    element and compacts; for the sorted duplicate-free dest it always holds
    that is dest ∩ union(rows): one ua_rows_union plus one pair intersect.
    rows: list of host uint64 arrays; dest: host uint64 array; returns a host
    array."""
    return intersect_with(engine, dest, dest_uids(engine, rows))


def _host_lists(lists):
    arrs = [_np_u64(x) for x in lists]
    k = len(arrs)
    ptrs = (_u64p * max(k, 1))(*[_hptr(a) for a in arrs])
    lens = (_u64 * max(k, 1))(*[a.size for a in arrs])
    return arrs, ptrs, lens, k


def intersect_sorted(engine, lists):
    arrs, ptrs, lens, k = _host_lists(lists)
    cap = min((a.size for a in arrs), default=0)
    out = np.empty(max(cap, 1), dtype=np.uint64)
    n = _u64()
    check(lib().ua_intersect_k(engine._ctx, ptrs, lens, k, _hptr(out), C.byref(n)))
    return out[:n.value]


def merge_sorted(engine, lists):
    arrs, ptrs, lens, k = _host_lists(lists)
    cap = sum(a.size for a in arrs)
    out = np.empty(max(cap, 1), dtype=np.uint64)
    n = _u64()
    check(lib().ua_merge_k(engine._ctx, ptrs, lens, k, _hptr(out), C.byref(n)))
    return out[:n.value]


def index_of(u, uid):
    """algo.IndexOf — host binary search, like the reference (uidlist.go:546)."""
    u = _np_u64(u)
    return int(lib().ua_index_of(_hptr(u), u.size, _u64(uid)))


def apply_filter(u, mask, engine=None):
    """algo.ApplyFilter (uidlist.go:21): boolean-mask compaction.

    The reference takes a Go closure; across a C ABI the filter arrives as a
    precomputed mask (the callers evaluate per-uid predicates upstream).
    With an Engine, host arrays go through the ua_apply_filter C-ABI export
    (in-place device compaction — the cgo drop-in path); CUDA tensors go
    through the batched device export."""
    import torch
    if isinstance(u, torch.Tensor):
        if engine is not None and u.is_cuda:
            m = mask if isinstance(mask, torch.Tensor) else \
                torch.as_tensor(np.asarray(mask, dtype=np.uint8), device=u.device)
            out = torch.empty_like(u)
            outs, lens = engine.apply_filter_batch([u], [m], [out])
            return out[:lens[0]]
        return u[mask]
    u = np.ascontiguousarray(_np_u64(u))
    m = np.ascontiguousarray(np.asarray(mask, dtype=bool).view(np.uint8))
    if engine is not None:
        from dgraph_amd._lib import _u8p
        n = _u64()
        check(lib().ua_apply_filter(engine._ctx, _hptr(u), u.size,
                                    m.ctypes.data_as(_u8p), C.byref(n)))
        return u[:n.value]
    return u[m.view(bool)]
