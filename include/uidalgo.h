/*
 * uidalgo — C-ABI boundary of the MI355X-native posting-list set-algebra
 * engine (libuidalgo.so).
 *
 * This is the drop-in surface for dgraph's `algo` package (reference
 * interfaces each export replaces are cited below; see INTEGRATION.md for the
 * cgo binding a dgraph maintainer would add).  All memory is caller-owned,
 * errors are int status codes, a ua_ctx wraps one GPU + one HIP stream and is
 * callable from any thread (calls on one ctx are serialized by its stream).
 *
 * Two levels:
 *  - host-pointer convenience calls that mirror algo's signatures 1:1
 *    (upload + compute + download; PCIe-inclusive), and
 *  - device-resident batched calls (`*_dev`), the batched engine that a
 *    worker/task.go:834-971 fan-out would feed: one grid per
 *    SubGraph's thousands of per-key list ops.
 *
 * No torch types, no C++ types: plain pointers and sizes only.
 */
#ifndef UIDALGO_H
#define UIDALGO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---- */
enum {
    UA_OK = 0,
    UA_ERR_HIP = 1,      /* HIP runtime error (see ua_last_hip_error) */
    UA_ERR_NOMEM = 2,    /* allocation failed */
    UA_ERR_INVALID = 3,  /* bad argument (e.g. block with num_uids > 256) */
    UA_ERR_NO_GPU = 4,   /* no HIP device visible */
};

const char *ua_strerror(int code);
int ua_version(void);

/* ---- context ---- */
typedef struct ua_ctx ua_ctx;
int ua_ctx_create(ua_ctx **out, int device);
void ua_ctx_destroy(ua_ctx *ctx);

/* ---- device memory (for callers without their own allocator) ---- */
int ua_dev_alloc(ua_ctx *, uint64_t bytes, void **dptr);
int ua_dev_free(ua_ctx *, void *dptr);
int ua_h2d(ua_ctx *, void *dst_dev, const void *src_host, uint64_t bytes);
int ua_d2h(ua_ctx *, void *dst_host, const void *src_dev, uint64_t bytes);
int ua_sync(ua_ctx *);

/* ---- engine stats (HIP-event timing of the dominant kernels, for the
 * roofline leg of bench.py: kernel_ms is accumulated on the engine's own
 * stream across launches since the last reset) ---- */
int ua_stats_reset(ua_ctx *);
int ua_stats_get(ua_ctx *, uint64_t *n_launches, double *kernel_ms,
                 uint64_t *bytes_algorithmic);

/* ---- pb.UidPack mirror (pb.proto:379-400) ---- */
typedef struct {
    uint64_t base;          /* pb.UidBlock.base */
    uint32_t num_uids;      /* pb.UidBlock.num_uids (includes base) */
    uint32_t deltas_len;
    const uint8_t *deltas;  /* group-varint deltas */
} ua_block;

typedef struct {
    uint32_t block_size;    /* pb.UidPack.block_size */
    uint64_t n_blocks;
    const ua_block *blocks;
} ua_pack;

/* Flattened pack in device memory — the engine's native layout. */
typedef struct {
    uint32_t block_size;
    uint64_t n_blocks;
    const uint64_t *bases;      /* device [n_blocks] */
    const uint32_t *num_uids;   /* device [n_blocks] */
    const uint64_t *delta_offs; /* device [n_blocks+1], offsets into deltas */
    const uint8_t *deltas;      /* device blob */
    uint64_t total_uids;        /* codec.ExactLen */
} ua_dpack;

/* ---- host-side codec (replaces codec.Encode, codec.go:393) ---- */
typedef struct ua_owned_pack ua_owned_pack;
int ua_encode(const uint64_t *uids, uint64_t n, uint32_t block_size,
              ua_owned_pack **out);
const ua_pack *ua_owned_pack_view(ua_owned_pack *);
void ua_owned_pack_free(ua_owned_pack *);

uint64_t ua_pack_exact_len(const ua_pack *);  /* codec.ExactLen  codec.go:427 */
uint64_t ua_pack_approx_len(const ua_pack *); /* codec.ApproxLen codec.go:418 */

/* Flatten a host pack into the engine layout (arrays caller-allocated:
 * bases[n_blocks], num_uids[n_blocks], delta_offs[n_blocks+1],
 * deltas_blob[total deltas bytes]).  Query sizes first. */
int ua_pack_flat_sizes(const ua_pack *, uint64_t *n_blocks,
                       uint64_t *deltas_bytes, uint64_t *total_uids);
int ua_pack_flatten(const ua_pack *, uint64_t *bases, uint32_t *num_uids,
                    uint64_t *delta_offs, uint8_t *deltas_blob);

/* Decode a pack on the GPU (replaces codec.Decode, codec.go:444).
 * out: device buffer, capacity total_uids. */
int ua_decode_dev(ua_ctx *, const ua_dpack *, uint64_t seek_uid,
                  uint64_t *out, uint64_t *out_n);

/* GPU codec.Encode (codec.go:393): uids (device, sorted) -> flattened pack
 * arrays (device, caller-allocated worst case: bases/num_uids/delta_offs for
 * max_blocks = n blocks (+1 for delta_offs), deltas capacity >= 6*n + 24
 * bytes).  Byte-identical to the host encoder / reference format.
 * block_size <= 256 (the engine's block bound); 0 packs per-uid blocks like
 * the reference. */
int ua_encode_dev(ua_ctx *, const uint64_t *uids, uint64_t n,
                  uint32_t block_size, uint64_t *bases, uint32_t *num_uids,
                  uint64_t *delta_offs, uint8_t *deltas,
                  uint64_t *n_blocks_out, uint64_t *deltas_bytes_out);

/* ---- batched device-resident set algebra ----
 * All pointers in ua_dpair are DEVICE pointers; the descriptor array itself
 * and out_lens live on the host.  Inputs are sorted uint64 lists; results are
 * bit-exact vs the reference on duplicate-free inputs (the parity domain
 * pinned by uidlist_test.go:394,536-542 — see DESIGN.md §semantics).
 * On inputs that violate the contract (duplicates / unsorted), results are
 * unspecified — like the reference's bin variants — but all writes stay
 * within each pair's out capacity (the engine clamps; the reference is
 * memory-safe on such inputs and so is this ABI). */
typedef struct {
    const uint64_t *u; /* device */
    uint64_t n;
    const uint64_t *v; /* device */
    uint64_t m;
    uint64_t *out;     /* device; capacity: intersect >= min(n,m),
                        *                   merge >= n+m, difference >= n */
} ua_dpair;

/* batched algo.IntersectWith (uidlist.go:142) */
int ua_intersect_batch_dev(ua_ctx *, const ua_dpair *pairs, int n_pairs,
                           uint64_t *out_lens);

/* Prepared batch (the repeated-query path): descriptor upload and the
 * merge-path tile partition are done ONCE at create; each run is launches
 * only, and the FIRST run additionally caches the per-thread merge-path
 * splits (4 B per tile-thread = 1 KiB per 2048-element tile, device; one
 * cache serves all three ops) that every later run loads instead of
 * re-searching.  A batch that runs intersect or difference builds a THIRD
 * cache ahead of its first such run: a 32-bit tile-major copy of its inputs
 * (one 8208-byte record per tile, about 4 B per input element, device).
 * Tiles whose elements all share their upper 32 bits (decided from the
 * data, per tile) are then filled and walked from that copy at half the
 * bytes; every other tile, and union, reads the lists as before.  The
 * allocation is tried once; if it fails, or with UA_NARROW=0 in the
 * environment, the batch runs without it.  ua_batch_info reports it.
 * All three caches rest on the same promise: the pairs' device contents must
 * not change between create and the runs (violating this gives unspecified
 * results but stays memory-safe); out capacities must fit the
 * op (intersect >= min(n,m), merge >= n+m, difference >= n). */
typedef struct ua_batch ua_batch;
enum { UA_OP_INTERSECT = 0, UA_OP_MERGE = 1, UA_OP_DIFFERENCE = 2 };
int ua_batch_create(ua_ctx *, const ua_dpair *pairs, int n_pairs, ua_batch **out);
int ua_batch_run(ua_ctx *, ua_batch *, int op, uint64_t *out_lens);
/* n_runs passes enqueued back-to-back with ONE sync (the repeated-query
 * serving shape); out_lens are the final pass's lengths (all passes over an
 * immutable batch produce identical results). */
int ua_batch_run_n(ua_ctx *, ua_batch *, int op, int n_runs,
                   uint64_t *out_lens);
void ua_batch_destroy(ua_ctx *, ua_batch *);
/* What the batch holds (any out pointer may be NULL): its tile count, how
 * many of the tiles run from the 32-bit copy, and that cache's device bytes.
 * Both are 0 until the first intersect/difference run has built the cache,
 * and stay 0 when it is disabled or could not be allocated.  (since v13) */
int ua_batch_info(ua_ctx *, ua_batch *, uint64_t *tiles, uint64_t *narrow_tiles,
                  uint64_t *narrow_bytes);
/* How many of the narrow tiles take the sentinel-terminated walk: full tiles
 * (2048 merge-path elements) none of whose low halves is 0xFFFFFFFF, each
 * range of whose record is closed by a sentinel, so that the walk tests no
 * range.  Every other narrow tile keeps the guarded walk; results do not
 * depend on which one a tile takes.  Counted on demand from the records; 0
 * until the 32-bit copy exists, and when it is disabled.  (since v15) */
int ua_batch_fast_tiles(ua_ctx *, ua_batch *, uint64_t *n);
/* batched pairwise algo.MergeSorted semantics (dedup union, uidlist.go:448) */
int ua_merge_batch_dev(ua_ctx *, const ua_dpair *pairs, int n_pairs,
                       uint64_t *out_lens);
/* batched algo.Difference (uidlist.go:332) */
int ua_difference_batch_dev(ua_ctx *, const ua_dpair *pairs, int n_pairs,
                            uint64_t *out_lens);

/* batched duplicate-KEEPING merge of sorted runs (no dedup, unlike
 * MergeSorted): out capacity exactly n+m; out_lens[i] = n+m.  The building
 * block of the segmented sort. */
int ua_merge_all_batch_dev(ua_ctx *, const ua_dpair *pairs, int n_pairs,
                           uint64_t *out_lens);

/* Batched segmented sort, u64 ascending, duplicates kept, in place.
 * tmp: device scratch with capacity n per segment.  The engine primitive
 * behind the sort path's UidMatrix shapes (worker/sort.go:48,139,189 —
 * SURVEY.md §8f row 3) and for unsorted ingest ahead of Encode. */
typedef struct {
    uint64_t *data; /* device, n elements; sorted ascending on return */
    uint64_t n;
    uint64_t *tmp;  /* device scratch, capacity n */
} ua_dseg;
int ua_sort_segments_dev(ua_ctx *, const ua_dseg *segs, int n_segs);

/* k-way fold algo.IntersectSorted (uidlist.go:297): lists/lens host arrays of
 * device pointers; out device, capacity min(lens). */
int ua_intersect_k_dev(ua_ctx *, const uint64_t *const *lists,
                       const uint64_t *lens, int k, uint64_t *out,
                       uint64_t *out_n);
/* k-way algo.MergeSorted (uidlist.go:448): pairwise tree on device.
 * out device, capacity sum(lens). */
int ua_merge_k_dev(ua_ctx *, const uint64_t *const *lists,
                   const uint64_t *lens, int k, uint64_t *out,
                   uint64_t *out_n);

/* batched algo.IndexOf (uidlist.go:546): queries/out device. */
int ua_index_of_batch_dev(ua_ctx *, const uint64_t *u, uint64_t n,
                          const uint64_t *queries, uint64_t nq, int64_t *out);

/* batched algo.ApplyFilter (uidlist.go:21; callers worker/task.go:1403,
 * query/query.go:1431): order-preserving mask compaction.  The reference
 * takes a Go closure f(uid, i); across the C-ABI the filter arrives as a
 * precomputed per-element byte mask (callers evaluate per-uid predicates
 * upstream).  out may equal u (in-place, the reference's shape). */
typedef struct {
    const uint64_t *u;    /* device */
    uint64_t n;
    const uint8_t *mask;  /* device, n bytes; nonzero = keep */
    uint64_t *out;        /* device, capacity >= n; may alias u */
} ua_dfilter;
int ua_apply_filter_batch_dev(ua_ctx *, const ua_dfilter *tasks, int n_tasks,
                              uint64_t *out_lens);

/* Row-wise UID-matrix filter against ONE shared sorted list — the "N rows x
 * one list" shape of the query path: query/query.go:1425-1437
 * updateUidMatrix (IntersectWith(row, DestUIDs, row) per row, or, for ordered
 * queries whose rows are not uid-sorted, ApplyFilter(row, IndexOf(DestUIDs,
 * uid) >= 0)) and worker/task.go:1352,1617,1692,1778
 * (IntersectWith(UidMatrix[i], filtered, UidMatrix[i]) per row).
 *
 * The matrix is in CSR form: vals[total] are the rows concatenated,
 * row_offs[n_rows+1] is non-decreasing with row_offs[0] = 0 and
 * row_offs[n_rows] = total.  Per row r, order preserved:
 *   UA_ROWS_INTERSECT:  out row r = [x for x in row r if x in shared]
 *   UA_ROWS_DIFFERENCE: out row r = [x for x in row r if x not in shared]
 * Output rows are packed: out_vals[0 .. *out_total) is a valid CSR body for
 * out_row_offs.  This is a per-element membership filter, so rows NEED NOT be
 * sorted and MAY hold duplicates: it always equals the ApplyFilter+IndexOf
 * form, and equals algo.IntersectWith / algo.Difference on the parity domain
 * (duplicate-free sorted rows).  shared must be sorted ascending; if it is
 * not, the result is unspecified but all accesses stay in bounds.
 *
 * out_vals must not overlap vals and out_row_offs must not overlap row_offs:
 * a packed flat compaction cannot run in place (one workgroup's writes land
 * in another's input range), so overlapping ranges are rejected with
 * UA_ERR_INVALID — callers ping-pong two buffers.  A row_offs that violates
 * the contract gives unspecified offsets but no out-of-bounds access (every
 * offset is clamped to total; vals is only indexed through [0, total)).
 * n_rows == 0 (then total must be 0), total == 0 and m == 0 are valid; with
 * m == 0 intersect yields all-empty rows and difference copies the input.
 * total < 2^42 (the tile count is 32-bit), else UA_ERR_INVALID.  One stream
 * sync per call; *out_total is the kept total, == out_row_offs[n_rows]. */
enum { UA_ROWS_INTERSECT = 0, UA_ROWS_DIFFERENCE = 1 };
typedef struct {
    const uint64_t *vals;      /* device, total */
    const uint64_t *row_offs;  /* device, n_rows+1 */
    uint64_t n_rows, total;
    const uint64_t *shared;    /* device, sorted, m */
    uint64_t m;
    uint64_t *out_vals;        /* device, capacity total; no overlap with vals */
    uint64_t *out_row_offs;    /* device, n_rows+1; no overlap with row_offs */
} ua_drows;
int ua_rows_filter_dev(ua_ctx *, const ua_drows *, int mode, uint64_t *out_total);

/* DestUIDs of a CSR UID matrix — algo.MergeSorted(UidMatrix) as the query
 * path calls it: query/query.go:1874, 2290, 2505, query/recurse.go:134,
 * worker/task.go:1629, 1706, worker/trigram.go:87, worker/match.go:100 — and,
 * for ordered queries whose rows are not uid-sorted, the set the reference's
 * updateDestUids fallback (query/query.go:2594-2609) filters DestUIDs by.
 *
 * out[0 .. *out_n) is the ascending duplicate-free set of the values in
 * vals[0 .. total), the matrix's rows concatenated.  As a set DestUIDs does
 * not depend on the row boundaries, so row_offs is NOT an argument: only
 * total = row_offs[n_rows] matters.  The call is defined for ANY order and
 * ANY duplicates in vals; whenever every row is sorted it equals
 * algo.MergeSorted(rows), rows with duplicates included (MergeSorted
 * collapses those too, uidlist.go:417).  0 and UINT64_MAX are ordinary
 * values; all comparisons are unsigned 64-bit.
 *
 * The flat array is cut into ceil(total / 2048) tiles, each sorted and
 * deduplicated by one workgroup, and the tiles are united by the pairwise
 * tree of ua_merge_k_dev: the work does not depend on the row lengths.
 * out may be vals EXACTLY (vals is consumed before out is written); any
 * other overlap of the two ranges is rejected with UA_ERR_INVALID.
 * total == 0 is valid (*out_n = 0, no launch).  A null ctx, a null out_n, or
 * a null vals/out with total > 0 give UA_ERR_INVALID.  The tile count must
 * fit the tree's int item counts: total <= (2^31 - 1) * 2048, else
 * UA_ERR_INVALID.  Engine scratch: 2 * total u64. */
int ua_rows_union_dev(ua_ctx *, const uint64_t *vals /* device */, uint64_t total,
                      uint64_t *out /* device, capacity total */, uint64_t *out_n);

/* The UID matrix of a per-key fan-out, decoded in ONE call: packs in, CSR
 * matrix out, one stream sync (since v14).  This is handleUidPostings
 * (worker/task.go:834-971) on its ordinary branch, opts.Intersect == nil: one
 * pl.Uids(opts) per key (posting/list.go:1786-1902), each result one row of
 * UidMatrix.  The count-only form (out_vals NULL, cap_vals 0) gives every
 * key's List.Length(readTs, afterUid) (posting/list.go:1345-1363), what
 * count(uid) asks for.  The output is directly the input of
 * ua_rows_filter_dev / ua_rows_union_dev.
 *
 * All rows' packs sit in one flat block arena, as in
 * ua_intersect_packed_batch_dev; row r owns blocks
 * [row_block_base[r], row_block_base[r+1]).  Unlike that call's boundaries,
 * row_block_base is a DEVICE array: nothing per row crosses to the host.
 *
 * SEMANTICS ARE List.Uids', NOT ua_ptask.after_uid's AND NOT ua_decode_dev's
 * seek.  Per row r, in this order:
 *   1. the decoded uids of the row's blocks, in order, restricted to
 *      x > after[r] — STRICTLY greater.  after[r] == 0 keeps everything, uid 0
 *      included (codec.go:284, list.go:1797); UINT64_MAX gives an empty row.
 *      (ua_decode_dev's seek keeps x >= seek.)
 *   2. ListOptions.First (list.go:1892-1900) over what step 1 kept:
 *      first[r] > 0 keeps the first first[r] of them, first[r] < 0 the last
 *      -first[r], first[r] == 0 all.  INT32_MIN is legal (negated in 64 bits).
 * after == NULL means all 0, first == NULL all 0.
 *
 * Capacity: *out_total is always the REQUIRED total and out_row_offs is always
 * complete (out_row_offs[n_rows] == *out_total), whatever cap_vals is.  Every
 * store into out_vals is bounded by cap_vals.  If *out_total > cap_vals and
 * out_vals is not NULL the call returns UA_ERR_INVALID; out_vals is then
 * unspecified but untouched past cap_vals: retry with the reported size, or
 * size the buffer from a count-only call first.
 *
 * Rejected with UA_ERR_INVALID before the context is touched, nothing
 * written: a null ctx, desc, out_total or out_row_offs; null pack arrays with
 * n_blocks > 0; a null row_block_base with n_rows > 0; a null out_vals with
 * cap_vals > 0; n_rows == 0 with n_blocks != 0; n_blocks > 2^24 - 1 (so the
 * uids of one call number below 2^32 and every count fits the engine's u32
 * scan); out_row_offs overlapping row_block_base; out_vals overlapping
 * out_row_offs or any input (deltas is checked at its first byte: its length
 * lives on the device).  n_rows == 0 and n_blocks == 0 are valid.
 *
 * Pack limits as everywhere: num_uids <= 256 and <= 1092 delta bytes per
 * block, else UA_ERR_INVALID and *out_total = 0.
 *
 * Memory safety does not depend on the data: a row_block_base that is not
 * non-decreasing from 0 to n_blocks, unsorted bases or garbage delta bytes
 * give unspecified rows and offsets, never an out-of-range access (every
 * index read from the device is clamped; delta_offs[n_blocks] is taken as the
 * blob's length). */
typedef struct {
    /* flat block arena of all rows' packs */
    const uint64_t *bases;          /* device [n_blocks] */
    const uint32_t *num_uids;       /* device [n_blocks] */
    const uint64_t *delta_offs;     /* device [n_blocks+1] */
    const uint8_t *deltas;          /* device blob */
    uint64_t n_blocks;
    const uint64_t *row_block_base; /* DEVICE [n_rows+1], non-decreasing,
                                     * [0] = 0, [n_rows] = n_blocks */
    uint64_t n_rows;
    const uint64_t *after;          /* device [n_rows] or NULL (= all 0) */
    const int32_t *first;           /* device [n_rows] or NULL (= all 0) */
    uint64_t *out_vals;             /* device, capacity cap_vals; NULL with
                                     * cap_vals == 0 = count only */
    uint64_t cap_vals;
    uint64_t *out_row_offs;         /* device [n_rows+1] */
} ua_drowpacks;
int ua_rows_decode_dev(ua_ctx *, const ua_drowpacks *, uint64_t *out_total);

/* The UID matrix of a per-key fan-out under a filter list, in ONE call: packs
 * and one shared sorted list in, CSR matrix out, one stream sync (since v16).
 * This is handleUidPostings (worker/task.go:834-971) on its hot branch,
 * opts.Intersect != nil: on an immutable pack pl.Uids(opts) is
 * algo.IntersectCompressedWith(pack, opts.AfterUid, opts.Intersect)
 * (posting/list.go:1823-1829, algo/uidlist.go:33), and every key of the
 * fan-out gets the same q.UidList.  The count-only form (out_vals NULL,
 * cap_vals 0) gives every key's count(uid) under the filter.  Input layout as
 * ua_rows_decode_dev: one flat block arena, row r owns blocks
 * [row_block_base[r], row_block_base[r+1]), row_block_base a DEVICE array.
 * The output is directly the input of ua_rows_filter_dev / ua_rows_union_dev.
 *
 * SEMANTICS.  Row r is the decoded uids of the row's blocks, in order, with
 *      x >= after[r]   and   x in shared.
 *  - after is INCLUSIVE: IntersectCompressedWith does dec.Seek(afterUID,
 *    SeekStart) (codec.go:279-329).  This is ua_ptask.after_uid's meaning and
 *    is NOT ua_rows_decode_dev's x > after.  after[r] == 0 keeps everything;
 *    after[r] == UINT64_MAX keeps UINT64_MAX if it is in both; after == NULL
 *    means all 0.
 *  - There is NO first.  On this branch getUidList returns
 *    applyIntersectWith == false and Uids returns before list.go:1892: the
 *    reference applies no ListOptions.First here.
 *  - shared holds m uids, sorted ascending and duplicate-free; 0 and
 *    UINT64_MAX are ordinary values.  m == 0 is valid: every row is empty.
 *    If shared is not sorted and duplicate-free the rows are unspecified, but
 *    every access stays in bounds and out_vals receives exactly what
 *    out_row_offs counts.
 *
 * Capacity, count-only and the pack limits are exactly ua_rows_decode_dev's:
 * *out_total is always the REQUIRED total and out_row_offs is always complete,
 * whatever cap_vals is; every store into out_vals is bounded by cap_vals; if
 * *out_total > cap_vals and out_vals is not NULL the call returns
 * UA_ERR_INVALID with out_vals unspecified but untouched past cap_vals.  A
 * block with num_uids > 256 or more than 1092 delta bytes gives
 * UA_ERR_INVALID and *out_total = 0 (not looked for when n_blocks == 0 or
 * m == 0: that call reads no pack).
 *
 * Rejected with UA_ERR_INVALID before the context is touched, nothing
 * written: a null ctx, desc, out_total or out_row_offs; null pack arrays with
 * n_blocks > 0; a null row_block_base with n_rows > 0; a null shared with
 * m > 0; a null out_vals with cap_vals > 0; a non-null reserved; n_rows == 0
 * with n_blocks != 0;
 * n_blocks > 2^24 - 1; m >= 2^61; out_vals overlapping out_row_offs;
 * out_vals or out_row_offs overlapping any input, shared and after included
 * (deltas is checked at its first byte).
 *
 * Memory safety does not depend on the data, as for ua_rows_decode_dev.
 *
 * Stats: 6 launches (5 count-only); bytes_algorithmic grows by
 * delta_offs[n_blocks] + 20*n_blocks + 8*(n_rows+1) + 8*m + 8*total, the size
 * of the call's input plus its output, not its memory traffic (blocks dropped
 * from their headers are never read; probed shared values are read again). */
typedef struct {
    /* flat block arena of all rows' packs */
    const uint64_t *bases;          /* device [n_blocks] */
    const uint32_t *num_uids;       /* device [n_blocks] */
    const uint64_t *delta_offs;     /* device [n_blocks+1] */
    const uint8_t *deltas;          /* device blob */
    uint64_t n_blocks;
    const uint64_t *row_block_base; /* DEVICE [n_rows+1], non-decreasing,
                                     * [0] = 0, [n_rows] = n_blocks */
    uint64_t n_rows;
    const uint64_t *after;          /* device [n_rows] or NULL (= all 0) */
    const void *reserved;           /* must be NULL: ua_drowpacks has first here
                                     * (the two structs share their first nine
                                     * slots), and this call has no first */
    const uint64_t *shared;         /* device [m], sorted, duplicate-free */
    uint64_t m;
    uint64_t *out_vals;             /* device, capacity cap_vals; NULL with
                                     * cap_vals == 0 = count only */
    uint64_t cap_vals;
    uint64_t *out_row_offs;         /* device [n_rows+1] */
} ua_drowisect;
int ua_rows_intersect_packed_dev(ua_ctx *, const ua_drowisect *, uint64_t *out_total);

/* The UID matrix of a per-key fan-out over LIVE lists, in ONE call: packs plus
 * per-row mutation layers in, CSR matrix out, one stream sync (since v17).
 * On a list with a mutable layer pl.Uids(opts) (List.Uids,
 * posting/list.go:1786-1902) is not a decode but List.iterate
 * (posting/list.go:1135-1251): a two-pointer merge of the pack with the picked
 * mutable postings (pickPostings, list.go:1099-1133), in which a Del posting
 * removes a uid and any other posting adds or overrides one.  The count-only
 * form (out_vals NULL, cap_vals 0) gives every key's
 * List.Length(readTs, afterUid) (list.go:1345-1363) on a mutated list.  Input
 * layout as ua_rows_decode_dev (slots 0-8 are ua_drowpacks'), plus all rows'
 * mutation slices concatenated: row r owns
 * mut_uids/mut_ops[row_mut_base[r], row_mut_base[r+1]).  The output is directly
 * the input of ua_rows_filter_dev / ua_rows_union_dev.
 *
 * SEMANTICS.  For row r let P be the decoded uids of the row's blocks, M the
 * row's mutation slice and S the uids of M whose op is not UA_MUT_DEL.  Then
 *   1. row = sorted((P - uids(M)) | S).  A set on a uid that P already holds
 *      emits it once; a delete of an absent uid does nothing.  ANY op other
 *      than UA_MUT_DEL sets (iterate tests only mp.Op != Del, list.go:1217, 1229,
 *      so Ovr = 3 is a set).
 *   2. then x > after[r], STRICTLY, on both sides of the merge: pitr.seek with
 *      SeekCurrent for the pack and afterUid < mp.Uid for the layer
 *      (list.go:1146).  after[r] == 0 keeps all.  This is ua_rows_decode_dev's
 *      rule.
 *   3. then ListOptions.First (list.go:1892-1900), word for word as in
 *      ua_rows_decode_dev: first[r] > 0 keeps the first first[r] of them,
 *      first[r] < 0 the last -first[r], first[r] == 0 all; INT32_MIN is legal.
 *   4. after == NULL means all 0, first == NULL all 0.
 * One divergence, not new: with a negative First the reference's own loop
 * stops after the first collected uid (len(res) > opt.First, list.go:1868),
 * so the window at 1892-1900 has nothing to cut; this call, like
 * ua_rows_decode_dev, implements the window as lines 1892-1900 state it.
 *
 * What the caller hands over: each row's slice is pickPostings' result with
 * only the newest version per uid kept (iterate's prevUid rule), strictly
 * ascending by uid; a row under a delete-all marker (deleteBelowTs > 0,
 * list.go:580-584) passes no blocks; only REF postings are in scope (a key
 * whose layer holds value postings keeps the Go path).  The parity domain is
 * uids >= 1 on both sides: iterate treats uid 0 as "iterator exhausted".  A 0
 * in P behaves as in ua_rows_decode_dev.  A 0 in M, or a slice that is not
 * strictly ascending, gives an unspecified row, but every access stays in
 * bounds and out_vals receives nothing past what out_row_offs counts.
 *
 * Capacity, count-only and the pack limits are exactly ua_rows_decode_dev's:
 * *out_total is always the REQUIRED total and out_row_offs is always complete,
 * whatever cap_vals is; every store into out_vals is bounded by cap_vals; if
 * *out_total > cap_vals and out_vals is not NULL the call returns
 * UA_ERR_INVALID with out_vals unspecified but untouched past cap_vals.  A
 * block with num_uids > 256 or more than 1092 delta bytes gives
 * UA_ERR_INVALID and *out_total = 0.
 *
 * n_mut == 0 IS ua_rows_decode_dev: its checks, kernels, launches and stats
 * (the three mutation arrays are then ignored and may be NULL).  Otherwise
 * rejected with UA_ERR_INVALID before the context is touched, nothing written:
 * everything ua_rows_decode_dev rejects; a null mut_uids, mut_ops or
 * row_mut_base; n_rows == 0; 256 * n_blocks + n_mut > 2^32 - 2 (every count,
 * the largest being one row's length, goes through the engine's u32 scan, and
 * 2^32 - 1 marks a count that is still open);
 * out_vals or out_row_offs overlapping mut_uids, mut_ops or row_mut_base.
 *
 * Memory safety does not depend on the data, as for ua_rows_decode_dev:
 * row_mut_base entries are clamped to [0, n_mut] and to m0 <= m1, and every
 * probe of mut_uids stays inside the row's clamped slice.
 *
 * Stats (n_mut > 0): 13 launches with blocks (10 count-only), 8 without (7
 * count-only), 3 more with first; bytes_algorithmic grows by
 * delta_offs[n_blocks] + 20*n_blocks + 16*(n_rows+1) + 9*n_mut + 8*total. */
enum { UA_MUT_SET = 1, UA_MUT_DEL = 2 }; /* list.go:49-53 Set / Del */
typedef struct {
    /* slots 0-8: exactly ua_drowpacks' */
    const uint64_t *bases;          /* device [n_blocks] */
    const uint32_t *num_uids;       /* device [n_blocks] */
    const uint64_t *delta_offs;     /* device [n_blocks+1] */
    const uint8_t *deltas;          /* device blob */
    uint64_t n_blocks;
    const uint64_t *row_block_base; /* DEVICE [n_rows+1], non-decreasing,
                                     * [0] = 0, [n_rows] = n_blocks */
    uint64_t n_rows;
    const uint64_t *after;          /* device [n_rows] or NULL (= all 0) */
    const int32_t *first;           /* device [n_rows] or NULL (= all 0) */
    const uint64_t *mut_uids;       /* device [n_mut]: all rows' picked postings,
                                     * concatenated; strictly ascending inside a row */
    const uint8_t *mut_ops;         /* device [n_mut]: UA_MUT_DEL deletes; ANY other
                                     * value sets */
    const uint64_t *row_mut_base;   /* DEVICE [n_rows+1], non-decreasing, [0] = 0,
                                     * [n_rows] = n_mut; NULL with n_mut == 0 */
    uint64_t n_mut;
    uint64_t *out_vals;             /* device, capacity cap_vals; NULL with
                                     * cap_vals == 0 = count only */
    uint64_t cap_vals;
    uint64_t *out_row_offs;         /* device [n_rows+1] */
} ua_drowmut;                       /* 16 slots, 128 bytes: n_mut at 96, cap_vals at 112 */
int ua_rows_decode_mut_dev(ua_ctx *, const ua_drowmut *, uint64_t *out_total);

/* A CSR UID matrix encoded into a fan-out of UidPacks in ONE call: the inverse
 * of the three row decoders, one stream sync (since v18).  The reference
 * encodes populations of lists one list after another, one
 * codec.Encoder{BlockSize} each (codec.go:57-136; codec.Encode, codec.go:393,
 * is that loop for one list): List.encode in the rollup, one encoder per
 * split part (posting/list.go:1609-1664), the bulk loader's reduce over every
 * key of a map shard (dgraph/cmd/bulk/reduce.go:811-861) and its count index
 * (dgraph/cmd/bulk/count_index.go:133-154).  Here every list is one row.
 *
 * Row r's blocks are what codec.Encoder{BlockSize: block_size} yields after
 * Add of each value of row r in order.  A new block starts at a row start,
 * wherever the upper 32 bits change, and every block_size uids inside a row's
 * 32-MSB run (block_size 0 behaves as 1, like ua_encode_dev).  bases[b] is the
 * block's first uid; its deltas are group-varint groups of four, the last
 * group zero-padded, and a one-uid block carries one all-zero group.  On every
 * strictly ascending row the bytes are those of ua_encode and of the oracle's
 * encoder.  Blocks are laid out in row order: row_block_base[r] is the index
 * of row r's first block, row_block_base[n_rows] == *n_blocks,
 * delta_offs[*n_blocks] == *deltas_bytes, and an empty row owns no block.  A
 * multi-part list (Splits) passes one row per part.  Rows are not
 * de-duplicated: the bulk reducer's uid == lastUid skip stays with the caller
 * (ua_rows_union_dev first).
 *
 * The output is, unchanged, the arena of ua_rows_decode_dev,
 * ua_rows_intersect_packed_dev and ua_rows_decode_mut_dev.  Their limit
 * n_blocks <= 2^24 - 1 is the consumers', not this call's.
 *
 * Capacity, by the family's rule: *n_blocks, *deltas_bytes and row_block_base
 * are always the REQUIRED and complete values, whatever the capacities.  Every
 * store is bounded by its capacity.  If either requirement exceeds its
 * capacity and the outputs are not NULL the call returns UA_ERR_INVALID; the
 * outputs are then unspecified but untouched past the capacities.  Count-only
 * form: all four pack outputs NULL with both capacities 0; it runs no write
 * pass and sizes the second call exactly.
 *
 * Rejected with UA_ERR_INVALID before the context is touched, nothing
 * written: a null ctx, desc, n_blocks, deltas_bytes or row_block_base; null
 * vals with total > 0; null row_offs with n_rows > 0; n_rows == 0 with
 * total != 0; block_size > 256; some but not all pack outputs NULL, or a NULL
 * output with a non-zero capacity; any output overlapping an input or another
 * output; total >= 2^42 or n_rows >= 2^39 (the tile grid, total / 2048, and the
 * row grid, n_rows / 256, are 32-bit block counts; a tile's counts, at most
 * 2048 blocks and 5 * 2048 + 3 bytes, always fit the engine's u32 scan);
 * cap_blocks >= 2^60.  total == 0 is valid: zero offsets and no launch.
 *
 * Memory safety does not depend on the data: row_offs entries are clamped to
 * total; rows that are not ascending or a row_offs that is not monotone give
 * unspecified packs, never an out-of-range access.  The write pass is the
 * count pass's code and stores exactly what that counted.
 *
 * Stats: 7 launches without the write pass (row bits, count, two scans of two
 * kernels, row bases) and 8 with it; kernel_ms is the count pass plus the
 * write pass.  bytes_algorithmic grows by input plus output:
 * 8*total + 8*(n_rows+1) plus *deltas_bytes + 20*(*n_blocks) + 8*(n_rows+1). */
typedef struct {
    const uint64_t *vals;           /* device [total]: rows concatenated */
    const uint64_t *row_offs;       /* device [n_rows+1], non-decreasing,
                                     * [0] = 0, [n_rows] = total */
    uint64_t n_rows, total;
    uint64_t block_size;            /* <= 256; 0 packs one uid per block */
    uint64_t *bases;                /* device [cap_blocks] */
    uint32_t *num_uids;             /* device [cap_blocks] */
    uint64_t *delta_offs;           /* device [cap_blocks+1] */
    uint64_t cap_blocks;
    uint8_t *deltas;                /* device [cap_deltas] */
    uint64_t cap_deltas;
    uint64_t *row_block_base;       /* device [n_rows+1], always written */
} ua_drowenc;                       /* 12 slots, 96 bytes */
int ua_rows_encode_dev(ua_ctx *, const ua_drowenc *, uint64_t *n_blocks,
                       uint64_t *deltas_bytes);

/* Sort and paginate every row of a CSR UID matrix by per-element keys in ONE
 * call (since v19): CSR matrix in, CSR matrix out, device
 * resident, one sync, nothing per row on the host.  It is the step between
 * ua_rows_filter_dev and ua_rows_union_dev that the reference runs once per row
 * for every ordered or paginated block (orderasc:, first:, offset:):
 *   applyPagination            query/query.go:2493-2507 (x.PageRange per row)
 *   applyOrderAndPagination    query/query.go:2511-2578 -> worker.SortOverNetwork
 *     -> sortWithoutIndex      worker/sort.go:139-187
 *        sortByValue           worker/sort.go:775-821
 *        paginate              worker/sort.go:740-772
 *   sortAndPaginateUsingVar    query/query.go:2697-2738
 *   the cascade paginations    query/query.go:1483-1487, 3006-3010
 *   x.PageRange                x/x.go:815-844
 *
 * Per row r (offsets clamped to total), n elements e_0 .. e_{n-1} in input order:
 *  1. keys == NULL: S is the row as it is (applyPagination, the cascades).
 *  2. Otherwise V = the elements with has != 0 (all when has == NULL), ordered
 *     by key as unsigned 64-bit, ascending, or descending with UA_SORT_DESC;
 *     ties by input position ASCENDING IN BOTH DIRECTIONS.  N = the other
 *     elements in input order.  The reference's types.Sort is unstable, so it
 *     leaves tie order open; position order is this project's refinement and
 *     is uid-ascending on uid-sorted rows, as in oracle/sortref.py.
 *  3. Without UA_SORT_DROP_NULLS, S = V then N (sortByValue appends the nulls
 *     whether ascending or descending, sort.go:813).
 *  4. With UA_SORT_DROP_NULLS, S = V (sortAndPaginateUsingVar,
 *     query.go:2709-2716); when V is empty the row stays exactly as it was,
 *     all n elements (the reference's `continue`, query.go:2718-2720).
 *  5. (start, end) = x.PageRange(count, offset, len(S)), word for word:
 *     count < 0 takes the last -count (clamped, offset ignored), offset < 0
 *     counts as 0, offset > len gives an empty page, count == 0 means "to the
 *     end".
 *  6. With UA_SORT_MULTI (len(ts.Order) > 1, sort.go:748-769) the page grows
 *     over equal keys at both edges, OVER V ONLY: while 0 < start < |V| and
 *     key(S[start]) == key(S[start-1]) start--; while end < |V| and
 *     key(S[end-1]) == key(S[end]) end++.  A null equals nothing: types.Equal
 *     on a types.Val{} reports false or an error, never true.
 *     oracle/sortref.py treats two nulls as equal; the two differ only when a
 *     page edge lies inside the null tail under UA_SORT_MULTI.  The extension
 *     is two binary searches in the sorted run, never a walk.
 *  7. Out row r = S[start:end]; out_src[o] = the flat INPUT index of output
 *     element o (so facets and values can be reordered without the IndexOf
 *     loop of query.go:2561-2569, and multiSortVals fetched);
 *     out_ms_offs[r] = start < offset ? offset - start : 0 (sort.go:170-178).
 * Rows need not be uid-sorted and may hold duplicate uids.  0 and UINT64_MAX
 * are ordinary keys and uids, also under UA_SORT_DESC.
 *
 * Capacity, by the family's rule: *out_total and out_row_offs are always the
 * REQUIRED and complete values.  Every store is bounded by cap_vals.  A short
 * cap_vals with non-NULL out_vals returns UA_ERR_INVALID, outputs untouched
 * past the capacity.  Count-only form: out_vals NULL with cap_vals 0; no sort
 * runs when the lengths do not depend on the order (keys == NULL, or neither
 * UA_SORT_MULTI nor UA_SORT_DROP_NULLS).
 *
 * Rejected with UA_ERR_INVALID before the context is touched, nothing
 * written: a null ctx, desc, out_total or out_row_offs; null vals with
 * total > 0; null row_offs with n_rows > 0; n_rows == 0 with total != 0;
 * flags != 0 or a non-NULL has with keys == NULL; unknown flag bits;
 * UA_SORT_MULTI together with UA_SORT_DROP_NULLS (no reference caller has
 * both); out_ms_offs without UA_SORT_MULTI; out_src with NULL out_vals; NULL
 * out_vals with cap_vals > 0; any output overlapping an input or another
 * output; total >= 2^31 or n_rows >= 2^31 (an element index plus the null bit
 * share 32 bits); cap_vals >= 2^60.  total == 0 and n_rows == 0 are valid.
 *
 * Memory safety does not depend on the data: row_offs entries are clamped to
 * total; a row_offs that is not monotone gives unspecified rows, never an
 * out-of-range access: when a clamped entry lies below its predecessor every
 * row is published empty (*out_total == 0), so rows never overlap and
 * *out_total <= total always holds; every index read from a record is clamped
 * below total; out_row_offs is a scan of the row lengths and out_vals
 * receives exactly what it counts.  Elements past row_offs[n_rows] belong to
 * no row and are left out.
 *
 * Engine scratch: 24 bytes per element (two buffers of an 8-byte key and a
 * 4-byte tag), one bit per element for the row starts, 8 bytes per 2048-element
 * tile, 16 bytes per row (length, first rank, scanned offset), the scan
 * partials and 16 bytes of words.  The page-only form needs the per-row part
 * only.
 *
 * Stats, with R = ceil(log2(ceil(total / 2048))): 6 + R launches for a sort
 * without the write pass (row bits, tile sort, R rounds, page, two scan
 * kernels, offsets), 7 + R with it; 4 and 5 for the page-only form, for
 * total == 0 and for a count-only call that needs no sort (the write pass is
 * also skipped when min(cap_vals, total) == 0).  kernel_ms is the whole
 * sequence.  bytes_algorithmic grows by input plus output: 8*total for vals,
 * 8*total for keys if given, total for has if given, 8*(n_rows+1) for each
 * offset array, 8 per stored output element, plus 8 per stored output element
 * for out_src. */
enum { UA_SORT_DESC = 1, UA_SORT_MULTI = 2, UA_SORT_DROP_NULLS = 4 };
typedef struct {
    const uint64_t *vals;       /* device [total]: rows concatenated */
    const uint64_t *row_offs;   /* device [n_rows+1] */
    uint64_t n_rows, total;
    const uint64_t *keys;       /* device [total], parallel to vals; NULL = page only */
    const uint8_t *has;         /* device [total], nonzero = the element has a key;
                                 * NULL = all have one */
    uint64_t flags;             /* UA_SORT_*; must be 0 when keys == NULL */
    int32_t count, offset;      /* ts.Count / ts.Offset, one 8-byte slot */
    uint64_t *out_vals;         /* device [cap_vals]; NULL with cap_vals 0 = count only */
    uint64_t cap_vals;
    uint64_t *out_row_offs;     /* device [n_rows+1], always complete */
    uint64_t *out_src;          /* optional, device [cap_vals]: flat INPUT index of
                                 * every output element (the permutation) */
    int32_t *out_ms_offs;       /* optional, device [n_rows]: multiSortOffsets */
} ua_drowsort;                  /* 13 slots, 104 bytes */
int ua_rows_sort_dev(ua_ctx *, const ua_drowsort *, uint64_t *out_total);

/* Transpose a CSR UID matrix in ONE call (since v20): given
 * src -> [dst...], produce dst -> [src...], device resident, one sync, nothing
 * per edge on the host.  It is the step the reference runs per edge or per
 * element, through a hash map or a posting-list mutation:
 *   formResult                 query/groupby.go:195-260
 *   fillGroupedVars            query/groupby.go:265-361
 *     uid child:   dedup.addValue(attr, uid, srcUid) per element
 *                              query/groupby.go:104-128, :210-221, :292-298
 *     value child: the same grouping, one element per row
 *                              query/groupby.go:224-234, :302-312
 *   rebuildReverseEdges        posting/index.go:1759-1791, one
 *     addReverseMutation       posting/index.go:276-298 per posting
 *   rebuildCountIndex          posting/index.go:1595-1640 (addCountMutation :431)
 *   the bulk mapper's reverse entries  dgraph/cmd/bulk/mapper.go:398-432
 *                              (x.ReverseKey at :345), sorted in reduce
 * With it a reverse-index rebuild is ua_rows_decode[_mut]_dev ->
 * ua_rows_transpose_dev -> ua_rows_encode_dev, and groupby over a uid
 * predicate is one call once the child's matrix exists; count(uid) per group
 * is the group's length.
 *
 *  1. An element is LIVE when its flat index i is below min(row_offs[n_rows],
 *     total), its row is the unique r with row_offs[r] <= i < row_offs[r+1],
 *     and row_keep is NULL or row_keep[r] != 0 (formResult's
 *     `IndexOf(ul, srcUid) < 0 -> continue`; the caller computes the mask with
 *     ua_index_of_batch_dev).  Every other element takes no part.
 *  2. out_keys[0 .. *n_groups) holds the distinct values of the live elements,
 *     ascending as unsigned 64-bit.  0 and UINT64_MAX are ordinary values.
 *     With row_keep == NULL and row_offs[n_rows] == total this is exactly the
 *     output of ua_rows_union_dev(vals, total).
 *  3. Group g holds one entry per live element whose value is out_keys[g],
 *     ordered by flat input index ascending: row ascending, then position,
 *     which is addValue's append order.  The entry's payload is
 *     out_vals = row_uids ? row_uids[r] : r; out_src is the flat INPUT index
 *     (a reverse edge carries the forward posting's facets, index.go:1775).
 *  4. out_offs[g] is the group's first entry; out_offs[*n_groups] == *out_total.
 *  5. Multiplicity is kept by default: a uid twice in one row yields its row
 *     twice, as addValue does.  UA_TR_UNIQUE collapses entries with the same
 *     (value, row) to the one with the lowest flat index, because a reverse
 *     posting list is a set.  On duplicate-free rows the two agree.
 *  6. Rows need not be sorted.  When row_uids is ascending every group is an
 *     ascending list, duplicate-free under UA_TR_UNIQUE or on duplicate-free
 *     rows: valid input for ua_rows_encode_dev, ua_rows_filter_dev and a
 *     second transpose.
 *  7. One element per row (row_offs = 0, 1, ..., n_rows) groups the rows by a
 *     per-row key: value-node groupby over order-independent u64 keys, or
 *     rebuildCountIndex with vals set to the list lengths.  No extra
 *     parameter is needed.
 *
 * Capacity, by the family's rule as far as it can hold with two sizes:
 * *n_groups and *out_total are always the REQUIRED values.  Every store is
 * bounded: keys by cap_keys, group offsets by cap_keys + 1, entries by
 * cap_vals.  A short capacity with non-NULL outputs returns UA_ERR_INVALID,
 * outputs untouched past the capacities.  Both requirements are at most total,
 * so a caller may size by total and skip a count call.  Three forms: full
 * (all outputs, out_src optional); groups only (out_vals and out_src NULL,
 * cap_vals 0: groupby with only count(uid)); count only (all four outputs
 * NULL, both capacities 0; no scan and no write pass run).  Group offsets are
 * written whenever keys are.
 *
 * Rejected with UA_ERR_INVALID before the context is touched, nothing
 * written: a null ctx, desc, n_groups or out_total; null vals with total > 0;
 * null row_offs with n_rows > 0; n_rows == 0 with total != 0; unknown flag
 * bits; out_keys and out_offs not both NULL or both non-NULL; either of them
 * NULL with cap_keys > 0; out_vals NULL with cap_vals > 0; out_src without
 * out_vals; out_vals without out_keys; any output overlapping an input or
 * another output; total >= 2^31 or n_rows >= 2^31 (a flat index and the dead
 * bit share a 32-bit tag); either capacity >= 2^60.  total == 0 and
 * n_rows == 0 are valid: zero groups, and out_offs[0] = 0 if given.
 *
 * Memory safety does not depend on the data: row_offs entries are clamped to
 * total (they are only compared against flat indices below total); with a
 * row_offs that is not monotone an element's row is unspecified, but it is
 * some index < n_rows that holds the element, or the element is dead; every
 * index read back from a record is clamped below total and every row below
 * n_rows; each input element is one record and is emitted at most once, so
 * *out_total <= total and *n_groups <= *out_total hold for any input; barriers
 * sit only under workgroup-uniform conditions.
 *
 * Engine scratch: 28 bytes per element (two buffers of an 8-byte value and a
 * 4-byte tag, and a 4-byte row), 24 bytes per 2048-element tile (two counts
 * and their scanned offsets), the scan partials and 16 bytes of words.
 *
 * Stats, with R = ceil(log2(ceil(total / 2048))): 2 + R launches for the
 * count-only form (tile sort, R rounds, flags), 5 + R for the groups-only and
 * the full form (two scan kernels and the write pass more), 0 for total == 0.
 * kernel_ms is the whole sequence.  bytes_algorithmic grows by input plus
 * stored output: 8*total for vals, 8*(n_rows+1) for row_offs, 8*n_rows for
 * row_uids if given, n_rows for row_keep if given, 8 per stored key, 8 per
 * stored group offset (stored keys + 1), 8 per stored entry, plus 8 per stored
 * entry for out_src. */
enum { UA_TR_UNIQUE = 1 };
typedef struct {
    const uint64_t *vals;      /* device [total]: rows concatenated */
    const uint64_t *row_offs;  /* device [n_rows+1], non-decreasing, [0]=0 */
    uint64_t n_rows, total;
    const uint64_t *row_uids;  /* device [n_rows] (SrcUIDs) or NULL = the row index */
    const uint8_t  *row_keep;  /* device [n_rows], nonzero = row takes part; NULL = all */
    uint64_t flags;            /* UA_TR_* */
    uint64_t *out_keys;        /* device [cap_keys]: distinct values, ascending */
    uint64_t *out_offs;        /* device [cap_keys+1]: CSR offsets of the groups */
    uint64_t cap_keys;
    uint64_t *out_vals;        /* device [cap_vals]: per group, the rows' uids */
    uint64_t *out_src;         /* optional, device [cap_vals]: flat INPUT index */
    uint64_t cap_vals;
} ua_drowtr;                   /* 13 slots, 104 bytes */
int ua_rows_transpose_dev(ua_ctx *, const ua_drowtr *, uint64_t *n_groups, uint64_t *out_total);

/* fused decode+intersect: algo.IntersectCompressedWith (uidlist.go:33) over a
 * device pack; v device; out device, capacity min(total_uids, m). */
int ua_intersect_packed_dev(ua_ctx *, const ua_dpack *, uint64_t after_uid,
                            const uint64_t *v, uint64_t m, uint64_t *out,
                            uint64_t *out_n);

/* Batched fused decode+intersect — ONE grid over a whole per-key fan-out
 * (worker/task.go:834-971 handleUidPostings: thousands of keys' packs, each
 * intersected with its filter list, often one shared q.UidList).  All packs
 * are concatenated into one flat block arena (bases/num_uids/delta_offs/
 * deltas, like ua_dpack); pack_block_base[n_packs+1] delimits each pack's
 * blocks.  Per-pack v/out/after are device pointers in the tasks array. */
typedef struct {
    const uint64_t *v; /* device */
    uint64_t m;
    uint64_t *out;     /* device, capacity >= min(pack uids, m) */
    uint64_t after_uid;
} ua_ptask;

int ua_intersect_packed_batch_dev(ua_ctx *, const uint64_t *bases,
                                  const uint32_t *num_uids,
                                  const uint64_t *delta_offs,
                                  const uint8_t *deltas,
                                  const uint64_t *pack_block_base /* host [n_packs+1] */,
                                  int n_packs, const ua_ptask *tasks /* host */,
                                  uint64_t *out_lens);

/* Prepared pack fan-out (a standing query plan): task/boundary upload and
 * workspace sizing once at create; each run is launches + one lens read.
 * The flat pack arena and the tasks' v/out buffers are caller-owned device
 * memory that must outlive the handle; their contents may change between
 * runs (the plan caches no data-dependent state, unlike ua_batch). */
typedef struct ua_pbatch ua_pbatch;
int ua_pbatch_create(ua_ctx *, const uint64_t *bases, const uint32_t *num_uids,
                     const uint64_t *delta_offs, const uint8_t *deltas,
                     const uint64_t *pack_block_base /* host [n_packs+1] */,
                     int n_packs, const ua_ptask *tasks /* host */,
                     ua_pbatch **out);
int ua_pbatch_run(ua_ctx *, ua_pbatch *, uint64_t *out_lens);
void ua_pbatch_destroy(ua_ctx *, ua_pbatch *);

/* ---- host-pointer convenience (upload+compute+download; mirrors the algo
 * package signatures 1:1 for the cgo shim) ---- */
int ua_intersect(ua_ctx *, const uint64_t *u, uint64_t n, const uint64_t *v,
                 uint64_t m, uint64_t *out, uint64_t *out_n);  /* IntersectWith */
int ua_intersect_k(ua_ctx *, const uint64_t *const *lists, const uint64_t *lens,
                   int k, uint64_t *out, uint64_t *out_n);     /* IntersectSorted */
int ua_merge_k(ua_ctx *, const uint64_t *const *lists, const uint64_t *lens,
               int k, uint64_t *out, uint64_t *out_n);         /* MergeSorted */
int ua_difference(ua_ctx *, const uint64_t *u, uint64_t n, const uint64_t *v,
                  uint64_t m, uint64_t *out, uint64_t *out_n); /* Difference */
int64_t ua_index_of(const uint64_t *u, uint64_t n, uint64_t uid); /* IndexOf:
                  * one log(n) probe — host binary search like the reference;
                  * the batched GPU form is ua_index_of_batch_dev */
int ua_apply_filter(ua_ctx *, uint64_t *u /* compacted in place */, uint64_t n,
                    const uint8_t *mask, uint64_t *out_n); /* ApplyFilter */
int ua_intersect_packed(ua_ctx *, const ua_pack *, uint64_t after_uid,
                        const uint64_t *v, uint64_t m, uint64_t *out,
                        uint64_t *out_n);            /* IntersectCompressedWith */
/* updateUidMatrix (query/query.go:1425-1437) and the worker/task.go:1352,
 * 1617,1692,1778 per-row IntersectWith loops as ONE call: host form of
 * ua_rows_filter_dev (same semantics and modes).  vals/row_offs/shared are
 * host arrays, total = row_offs[n_rows]; the compacted rows go to
 * out_vals (capacity total) and the new offsets to out_row_offs[n_rows+1].
 * out_vals may be vals and out_row_offs may be row_offs (the reference's
 * in-place shape): the device works on its own buffers. */
int ua_rows_filter(ua_ctx *, const uint64_t *vals, const uint64_t *row_offs,
                   uint64_t n_rows, const uint64_t *shared, uint64_t m, int mode,
                   uint64_t *out_vals, uint64_t *out_row_offs, uint64_t *out_total);
/* DestUIDs = MergeSorted(UidMatrix) (query/query.go:1874, 2290, 2505 and the
 * other callers listed at ua_rows_union_dev) over the rows' concatenation:
 * host form of ua_rows_union_dev, same semantics and checks.  vals and out
 * are host arrays, total = row_offs[n_rows]; the device works on its own
 * buffer, so out may overlap vals in any way. */
int ua_rows_union(ua_ctx *, const uint64_t *vals /* host */, uint64_t total,
                  uint64_t *out /* host, capacity total */, uint64_t *out_n);
/* The handleUidPostings loop (worker/task.go:834-971) with opts.Intersect ==
 * nil as ONE call: host form of ua_rows_decode_dev, same semantics (x >
 * after[r], then first[r]), same capacity rule and checks.  packs[r] is row
 * r's pack (NULL = an empty row); after and first are host arrays of n_rows
 * or NULL; out_vals (host, capacity cap_vals; NULL with cap_vals == 0 = count
 * only) and out_row_offs (host, n_rows+1) receive the CSR matrix.  On a
 * short cap_vals the offsets and *out_total are still delivered. */
int ua_rows_decode(ua_ctx *, const ua_pack *const *packs, uint64_t n_rows,
                   const uint64_t *after, const int32_t *first, uint64_t *out_vals,
                   uint64_t cap_vals, uint64_t *out_row_offs, uint64_t *out_total);
/* The handleUidPostings loop over lists with mutable layers as ONE call: host
 * form of ua_rows_decode_mut_dev (since v17), same semantics (List.iterate's
 * merge, then x > after[r], then first[r]), same capacity rule and checks.
 * packs[r] is row r's pack (NULL = a row without blocks); mut_uids, mut_ops
 * and row_mut_base (host [n_rows+1], n_mut = row_mut_base[n_rows]; NULL = no
 * mutation at all, which is ua_rows_decode) are host arrays; so are after,
 * first and the outputs, as for ua_rows_decode. */
int ua_rows_decode_mut(ua_ctx *, const ua_pack *const *packs, uint64_t n_rows,
                       const uint64_t *mut_uids, const uint8_t *mut_ops,
                       const uint64_t *row_mut_base /* host [n_rows+1] */,
                       const uint64_t *after, const int32_t *first,
                       uint64_t *out_vals, uint64_t cap_vals,
                       uint64_t *out_row_offs, uint64_t *out_total);
/* The handleUidPostings loop with opts.Intersect != nil
 * (posting/list.go:1823-1829: one IntersectCompressedWith per key against
 * q.UidList) as ONE call: host form of ua_rows_intersect_packed_dev (since v16), same semantics
 * (x >= after[r] and x in shared, no first), same capacity rule and checks.
 * packs[r] is row r's pack (NULL = an empty row); after is a host array of
 * n_rows or NULL; shared a host array of m sorted duplicate-free uids;
 * out_vals (host, capacity cap_vals; NULL with cap_vals == 0 = count only) and
 * out_row_offs (host, n_rows+1) receive the CSR matrix.  On a short cap_vals
 * the offsets and *out_total are still delivered. */
int ua_rows_intersect_packed(ua_ctx *, const ua_pack *const *packs, uint64_t n_rows,
                             const uint64_t *after, const uint64_t *shared, uint64_t m,
                             uint64_t *out_vals, uint64_t cap_vals,
                             uint64_t *out_row_offs, uint64_t *out_total);
/* One codec.Encoder{BlockSize} per list over a population of lists
 * (codec.go:57-136, codec.go:393; posting/list.go:1609-1664;
 * dgraph/cmd/bulk/reduce.go:811-861, count_index.go:133-154) as ONE call: host
 * form of ua_rows_encode_dev (since v18), same semantics, capacity rule and
 * checks.  vals and row_offs are host arrays, total = row_offs[n_rows]; the
 * five outputs are host arrays with ua_drowenc's capacities (count only: the
 * four pack outputs NULL, both capacities 0).  On a short capacity
 * row_block_base and both sizes are still delivered. */
int ua_rows_encode(ua_ctx *, const uint64_t *vals, const uint64_t *row_offs,
                   uint64_t n_rows, uint64_t block_size, uint64_t *bases,
                   uint32_t *num_uids, uint64_t *delta_offs, uint64_t cap_blocks,
                   uint8_t *deltas, uint64_t cap_deltas, uint64_t *row_block_base,
                   uint64_t *n_blocks, uint64_t *deltas_bytes);
/* Order and pagination of every row of a UID matrix (applyPagination,
 * query/query.go:2493-2507; sortWithoutIndex, worker/sort.go:139-187;
 * sortAndPaginateUsingVar, query/query.go:2697-2738; x.PageRange,
 * x/x.go:815-844) as ONE call: host form of ua_rows_sort_dev (since v19),
 * same semantics, capacity rule and checks.  vals, row_offs, keys (or NULL)
 * and has (or NULL) are host arrays, total = row_offs[n_rows]; out_vals
 * (capacity cap_vals; NULL with cap_vals == 0 = count only), out_row_offs
 * (n_rows+1), out_src (optional, cap_vals) and out_ms_offs (optional, n_rows)
 * are host arrays.  The device works on its own buffers, so the outputs may
 * overlap the inputs.  On a short cap_vals the offsets, out_ms_offs and
 * *out_total are still delivered. */
int ua_rows_sort(ua_ctx *, const uint64_t *vals, const uint64_t *row_offs,
                 uint64_t n_rows, const uint64_t *keys, const uint8_t *has,
                 uint64_t flags, int32_t count, int32_t offset, uint64_t *out_vals,
                 uint64_t cap_vals, uint64_t *out_row_offs, uint64_t *out_src,
                 int32_t *out_ms_offs, uint64_t *out_total);
/* The transpose of a UID matrix (dedup.addValue's grouping,
 * query/groupby.go:104-128, 195-260, 265-361; rebuildReverseEdges,
 * posting/index.go:1759-1791) as ONE call: host form of ua_rows_transpose_dev
 * (since v20), same semantics, forms, capacity rule and checks.  vals,
 * row_offs, row_uids (or NULL) and row_keep (or NULL) are host arrays,
 * total = row_offs[n_rows]; out_keys (cap_keys), out_offs (cap_keys + 1),
 * out_vals (cap_vals) and out_src (optional, cap_vals) are host arrays.  The
 * device works on its own buffers, so the outputs may overlap the inputs.  On
 * a short capacity *n_groups and *out_total are still delivered and the output
 * arrays are left as they were. */
int ua_rows_transpose(ua_ctx *, const uint64_t *vals, const uint64_t *row_offs,
                      uint64_t n_rows, const uint64_t *row_uids, const uint8_t *row_keep,
                      uint64_t flags, uint64_t *out_keys, uint64_t *out_offs,
                      uint64_t cap_keys, uint64_t *out_vals, uint64_t *out_src,
                      uint64_t cap_vals, uint64_t *n_groups, uint64_t *out_total);

#ifdef __cplusplus
}
#endif
#endif /* UIDALGO_H */
