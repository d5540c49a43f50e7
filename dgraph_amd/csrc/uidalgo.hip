/*
 * uidalgo — MI355X-native (gfx950 / CDNA4) posting-list set-algebra engine.
 *
 * Implements the C-ABI in include/uidalgo.h: a from-scratch GPU engine for
 * the dgraph algo/uidlist.go + codec/ hot path (reference interfaces cited
 * per function).  Design:
 *
 *  - batched merge-path set algebra: every (u,v) list pair is cut into
 *    TILE-element merge-path tiles; one 256-thread workgroup intersects /
 *    unions / differences one tile out of LDS; per-tile match counts are
 *    scanned (flat hierarchical scan) and compacted so outputs stay sorted.
 *    All pairs of a batch go through ONE grid (the reference fans out one
 *    goroutine per key, worker/task.go:834-971; here the whole fan-out is
 *    one launch).
 *  - fused decode+intersect: one 64-lane wavefront decodes one group-varint
 *    block (codec.go:154 UnpackBlock format) into LDS — control-byte walk,
 *    per-lane 4-delta extract, wave prefix-sum — and intersects it with its
 *    v-range without a global round trip.
 *
 * Everything is integer/HBM-bound: no MFMA.  Wavefront = 64; ballot masks
 * are 64-bit.
 *
 * Semantics contract (parity with the Go reference is bit-exact on
 * duplicate-free sorted inputs — the domain the reference itself pins:
 * uidlist_test.go:394 "behaviour of bin intersect is not defined when
 * duplicates are present"; posting lists are sorted sets, paper/dgraph.tex:269).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <iterator>
#include <mutex>
#include <vector>

#include "../../include/uidalgo.h"

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef uint8_t u8;

#ifndef UA_ABLATE
#define UA_ABLATE 0 /* perf-bisection builds only (tools/ubench.py): 1 = fill-only,
                     * 2 = walk-on-garbage (no fill), 3 = no scan/write-back */
#endif

#ifndef UA_TILE
#define UA_TILE 2048
#endif      /* merge-path elements per tile */
#define UA_BLOCK 256      /* threads per workgroup (aux kernels) */
#ifndef UA_TBLOCK
#define UA_TBLOCK 256     /* threads per TILE-kernel workgroup: smaller WGs on
                           * smaller tiles raise independent tiles per CU (the
                           * 16-blocks/CU cap) — the chip's own latency hiding,
                           * which measured better than every software pipeline */
#endif
#define UA_WPT (UA_TILE / UA_TBLOCK) /* path elements per thread */
#define UA_SMEMN (UA_TILE + 4) /* tile LDS: A|B + parity shifts + B lookahead */
#define UA_SCAN_CHUNK 2048
#define UA_STAGE_P 64 /* dense primary staging slots (u64/tile): tiles whose
                       * total emission fits go here (512 B apart -> DRAM
                       * row-local compaction reads) instead of the sparse
                       * stage_stride region (8-16 KB apart), which stays as
                       * the overflow path for dense-overlap tiles */
#define UA_PKW 4          /* packed-decode waves (blocks) per workgroup */
#define UA_MAX_BLOCK_UIDS 256
#define UA_MAX_DELTAS 1092 /* 64 groups x 17 B, padded */

static_assert(UA_TILE % UA_TBLOCK == 0, "tile must divide evenly over threads");
static_assert(UA_TILE / UA_TBLOCK >= 1 && UA_TILE / UA_TBLOCK <= 32,
              "emission flags are one u32 bit per path step per thread");
static_assert(UA_TBLOCK % 64 == 0 && UA_TBLOCK >= 64 && UA_TBLOCK <= 1024,
              "tile kernel is built from whole wavefronts");
#ifndef UA_FILL_NT
#define UA_FILL_NT 1 /* 1 = intersect's tile fill (LDS-DMA bodies, remainders,
                      * boundary elements: every input byte is read once per
                      * step and little is written) is issued non-temporal;
                      * 0 = default cache policy.  Union reads its inputs
                      * twice (COUNT, then WRITE), a merge tree reads what
                      * the round before wrote, and difference measured
                      * slower with it on dense tiles: their fills keep the
                      * default policy, and so do the split words, tile
                      * words, descs and all stores.  Measured:
                      * profiles/split_cache.md */
#endif

static_assert(UA_BLOCK == 256, "wave geometry (4 waves/WG) is hard-coded in "
                               "scan/compact/packed kernels");

/* ==================== device helpers ==================== */

__device__ __forceinline__ u64 d_lower_bound(const u64 *__restrict__ a, u64 n, u64 key) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        u64 mid = (lo + hi) >> 1;
        if (a[mid] >= key) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

/* merge-path split of one tile in LDS: #A consumed after `diag` merge steps,
 * A-priority on ties.  A and B sit at element offsets aoff/boff of smem
 * (E = u64, or u32 on a narrow tile: see k_narrow). */
template <typename E>
__device__ __forceinline__ int d_merge_path_tile(const E *smem, int aoff, int n,
                                                 int boff, int m, int diag) {
    int lo = diag > m ? diag - m : 0;
    int hi = diag < n ? diag : n;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (smem[aoff + mid] <= smem[boff + diag - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

/* one element of the tile fill, under the fill's cache policy */
template <bool NT>
__device__ __forceinline__ u64 d_fill_load(const u64 *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

/* No scan-3 pass: the flat exclusive scan stays split as (chunk-local offs,
 * chunk partials); every consumer computes the final offset with one extra
 * L2 load — saves a full read+write sweep of offs plus a launch. */
__device__ __forceinline__ u64 d_off(const u64 *__restrict__ offs,
                                     const u64 *__restrict__ partials, u64 x) {
    return offs[x] + partials[x / UA_SCAN_CHUNK];
}

/* ==================== batch descriptors ==================== */

struct alignas(16) UaDesc {
    const u64 *u;
    u64 n;
    const u64 *v;
    u64 m;
    u64 *out;
    u64 tile_base; /* index of this pair's first tile in the global tile array */
};

/* ==================== kernel: tile partition ==================== */

/* Two-level tile partition.  Phase 0: full-range diagonal search for every
 * 8th tile of each pair (and records tile->pair for all tiles).  Phase 1:
 * the other 7/8 of tiles search only inside the bracket their two coarse
 * neighbours pin (merge path is monotone), a <=16k-element window that lands
 * in L2 — ~8x less random HBM fetch than a flat per-tile search. */
#define UA_COARSE 8
__global__ __launch_bounds__(UA_BLOCK) void k_partition(
    const UaDesc *__restrict__ descs, const u64 *__restrict__ tb, int n_pairs,
    u64 total_tiles, u32 *__restrict__ tile_pair, u32 *__restrict__ tile_a0, int phase) {
    u64 t = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (t >= total_tiles) return;
    /* find pair p with tb[p] <= t < tb[p+1] */
    int lo = 0, hi = n_pairs - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (tb[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    int p = lo;
    u64 lt = t - tb[p];
    int is_coarse = ((lt & (UA_COARSE - 1)) == 0);
    if (phase == 0) {
        tile_pair[t] = (u32)p;
        if (!is_coarse) return;
    } else {
        if (is_coarse) return;
    }
    UaDesc d = descs[p];
    u64 path = d.n + d.m;
    u64 diag = lt * UA_TILE;
    if (diag > path) diag = path;
    u64 slo = (diag > d.m) ? diag - d.m : 0;
    u64 shi = diag < d.n ? diag : d.n;
    if (phase == 1) {
        u64 t_down = t - (lt & (UA_COARSE - 1));
        u64 bl = tile_a0[t_down];
        u64 t_up = t_down + UA_COARSE;
        u64 bh = (t_up < tb[p + 1]) ? (u64)tile_a0[t_up] : d.n;
        if (bl > slo) slo = bl;
        if (bh < shi) shi = bh;
    }
    while (slo < shi) {
        u64 mid = (slo + shi) >> 1;
        if (d.u[mid] <= d.v[diag - 1 - mid]) slo = mid + 1;
        else shi = mid;
    }
    tile_a0[t] = (u32)slo;
}

/* ==================== kernel: tile set-algebra ==================== */

enum { OP_INTERSECT = 0, OP_UNION = 1, OP_DIFF = 2, OP_MERGE_ALL = 3 };
enum { MODE_STAGE = 0, MODE_COUNT = 1, MODE_WRITE = 2, MODE_DIRECT = 3 };

/* block-wide exclusive scan of per-thread counts: wave __shfl scan + one
 * cross-wave combine — 1 barrier instead of Hillis-Steele's 17 */
template <int NB>
__device__ __forceinline__ void d_block_scan(int tid, u32 cnt, u32 *wsum,
                                             u32 &excl, u32 &total) {
    int lane = tid & 63, wv = tid >> 6;
    u32 incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u32 x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    u32 wbase = 0;
    u32 tot = 0;
#pragma unroll
    for (int w = 0; w < NB / 64; w++) {
        u32 s = wsum[w];
        if (w < wv) wbase += s;
        tot += s;
    }
    total = tot;
    excl = wbase + incl - cnt;
}

/* Branchless walk for union / merge-all, one pass over the thread's
 * merge-path segment.  An if/else walk is ~25% exec-mask control
 * (s_and_saveexec/s_or_b64/s_cbranch per step); this one keeps a 2-deep
 * frontier per side in registers and does ONE unconditional LDS gather per
 * step at a selected clamped address — no divergent branches in the loop
 * body.  As and Bs must live in the SAME LDS array (smem) so the refill
 * address can select between them.  aoff/boff are u64-element offsets of
 * As/Bs within smem.  Emissions are recorded in a statically-indexed
 * register array (em[s], flag bit s) so the walk runs ONCE: count + payload
 * together, no re-walk, no scratch spill (runtime-indexed local arrays go to
 * scratch; per-step static indices do not).
 *
 * UNION dedup: the reference's MergeSorted emits the merged stream with ALL
 * duplicates collapsed (uidlist.go:417: output==last skips), including
 * duplicates WITHIN one list (TestMergeSorted6/9/10).  Rule: emit iff value
 * != previous emitted value == previous merged-stream value.  A thread's
 * initial "previous" is max(last A before it, last B before it), using the
 * staged tile-boundary elements when its segment starts at a range head.
 *
 * VALUES = false is the COUNT-only walk: MODE_COUNT needs only the per-thread
 * emission count (union's first pass; intersect and difference never run a
 * count pass), so the em[] and flags bookkeeping is dropped (flags = 0, em
 * untouched).  The dedup state is the same code, so union counts match the
 * value walk exactly. */
template <int OP, bool VALUES, int W>
__device__ __forceinline__ int tile_walk2(const u64 *smembase, int aoff, int alen,
                                          int boff, int blen, u64 a_before, bool has_ab,
                                          u64 b_before, bool has_bb,
                                          bool has_bn, int s0, int s1, int i0,
                                          u64 (&em)[W], u32 &flags) {
    static_assert(OP == OP_UNION || OP == OP_MERGE_ALL,
                  "intersect/difference take tile_walk3x");
    int i = i0, j = s0 - i0;
    int cnt = 0;
    flags = 0;
    int steps = s1 - s0;
    int blen_ext = blen + (has_bn ? 1 : 0);
    int amax = alen > 0 ? alen - 1 : 0;
    int bmax = blen_ext > 0 ? blen_ext - 1 : 0;
    /* frontier: cur + next per side, clamped loads (garbage guarded by
     * i/j bound checks in the predicates) */
    u64 a = smembase[aoff + (i < alen ? i : amax)];
    u64 an = smembase[aoff + ((i + 1) < alen ? (i + 1) : amax)];
    u64 b = smembase[boff + (j < blen_ext ? j : bmax)];
    u64 bn = smembase[boff + ((j + 1) < blen_ext ? (j + 1) : bmax)];
    bool has_prev = false;
    u64 prev_out = 0;
    if (OP == OP_UNION) {
        u64 pa = (i > 0) ? smembase[aoff + i - 1] : a_before;
        bool hpa = (i > 0) || has_ab;
        u64 pb = (j > 0) ? smembase[boff + j - 1] : b_before;
        bool hpb = (j > 0) || has_bb;
        has_prev = hpa || hpb;
        prev_out = !hpa ? pb : (!hpb ? pa : (pa > pb ? pa : pb));
    }
#pragma unroll
    for (int s = 0; s < W; s++) {
        if (s >= steps) break;
        bool inA = i < alen, inB = j < blen;
        if (!inA && !inB) break;
        bool takeA = inA && (!inB || a <= b);
        u64 val = takeA ? a : b;
        bool emit;
        if (OP == OP_MERGE_ALL) { /* duplicate-keeping merge (sort runs) */
            emit = true;
        } else { /* UNION: emit iff != previous merged-stream value */
            emit = !has_prev || val != prev_out;
            prev_out = val;
            has_prev = true;
        }
        if constexpr (VALUES) {
            em[s] = val;
            flags |= ((u32)emit) << s;
        }
        cnt += emit;
        int ni = i + (takeA ? 1 : 0);
        int nj = j + (takeA ? 0 : 1);
        /* one refill: next lookahead of the consumed side */
        int ra = (ni + 1) < alen ? (ni + 1) : amax;
        int rb = (nj + 1) < blen_ext ? (nj + 1) : bmax;
        int raddr = takeA ? (aoff + ra) : (boff + rb);
        u64 r = smembase[raddr];
        a = takeA ? an : a;
        b = takeA ? b : bn;
        an = takeA ? r : an;
        bn = takeA ? bn : r;
        i = ni;
        j = nj;
    }
    return cnt;
}

/* INTERSECT/DIFF walk with NO value array: emissions are always A-values,
 * so instead of maintaining em[W] (whose per-step conditional writes and
 * register shuffling dominate the issue-bound walk loop), track a takeA
 * bitmask and reconstruct the few matched values from LDS after the scan:
 * A-index at step s = i0 + popcount(mask below s).  ~0.04 matches/thread on
 * the 1%-overlap headline shape.
 * Dual chain: two independent 4-step gather chains per thread (halved serial
 * LDS latency), one mask each.  Viable because the prepared batch caches
 * BOTH splits (i0 at s0, i0b at smid) — round 1 rejected a dual-chain em[]
 * walk precisely because its second diagonal search cost more than the added
 * MLP recovered.
 * E is the LDS element type: u64, or u32 on a narrow tile, whose elements all
 * share their high 32 bits so that the unsigned 32-bit compares of the low
 * halves order and match exactly as the 64-bit ones do (see k_narrow). */
template <int OP, int W, typename E>
__device__ __forceinline__ int tile_walk3x(const E *smembase, int aoff, int alen,
                                           int boff, int blen, bool has_bn,
                                           int s0, int smid, int s1, int i0a,
                                           int i0b, u32 &flags, u32 &amA, u32 &amB) {
    static_assert(W <= 32, "masks are u32");
    constexpr int H = W / 2;
    int blen_ext = blen + (has_bn ? 1 : 0);
    int amax = alen > 0 ? alen - 1 : 0;
    int bmax = blen_ext > 0 ? blen_ext - 1 : 0;
    int ia = i0a, ja = s0 - i0a;
    int ib = i0b, jb = smid - i0b;
    int stepsA = smid - s0, stepsB = s1 - smid;
    E aA = smembase[aoff + (ia < alen ? ia : amax)];
    E bA = smembase[boff + (ja < blen_ext ? ja : bmax)];
    E aB = smembase[aoff + (ib < alen ? ib : amax)];
    E bB = smembase[boff + (jb < blen_ext ? jb : bmax)];
    int cnt = 0;
    flags = 0;
    amA = 0;
    amB = 0;
    /* One merge step of one chain: its frontier (a, b) at (i, j), its takeA
     * mask, and where its emission bits start in flags.  The form is load-
     * bearing: the tile's constants are captured by value and the chain's
     * state is copied to locals before the test, so that the step is
     * simplified on plain values before it is inlined, as the spelled-out
     * step was.  With by-reference captures, or with the test reading i and j
     * through their references, the same source compiles to a longer loop
     * (profiles/tile_refactor.md). */
    auto step = [=, &flags, &cnt](int q, int steps, E &a, E &b, int &i, int &j, u32 &mask,
                                  int fshift) __attribute__((always_inline)) {
        const int ci = i, cj = j;
        const E ca = a, cb = b;
        if (q < steps && (ci < alen || cj < blen)) {
            bool inA = ci < alen, inB = cj < blen;
            bool takeA = inA && (!inB || ca <= cb);
            bool eq = (ca == cb) && (cj < blen_ext);
            bool emit = (OP == OP_INTERSECT) ? (takeA && eq) : (takeA && !eq);
            flags |= ((u32)emit) << (fshift + q);
            mask |= ((u32)takeA) << q;
            cnt += emit;
            int ni = ci + (takeA ? 1 : 0), nj = cj + (takeA ? 0 : 1);
            int raddr = takeA ? (aoff + (ni < alen ? ni : amax))
                              : (boff + (nj < blen_ext ? nj : bmax));
            E r = smembase[raddr];
            a = takeA ? r : ca;
            b = takeA ? cb : r;
            i = ni;
            j = nj;
        }
    };
    /* A's step, then B's: the two gather chains stay interleaved */
#pragma unroll
    for (int q = 0; q < H; q++) {
        step(q, stepsA, aA, bA, ia, ja, amA, 0);
        step(q, stepsB, aB, bB, ib, jb, amB, H);
    }
    return cnt;
}

/* The same walk over a FAST narrow tile (see k_narrow): L is the tile's
 * record in LDS, A at 0 and B at boff, each range closed by a sentinel, and
 * the tile is full, so that every chain walks W / 2 steps and no step tests a
 * range, clamps an index or masks itself off.  A step compares, sets its flag
 * and mask bits, advances the taken side and reads that side's next element;
 * the last step of a chain reads nothing.  flags, amA and amB are
 * tile_walk3x's, bit for bit. */
template <int OP, int W>
__device__ __forceinline__ int tile_walk3x_fast(const u32 *L, int boff, int s0, int i0a,
                                                int i0b, u32 &flags, u32 &amA, u32 &amB) {
    static_assert(W <= 32 && W % 2 == 0, "masks are u32; two equal chains");
    static_assert(OP == OP_INTERSECT || OP == OP_DIFF, "A-only ops");
    constexpr int H = W / 2;
    int ia = i0a, ja = boff + s0 - i0a; /* j counts from L, not from boff */
    int ib = i0b, jb = boff + s0 + H - i0b;
    u32 aA = L[ia], bA = L[ja];
    u32 aB = L[ib], bB = L[jb];
    u32 f = 0, mA = 0, mB = 0;
    auto step = [&](int q, u32 &a, u32 &b, int &i, int &j, u32 &mask, int fshift)
                    __attribute__((always_inline)) {
        const bool t = a <= b;
        const bool emit = (OP == OP_INTERSECT) ? (a == b) : (a < b);
        f |= ((u32)emit) << (fshift + q);
        mask |= ((u32)t) << q;
        if (q + 1 < H) {
            i += t ? 1 : 0;
            j += t ? 0 : 1;
            u32 r = L[t ? i : j];
            a = t ? r : a;
            b = t ? b : r;
        }
    };
#pragma unroll
    for (int q = 0; q < H; q++) {
        step(q, aA, bA, ia, ja, mA, 0);
        step(q, aB, bB, ib, jb, mB, H);
    }
    flags = f;
    amA = mA;
    amB = mB;
    return __popc(f);
}

/* MODE_STAGE: where a thread's emissions go (dst) and how many of them fit
 * (lim).  Clamped to the staging stride: invalid (duplicate/unsorted) inputs
 * can emit more than stride entries per tile; results there are unspecified,
 * OOB writes are not.  Small totals go to the dense primary
 * region; stage_stride stays the sparse overflow. */
__device__ __forceinline__ u64 *d_stage_dst(u64 t, int tid, u32 cnt, u32 excl, u32 total,
                                            u64 *__restrict__ staging, u64 stage_stride,
                                            const u64 *__restrict__ primary,
                                            u32 *__restrict__ tile_cnt, u32 &lim) {
    bool prim = (primary != nullptr) && (total <= UA_STAGE_P);
    u32 cap_t = prim ? (u32)UA_STAGE_P : (u32)stage_stride;
    u32 c0 = excl < cap_t ? cap_t - excl : 0;
    lim = cnt < c0 ? cnt : c0;
    u64 *dst = prim ? ((u64 *)primary + t * UA_STAGE_P) : (staging + t * stage_stride + excl);
    if (prim) dst += excl;
    if (tid == 0) tile_cnt[t] = total < (u32)stage_stride ? total : (u32)stage_stride;
    return dst;
}

/* The consumer side of the same rule: where the compactors (k_compact_small,
 * k_compact, k_tail_fused) find the cnt = tile_cnt[t] values that
 * d_stage_dst placed for tile t.  prim is the dense primary region, or null
 * when the batch has none. */
__device__ __forceinline__ const u64 *d_stage_src(u64 t, u32 cnt,
                                                  const u64 *__restrict__ staging,
                                                  u64 stage_stride,
                                                  const u64 *__restrict__ prim) {
    return (prim && cnt <= (u32)UA_STAGE_P) ? prim + t * UA_STAGE_P
                                            : staging + t * stage_stride;
}

/* A pair's output capacity: the most a valid pair can emit, and so the size
 * its out buffer is promised to have.  Every compactor clamps to it: invalid
 * (duplicate/unsorted) inputs can emit more and must stay memory-safe, like
 * the reference. */
__device__ __forceinline__ u64 d_pair_cap(const UaDesc &d, int op) {
    return (op == OP_INTERSECT) ? (d.n < d.m ? d.n : d.m)
           : (op == OP_DIFF)    ? d.n
                                : (d.n + d.m);
}

/* ==================== tile geometry, splits, write-back ====================
 * One copy of what k_narrow (which builds a tile's record), tile_narrow and
 * tile_wide (which walk it) and the split cache (producer and consumer) have
 * to agree on bit for bit. */

/* A tile's ranges: A = d.u[a0, a0 + alen), B = d.v[b0, b1) with blen = b1 - b0,
 * from merge-path diagonal d0.  has_bn: B's lookahead d.v[b1] exists.  t/tn,
 * p/pn, a0/a0n are the tile's and its (clamped) neighbour's index, pair and
 * partition word: the A range ends where the next tile of the same pair
 * starts, else at the list's end. */
struct UaTileGeom {
    u64 d0;
    u32 b0, b1;
    int alen, blen;
    bool has_bn;
};

__device__ __forceinline__ UaTileGeom d_tile_geom(const UaDesc &d, u64 t, u64 tn, u32 p,
                                                  u32 pn, u32 a0, u32 a0n) {
    UaTileGeom g;
    u64 lt = t - d.tile_base;
    u64 path = d.n + d.m;
    g.d0 = lt * UA_TILE;
    if (g.d0 > path) g.d0 = path; /* capacity-tiled batches can overshoot the path */
    u64 d1 = g.d0 + UA_TILE;
    if (d1 > path) d1 = path;
    u32 a1 = (tn != t && pn == p) ? a0n : (u32)d.n;
    g.b0 = (u32)(g.d0 - a0);
    g.b1 = (u32)(d1 - a1);
    g.alen = (int)(a1 - a0);
    g.blen = (int)(g.b1 - g.b0);
    g.has_bn = ((u64)g.b1 < d.m);
    return g;
}

/* A thread's merge-path segment [s0, s1) of the tile, cut at smid into the
 * two chains of tile_walk3x; all three clamped to the tile's length. */
struct UaSeg {
    int s0, smid, s1;
};

__device__ __forceinline__ UaSeg d_thread_seg(int tid, int tilelen) {
    UaSeg sg;
    sg.s0 = tid * UA_WPT;
    sg.s1 = sg.s0 + UA_WPT;
    if (sg.s0 > tilelen) sg.s0 = tilelen;
    if (sg.s1 > tilelen) sg.s1 = tilelen;
    sg.smid = sg.s0 + UA_WPT / 2;
    if (sg.smid > tilelen) sg.smid = tilelen;
    if (sg.smid < sg.s0) sg.smid = sg.s0;
    if (sg.smid > sg.s1) sg.smid = sg.s1;
    return sg;
}

/* The thread's splits: i0 = #A consumed at diagonal s0, i0b at smid.  From the
 * cached word split_w when the batch has one (PACKED lo16 = i0, hi16 = i0b),
 * else by two searches of the tile in LDS; stored in the same format when
 * isplit_out is set.  Called below the fill's barrier: the opaque pin here is
 * the first use of split_w, which was the tile's first vector load, so that no
 * wait stands between that load and the fill behind it. */
struct UaSplit {
    int i0, i0b;
};

template <typename E>
__device__ __forceinline__ UaSplit d_resolve_splits(const E *lds, int aoff, int alen, int boff,
                                                    int blen, UaSeg sg, bool have_split,
                                                    u32 split_w, u32 *__restrict__ isplit_out,
                                                    u64 t, int tid) {
    UaSplit sp;
    if (have_split) {
        asm volatile("" : "+v"(split_w));
        sp.i0 = (int)(split_w & 0xffffu);
        sp.i0b = (int)(split_w >> 16);
    } else {
        sp.i0 = d_merge_path_tile(lds, aoff, alen, boff, blen, sg.s0);
        sp.i0b = d_merge_path_tile(lds, aoff, alen, boff, blen, sg.smid);
    }
    if (isplit_out) isplit_out[t * UA_TBLOCK + tid] = (u32)sp.i0 | ((u32)sp.i0b << 16);
    return sp;
}

/* Write-back of tile_walk3x: the emitted A-values are rebuilt from the
 * per-chain takeA masks (A-index at step s = the chain's split + popcount of
 * its mask below s) and read from As, the tile's A range in LDS; at most lim
 * of them go to dst.  A narrow tile (E = u32) gets its common high half hi64
 * back on the way; the 64-bit path has no OR. */
template <typename E>
__device__ __forceinline__ void d_write_a_only(const E *As, u32 flags, u32 amA, u32 amB,
                                               UaSplit sp, u32 lim, u64 *dst, u64 hi64) {
    constexpr int H = UA_WPT / 2;
    u32 f = flags;
    u32 k = 0;
    while (f && k < lim) {
        int s = __builtin_ctz(f);
        f &= f - 1;
        int idx = (s < H) ? sp.i0 + __popc(amA & ((1u << s) - 1))
                          : sp.i0b + __popc(amB & ((1u << (s - H)) - 1));
        if constexpr (sizeof(E) == 8) dst[k++] = As[idx];
        else dst[k++] = hi64 | As[idx];
    }
}

/* ==================== narrow tiles (prepared batches) ====================
 * A prepared batch promises that its pairs' device contents do not change
 * while it lives.  On that promise it keeps, beside the tile partition and
 * the per-thread splits, a 32-bit tile-major copy of its inputs: one record
 * per tile, UA_NREC_W u32 at a fixed 16-byte-aligned stride.  A record holds
 * a logical array L of alen + blen + 2 words, each range closed by a sentinel:
 *
 *   L[0, alen)                   low halves of the tile's A range
 *   L[alen]                      sa = 0xFFFFFFFF
 *   L[alen + 1, alen + 1 + blen) low halves of its B range
 *   L[alen + 1 + blen]           sb = low half of B's lookahead d.v[b1] when
 *                                there is one (has_bn), else 0xFFFFFFFF
 *
 * L[0, UA_TILE) are the record's first UA_TILE words (whatever L leaves of
 * them is unused: anything), and its 4-word tail is
 *
 *   the tile's common high half | L[UA_TILE] | L[UA_TILE + 1] | fast
 *
 * with 0 where L is shorter.  In LDS the tile is L itself: A at aoff = 0, B at
 * boff = alen + 1, so that sb is B's element blen, where the guarded walk has
 * always looked for the lookahead.
 *
 * A tile is NARROW iff every element of its A range, of its B range and its
 * lookahead element share one value of x >> 32; k_narrow decides that from
 * the data, per tile.  Inside such a tile the unsigned compare of two low
 * halves equals the 64-bit compare, so the walk over the record gives the
 * wide walk's flags, masks and splits bit for bit, on invalid inputs too.
 * Every other tile keeps the 64-bit fill and walk.  The record's address
 * depends on the tile index alone, its source needs no alignment work, and a
 * step reads 4 B per input element instead of 8.
 *
 * A narrow tile is FAST (the tail's fast word is 1) iff also
 *   (c0) alen + blen == UA_TILE: every thread walks UA_WPT steps;
 *   (c1) no low half of its A or B range is 0xFFFFFFFF;
 *   (c2) there is no lookahead, or every A element of the tile is <= it
 *        (always so on sorted input).
 * Such a tile takes tile_walk3x_fast, which tests no range: the sentinels end
 * the ranges by value.  Its splits obey 0 <= i0 <= alen and
 * 0 <= s - i0 <= blen (d_merge_path_tile), and i + j < UA_TILE at every step.
 * So i == alen forces j < blen, where a = sa is above every b by c1: B is
 * taken and nothing is emitted, as in the guarded walk.  And j == blen forces
 * i < alen, where a <= sb by c2, or because sb is the maximum and, by c1, a is
 * not: A is taken, and it emits on a == sb only where sb is the lookahead, as
 * in the guarded walk.  No read therefore passes L[alen] on A's side or
 * L[alen + 1 + blen] on B's, and flags and masks are the guarded walk's on
 * every input.  (Memory safety does not rest on this: a chain advances three
 * times from its split, which keeps any index inside the tile LDS.)  Partial
 * tiles and tiles that miss c1 or c2 keep the guarded walk on the same
 * record; the lookahead itself may be 0xFFFFFFFF. */
#define UA_NREC_W (UA_TILE + 4) /* u32 per record: L[0, UA_TILE) + tail */
#define UA_NARROW_BIT 0x80000000u /* in a batch-private tile-pair word; pair
                                   * indices are < 2^31 (n_pairs is an int) */
#define UA_NROUNDS ((UA_TILE * 4) / (UA_TBLOCK * 16)) /* LDS-DMA rounds per record */
static_assert((UA_TILE * 4) % (UA_TBLOCK * 16) == 0 && UA_NROUNDS >= 1,
              "a record's data is whole rounds of 16 B per lane");
static_assert((UA_NREC_W * 4) % 16 == 0, "records stay 16-byte aligned");
static_assert((UA_TILE + 2 + UA_WPT / 2) * 4 <= UA_SMEMN * 8,
              "narrow tile + both sentinels fit the tile LDS, and so does any "
              "index the fast walk can form");

typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));

/* Builds the records and votes each tile's eligibility: one workgroup per
 * tile, list pointers at any 8-byte parity.  tile_pair_n[t] = tile_pair[t],
 * with UA_NARROW_BIT set on a narrow tile.  Every load of the tile is in
 * flight at once; thread 0, which holds the tile's first element and the
 * lookahead, publishes the reference high half and the lookahead's low half
 * through LDS and writes the two sentinels.  L[UA_TILE] and L[UA_TILE + 1]
 * belong to the tail, which thread 0 stores: whoever holds one of them hands
 * it over through LDS.  A tile whose partition words do not describe a sane
 * range (possible only on unsorted input) stays wide and is not copied. */
__global__ __launch_bounds__(UA_TBLOCK) void k_narrow(
    const UaDesc *__restrict__ descs, const u32 *__restrict__ tile_pair,
    const u32 *__restrict__ tile_a0, u64 total_tiles, u32 *__restrict__ slab,
    u32 *__restrict__ tile_pair_n) {
    __shared__ u32 sh_hi, sh_look;
    __shared__ u32 sh_tail[2]; /* L[UA_TILE], L[UA_TILE + 1] */
    __shared__ u32 sh_bad;     /* the vote: the OR of every thread's bad bits */
    u64 t = blockIdx.x;
    int tid = threadIdx.x;
    u64 tn = (t + 1 < total_tiles) ? t + 1 : t;
    u32 p = tile_pair[t];
    u32 pn = tile_pair[tn];
    u32 a0 = tile_a0[t];
    u32 a0n = tile_a0[tn];
    UaDesc d = descs[p];
    const UaTileGeom g = d_tile_geom(d, t, tn, p, pn, a0, a0n);
    const u32 b0 = g.b0, b1 = g.b1;
    const int alen = g.alen, blen = g.blen;
    const bool has_bn = g.has_bn;
    bool sane = alen >= 0 && blen >= 0 && alen + blen >= 1 && alen + blen <= UA_TILE &&
                (u64)a0 + (u64)alen <= d.n && (u64)b0 + (u64)blen <= d.m;
    u32 *rec = slab + t * UA_NREC_W;
    u32 hi = 0;
    int bad = sane ? 0 : 3; /* bit 0: not narrow; bit 1: misses c1 or c2 */
    if (sane) { /* workgroup-uniform */
        int tilelen = alen + blen;
        /* unconditional loads at clamped indices (a thread past the tile's
         * end re-reads its last element), so that all are issued before any
         * is waited for; thread 0 adds the lookahead */
        const u64 *ua = d.u + a0;
        const u64 *vb = d.v + b0;
        u64 x[UA_WPT];
#pragma unroll
        for (int k = 0; k < UA_WPT; k++) {
            int e = k * UA_TBLOCK + tid;
            if (e > tilelen - 1) e = tilelen - 1;
            const u64 *src = (e < alen) ? ua + e : vb + (e - alen);
            x[k] = *src;
        }
        u64 look = 0;
        if (tid == 0 && has_bn) look = d.v[b1];
        if (tid == 0) {
            sh_hi = (u32)(x[0] >> 32); /* element 0 exists: tilelen >= 1 */
            sh_look = (u32)look;
            sh_tail[0] = 0;
            sh_tail[1] = 0;
            sh_bad = 0;
        }
        __syncthreads();
        hi = sh_hi;
        const u32 look_lo = sh_look;
#pragma unroll
        for (int k = 0; k < UA_WPT; k++) {
            /* branch-free: element e goes to L[e + (e >= alen)], past sa; a
             * thread past the tile's end stores its clamped element again.
             * Only element UA_TILE - 1 of a full tile can land on L[UA_TILE] */
            int e = k * UA_TBLOCK + tid;
            if (e > tilelen - 1) e = tilelen - 1;
            u32 lo = (u32)x[k];
            bad |= ((u32)(x[k] >> 32) != hi) ? 1 : 0;
            bad |= (lo == 0xFFFFFFFFu || (has_bn && e < alen && lo > look_lo)) ? 2 : 0;
            int dst = e + (e >= alen ? 1 : 0);
            if (dst < UA_TILE) rec[dst] = lo;
            else sh_tail[0] = lo;
        }
        if (tid == 0) {
            if (has_bn) bad |= ((u32)(look >> 32) != hi) ? 1 : 0;
            const u32 sb = has_bn ? look_lo : 0xFFFFFFFFu;
            int isb = alen + 1 + blen; /* <= UA_TILE + 1 */
            if (alen < UA_TILE) rec[alen] = 0xFFFFFFFFu;
            else sh_tail[0] = 0xFFFFFFFFu;
            if (isb < UA_TILE) rec[isb] = sb;
            else sh_tail[isb - UA_TILE] = sb;
        }
        if (bad) atomicOr(&sh_bad, (u32)bad); /* rare: most tiles vote nothing */
    }
    __syncthreads();
    if (sane) bad = (int)sh_bad;
    if (tid == 0) {
        const bool narrow = !(bad & 1);
        const bool fast = (bad == 0) && (alen + blen == UA_TILE);
        rec[UA_TILE + 0] = hi;
        rec[UA_TILE + 1] = sane ? sh_tail[0] : 0u;
        rec[UA_TILE + 2] = sane ? sh_tail[1] : 0u;
        rec[UA_TILE + 3] = fast ? 1u : 0u;
        tile_pair_n[t] = p | (narrow ? UA_NARROW_BIT : 0u);
    }
}

/* tile LDS + two boundary slots (union's a_before / b_before) */
constexpr int UA_SLOT_AB = UA_SMEMN, UA_SLOT_BB = UA_SMEMN + 1;
constexpr int UA_TILE_LDS = UA_SMEMN + 2; /* u64 */

/* the fill's cache policy (see UA_FILL_NT) */
constexpr bool d_fill_nt(int op) { return (UA_FILL_NT != 0) && (op == OP_INTERSECT); }

/* perf-bisection builds (UA_ABLATE): the stages they cut, named once */
constexpr bool UA_DO_FILL = (UA_ABLATE != 2);
constexpr bool UA_DO_WALK = (UA_ABLATE != 1);
constexpr bool UA_DO_EMIT = (UA_ABLATE != 3);

/* Everything behind the fill's barrier, for both tile bodies: the thread's
 * segment and splits, the walk, the block scan and the write-back.  lds holds
 * the tile as E (u64, or u32 on a narrow tile): A at aoff, B at boff with its
 * lookahead as element blen when has_bn, and for union the two boundary
 * slots.  hi64 is a narrow tile's common high half (unused when E = u64);
 * fast (workgroup-uniform) sends a narrow tile through tile_walk3x_fast. */
template <int OP, int MODE, typename E>
__device__ __forceinline__ void tile_finish(
    const E *lds, int aoff, int alen, int boff, int blen, bool has_ab, bool has_bb,
    bool has_bn, u64 hi64, const UaDesc &d, u64 d0, u64 t, u32 *scan,
    u64 *__restrict__ staging, u64 stage_stride, u32 *__restrict__ tile_cnt,
    const u64 *__restrict__ offs, const u64 *__restrict__ partials, bool have_split,
    u32 split_w, u32 *__restrict__ isplit_out, bool fast) {
    /* intersect/difference emit A-values only: maskless walk, values rebuilt
     * from LDS at write-back; union/merge-all carry them in em[] */
    constexpr bool A_ONLY = (OP == OP_INTERSECT || OP == OP_DIFF);
    int tid = threadIdx.x;
    u64 em[UA_WPT];
    u32 flags = 0;
    u32 amA = 0, amB = 0; /* walk3x: per-chain takeA bits for reconstruction */
    UaSplit sp = {0, 0};
    int cnt = 0;
    if constexpr (!UA_DO_WALK) { /* fill-only: keep the loads live, skip search+walk */
        E ablate_x = lds[aoff + tid] + lds[boff + (tid & 127)];
        asm volatile("" ::"v"(ablate_x));
    } else {
        UaSeg sg = d_thread_seg(tid, alen + blen);
        sp = d_resolve_splits(lds, aoff, alen, boff, blen, sg, have_split, split_w,
                              isplit_out, t, tid);
        if constexpr (A_ONLY) {
            bool walked = false;
            if constexpr (sizeof(E) == 4) {
                if (fast) { /* workgroup-uniform; a full tile: s0 = tid * UA_WPT */
                    cnt = tile_walk3x_fast<OP, UA_WPT>(lds, boff, tid * UA_WPT, sp.i0, sp.i0b,
                                                       flags, amA, amB);
                    walked = true;
                }
            }
            if (!walked)
                cnt = tile_walk3x<OP, UA_WPT>(lds, aoff, alen, boff, blen, has_bn, sg.s0,
                                              sg.smid, sg.s1, sp.i0, sp.i0b, flags, amA, amB);
        } else {
            u64 a_before = 0, b_before = 0;
            if constexpr (OP == OP_UNION) {
                a_before = lds[UA_SLOT_AB];
                b_before = lds[UA_SLOT_BB];
            }
            /* the count pass needs no values — no em[] bookkeeping */
            cnt = tile_walk2<OP, MODE != MODE_COUNT>(lds, aoff, alen, boff, blen, a_before,
                                                     has_ab, b_before, has_bb, has_bn, sg.s0,
                                                     sg.s1, sp.i0, em, flags);
        }
        if constexpr (MODE == MODE_DIRECT) {
            /* OP_MERGE_ALL: every path element emits, so the output position
             * IS the path position — no scan, no staging, no compaction */
            u64 *dst = d.out + d0 + (u64)sg.s0;
            int steps = sg.s1 - sg.s0;
#pragma unroll
            for (int s = 0; s < UA_WPT; s++) {
                if (s < steps) dst[s] = em[s];
            }
            return;
        }
    }
    if constexpr (!UA_DO_EMIT) { /* fill+walk, skip scan/write-back */
        asm volatile("" ::"v"(cnt), "v"(flags));
        cnt = 0;
        flags = 0;
    }

    u32 excl, total;
    d_block_scan<UA_TBLOCK>(tid, (u32)cnt, scan, excl, total);

    if (MODE == MODE_COUNT) {
        if (tid == 0) tile_cnt[t] = total;
        return;
    }
    u64 *dst;
    u32 lim = (u32)cnt;
    if (MODE == MODE_STAGE) {
        /* offs = the dense primary region's base, see enqueue_tiles */
        dst = d_stage_dst(t, tid, (u32)cnt, excl, total, staging, stage_stride, offs,
                          tile_cnt, lim);
    } else { /* MODE_WRITE: (offs, partials) is the split flat scan */
        dst = d.out +
              (d_off(offs, partials, t) - d_off(offs, partials, d.tile_base)) + excl;
    }
    if (cnt > 0) {
        if constexpr (A_ONLY) {
            d_write_a_only(lds + aoff, flags, amA, amB, sp, lim, dst, hi64);
        } else {
            u32 k = 0;
#pragma unroll
            for (int s = 0; s < UA_WPT; s++) {
                if (flags & (1u << s)) {
                    if (k < lim) dst[k] = em[s];
                    k++;
                }
            }
        }
    }
}

/* One narrow tile of k_tiles<OP_INTERSECT | OP_DIFF, MODE_STAGE>: the record
 * goes to LDS by LDS-DMA as soon as t is known (its address needs no
 * descriptor), descs[p] arrives behind it, and the walk runs on u32: the
 * sentinel walk when the record's tail says the tile is fast, else the guarded
 * one.  Masks, the cached split format, the scan and the staging are the wide
 * path's (tile_finish); emitted A-values get the tile's high half back on the
 * way to staging. */
template <int OP>
__device__ __forceinline__ void tile_narrow(
    const UaDesc *__restrict__ descs, u32 p, u32 pn, u32 a0, u32 a0n, u64 t, u64 tn,
    const u32 *__restrict__ slab, u64 *smem, u32 *scan, u64 *__restrict__ staging,
    u64 stage_stride, u32 *__restrict__ tile_cnt, const u64 *__restrict__ primary,
    const u32 *__restrict__ isplit_in, u32 *__restrict__ isplit_out) {
    constexpr bool FILL_NT = d_fill_nt(OP);
    constexpr int FILL_AUX = FILL_NT ? 2 : 0; /* 2 = nt for global_load_lds */
    int tid = threadIdx.x;
    /* cached splits: still the first vector load, opaque until the barrier */
    const bool have_split = (isplit_in != nullptr);
    u32 split_w = 0;
    if (have_split) split_w = isplit_in[t * UA_TBLOCK + tid];
    u32 *s32 = (u32 *)smem;
    const u32 *rec = slab + t * UA_NREC_W;
    u32x4 tl = {0, 0, 0, 0}; /* the record's tail: high half, L[UA_TILE], L[UA_TILE + 1], fast */
    if constexpr (UA_DO_FILL) {
        int wv4 = tid >> 6, lane = tid & 63;
#pragma unroll
        for (int r = 0; r < UA_NROUNDS; r++) {
            int w = (r * (UA_TBLOCK / 64) + wv4) * 256; /* 64 lanes x 16 B = 256 u32 */
            __builtin_amdgcn_global_load_lds(rec + w + lane * 4, s32 + w, 16, 0, FILL_AUX);
        }
        /* the tail, to registers; the opaque zero keeps it a vector load,
         * in order behind the fill and drained with it */
        int z = 0;
        asm volatile("" : "+v"(z));
        const u32x4 *tp = (const u32x4 *)(rec + UA_TILE) + z;
        if constexpr (FILL_NT) tl = __builtin_nontemporal_load(tp);
        else tl = *tp;
    }
    UaDesc d = descs[p];
    const UaTileGeom g = d_tile_geom(d, t, tn, p, pn, a0, a0n);
    constexpr int aoff = 0;
    int boff = g.alen + 1; /* past sa */
    bool fast;
    if constexpr (UA_DO_FILL) {
        /* the one drain (see the wide fill); all four tail words pass through
         * it, so no register of the load is reused, and waited for, earlier */
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(tl)::"memory");
        /* the two words of L behind the DMA part, in one 8-byte LDS store */
        if (tid == 0) *(u32x2 *)(s32 + UA_TILE) = (u32x2){tl.y, tl.z};
        fast = __builtin_amdgcn_readfirstlane(tl.w) != 0; /* uniform: a scalar branch */
    } else {
        fast = (g.alen + g.blen == UA_TILE); /* no record was read: walk what it would hold */
    }
    const u64 hi64 = (u64)tl.x << 32;
    __syncthreads();
    tile_finish<OP, MODE_STAGE>(s32, aoff, g.alen, boff, g.blen, false, false, g.has_bn, hi64,
                                d, g.d0, t, scan, staging, stage_stride, tile_cnt, primary,
                                nullptr, have_split, split_w, isplit_out, fast);
}

/* One 64-bit tile of k_tiles: every op and mode, and every tile that is not
 * narrow. */
template <int OP, int MODE>
__device__ __forceinline__ void tile_wide(
    const UaDesc *__restrict__ descs, u32 p, u32 pn, u32 a0, u32 a0n, u64 t, u64 tn,
    u64 *smem, u32 *scan, u64 *__restrict__ staging, u64 stage_stride,
    u32 *__restrict__ tile_cnt, const u64 *__restrict__ offs,
    const u64 *__restrict__ partials, const u32 *__restrict__ isplit_in,
    u32 *__restrict__ isplit_out) {
    constexpr bool FILL_NT = d_fill_nt(OP);
    constexpr int FILL_AUX = FILL_NT ? 2 : 0; /* 2 = nt for global_load_lds */
    int tid = threadIdx.x;
    UaDesc d = descs[p];
    const UaTileGeom tg = d_tile_geom(d, t, tn, p, pn, a0, a0n);
    const u32 b0 = tg.b0;
    const int alen = tg.alen, blen = tg.blen;
    /* cached splits: the first vector load of the tile.  The word stays
     * opaque (d_resolve_splits pins it below the barrier) so that no wait
     * stands between this load and the fill behind it */
    const bool have_split = (isplit_in != nullptr);
    u32 split_w = 0;
    if (have_split) split_w = isplit_in[t * UA_TBLOCK + tid];

    /* The fill is global_load_lds (LDS-DMA): +13% over a 16B register-staged
     * fill (4.03 vs 3.58 TB/s on cfg2).  LDS bases are chosen so each side's
     * 16B-aligned glds body lines up with its source POINTER parity (glds
     * writes wave-uniform base + lane*16; list base pointers are not always
     * 16B aligned — merge-tree runs and sliced outputs sit at odd u64
     * offsets) */
    int ashift = (int)((((uintptr_t)(d.u + a0)) >> 3) & 1);
    int bshift = (int)((((uintptr_t)(d.v + b0)) >> 3) & 1);
    u64 *As = smem + ashift;
    int boff_base = ((ashift + alen + 1) & ~1) + bshift;
    u64 *Bs = smem + boff_base;
    int aoff = (int)(As - smem);
    int boff = (int)(Bs - smem);

    bool has_ab = (a0 > 0);
    bool has_bb = (b0 > 0);
    bool has_bn = tg.has_bn;
    if constexpr (UA_ABLATE == 5) { /* meta + dispatch floor: no fill, no walk, no scan */
        if (tid == 0) tile_cnt[t] = (u32)((a0 ^ (u32)d.m) & 1u);
        return;
    }
    if constexpr (UA_DO_FILL) {
        /* Issue everything, wait once.  Per-wave LDS-DMA bodies (128 u64 per
         * wave-call: 64 lanes x 16 B) for A and B, then each side's
         * remainder (< 128 elements: one predicated load per thread) and the
         * boundary elements go to REGISTERS; nothing is waited on until the
         * single drain below, after which the registers are written to LDS.
         * A load->wait->ds_write loop here would drain A's LDS-DMA before
         * B's first load is issued (vmcnt completes in order). */
        static_assert(UA_TBLOCK >= 128, "one remainder element per thread per side");
        int wv4 = tid >> 6, lane = tid & 63;
        int ahead = ashift; /* elements before the aligned body (0 or 1) */
        if (ahead > alen) ahead = alen;
        int abody = (alen - ahead) & ~127;
        for (int e = wv4 * 128; e < abody; e += (UA_TBLOCK / 64) * 128) {
            const u64 *g = d.u + a0 + ahead + e + lane * 2;
            __builtin_amdgcn_global_load_lds((const u32 *)g,
                                             (u32 *)&smem[ashift + ahead + e], 16, 0,
                                             FILL_AUX);
        }
        int bhead = bshift;
        if (bhead > blen) bhead = blen;
        int bbody = (blen - bhead) & ~127;
        for (int e = wv4 * 128; e < bbody; e += (UA_TBLOCK / 64) * 128) {
            const u64 *g = d.v + b0 + bhead + e + lane * 2;
            __builtin_amdgcn_global_load_lds((const u32 *)g,
                                             (u32 *)&smem[boff_base + bhead + e], 16, 0,
                                             FILL_AUX);
        }
        /* remainders; B's carries the lookahead element d.v[b1] as element
         * blen when has_bn (else that slot gets 0 and d.v[m] is not read) */
        int ia = ahead + abody + tid;
        int ib = bhead + bbody + tid;
        u64 ra = 0, rb = 0;
        if (ia < alen) ra = d_fill_load<FILL_NT>(d.u + a0 + ia);
        if (ib < blen + (has_bn ? 1 : 0)) rb = d_fill_load<FILL_NT>(d.v + b0 + ib);
        /* boundary elements, one lane each: the two parity heads, and for
         * union the elements just before the tile (dedup state; no other op
         * reads them) */
        const u64 *xsrc = nullptr;
        int xslot = -1;
        if (tid == 0) {
            if (ahead) { xsrc = d.u + a0; xslot = aoff; }
        } else if (tid == 1) {
            if (bhead) { xsrc = d.v + b0; xslot = boff; }
        } else if (OP == OP_UNION && tid == 2) {
            xslot = UA_SLOT_AB;
            if (has_ab) xsrc = d.u + a0 - 1;
        } else if (OP == OP_UNION && tid == 3) {
            xslot = UA_SLOT_BB;
            if (has_bb) xsrc = d.v + b0 - 1;
        }
        u64 rx = 0;
        if (xsrc) rx = d_fill_load<FILL_NT>(xsrc);
        /* the one drain: the glds writes count on vmcnt and the compiler
         * does not track them, so its barrier wait cannot be relied on.
         * The registers pass through it, so whatever wait the compiler adds
         * for them lands right here and not in front of each LDS write */
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(ra), "+v"(rb), "+v"(rx)::"memory");
        if (ia < alen) As[ia] = ra;
        if (ib <= blen) Bs[ib] = rb;
        if (xslot >= 0) smem[xslot] = rx;
    }
    __syncthreads();
    tile_finish<OP, MODE>(smem, aoff, alen, boff, blen, has_ab, has_bb, has_bn, 0, d, tg.d0, t,
                          scan, staging, stage_stride, tile_cnt, offs, partials, have_split,
                          split_w, isplit_out, false);
}

template <int OP, int MODE>
__global__ __launch_bounds__(UA_TBLOCK) void k_tiles(
    const UaDesc *__restrict__ descs, const u32 *__restrict__ tile_pair,
    const u32 *__restrict__ tile_a0, u64 total_tiles,
    u64 *__restrict__ staging, u64 stage_stride, u32 *__restrict__ tile_cnt,
    const u64 *__restrict__ offs, const u64 *__restrict__ partials /* MODE_WRITE only */,
    const u32 *__restrict__ isplit_in /* cached per-thread merge-path splits,
        PACKED lo16 = i0 at diagonal s0, hi16 = i0b at smid (prepared batch:
        inputs immutable, so splits are run-invariant like the tile
        partition); null = compute */,
    u32 *__restrict__ isplit_out /* store packed splits on the first run */,
    const u32 *__restrict__ slab /* prepared batch's narrow records (then
        tile_pair is its private copy with UA_NARROW_BIT), or null */) {
    __shared__ __align__(16) u64 smem[UA_TILE_LDS];
    __shared__ u32 scan[UA_TBLOCK / 64]; /* per-wave totals for d_block_scan */
    u64 t = blockIdx.x;
    /* all four tile words are requested together (one scalar round trip);
     * the neighbour index is clamped, not branched on, so nothing past the
     * arrays is read and no load waits on another's result */
    u64 tn = (t + 1 < total_tiles) ? t + 1 : t;
    u32 p = tile_pair[t];
    u32 pn = tile_pair[tn];
    u32 a0 = tile_a0[t];
    u32 a0n = tile_a0[tn];
    if constexpr ((OP == OP_INTERSECT || OP == OP_DIFF) && MODE == MODE_STAGE) {
        /* eligibility rides in the first scalar round trip: nothing new
         * stands between it and the fill */
        const bool narrow = (slab != nullptr) && (p & UA_NARROW_BIT);
        p &= ~UA_NARROW_BIT;
        pn &= ~UA_NARROW_BIT;
        if (narrow) {
            tile_narrow<OP>(descs, p, pn, a0, a0n, t, tn, slab, smem, scan, staging,
                            stage_stride, tile_cnt, offs, isplit_in, isplit_out);
            return;
        }
    }
    tile_wide<OP, MODE>(descs, p, pn, a0, a0n, t, tn, smem, scan, staging, stage_stride,
                        tile_cnt, offs, partials, isplit_in, isplit_out);
}

/* ==================== kernel: bitonic chunk sort (segmented sort stage 1) ====================
 * One workgroup sorts one <=2048-element chunk in LDS (u64 ascending,
 * duplicates kept; padded with UINT64_MAX).  Stage 2 is the merge-path
 * OP_MERGE_ALL tree. */

#define UA_SORT_N 2048 /* bitonic chunk length: power of two, independent of UA_TILE */

struct UaChunk {
    const u64 *src;
    u64 *dst;
    u32 len;
    u32 pad_;
};

__global__ __launch_bounds__(UA_BLOCK) void k_sort_chunks(
    const UaChunk *__restrict__ chunks, u64 n_chunks) {
    __shared__ u64 s[UA_SORT_N];
    u64 cidx = blockIdx.x;
    if (cidx >= n_chunks) return;
    UaChunk ch = chunks[cidx];
    int tid = threadIdx.x;
    for (int i = tid; i < UA_SORT_N; i += UA_BLOCK)
        s[i] = (i < (int)ch.len) ? ch.src[i] : UINT64_MAX;
    __syncthreads();
    for (int k = 2; k <= UA_SORT_N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < UA_SORT_N; i += UA_BLOCK) {
                int p = i ^ j;
                if (p > i) {
                    bool up = ((i & k) == 0);
                    u64 x = s[i], y = s[p];
                    if ((x > y) == up) {
                        s[i] = y;
                        s[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < (int)ch.len; i += UA_BLOCK) ch.dst[i] = s[i];
}

/* k_sort_chunks' bitonic network over s[0..UA_SORT_N) in LDS, ascending, as a
 * function: every thread of the workgroup calls it (it holds barriers) and s
 * is complete and visible on return.  A second copy on purpose: calling it
 * from k_sort_chunks changes that kernel's generated code (the compiler
 * rotates the outer loop's exit test differently once the loops arrive by
 * inlining), and the segmented sort's code is pinned. */
__device__ __forceinline__ void d_bitonic_sort_lds(u64 *s, int tid) {
    for (int k = 2; k <= UA_SORT_N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < UA_SORT_N; i += UA_BLOCK) {
                int p = i ^ j;
                if (p > i) {
                    bool up = ((i & k) == 0);
                    u64 x = s[i], y = s[p];
                    if ((x > y) == up) {
                        s[i] = y;
                        s[p] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

/* ==================== kernel: sort-unique leaves of a flat UID matrix ====================
 * DestUIDs = MergeSorted(rows) (query/query.go:1874,2290,2505, recurse.go:134,
 * worker/task.go:1629,1706, trigram.go:87, match.go:100) is, as a set, the
 * sorted distinct values of the flat CSR body vals[0..total) — independent of
 * the row boundaries.  One workgroup turns UA_SORT_N consecutive flat elements
 * into one sorted duplicate-free run: runs[leaf*UA_SORT_N ..) of lens[leaf]
 * values.  The runs are the leaves of the pairwise OP_UNION tree
 * (union_tree_locked).  Nothing communicates across workgroups.
 *
 * The last leaf is padded with UINT64_MAX, which is a legal uid (as is 0): no
 * value marks "absent".  Only the first len entries of the sorted tile are
 * real; a real UINT64_MAX tying with the padding is harmless, either copy
 * lands at an index < len.  A tile that is already non-decreasing (every tile
 * inside one sorted row) skips the network; the dedup always runs.
 *
 * Dedup keeps s[i] iff i == 0 || s[i] != s[i-1].  Elements are owned strided
 * (i = step*256 + tid, so LDS and global accesses are conflict-free and
 * coalesced); one ballot per (step, wave) gives the keep-word of 64
 * consecutive elements, the 32 word counts are scanned by one wave, and an
 * element's output rank is its word's base plus the popcount below its lane. */
#define UA_LSTEPS (UA_SORT_N / UA_BLOCK) /* coalesced 256-wide steps per leaf */
#define UA_LWORDS (UA_SORT_N / 64)       /* keep-words per leaf */
static_assert(UA_LWORDS == 32 && UA_LSTEPS * (UA_BLOCK / 64) == UA_LWORDS,
              "one keep-word per (step, wave); one wave scans the 32 word counts");

__global__ __launch_bounds__(UA_BLOCK) void k_union_leaves(
    const u64 *__restrict__ vals, u64 total, u64 *__restrict__ runs,
    u64 *__restrict__ lens) {
    __shared__ u64 s[UA_SORT_N];
    __shared__ u32 wbase[UA_LWORDS + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 base = (u64)blockIdx.x * UA_SORT_N;
    if (base >= total) return; /* uniform; the grid is ceil(total / UA_SORT_N) */
    const int len = (int)((total - base < UA_SORT_N) ? total - base : UA_SORT_N);
#pragma unroll
    for (int k = 0; k < UA_LSTEPS; k++) {
        int i = k * UA_BLOCK + tid;
        s[i] = (i < len) ? vals[base + i] : UINT64_MAX;
    }
    __syncthreads();
    /* block-wide vote, outside any divergent branch: already non-decreasing?
     * (the padding is >= every value, so only pairs inside len matter) */
    int ok = 1;
#pragma unroll
    for (int k = 0; k < UA_LSTEPS; k++) {
        int i = k * UA_BLOCK + tid;
        if (i + 1 < len && s[i] > s[i + 1]) ok = 0;
    }
    if (!__syncthreads_and(ok)) d_bitonic_sort_lds(s, tid); /* uniform branch */
    u64 v[UA_LSTEPS], kw[UA_LSTEPS];
#pragma unroll
    for (int k = 0; k < UA_LSTEPS; k++) {
        int i = k * UA_BLOCK + tid;
        v[k] = s[i];
        bool keep = i < len && (i == 0 || v[k] != s[i - 1]);
        kw[k] = __ballot(keep);
        if (lane == 0) wbase[k * (UA_BLOCK / 64) + wv] = (u32)__popcll(kw[k]);
    }
    __syncthreads();
    if (wv == 0) { /* exclusive scan of the 32 word counts; [32] = leaf length */
        u32 c = lane < UA_LWORDS ? wbase[lane] : 0, incl = c;
#pragma unroll
        for (int o = 1; o < UA_LWORDS; o <<= 1) {
            u32 x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        if (lane < UA_LWORDS) wbase[lane] = incl - c;
        if (lane == UA_LWORDS - 1) wbase[UA_LWORDS] = incl;
    }
    __syncthreads();
    u64 *dst = runs + base;
#pragma unroll
    for (int k = 0; k < UA_LSTEPS; k++) {
        if ((kw[k] >> lane) & 1) {
            u32 pos = wbase[k * (UA_BLOCK / 64) + wv] +
                      (u32)__popcll(kw[k] & (((u64)1 << lane) - 1));
            dst[pos] = v[k]; /* pos < leaf length <= len */
        }
    }
    if (tid == 0) lens[blockIdx.x] = wbase[UA_LWORDS];
}

/* ==================== kernels: flat hierarchical scan (u32 -> u64) ==================== */

__global__ __launch_bounds__(UA_BLOCK) void k_scan1(const u32 *__restrict__ cnt, u64 n,
                                                    u64 *__restrict__ offs,
                                                    u64 *__restrict__ partials) {
    __shared__ u64 sblk[UA_BLOCK];
    u64 base = (u64)blockIdx.x * UA_SCAN_CHUNK;
    int tid = threadIdx.x;
    u64 loc[UA_SCAN_CHUNK / UA_BLOCK];
    u64 sum = 0;
    for (int j = 0; j < UA_SCAN_CHUNK / UA_BLOCK; j++) {
        u64 i = base + (u64)tid * (UA_SCAN_CHUNK / UA_BLOCK) + j;
        u32 c = (i < n) ? cnt[i] : 0;
        loc[j] = sum;
        sum += c;
    }
    sblk[tid] = sum;
    __syncthreads();
    for (int off = 1; off < UA_BLOCK; off <<= 1) {
        u64 x = (tid >= off) ? sblk[tid - off] : 0;
        __syncthreads();
        sblk[tid] += x;
        __syncthreads();
    }
    u64 excl = sblk[tid] - sum;
    for (int j = 0; j < UA_SCAN_CHUNK / UA_BLOCK; j++) {
        u64 i = base + (u64)tid * (UA_SCAN_CHUNK / UA_BLOCK) + j;
        if (i < n) offs[i] = excl + loc[j];
    }
    if (tid == UA_BLOCK - 1) partials[blockIdx.x] = sblk[UA_BLOCK - 1];
}

__global__ __launch_bounds__(UA_BLOCK) void k_scan2(u64 *__restrict__ partials, u64 nchunks) {
    __shared__ u64 sblk[UA_BLOCK];
    int tid = threadIdx.x;
    u64 carry = 0;
    for (u64 base = 0; base < nchunks; base += UA_BLOCK) {
        u64 i = base + tid;
        u64 x = (i < nchunks) ? partials[i] : 0;
        sblk[tid] = x;
        __syncthreads();
        for (int off = 1; off < UA_BLOCK; off <<= 1) {
            u64 y = (tid >= off) ? sblk[tid - off] : 0;
            __syncthreads();
            sblk[tid] += y;
            __syncthreads();
        }
        if (i < nchunks) partials[i] = carry + sblk[tid] - x;
        u64 tot = sblk[UA_BLOCK - 1];
        __syncthreads();
        carry += tot;
    }
}

__global__ __launch_bounds__(UA_BLOCK) void k_pair_out(const u64 *__restrict__ offs,
                                                       const u64 *__restrict__ partials,
                                                       const u64 *__restrict__ tb, int n_pairs,
                                                       u64 *__restrict__ pout) {
    int p = blockIdx.x * UA_BLOCK + threadIdx.x;
    if (p < n_pairs) pout[p] = d_off(offs, partials, tb[p + 1]) - d_off(offs, partials, tb[p]);
}

/* ==================== kernel: compaction ==================== */

/* one wavefront per tile, 4 tiles per wave, 16 per workgroup: few blocks to
 * dispatch, and tiles with cnt==0 cost one load */
#define UA_COMPACT_SMALL 32 /* cnt <= SMALL tiles go to the thread-per-tile
                              * compactor; the wave compactor keeps the rest
                              * (headline tiles emit ~10, so one thread per
                              * tile amortizes the 3-load dependent chain
                              * over 187k parallel threads instead of 47k
                              * waves) */

/* thread-per-tile compactor for small counts (1..UA_COMPACT_SMALL) */
__global__ __launch_bounds__(UA_BLOCK) void k_compact_small(
    const UaDesc *__restrict__ descs, const u32 *__restrict__ tile_pair,
    const u64 *__restrict__ tb, const u32 *__restrict__ tile_cnt,
    const u64 *__restrict__ offs, const u64 *__restrict__ partials,
    const u64 *__restrict__ staging, u64 stage_stride,
    const u64 *__restrict__ prim, u64 total_tiles, int op) {
    u64 t = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (t >= total_tiles) return;
    u32 cnt = tile_cnt[t];
    if (cnt == 0 || cnt > UA_COMPACT_SMALL) return;
    u32 p = tile_pair[t];
    UaDesc d = descs[p];
    u64 goff = d_off(offs, partials, t) - d_off(offs, partials, tb[p]);
    u64 cap = d_pair_cap(d, op);
    if (goff >= cap) return;
    u64 room = cap - goff;
    if ((u64)cnt > room) cnt = (u32)room;
    u64 *dst = d.out + goff;
    const u64 *src = d_stage_src(t, cnt, staging, stage_stride, prim);
    for (u32 i = 0; i < cnt; i++) dst[i] = src[i];
}

__global__ __launch_bounds__(UA_BLOCK) void k_compact(
    const UaDesc *__restrict__ descs, const u32 *__restrict__ tile_pair,
    const u64 *__restrict__ tb /* per-pair first tile (== UaDesc.tile_base) */,
    const u32 *__restrict__ tile_cnt, const u64 *__restrict__ offs,
    const u64 *__restrict__ partials, const u64 *__restrict__ staging,
    u64 stage_stride, const u64 *__restrict__ prim, u64 total_tiles, int op) {
    u64 base = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    int lane = threadIdx.x & 63;
    if (base >= total_tiles) return;
    /* batch the whole dependent chain per 4-tile group: cnts, pairs, offs
     * issue together (independent), then descs (one dependent hop), so the
     * wave pays ~2 scattered-load round trips instead of 4x3 */
    u32 cnts4[4], pair4[4];
    u64 off4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        bool v = base + q < total_tiles;
        cnts4[q] = v ? tile_cnt[base + q] : 0;
        pair4[q] = v ? tile_pair[base + q] : 0;
        off4[q] = v ? d_off(offs, partials, base + q) : 0;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
        u64 t = base + q;
        u32 cnt = cnts4[q];
        if (cnt <= UA_COMPACT_SMALL) continue; /* k_compact_small's tiles */
        UaDesc d = descs[pair4[q]];
        u64 goff = off4[q] - d_off(offs, partials, tb[pair4[q]]);
        u64 cap = d_pair_cap(d, op);
        if (goff >= cap) continue;
        u64 room = cap - goff;
        if ((u64)cnt > room) cnt = (u32)room;
        u64 *dst = d.out + goff;
        const u64 *src = d_stage_src(t, cnt, staging, stage_stride, prim);
        for (u32 i = lane; i < cnt; i += 64) dst[i] = src[i];
    }
}

/* ==================== kernel: fused per-pair tail ==================== */

/* Replaces k_scan1 + k_scan2 + k_compact + k_compact_small + k_pair_out for
 * the staged intersect/difference pipeline.
 * Outputs are per-pair buffers, so a tile only needs its offset WITHIN its
 * pair: no batch-wide prefix is built.  A workgroup owns one chunk of at
 * most UA_TAIL_C consecutive tiles of ONE pair (host-built map, chunks never
 * straddle pairs).  It sums the counts of the pair's earlier tiles (coalesced
 * L2-hot re-read, Tp^2/(2C) u32 per pair — bounded by the host's per-pair
 * chunk limit), scans its own counts in LDS and copies.  No workgroup reads
 * anything another workgroup of this kernel writes: no atomics, fences or
 * flags.
 *
 * UA_TAIL_C: any value up to UA_BLOCK keeps one count per thread (a single
 * d_block_scan, no per-thread loop).  MEASURED on one box (cfg2 headline /
 * cfg3 zipf difference, ms per batch; old tail 3.69 on difference):
 *   C=256  279k pairs/s  3.88     C=32  277k  3.62
 *   C=64   279k          3.65     C=16  273k  3.59
 * The sparse headline does not care until the grid gets large (C=16), but a
 * dense chunk is a 2*C*stride*8-byte copy by ONE workgroup: at C=256 the
 * whole grid is resident at once (6 workgroups per CU on cfg3) and the
 * slowest CU sets the time, 5% behind the old 16-tile compactor.  C=64 is
 * the largest chunk that is not slower than it.  See profiles/tail_fused.md. */
#ifndef UA_TAIL_C
#define UA_TAIL_C 64
#endif
#ifndef UA_TAIL_MLP
#define UA_TAIL_MLP 8 /* dense copy: independent loads in flight per lane
                       * (cfg3 difference at C=128: 3.75 ms vs 3.84 at 4) */
#endif
#define UA_TAIL_MAX_TILES 16384 /* per-pair tile cap of the fused tail, see
                                 * tail_chunk_limit() */
static_assert(UA_TAIL_C >= 1 && UA_TAIL_C <= UA_BLOCK, "one count per thread");

struct alignas(16) UaTChunk {
    u64 t0;     /* global index of the chunk's first tile */
    u32 pair;   /* owning pair */
    u32 lfirst; /* tiles of this pair before the chunk */
};
/* the map holds n_chunks + 1 entries: the sentinel {total_tiles, ~0u, 0}
 * lets a chunk read its tile count (tiles are globally contiguous) and
 * whether it is its pair's last from the next entry. */

__global__ __launch_bounds__(UA_BLOCK) void k_tail_fused(
    const UaDesc *__restrict__ descs, const UaTChunk *__restrict__ cmap,
    const u32 *__restrict__ tile_cnt, const u64 *__restrict__ staging,
    u64 stage_stride, const u64 *__restrict__ prim, u64 *__restrict__ pout, int op) {
    __shared__ u32 s_ex[UA_BLOCK + 1]; /* exclusive scan of the chunk's counts */
    __shared__ u32 s_ws[UA_BLOCK / 64];
    __shared__ u64 s_pre[UA_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const UaTChunk ck = cmap[blockIdx.x];
    const UaTChunk nx = cmap[blockIdx.x + 1];
    const u32 nt = (u32)(nx.t0 - ck.t0); /* 1..UA_TAIL_C */
    const UaDesc d = descs[ck.pair];
    /* the producer clamps tile_cnt to the stride; re-clamp so a corrupt
     * count can never index past a staging row */
    const u32 strd = (u32)stage_stride;
    u32 mine = 0;
    if ((u32)tid < nt) {
        mine = tile_cnt[ck.t0 + tid];
        if (mine > strd) mine = strd;
    }
    /* chunk base: counts of the pair's earlier tiles */
    const u32 *pc = tile_cnt + (ck.t0 - ck.lfirst);
    u64 pre = 0;
    for (u32 i = tid; i < ck.lfirst; i += 4 * UA_BLOCK) {
        u32 x[4]; /* 4 independent L2 loads per round trip */
#pragma unroll
        for (int q = 0; q < 4; q++) {
            u32 j = i + q * UA_BLOCK;
            x[q] = j < ck.lfirst ? pc[j] : 0;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) pre += x[q] < strd ? x[q] : strd;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) pre += __shfl_xor(pre, o);
    if (lane == 0) s_pre[wv] = pre;
    u32 excl, total;
    d_block_scan<UA_BLOCK>(tid, mine, s_ws, excl, total); /* barrier inside */
    s_ex[tid] = excl;
    if (tid == 0) s_ex[UA_BLOCK] = total; /* s_ex[nt] == total for any nt */
    u64 base = 0;
#pragma unroll
    for (int w = 0; w < UA_BLOCK / 64; w++) base += s_pre[w];
    __syncthreads();
    /* per-pair capacity clamp, as k_compact: an element at pair offset g is
     * written iff g < cap (invalid duplicate/unsorted inputs stay
     * memory-safe) */
    const u64 cap = d_pair_cap(d, op);
    if (tid == 0 && nx.pair != ck.pair) {
        /* pair's last chunk publishes the length, CLAMPED to cap; the old
         * k_pair_out publishes the unclamped sum.  They agree on valid
         * inputs, and the clamped value is the number of elements written. */
        u64 len = base + total;
        pout[ck.pair] = len < cap ? len : cap;
    }
    if (base >= cap || total == 0) return;
    const u64 room = cap - base;
    u64 *__restrict__ dst = d.out + base;
    /* Copy-mode switch at a mean of one wave row (64) per tile.  Below it a
     * wave-per-tile copy leaves most lanes idle and pays a load->store round
     * trip per tile, so copy output-indexed (log2 C LDS probes per element buy
     * fully coalesced stores); at or above it every wave iteration is at
     * least half full without any search. */
    if (total < 64u * nt) {
        const u32 lim = (u64)total < room ? total : (u32)room;
        for (u32 e = tid; e < lim; e += UA_BLOCK) {
            /* largest j in [0, nt) with s_ex[j] <= e (skips empty tiles) */
            u32 lo = 0, hi = nt;
            while (hi - lo > 1) {
                u32 mid = (lo + hi) >> 1;
                if (s_ex[mid] <= e) lo = mid;
                else hi = mid;
            }
            u32 cnt = s_ex[lo + 1] - s_ex[lo];
            u64 t = ck.t0 + lo;
            const u64 *src = d_stage_src(t, cnt, staging, stage_stride, prim);
            dst[e] = src[e - s_ex[lo]];
        }
    } else {
        for (u32 j = wv; j < nt; j += UA_BLOCK / 64) {
            u32 off = s_ex[j];
            u32 cnt = s_ex[j + 1] - off;
            if (cnt == 0 || (u64)off >= room) continue;
            u64 t = ck.t0 + j;
            const u64 *src = d_stage_src(t, cnt, staging, stage_stride, prim);
            if ((u64)cnt > room - off) cnt = (u32)(room - off);
            u64 *o = dst + off;
            /* UA_TAIL_MLP independent loads in flight per lane, then the
             * stores: a wave walks its tiles serially, so the copy is bound
             * by load->store round trips unless each one carries enough */
            for (u32 i = lane; i < cnt; i += 64 * UA_TAIL_MLP) {
                u64 val[UA_TAIL_MLP];
#pragma unroll
                for (int q = 0; q < UA_TAIL_MLP; q++)
                    val[q] = (i + 64 * q < cnt) ? src[i + 64 * q] : 0;
#pragma unroll
                for (int q = 0; q < UA_TAIL_MLP; q++)
                    if (i + 64 * q < cnt) o[i + 64 * q] = val[q];
            }
        }
    }
}

__global__ __launch_bounds__(UA_BLOCK) void k_compact_flat(
    u64 *__restrict__ out, const u32 *__restrict__ cnts, const u64 *__restrict__ offs,
    const u64 *__restrict__ partials, const u64 *__restrict__ staging,
    u64 stage_stride, u64 n_blocks) {
    u64 base = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    int lane = threadIdx.x & 63;
    if (base >= n_blocks) return;
    u32 cnts4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cnts4[q] = (base + q < n_blocks) ? cnts[base + q] : 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        u64 b = base + q;
        u32 cnt = cnts4[q];
        if (cnt == 0) continue;
        u64 *dst = out + d_off(offs, partials, b);
        const u64 *src = staging + b * stage_stride;
        for (u32 i = lane; i < cnt; i += 64) dst[i] = src[i];
    }
}

/* ==================== kernel: batched ApplyFilter ==================== */

/* algo.ApplyFilter (uidlist.go:21): in-place mask compaction.  The Go
 * closure f(uid, i) becomes a precomputed per-element byte mask across the
 * C-ABI (callers evaluate predicates upstream, worker/task.go:1403).  One
 * workgroup per 2048-element chunk; per-task output offsets by a
 * decoupled-lookback prefix (below).  out == u (in-place, the reference's
 * shape) is safe: every chunk's loads land (vmcnt) before its count is
 * published, and successors only write after all predecessors published. */
struct alignas(16) UaFDesc {
    const u64 *u;
    u64 n;
    const u8 *mask;
    u64 *out;
    u64 tile_base;
};

/* ---- decoupled-lookback chunk prefix ----
 * Single pass: each chunk publishes its emission count, resolves its
 * task-local exclusive prefix by looking back over predecessor chunks
 * (CUB-style: 64 lanes inspect 64 predecessors per round), and writes its
 * emissions at final positions — no staging buffer, no separate scan /
 * compact launches.  Safe on CDNA4: workgroups dispatch first->last
 * (the same assumption rocPRIM's device scan ships on), and the 8-byte flag
 * word is an untorn agent-scope load/store granule, so no fences are needed —
 * the word itself carries the value.  (The tile kernel once had this as a
 * mode too; it doubled the intersect kernel and was removed)
 *
 * Flag word: [63:48] generation (stale-run guard, wraps via memset),
 * [47:46] status (0 invalid / 1 aggregate / 2 task-local inclusive prefix),
 * [45:0] value. */
#define UA_LB_GEN_MAX 0xFFFFull
__device__ __forceinline__ u64 d_lb_word(u64 gen, u64 status, u64 val) {
    return (gen << 48) | (status << 46) | val;
}

/* wave0 (tid<64) resolves the task-local exclusive prefix of chunk t */
__device__ __forceinline__ u64 d_lb_resolve(u64 *look, u64 gen, u64 t, u64 base_t,
                                            int lane) {
    u64 run = 0;
    u64 hi = t;
    for (;;) {
        long idx = (long)hi - 1 - lane;
        int st = 2;
        u64 val = 0;
        if (idx >= (long)base_t) {
            u64 w = __hip_atomic_load(&look[idx], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
            while ((w >> 48) != gen || !((w >> 46) & 3)) {
                __builtin_amdgcn_s_sleep(1);
                w = __hip_atomic_load(&look[idx], __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
            }
            st = (int)((w >> 46) & 3);
            val = w & ((1ull << 46) - 1);
        }
        u64 pm = __ballot(st == 2);
        /* nearest PREFIX lane (smallest back distance); lanes past it add
         * nothing.  pm==0: whole window is aggregates — sum and slide. */
        u64 contrib;
        if (pm) {
            int k = __ffsll((unsigned long long)pm) - 1;
            contrib = (lane <= k) ? val : 0;
        } else {
            contrib = val;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) contrib += __shfl_xor(contrib, o);
        run += contrib;
        if (pm) return run;
        hi -= 64;
    }
}

__global__ __launch_bounds__(UA_BLOCK) void k_filter(
    const UaFDesc *__restrict__ descs, const u64 *__restrict__ tb, int n_tasks,
    u64 total_tiles, u64 *__restrict__ look, u64 gen, u64 *__restrict__ pout) {
    __shared__ u32 scan[UA_BLOCK / 64];
    __shared__ u64 s_run;
    u64 t = blockIdx.x;
    int tid = threadIdx.x;
    /* task p with tb[p] <= t < tb[p+1] */
    int lo = 0, hi = n_tasks - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (tb[mid] <= t) lo = mid;
        else hi = mid - 1;
    }
    int p = lo;
    UaFDesc d = descs[p];
    u64 lt = t - d.tile_base;
    u64 d0 = lt * UA_TILE;
    u64 d1 = d0 + UA_TILE;
    if (d1 > d.n) d1 = d.n;
    /* per-thread contiguous 8-element run (order-preserving compaction;
     * the 64-B-strided lane pattern coalesces through L1 over the 8 steps) */
    u64 base = d0 + (u64)tid * UA_WPT;
    u64 vals[UA_WPT];
    u32 flags = 0;
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < UA_WPT; s++) {
        u64 i = base + s;
        if (i < d1) {
            vals[s] = d.u[i];
            u32 keep = d.mask[i] ? 1u : 0u;
            flags |= keep << s;
            cnt += (int)keep;
        }
    }
    /* in-place safety: loads must LAND chip-wide before this chunk's count
     * is published (a successor may overwrite these addresses) */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    u32 excl, total;
    d_block_scan<UA_BLOCK>(tid, (u32)cnt, scan, excl, total);
    if (tid == 0) {
        u64 st = (lt == 0) ? 2ull : 1ull;
        __hip_atomic_store(&look[t], d_lb_word(gen, st, total), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        if (lt == 0) s_run = 0;
    }
    if (lt != 0 && tid < 64) {
        u64 run = d_lb_resolve(look, gen, t, d.tile_base, tid);
        if (tid == 0) {
            s_run = run;
            __hip_atomic_store(&look[t], d_lb_word(gen, 2ull, run + total),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    u64 run = s_run;
    if (cnt > 0) {
        u64 *dst = d.out + run + excl;
        int k = 0;
#pragma unroll
        for (int s = 0; s < UA_WPT; s++) {
            if (flags & (1u << s)) dst[k++] = vals[s];
        }
    }
    if (tid == 0) {
        bool lastt = (lt + 1) * UA_TILE >= d.n;
        if (lastt) pout[p] = run + total;
    }
}

/* ==================== kernel: batched IndexOf ==================== */

__global__ __launch_bounds__(UA_BLOCK) void k_index_of(const u64 *__restrict__ u, u64 n,
                                                       const u64 *__restrict__ q, u64 nq,
                                                       int64_t *__restrict__ out) {
    u64 i = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (i >= nq) return;
    u64 key = q[i];
    u64 pos = d_lower_bound(u, n, key);
    out[i] = (pos < n && u[pos] == key) ? (int64_t)pos : -1;
}

/* ==================== kernel: fused group-varint decode (+intersect) ====================
 * One 64-lane wave per pb.UidBlock: load deltas to LDS, lane-0 control-byte
 * walk -> group offsets, per-lane 4-delta extract, wave prefix-sum (+base),
 * then either emit uids >= after (decode) or match a v-range against the
 * decoded block (intersect).  Format: codec.go:57-101 packBlock /
 * go-groupvarint Encode4 (see oracle.h header). */

__device__ __forceinline__ u32 d_load_le(const u8 *p, int len) {
    u32 x = 0;
    for (int b = 0; b < len; b++) x |= ((u32)p[b]) << (8 * b);
    return x;
}

/* per-block pack lookup for the batched form */
__device__ __forceinline__ int d_pack_of(const u64 *__restrict__ pbb, int n_packs, u64 b) {
    int lo = 0, hi = n_packs - 1;
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if (pbb[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

template <int DECODE_ONLY>
__global__ __launch_bounds__(UA_BLOCK) void k_packed(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, const u8 *__restrict__ deltas, u64 n_blocks,
    u64 after, const u64 *v, u64 m, u64 *__restrict__ staging,
    u32 *__restrict__ blk_cnt,
    const u64 *__restrict__ pbb /* batch: [n_packs+1] or null */, int n_packs,
    const ua_ptask *__restrict__ tasks /* batch: per-pack v/m/out/after */) {
    __shared__ u8 sdel[UA_PKW][UA_MAX_DELTAS];
    __shared__ u64 sdec[UA_PKW][UA_MAX_BLOCK_UIDS + 4];
    __shared__ u16 sgoff[UA_PKW][64];

    int wv = threadIdx.x >> 6;
    int lane = threadIdx.x & 63;
    u64 b = (u64)blockIdx.x * UA_PKW + wv;
    /* no early return: __syncthreads() below must be reached by every thread */
    bool active = (b < n_blocks);
    u32 num = 0;
    u64 base = 0, off0 = 0;
    u32 dlen = 0;
    if (active) {
        num = nums[b];
        base = bases[b];
        off0 = doffs[b];
        dlen = (u32)(doffs[b + 1] - off0);
        if (num == 0 || num > UA_MAX_BLOCK_UIDS || dlen > UA_MAX_DELTAS) {
            /* host validates; guard anyway */
            if (lane == 0) blk_cnt[b] = 0;
            active = false;
        }
    }
    if (active && tasks != nullptr) {
        ua_ptask tk = tasks[d_pack_of(pbb, n_packs, b)];
        after = tk.after_uid;
        v = tk.v;
        m = tk.m;
    }
    if (active) {
        for (u32 i = lane; i < dlen; i += 64) sdel[wv][i] = deltas[off0 + i];
    }
    __syncthreads(); /* sdel visible to lane 0's control-byte walk */

    u32 ng = (num > 1) ? ((num + 2) >> 2) : 0; /* ceil((num-1)/4) */
    if (active && lane == 0) {
        u32 o = 0;
        for (u32 g = 0; g < ng; g++) {
            sgoff[wv][g] = (u16)o;
            u8 tag = sdel[wv][o];
            o += 5 + (tag & 3) + ((tag >> 2) & 3) + ((tag >> 4) & 3) + ((tag >> 6) & 3);
        }
    }
    __syncthreads(); /* sgoff visible to all lanes */

    u32 d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    u64 s_local = 0;
    if (active && lane < (int)ng) {
        u32 o = sgoff[wv][lane];
        u8 tag = sdel[wv][o];
        const u8 *p = &sdel[wv][o + 1];
        int l0 = (tag & 3) + 1, l1 = ((tag >> 2) & 3) + 1, l2 = ((tag >> 4) & 3) + 1,
            l3 = ((tag >> 6) & 3) + 1;
        d0 = d_load_le(p, l0);
        p += l0;
        d1 = d_load_le(p, l1);
        p += l1;
        d2 = d_load_le(p, l2);
        p += l2;
        d3 = d_load_le(p, l3);
        s_local = (u64)d0 + d1 + d2 + d3;
    }
    u64 incl = s_local;
    for (int o = 1; o < 64; o <<= 1) {
        u64 x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    u64 excl = incl - s_local;
    if (active && lane == 0) sdec[wv][0] = base;
    if (active && lane < (int)ng) {
        u64 acc = base + excl;
        acc += d0; sdec[wv][lane * 4 + 1] = acc;
        acc += d1; sdec[wv][lane * 4 + 2] = acc;
        acc += d2; sdec[wv][lane * 4 + 3] = acc;
        acc += d3; sdec[wv][lane * 4 + 4] = acc;
    }
    __syncthreads(); /* decoded block visible to every lane */
    if (!active) return;
    /* writes past num land in the +4 pad and are logically truncated (codec.go:198) */
    u64 first = base;
    u64 last = sdec[wv][num - 1];
    u64 out_base = b * (u64)UA_MAX_BLOCK_UIDS;
    u32 cnt = 0;

    if (DECODE_ONLY) {
        for (u32 s0 = 0; s0 < num; s0 += 64) {
            u32 idx = s0 + lane;
            bool ok = false;
            u64 val = 0;
            if (idx < num) {
                val = sdec[wv][idx];
                ok = (val >= after);
            }
            u64 mask = __ballot(ok);
            if (ok) {
                u32 r = (u32)__popcll(mask & ((1ull << lane) - 1));
                staging[out_base + cnt + r] = val;
            }
            cnt += (u32)__popcll(mask);
        }
    } else {
        u64 lo = d_lower_bound(v, m, first > after ? first : after);
        u64 hi = (last == UINT64_MAX) ? m : d_lower_bound(v, m, last + 1);
        for (u64 s0 = lo; s0 < hi; s0 += 64) {
            u64 idx = s0 + lane;
            bool ok = false;
            u64 val = 0;
            if (idx < hi) {
                val = v[idx];
                u64 pos = d_lower_bound(sdec[wv], num, val);
                ok = (pos < num && sdec[wv][pos] == val);
            }
            u64 mask = __ballot(ok);
            if (ok) {
                u32 r = (u32)__popcll(mask & ((1ull << lane) - 1));
                staging[out_base + cnt + r] = val;
            }
            cnt += (u32)__popcll(mask);
        }
    }
    if (lane == 0) blk_cnt[b] = cnt;
}

/* compact for the multi-pack batch: per-pack out destinations */
__global__ __launch_bounds__(UA_BLOCK) void k_compact_pack(
    const ua_ptask *__restrict__ tasks, const u64 *__restrict__ pbb, int n_packs,
    const u32 *__restrict__ cnts, const u64 *__restrict__ offs,
    const u64 *__restrict__ partials, const u64 *__restrict__ staging, u64 n_blocks) {
    u64 basei = ((u64)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
    int lane = threadIdx.x & 63;
    if (basei >= n_blocks) return;
    u32 cnts4[4];
#pragma unroll
    for (int q = 0; q < 4; q++) cnts4[q] = (basei + q < n_blocks) ? cnts[basei + q] : 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        u64 b = basei + q;
        u32 cnt = cnts4[q];
        if (cnt == 0) continue;
        int p = d_pack_of(pbb, n_packs, b);
        u64 *dst = tasks[p].out +
                   (d_off(offs, partials, b) - d_off(offs, partials, pbb[p]));
        const u64 *src = staging + b * (u64)UA_MAX_BLOCK_UIDS;
        for (u32 i = lane; i < cnt; i += 64) dst[i] = src[i];
    }
}

/* ==================== kernels: fan-out decode into a CSR UID matrix ====================
 * ua_rows_decode_dev: count -> scan -> write, no staging
 * area and no per-row host descriptor.  One wave per pb.UidBlock, UA_PKW
 * blocks per workgroup as in k_packed; the decode body below is a second copy
 * of k_packed's so that kernel keeps its code (the d_bitonic_sort_lds
 * precedent, §4.6).  Every index that comes from device data (row boundaries,
 * delta offsets, num_uids) is clamped before it is used: malformed input gives
 * wrong answers, never an out-of-range access. */

enum { RD_DROP = 0, RD_ALL = 1, RD_PART = 2 };

struct UaRdBlk {
    u64 base, off0;
    u32 num, dlen;
    bool ok; /* within the pack limits */
};

/* the 20 header bytes of block b; the delta range is clamped to the blob */
__device__ __forceinline__ UaRdBlk d_rowdec_header(const u64 *__restrict__ bases,
                                                   const u32 *__restrict__ nums,
                                                   const u64 *__restrict__ doffs, u64 nb,
                                                   u64 b) {
    UaRdBlk h;
    h.num = nums[b];
    h.base = bases[b];
    u64 blob = doffs[nb], o0 = doffs[b], o1 = doffs[b + 1];
    if (o0 > blob) o0 = blob;
    if (o1 < o0) o1 = o0;
    if (o1 > blob) o1 = blob;
    h.off0 = o0;
    h.ok = h.num >= 1 && h.num <= UA_MAX_BLOCK_UIDS && o1 - o0 <= UA_MAX_DELTAS;
    h.dlen = h.ok ? (u32)(o1 - o0) : 0;
    return h;
}

/* the row of block b: the last r in [0, n_rows) with rbb[r] <= b (n_rows >= 1) */
__device__ __forceinline__ u64 d_row_of(const u64 *__restrict__ rbb, u64 n_rows, u64 b) {
    u64 lo = 0, hi = n_rows - 1;
    while (lo < hi) {
        u64 mid = (lo + hi + 1) >> 1;
        if (rbb[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

/* row r's block range, clamped to [0, nb] and to rb0 <= rb1 */
__device__ __forceinline__ void d_row_blocks(const u64 *__restrict__ rbb, u64 r, u64 nb,
                                             u64 &rb0, u64 &rb1) {
    rb0 = rbb[r];
    rb1 = rbb[r + 1];
    if (rb0 > nb) rb0 = nb;
    if (rb1 > nb) rb1 = nb;
    if (rb1 < rb0) rb1 = rb0;
}

/* List.Uids with Intersect == nil keeps x > after, and everything when after
 * is 0 (codec.go:284, list.go:1797).  From the headers alone: a block whose
 * base passes is kept whole, a block followed in its row by a base <= after
 * is dropped whole, and the at most one other block per row is decoded. */
__device__ __forceinline__ int d_rowdec_class(const u64 *__restrict__ bases, u64 b, u64 rb1,
                                              u64 base, u64 after) {
    if (after == 0 || base > after) return RD_ALL;
    if (b + 1 < rb1 && bases[b + 1] <= after) return RD_DROP;
    return RD_PART;
}

/* ListOptions.First over a row of L kept uids (list.go:1892-1900): the kept
 * window [lo, hi) in row-rank space */
__device__ __forceinline__ void d_row_window(u64 L, int32_t f, u64 &lo, u64 &hi) {
    lo = 0;
    hi = L;
    if (f > 0) {
        if ((u64)f < L) hi = (u64)f;
    } else if (f < 0) {
        u64 n = (u64)(-(int64_t)f); /* INT32_MIN negates in 64 bits */
        if (n < L) lo = L - n;
    }
}

/* k_packed's decode: deltas to LDS, lane-0 control-byte walk, per-lane
 * 4-delta extract, wave prefix + base -> sdec[wv][0 .. num).  Called by every
 * thread of the workgroup (three barriers inside); waves with active == false
 * only pass the barriers. */
__device__ __forceinline__ void d_rowdec_decode(bool active, int wv, int lane, const UaRdBlk &h,
                                                const u8 *__restrict__ deltas,
                                                u8 (*sdel)[UA_MAX_DELTAS],
                                                u64 (*sdec)[UA_MAX_BLOCK_UIDS + 4],
                                                u16 (*sgoff)[64]) {
    if (active) {
        for (u32 i = lane; i < h.dlen; i += 64) sdel[wv][i] = deltas[h.off0 + i];
    }
    __syncthreads(); /* sdel visible to lane 0's control-byte walk */

    u32 ng = (h.num > 1) ? ((h.num + 2) >> 2) : 0; /* ceil((num-1)/4) <= 64 */
    if (active && lane == 0) {
        u32 o = 0; /* <= 17 * 63: the walk stays inside sdel whatever the bytes */
        for (u32 g = 0; g < ng; g++) {
            sgoff[wv][g] = (u16)o;
            u8 tag = sdel[wv][o];
            o += 5 + (tag & 3) + ((tag >> 2) & 3) + ((tag >> 4) & 3) + ((tag >> 6) & 3);
        }
    }
    __syncthreads(); /* sgoff visible to all lanes */

    u32 d0 = 0, d1 = 0, d2 = 0, d3 = 0;
    u64 s_local = 0;
    if (active && lane < (int)ng) {
        u32 o = sgoff[wv][lane];
        u8 tag = sdel[wv][o];
        const u8 *p = &sdel[wv][o + 1];
        int l0 = (tag & 3) + 1, l1 = ((tag >> 2) & 3) + 1, l2 = ((tag >> 4) & 3) + 1,
            l3 = ((tag >> 6) & 3) + 1;
        d0 = d_load_le(p, l0);
        p += l0;
        d1 = d_load_le(p, l1);
        p += l1;
        d2 = d_load_le(p, l2);
        p += l2;
        d3 = d_load_le(p, l3);
        s_local = (u64)d0 + d1 + d2 + d3;
    }
    u64 incl = s_local;
    for (int o = 1; o < 64; o <<= 1) {
        u64 x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    u64 excl = incl - s_local;
    if (active && lane == 0) sdec[wv][0] = h.base;
    if (active && lane < (int)ng) {
        /* writes past num land in the +4 pad (codec.go:198) */
        u64 acc = h.base + excl;
        acc += d0; sdec[wv][lane * 4 + 1] = acc;
        acc += d1; sdec[wv][lane * 4 + 2] = acc;
        acc += d2; sdec[wv][lane * 4 + 3] = acc;
        acc += d3; sdec[wv][lane * 4 + 4] = acc;
    }
    __syncthreads(); /* decoded block visible to every lane */
}

/* cnt[b] = how many uids of block b pass its row's after (launched when the
 * call has an after array; k_rowdec_count_hdr otherwise) */
__global__ __launch_bounds__(UA_BLOCK) void k_rowdec_count(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, const u8 *__restrict__ deltas, u64 nb,
    const u64 *__restrict__ rbb, u64 n_rows, const u64 *__restrict__ after,
    u32 *__restrict__ cnt) {
    __shared__ u8 sdel[UA_PKW][UA_MAX_DELTAS];
    __shared__ u64 sdec[UA_PKW][UA_MAX_BLOCK_UIDS + 4];
    __shared__ u16 sgoff[UA_PKW][64];

    int wv = threadIdx.x >> 6;
    int lane = threadIdx.x & 63;
    u64 b = (u64)blockIdx.x * UA_PKW + wv;
    /* no early return before the decode: its barriers need every thread */
    bool inb = (b < nb);
    UaRdBlk h = {};
    int cls = RD_DROP;
    u64 aft = 0;
    if (inb) {
        h = d_rowdec_header(bases, nums, doffs, nb, b);
        if (h.ok) {
            u64 r = d_row_of(rbb, n_rows, b), rb0, rb1;
            d_row_blocks(rbb, r, nb, rb0, rb1);
            aft = after[r];
            cls = d_rowdec_class(bases, b, rb1, h.base, aft);
        }
    }
    bool active = (cls == RD_PART);
    d_rowdec_decode(active, wv, lane, h, deltas, sdel, sdec, sgoff);
    if (!inb) return;
    u32 c = (cls == RD_ALL) ? h.num : 0;
    if (active) {
        for (u32 s0 = 0; s0 < h.num; s0 += 64) {
            u32 idx = s0 + lane;
            bool ok = (idx < h.num) && (sdec[wv][idx] > aft);
            c += (u32)__popcll(__ballot(ok));
        }
    }
    if (lane == 0) cnt[b] = c;
}

/* k_rowdec_count without after: every block within the limits keeps all its
 * uids, so the count is its header's num_uids — one thread per block */
__global__ __launch_bounds__(UA_BLOCK) void k_rowdec_count_hdr(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, u64 nb, u32 *__restrict__ cnt) {
    u64 b = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (b >= nb) return;
    UaRdBlk h = d_rowdec_header(bases, nums, doffs, nb, b);
    cnt[b] = h.ok ? h.num : 0;
}

/* One thread per row boundary r in [0, n_rows].  Without first the block
 * scan already is the CSR offsets: out_row_offs[r] = kept uids before row r's
 * first block.  With first, kcnt[r] = the length of row r's kept window (and
 * 0 at n_rows), to be scanned into the offsets by k_rowdec_offs. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowdec_rows(
    const u64 *__restrict__ rbb, u64 n_rows, u64 nb, const u64 *__restrict__ offs,
    const u64 *__restrict__ part, const int32_t *__restrict__ first /* or null */,
    u32 *__restrict__ kcnt, u64 *__restrict__ out_row_offs) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r > n_rows) return;
    if (first == nullptr) {
        u64 rb = rbb[r];
        out_row_offs[r] = d_off(offs, part, rb < nb ? rb : nb);
        return;
    }
    u32 k = 0;
    if (r < n_rows) {
        u64 rb0, rb1, lo, hi;
        d_row_blocks(rbb, r, nb, rb0, rb1);
        d_row_window(d_off(offs, part, rb1) - d_off(offs, part, rb0), first[r], lo, hi);
        k = (u32)(hi - lo); /* <= sum(num_uids) < 2^32 */
    }
    kcnt[r] = k;
}

/* the window-length scan -> out_row_offs[0 .. n_rows] */
__global__ __launch_bounds__(UA_BLOCK) void k_rowdec_offs(const u64 *__restrict__ offs2,
                                                          const u64 *__restrict__ part2,
                                                          u64 n_rows,
                                                          u64 *__restrict__ out_row_offs) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r <= n_rows) out_row_offs[r] = d_off(offs2, part2, r);
}

/* Decode block b and store the uids that pass after and fall into the row's
 * first window straight to out_vals[out_row_offs[r] + rank - lo]: 64
 * consecutive u64 per wave-step, each store bounded by cap_vals.  A block
 * that kept nothing, or whose rank range misses the window, ends after its
 * header. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowdec_write(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, const u8 *__restrict__ deltas, u64 nb,
    const u64 *__restrict__ rbb, u64 n_rows, const u64 *__restrict__ after /* or null */,
    const int32_t *__restrict__ first /* or null */, const u32 *__restrict__ cnt,
    const u64 *__restrict__ offs, const u64 *__restrict__ part,
    const u64 *__restrict__ out_row_offs, u64 *__restrict__ out_vals, u64 cap_vals) {
    __shared__ u8 sdel[UA_PKW][UA_MAX_DELTAS];
    __shared__ u64 sdec[UA_PKW][UA_MAX_BLOCK_UIDS + 4];
    __shared__ u16 sgoff[UA_PKW][64];

    int wv = threadIdx.x >> 6;
    int lane = threadIdx.x & 63;
    u64 b = (u64)blockIdx.x * UA_PKW + wv;
    /* no early return before the decode: its barriers need every thread */
    UaRdBlk h = {};
    u32 c = 0;
    if (b < nb) {
        h = d_rowdec_header(bases, nums, doffs, nb, b);
        if (h.ok) c = cnt[b];
    }
    bool active = (c > 0);
    bool all = true; /* every uid of the block passes after */
    u64 aft = 0;
    u64 pos0 = 0;         /* out_vals index of kept uid jlo of this block */
    u32 jlo = 0, jhi = c; /* the block's kept uids [jlo, jhi) are stored */
    if (active) {
        u64 g = d_off(offs, part, b);
        if (after == nullptr && first == nullptr) {
            pos0 = g; /* the block scan is the output position */
        } else {
            u64 r = d_row_of(rbb, n_rows, b), rb0, rb1;
            d_row_blocks(rbb, r, nb, rb0, rb1);
            if (after != nullptr) {
                aft = after[r];
                all = (d_rowdec_class(bases, b, rb1, h.base, aft) == RD_ALL);
            }
            u64 g0 = d_off(offs, part, rb0);
            u64 rank0 = g - g0; /* row rank of this block's first kept uid */
            if (first == nullptr) {
                pos0 = out_row_offs[r] + rank0;
            } else {
                u64 lo, hi;
                d_row_window(d_off(offs, part, rb1) - g0, first[r], lo, hi);
                u64 a = rank0 > lo ? rank0 : lo;
                u64 e = rank0 + c < hi ? rank0 + c : hi;
                if (a >= e) {
                    active = false;
                } else {
                    jlo = (u32)(a - rank0);
                    jhi = (u32)(e - rank0);
                    pos0 = out_row_offs[r] + (a - lo);
                }
            }
        }
    }
    d_rowdec_decode(active, wv, lane, h, deltas, sdel, sdec, sgoff);
    if (!active) return;
    u32 k = 0; /* kept uids of the block before this wave-step */
    for (u32 s0 = 0; s0 < h.num && k < jhi; s0 += 64) {
        u32 idx = s0 + lane;
        bool ok = false;
        u64 val = 0;
        if (idx < h.num) {
            val = sdec[wv][idx];
            ok = all || val > aft;
        }
        u64 mask = __ballot(ok);
        if (ok) {
            u32 j = k + (u32)__popcll(mask & ((1ull << lane) - 1));
            u64 p = pos0 + (j - jlo);
            if (j >= jlo && j < jhi && p < cap_vals) out_vals[p] = val;
        }
        k += (u32)__popcll(mask);
    }
}

/* ==================== kernel: fan-out intersect into a CSR UID matrix ====================
 * ua_rows_intersect_packed_dev: every row's
 * algo.IntersectCompressedWith(pack, after[r], shared) (uidlist.go:33), count
 * -> scan -> write like the decode above and on its helpers.  One wave per
 * block; the wave index goes through readfirstlane, so the header, the row
 * lookup and the two bounding searches of `shared` are wave-uniform.
 *
 * A block is bounded from headers alone: its matches lie in shared[lo, hi)
 * with lo = lower_bound(max(base, after[r])) and hi = lower_bound(the next
 * base of the SAME row) (row r+1 may hold smaller uids than row r).  lo >= hi
 * drops the block undecoded.  Otherwise the decoded last uid tightens hi
 * (unless the range is within UA_RI_RATIO * num already: a shorter one would
 * be too, with the same matches), and R = hi - lo against num_uids picks the
 * match form:
 *   list-driven  (R <= UA_RI_RATIO * num): 64 shared values per wave-step,
 *                each looked up in the decoded block in LDS (k_packed's match);
 *   block-driven (otherwise): 64 decoded uids per wave-step, at most 4 steps,
 *                each >= key looked up in shared[lo, hi): about 256 * log2 m
 *                probes per block however long the range is.
 * Both emit in ascending order, and the choice depends only on values that the
 * count and the write pass compute identically.  The count is clamped to num
 * (only a shared list with duplicates could pass it) and the write pass stores
 * match j only for j < cnt[b] and below cap_vals, so it stores what was
 * counted whatever the data.
 *
 * A wave is latency-bound on its chain of dependent loads, so the wave-uniform
 * searches probe 64 places per step (d_wave_lower_bound: 4 steps at m = 1M
 * where a binary search takes 20), and lo and hi are searched in step.
 * With UA_RI_KEEP the count pass also leaves, for a list-driven block of
 * R <= 64, lo and the 64-bit match mask, and the write pass copies those
 * shared values without decoding the block again.  Measured:
 * profiles/rows_isect.md. */
#ifndef UA_RI_RATIO
#define UA_RI_RATIO 4 /* list-driven up to this many shared values per uid of
                       * the block; 1, 4, 16 measured: profiles/rows_isect.md */
#endif
static_assert(UA_RI_RATIO >= 1 && UA_RI_RATIO <= 16, "UA_RI_RATIO is held to [1, 16]");
#ifndef UA_RI_KEEP
#define UA_RI_KEEP 1 /* 0 = the write pass always decodes and matches again */
#endif
#define UA_RI_NOKEEP UINT64_MAX /* keep[2b]: no mask was left for block b */

/* N lower_bounds by the whole wave, in step so that their loads overlap:
 * r[q] = lower_bound(a[q], n[q], key[q]).  64 probes per step cut a range to
 * 1/64.  Every lane must be active; the results are the same in all of them.
 * Every load is below n[q] whatever the data. */
/* one search's step: its 64 probes narrow [lo, lo + len] (wave-uniform) */
__device__ __forceinline__ void d_wave_narrow(u64 &lo, u64 &len, u64 step, bool in, u64 x,
                                              u64 key) {
    if (len == 0) return;
    u64 mask = __ballot(!in || x >= key);
    u64 f = mask ? (u64)__ffsll((long long)mask) - 1 : 64;
    u64 end = lo + len;
    lo += f * step; /* everything up to probe f - 1 is below key */
    if (lo > end) lo = end;
    len = (step - 1 < end - lo) ? step - 1 : end - lo;
}

template <int N> /* 1 or 2 */
__device__ __forceinline__ void d_wave_lower_bound(const u64 *const (&a)[N], const u64 (&n)[N],
                                                   const u64 (&key)[N], int lane, u64 (&r)[N]) {
    u64 len[N]; /* the answer is in [r[q], r[q] + len[q]] */
#pragma unroll
    for (int q = 0; q < N; q++) {
        r[q] = 0;
        len[q] = n[q];
    }
    for (;;) {
        u64 left = 0;
#pragma unroll
        for (int q = 0; q < N; q++) left |= len[q];
        if (left == 0) break;
        u64 step[N], x[N];
        bool in[N];
#pragma unroll
        for (int q = 0; q < N; q++) { /* probes r + step - 1, r + 2 step - 1, ... */
            step[q] = (len[q] + 63) >> 6;
            u64 p = r[q] + (u64)(lane + 1) * step[q] - 1;
            in[q] = (len[q] > 0) && (p < r[q] + len[q]);
            x[q] = in[q] ? a[q][p] : UINT64_MAX;
        }
        d_wave_narrow(r[0], len[0], step[0], in[0], x[0], key[0]);
        if (N > 1) d_wave_narrow(r[N > 1 ? 1 : 0], len[N > 1 ? 1 : 0], step[N > 1 ? 1 : 0],
                                 in[N > 1 ? 1 : 0], x[N > 1 ? 1 : 0], key[N > 1 ? 1 : 0]);
    }
}

__device__ __forceinline__ u64 d_wave_lower_bound(const u64 *a, u64 n, u64 key, int lane) {
    const u64 *const as[1] = {a};
    const u64 ns[1] = {n}, keys[1] = {key};
    u64 r[1];
    d_wave_lower_bound<1>(as, ns, keys, lane, r);
    return r[0];
}

template <bool WRITE>
__global__ __launch_bounds__(UA_BLOCK) void k_rowisect(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, const u8 *__restrict__ deltas, u64 nb,
    const u64 *__restrict__ rbb, u64 n_rows, const u64 *__restrict__ after /* or null */,
    const u64 *__restrict__ shared, u64 m, u32 *__restrict__ cnt /* WRITE: read */,
    const u64 *__restrict__ offs, const u64 *__restrict__ part, u64 *__restrict__ out_vals,
    u64 cap_vals, u64 *__restrict__ keep /* [2 * nb]: (lo, mask); WRITE: read; or null */) {
    __shared__ u8 sdel[UA_PKW][UA_MAX_DELTAS];
    __shared__ u64 sdec[UA_PKW][UA_MAX_BLOCK_UIDS + 4];
    __shared__ u16 sgoff[UA_PKW][64];

    int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int lane = threadIdx.x & 63;
    u64 b = (u64)blockIdx.x * UA_PKW + wv;
    /* no early return before the decode: its barriers need every thread */
    bool inb = (b < nb);
    UaRdBlk h = {};
    u32 c = 0; /* WRITE: the count pass's matches of this block */
    u64 key = 0, lo = 0, hi = 0;
    u64 klo = UA_RI_NOKEEP, kmask = 0; /* the block's kept mask, if any */
    bool active = false;
    const u64 below = (1ull << lane) - 1;
    if (inb) {
        bool go = true;
        if (WRITE) { /* a block that matched nothing ends here, before its header */
            c = cnt[b];
            go = (c > 0);
            if (go && keep != nullptr) {
                klo = keep[2 * b];
                if (klo != UA_RI_NOKEEP) {
                    kmask = keep[2 * b + 1];
                    go = false;
                }
            }
        }
        if (go) {
            h = d_rowdec_header(bases, nums, doffs, nb, b);
            go = h.ok;
        }
        if (go) {
            /* the next base rides with the header; it counts only inside the row */
            u64 nbase = bases[b + 1 < nb ? b + 1 : b];
            /* d_row_of by the whole wave: the last r with rbb[r] <= b */
            u64 r = d_wave_lower_bound(rbb, n_rows, b + 1, lane), rb0, rb1;
            r = r ? r - 1 : 0;
            d_row_blocks(rbb, r, nb, rb0, rb1);
            u64 aft = after ? after[r] : 0;
            key = h.base > aft ? h.base : aft; /* x >= after[r]: Seek(afterUID, SeekStart) */
            if (b + 1 < rb1) {
                const u64 *const as[2] = {shared, shared};
                const u64 ns[2] = {m, m}, keys[2] = {key, nbase};
                u64 res[2];
                d_wave_lower_bound<2>(as, ns, keys, lane, res);
                lo = res[0];
                hi = res[1];
            } else {
                lo = d_wave_lower_bound(shared, m, key, lane);
                hi = m;
            }
            active = (lo < hi);
        }
    }
    d_rowdec_decode(active, wv, lane, h, deltas, sdel, sdec, sgoff);
    if (WRITE && klo != UA_RI_NOKEEP) { /* copy what the count pass marked */
        u64 idx = klo + lane;
        if (((kmask >> lane) & 1) && idx < m) {
            u32 j = (u32)__popcll(kmask & below);
            u64 p = d_off(offs, part, b) + j;
            if (j < c && p < cap_vals) out_vals[p] = shared[idx];
        }
        return;
    }
    if (!active) {
        if (!WRITE && inb && lane == 0) cnt[b] = 0;
        return;
    }
    const u32 num = h.num;
    u64 last = sdec[wv][num - 1];
    /* tighten hi by the block's last uid, unless the range is list-driven
     * already: a shorter range would be too, with the same matches */
    if (hi - lo > (u64)UA_RI_RATIO * num && last != UINT64_MAX)
        hi = lo + d_wave_lower_bound(shared + lo, hi - lo, last + 1, lane);
    const u64 R = hi - lo;
    const u64 pos0 = WRITE ? d_off(offs, part, b) : 0;
    u32 k = 0; /* matches before this wave-step */
    if (R <= (u64)UA_RI_RATIO * num) {
        for (u64 s0 = lo; s0 < hi; s0 += 64) {
            u64 idx = s0 + lane;
            bool ok = false;
            u64 val = 0;
            if (idx < hi) {
                val = shared[idx];
                u64 pos = d_lower_bound(sdec[wv], num, val);
                ok = (pos < num && sdec[wv][pos] == val);
            }
            u64 mask = __ballot(ok);
            if (WRITE && ok) {
                u32 j = k + (u32)__popcll(mask & below);
                if (j < c && pos0 + j < cap_vals) out_vals[pos0 + j] = val;
            }
            k += (u32)__popcll(mask);
            if (!WRITE && R <= 64) { /* the only step: its mask is the block's result */
                klo = lo;
                kmask = mask;
            }
        }
    } else {
        for (u32 s0 = 0; s0 < num; s0 += 64) {
            u32 idx = s0 + lane;
            bool ok = false;
            u64 val = 0;
            if (idx < num) {
                val = sdec[wv][idx];
                if (val >= key) {
                    u64 pos = lo + d_lower_bound(shared + lo, R, val);
                    ok = (pos < hi && shared[pos] == val);
                }
            }
            u64 mask = __ballot(ok);
            if (WRITE && ok) {
                u32 j = k + (u32)__popcll(mask & below);
                if (j < c && pos0 + j < cap_vals) out_vals[pos0 + j] = val;
            }
            k += (u32)__popcll(mask);
        }
    }
    if (!WRITE && lane == 0) {
        cnt[b] = k < num ? k : num;
        if (keep != nullptr && k > 0) {
            keep[2 * b] = klo;
            keep[2 * b + 1] = kmask;
        }
    }
}

/* ==================== kernels: fan-out decode with mutation layers ====================
 * ua_rows_decode_mut_dev: every row's List.Uids on a list
 * with a mutable layer (List.iterate, posting/list.go:1135-1251), count -> scan
 * -> k_rowdec_rows -> write like the two calls above and on their helpers.
 *
 * Output order is a sequence of nb + n_rows ITEMS: one head per row followed
 * by that row's blocks, so row r's head is item min(rbb[r], nb) + r and block
 * b of row r is item b + r + 1.  The head owns the row's mutations below the
 * row's first base (all of them when the row has no block); block b owns
 * those in [bases[b], bases[b+1]), the row's last block [bases[b], inf).  The
 * item boundaries ribb[r] = min(rbb[r], nb) + r make the existing
 * k_rowdec_rows / k_rowdec_offs produce the offsets and the first windows.
 *
 * The grids stay one thread or wave per BLOCK (k_rowmut_blocks, k_rowmut,
 * k_rowmut_plain_write) and per ROW (k_rowmut_head, k_rowmut_head_write): an
 * item is reached from its block or its row, never a block or row from an
 * item index, so no inverse of the unvalidated rbb is needed.  pre[] is the
 * exclusive scan of the per-mutation "emitted" flag (d_mut_emits); an item
 * owning slice [s0, s1) emits pre[s1] - pre[s0] mutations.  A block with an
 * empty slice keeps §4.7's header-only classes, decided by one thread per
 * block; the wave passes run over the lists of the blocks that are left.
 * Count and write share d_rowmut_locate, d_rowmut_slice, d_rowmut_keeps and
 * d_mut_emits, and the write stores rank j only for j < cnt[item] and below
 * cap_vals.
 * Every index read from device data is clamped (d_row_blocks, d_row_muts) and
 * every probe of mut_uids stays inside the row's clamped slice. */

struct UaMutView {
    const u64 *uids;  /* [n_mut] */
    const u8 *ops;    /* [n_mut] */
    const u64 *rmb;   /* row_mut_base [n_rows + 1] */
    u64 n_mut;
    const u64 *poffs; /* pre[]: split scan of the emitted flags, n_mut + 1 */
    const u64 *ppart;
};

/* row r's mutation slice, clamped to [0, n_mut] and to m0 <= m1 */
__device__ __forceinline__ void d_row_muts(const u64 *__restrict__ rmb, u64 r, u64 n_mut,
                                           u64 &m0, u64 &m1) {
    m0 = rmb[r];
    m1 = rmb[r + 1];
    if (m0 > n_mut) m0 = n_mut;
    if (m1 > n_mut) m1 = n_mut;
    if (m1 < m0) m1 = m0;
}

/* iterate emits a mutable posting iff mp.Op != Del (list.go:1217, 1229) and
 * afterUid < mp.Uid (list.go:1146); after == 0 keeps all, as for the pack */
__device__ __forceinline__ bool d_mut_emits(u8 op, u64 uid, u64 aft) {
    return op != UA_MUT_DEL && (aft == 0 || uid > aft);
}

/* flag[j] = mutation j is emitted by its row, j in [0, n_mut); flag[n_mut] = 0 */
__global__ __launch_bounds__(UA_BLOCK) void k_rowmut_flags(UaMutView M, u64 n_rows,
                                                           const u64 *__restrict__ after,
                                                           u32 *__restrict__ flag) {
    u64 j = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (j > M.n_mut) return;
    u32 f = 0;
    if (j < M.n_mut) {
        u64 aft = after ? after[d_row_of(M.rmb, n_rows, j)] : 0;
        f = d_mut_emits(M.ops[j], M.uids[j], aft);
    }
    flag[j] = f;
}

/* One thread per row boundary r in [0, n_rows]: the item boundary ribb[r],
 * and for r < n_rows the head's count: the emitted mutations of the row's
 * slice below the row's first base (all of them for a row without blocks). */
__global__ __launch_bounds__(UA_BLOCK) void k_rowmut_head(
    const u64 *__restrict__ rbb, u64 n_rows, u64 nb, const u64 *__restrict__ bases,
    UaMutView M, u32 *__restrict__ cnt, u64 *__restrict__ ribb) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r > n_rows) return;
    if (r == n_rows) {
        ribb[r] = nb + n_rows; /* whatever rbb[n_rows] says: the items end here */
        return;
    }
    u64 rb0, rb1, m0, m1;
    d_row_blocks(rbb, r, nb, rb0, rb1);
    ribb[r] = rb0 + r;
    d_row_muts(M.rmb, r, M.n_mut, m0, m1);
    u32 c = 0;
    if (m0 < m1) {
        u64 e = m1;
        if (rb0 < rb1) e = m0 + d_lower_bound(M.uids + m0, m1 - m0, bases[rb0]);
        c = (u32)(d_off(M.poffs, M.ppart, e) - d_off(M.poffs, M.ppart, m0));
    }
    cnt[rb0 + r] = c;
}

/* Per block, left by k_rowmut_blocks for the two wave passes: the block's row,
 * with UA_MUT_OWNS set when the block owns mutations.  cnt[item] ==
 * UA_MUT_WAVE asks the wave count pass for the block's count (every real
 * count is smaller: 256 * n_blocks + n_mut <= 2^32 - 2). */
#define UA_MUT_OWNS ((u64)1 << 63)
#define UA_MUT_WAVE UINT32_MAX

/* Block b's owned slice [s0, s1) of its row's clamped slice [m0, m1): the
 * mutations in [base, the row's next base), or [base, inf) for the row's last
 * block.  Every probe is inside [m0, m1). */
__device__ __forceinline__ void d_rowmut_slice(const u64 *__restrict__ bases, u64 b, u64 rb1,
                                               u64 base, const UaMutView &M, u64 m0, u64 m1,
                                               u64 &s0, u64 &s1) {
    s0 = s1 = m0;
    if (m0 >= m1) return; /* a row with an empty layer skips both searches */
    s0 = m0 + d_lower_bound(M.uids + m0, m1 - m0, base);
    s1 = (b + 1 < rb1) ? m0 + d_lower_bound(M.uids + m0, m1 - m0, bases[b + 1]) : m1;
    if (s1 < s0) s1 = s0; /* bases not ascending inside the row */
}

/* list[*n ...] = val for every lane with pred, one atomic per wave.  Every
 * lane of the wave must call it. */
__device__ __forceinline__ void d_wave_append(bool pred, u32 val, u32 *__restrict__ n,
                                              u32 *__restrict__ list) {
    const int lane = threadIdx.x & 63;
    const u64 mask = __ballot(pred);
    const int leader = mask ? __ffsll((long long)mask) - 1 : 0;
    u32 base = 0;
    if (mask && lane == leader) base = atomicAdd(n, (u32)__popcll(mask));
    base = __shfl(base, leader);
    if (pred) list[base + (u32)__popcll(mask & ((1ull << lane) - 1))] = val;
}

/* One thread per block: the block's row (brow), whether it owns mutations,
 * and its count where the header decides it: a block without mutations that
 * is kept or dropped whole (§4.7's classes), or a dropped block's mutations.
 * Every other block is left to the wave count pass (UA_MUT_WAVE) and put on
 * wlist; every owner is put on olist for the wave write pass.  The two wave
 * passes run over these lists, so a sparse layer costs them next to nothing.
 * The order of a list varies from run to run; no result depends on it. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowmut_blocks(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, u64 nb, const u64 *__restrict__ rbb, u64 n_rows,
    const u64 *__restrict__ after /* or null */, UaMutView M, u32 *__restrict__ cnt,
    u64 *__restrict__ brow, u32 *__restrict__ list_n /* [2], zeroed */,
    u32 *__restrict__ wlist, u32 *__restrict__ olist) {
    u64 b = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    bool owns = false, wave = false;
    if (b < nb) {
        UaRdBlk h = d_rowdec_header(bases, nums, doffs, nb, b);
        u64 r = d_row_of(rbb, n_rows, b), rb0, rb1, m0, m1, s0, s1;
        d_row_blocks(rbb, r, nb, rb0, rb1);
        d_row_muts(M.rmb, r, M.n_mut, m0, m1);
        if (!h.ok) m1 = m0;
        d_rowmut_slice(bases, b, rb1, h.base, M, m0, m1, s0, s1);
        int cls = h.ok ? d_rowdec_class(bases, b, rb1, h.base, after ? after[r] : 0) : RD_DROP;
        owns = (s0 < s1);
        brow[b] = r | (owns ? UA_MUT_OWNS : 0);
        u32 c = UA_MUT_WAVE;
        if (cls == RD_DROP) /* its mutations lie below the next base <= after: none emitted */
            c = (u32)(d_off(M.poffs, M.ppart, s1) - d_off(M.poffs, M.ppart, s0));
        else if (!owns && cls == RD_ALL)
            c = h.num;
        wave = (c == UA_MUT_WAVE);
        cnt[b + r + 1] = c;
    }
    d_wave_append(wave, (u32)b, list_n + 0, wlist);
    d_wave_append(owns, (u32)b, list_n + 1, olist);
}

/* What both wave passes know of block b, from brow: row, item, after, class
 * and owned slice.  Wave-uniform. */
struct UaMutBlk {
    u64 r, item, aft, s0, s1;
    int cls;
};
__device__ __forceinline__ UaMutBlk d_rowmut_locate(const u64 *__restrict__ bases, u64 nb,
                                                    const u64 *__restrict__ rbb,
                                                    const u64 *__restrict__ after,
                                                    const UaMutView &M, u64 b, u64 base,
                                                    u64 w) {
    UaMutBlk k;
    k.r = w & ~UA_MUT_OWNS;
    k.item = b + k.r + 1;
    k.aft = after ? after[k.r] : 0;
    k.cls = RD_ALL;
    k.s0 = k.s1 = 0;
    if (after != nullptr || (w & UA_MUT_OWNS)) {
        u64 rb0, rb1, m0, m1;
        d_row_blocks(rbb, k.r, nb, rb0, rb1);
        k.cls = d_rowdec_class(bases, b, rb1, base, k.aft);
        if (w & UA_MUT_OWNS) {
            d_row_muts(M.rmb, k.r, M.n_mut, m0, m1);
            d_rowmut_slice(bases, b, rb1, base, M, m0, m1, k.s0, k.s1);
        }
    }
    return k;
}

/* WRITE pass: where the item's ranks go.  The item's ranks [jlo, jhi) are
 * stored from out_vals[pos0] on; false when its rank range misses its row's
 * first window (k_rowdec_write's rule, in item space). */
__device__ __forceinline__ bool d_rowmut_place(const UaMutBlk &k, u32 c, u64 n_items,
                                               const int32_t *__restrict__ first,
                                               const u64 *__restrict__ ribb,
                                               const u64 *__restrict__ offs,
                                               const u64 *__restrict__ part,
                                               const u64 *__restrict__ out_row_offs,
                                               u64 &pos0, u32 &jlo, u32 &jhi) {
    jlo = 0;
    jhi = c;
    u64 g = d_off(offs, part, k.item);
    if (first == nullptr) {
        pos0 = g; /* no window: the item scan is the output position */
        return true;
    }
    u64 ib0, ib1, lo, hi;
    d_row_blocks(ribb, k.r, n_items, ib0, ib1);
    u64 g0 = d_off(offs, part, ib0);
    u64 rank0 = g - g0; /* row rank of this item's rank 0 */
    d_row_window(d_off(offs, part, ib1) - g0, first[k.r], lo, hi);
    u64 a = rank0 > lo ? rank0 : lo;
    u64 e = rank0 + c < hi ? rank0 + c : hi;
    if (a >= e) return false;
    jlo = (u32)(a - rank0);
    jhi = (u32)(e - rank0);
    pos0 = out_row_offs[k.r] + (a - lo);
    return true;
}

/* a uid of a block WITHOUT mutations is kept */
__device__ __forceinline__ bool d_rowmut_keeps(const UaMutBlk &k, u64 val) {
    return k.cls != RD_DROP && (k.aft == 0 || val > k.aft);
}

/* One wave per LISTED block, UA_PKW per workgroup-step.  WRITE == false, over
 * wlist: the count of every block that k_rowmut_blocks left open: its kept
 * uids plus its emitted mutations.  WRITE == true, over olist: an owner's
 * kept uids and emitted mutations go to their merged ranks.  A kept uid i has
 * rank keptpre[i] + (pre[lb_M(D[i])] - pre[s0]) in its item and emitted
 * mutation j has (pre[j] - pre[s0]) + keptpre[lb_D(M[j])]; the first window
 * applies in row-rank space as in k_rowdec_write. */
template <bool WRITE>
__global__ __launch_bounds__(UA_BLOCK) void k_rowmut(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, const u8 *__restrict__ deltas, u64 nb,
    const u64 *__restrict__ rbb, u64 n_rows, const u64 *__restrict__ after /* or null */,
    const int32_t *__restrict__ first /* or null */, UaMutView M,
    const u64 *__restrict__ brow, const u32 *__restrict__ list,
    const u32 *__restrict__ list_n, const u64 *__restrict__ ribb,
    u32 *__restrict__ cnt /* WRITE: read */, const u64 *__restrict__ offs,
    const u64 *__restrict__ part, const u64 *__restrict__ out_row_offs,
    u64 *__restrict__ out_vals, u64 cap_vals) {
    __shared__ u8 sdel[UA_PKW][UA_MAX_DELTAS];
    __shared__ u64 sdec[UA_PKW][UA_MAX_BLOCK_UIDS + 4];
    __shared__ u16 sgoff[UA_PKW][64];
    __shared__ u16 skp[UA_PKW][UA_MAX_BLOCK_UIDS + 2]; /* WRITE: kept uids before uid i */

    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const u64 below = (1ull << lane) - 1;
    u64 n_list = *list_n;
    if (n_list > nb) n_list = nb;
    /* every wave of the workgroup takes the same number of steps: the
     * barriers inside need every thread.  A wave's LDS rows are its own. */
    for (u64 i0 = (u64)blockIdx.x * UA_PKW; i0 < n_list; i0 += (u64)gridDim.x * UA_PKW) {
        UaRdBlk h = {};
        UaMutBlk k = {};
        u32 c = 0;            /* WRITE: the count pass's count of this item */
        u64 pos0 = 0;         /* WRITE: out_vals index of the item's rank jlo */
        u32 jlo = 0, jhi = 0; /* WRITE: the item's ranks [jlo, jhi) are stored */
        bool active = false;
        u64 b = (i0 + wv < n_list) ? list[i0 + wv] : nb;
        if (b < nb) {
            const u64 w = brow[b];
            c = cnt[b + (w & ~UA_MUT_OWNS) + 1];
            active = WRITE ? (c > 0 && (w & UA_MUT_OWNS)) : (c == UA_MUT_WAVE);
            if (active) { /* k_rowmut_blocks saw h.ok, or it had counted 0 */
                h = d_rowdec_header(bases, nums, doffs, nb, b);
                k = d_rowmut_locate(bases, nb, rbb, after, M, b, h.base, w);
                active = h.ok;
            }
        }
        if (WRITE && active)
            active = d_rowmut_place(k, c, nb + n_rows, first, ribb, offs, part, out_row_offs,
                                    pos0, jlo, jhi);
        const bool mut = active && (k.s0 < k.s1);
        const u64 nm = k.s1 - k.s0;
        const u64 *ms = M.uids + k.s0;
        const u64 pre0 = mut ? d_off(M.poffs, M.ppart, k.s0) : 0;
        d_rowdec_decode(active, wv, lane, h, deltas, sdel, sdec, sgoff);

        /* uid val of the block is kept; pos = lower_bound of val in the slice */
        auto kept = [&](u64 val, u64 &pos) -> bool {
            pos = 0;
            if (!d_rowmut_keeps(k, val)) return false;
            if (!mut) return true;
            pos = d_lower_bound(ms, nm, val);
            return !(pos < nm && ms[pos] == val);
        };

        if (!WRITE) {
            if (!active) continue;
            c = 0;
            for (u32 s = 0; s < h.num; s += 64) {
                u32 idx = s + lane;
                u64 pos;
                bool ok = (idx < h.num) && kept(sdec[wv][idx], pos);
                c += (u32)__popcll(__ballot(ok));
            }
            if (mut) c += (u32)(d_off(M.poffs, M.ppart, k.s1) - pre0);
            if (lane == 0) cnt[k.item] = c;
            continue;
        }

        u32 kk = 0; /* kept uids of the block before this wave-step */
        if (mut) {
            for (u32 s = 0; s < h.num; s += 64) {
                u32 idx = s + lane;
                bool ok = false;
                u64 val = 0, pos = 0;
                if (idx < h.num) {
                    val = sdec[wv][idx];
                    ok = kept(val, pos);
                }
                u64 mask = __ballot(ok);
                u32 j = kk + (u32)__popcll(mask & below);
                if (idx < h.num) skp[wv][idx] = (u16)j;
                if (ok) {
                    j += (u32)(d_off(M.poffs, M.ppart, k.s0 + pos) - pre0);
                    u64 p = pos0 + (j - jlo);
                    if (j >= jlo && j < jhi && p < cap_vals) out_vals[p] = val;
                }
                kk += (u32)__popcll(mask);
            }
            if (lane == 0) skp[wv][h.num] = (u16)kk;
        }
        __syncthreads(); /* skp visible to every lane */
        if (!mut) continue;
        for (u64 s = 0; s < nm; s += 64) { /* the slice, 64 at a time however long */
            u64 i = s + lane;
            if (i >= nm) continue;
            u64 uid = ms[i];
            if (!d_mut_emits(M.ops[k.s0 + i], uid, k.aft)) continue;
            u32 j = (u32)(d_off(M.poffs, M.ppart, k.s0 + i) - pre0) +
                    skp[wv][d_lower_bound(sdec[wv], h.num, uid)];
            u64 p = pos0 + (j - jlo);
            if (j >= jlo && j < jhi && p < cap_vals) out_vals[p] = uid;
        }
    }
}

/* One wave per block: k_rowdec_write for the blocks that own no mutation,
 * their positions taken from the item scan.  Owners are k_rowmut<true>'s. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowmut_plain_write(
    const u64 *__restrict__ bases, const u32 *__restrict__ nums,
    const u64 *__restrict__ doffs, const u8 *__restrict__ deltas, u64 nb,
    const u64 *__restrict__ rbb, u64 n_rows, const u64 *__restrict__ after /* or null */,
    const int32_t *__restrict__ first /* or null */, UaMutView M,
    const u64 *__restrict__ brow, const u64 *__restrict__ ribb, const u32 *__restrict__ cnt,
    const u64 *__restrict__ offs, const u64 *__restrict__ part,
    const u64 *__restrict__ out_row_offs, u64 *__restrict__ out_vals, u64 cap_vals) {
    __shared__ u8 sdel[UA_PKW][UA_MAX_DELTAS];
    __shared__ u64 sdec[UA_PKW][UA_MAX_BLOCK_UIDS + 4];
    __shared__ u16 sgoff[UA_PKW][64];

    int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int lane = threadIdx.x & 63;
    u64 b = (u64)blockIdx.x * UA_PKW + wv;
    /* no early return before the decode: its barriers need every thread */
    UaRdBlk h = {};
    UaMutBlk k = {};
    u32 c = 0, jlo = 0, jhi = 0;
    u64 pos0 = 0;
    bool active = false;
    if (b < nb) {
        const u64 w = brow[b];
        if (!(w & UA_MUT_OWNS)) c = cnt[b + w + 1];
        if (c > 0) {
            h = d_rowdec_header(bases, nums, doffs, nb, b);
            k = d_rowmut_locate(bases, nb, rbb, after, M, b, h.base, w & ~UA_MUT_OWNS);
            active = h.ok && d_rowmut_place(k, c, nb + n_rows, first, ribb, offs, part,
                                            out_row_offs, pos0, jlo, jhi);
        }
    }
    d_rowdec_decode(active, wv, lane, h, deltas, sdel, sdec, sgoff);
    if (!active) return;
    u32 kk = 0; /* kept uids of the block before this wave-step */
    for (u32 s0 = 0; s0 < h.num && kk < jhi; s0 += 64) {
        u32 idx = s0 + lane;
        bool ok = false;
        u64 val = 0;
        if (idx < h.num) {
            val = sdec[wv][idx];
            ok = d_rowmut_keeps(k, val);
        }
        u64 mask = __ballot(ok);
        if (ok) {
            u32 j = kk + (u32)__popcll(mask & ((1ull << lane) - 1));
            u64 p = pos0 + (j - jlo);
            if (j >= jlo && j < jhi && p < cap_vals) out_vals[p] = val;
        }
        kk += (u32)__popcll(mask);
    }
}

/* One wave per row: the head's emitted mutations go to out_vals.  The head
 * is its row's first item, so its rank 0 is row rank 0; it ends at the first
 * wave-step whose ranks lie past its count or its row's window. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowmut_head_write(
    const u64 *__restrict__ rbb, u64 n_rows, u64 nb, const u64 *__restrict__ after,
    const int32_t *__restrict__ first, UaMutView M, const u64 *__restrict__ ribb,
    const u32 *__restrict__ cnt, const u64 *__restrict__ offs, const u64 *__restrict__ part,
    const u64 *__restrict__ out_row_offs, u64 *__restrict__ out_vals, u64 cap_vals) {
    int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int lane = threadIdx.x & 63;
    for (u64 r = (u64)blockIdx.x * UA_PKW + wv; r < n_rows; r += (u64)gridDim.x * UA_PKW) {
        u64 rb0, rb1, m0, m1, lo = 0, hi;
        d_row_blocks(rbb, r, nb, rb0, rb1);
        u64 c = cnt[rb0 + r];
        if (c == 0) continue;
        hi = c;
        if (first != nullptr) {
            u64 ib0, ib1;
            d_row_blocks(ribb, r, nb + n_rows, ib0, ib1);
            d_row_window(d_off(offs, part, ib1) - d_off(offs, part, ib0), first[r], lo, hi);
            if (hi > c) hi = c;
        }
        if (lo >= hi) continue;
        d_row_muts(M.rmb, r, M.n_mut, m0, m1);
        const u64 aft = after ? after[r] : 0;
        const u64 pre0 = d_off(M.poffs, M.ppart, m0);
        const u64 pos0 = out_row_offs[r]; /* the position of row rank lo */
        for (u64 s = m0; s < m1; s += 64) {
            if (d_off(M.poffs, M.ppart, s) - pre0 >= hi) break;
            u64 i = s + lane;
            if (i >= m1) continue;
            u64 uid = M.uids[i];
            if (!d_mut_emits(M.ops[i], uid, aft)) continue;
            u64 j = d_off(M.poffs, M.ppart, i) - pre0, p = pos0 + (j - lo);
            if (j >= lo && j < hi && p < cap_vals) out_vals[p] = uid;
        }
    }
}

/* ==================== kernels: GPU codec.Encode ====================
 * Parallel restatement of codec.go:57-136 (packBlock/Add): block boundaries
 * are 32-MSB changes (match32MSB :469) plus every block_size-th element
 * within a 32-MSB run; each block's group-varint bytes are produced by one
 * wavefront (lane g encodes group g; a wave shfl-scan of group byte-lengths
 * places them).  Byte-identical to the reference format. */

#define UA_ENC_STRIDE 1104 /* per-block staging bytes (64 groups x 17, padded) */

__global__ __launch_bounds__(UA_BLOCK) void k_enc_msb_flags(
    const u64 *__restrict__ uids, u64 n, u32 *__restrict__ flags) {
    u64 i = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0) || (((uids[i] ^ uids[i - 1]) >> 32) != 0);
}

/* run/block starts: out[rank(i)] = i for flagged i; thread n writes the
 * total sentinel out[count] = n */
__global__ __launch_bounds__(UA_BLOCK) void k_enc_mark_start(
    const u32 *__restrict__ flags, const u64 *__restrict__ offs,
    const u64 *__restrict__ partials, u64 n, u64 *__restrict__ out) {
    u64 i = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        out[d_off(offs, partials, n)] = n;
        return;
    }
    if (flags[i]) out[d_off(offs, partials, i)] = i;
}

/* msb flags -> block flags (in place): also split every block_size-th
 * element of each 32-MSB run (codec.go:117-126; blockSize 0 -> 1-uid blocks) */
__global__ __launch_bounds__(UA_BLOCK) void k_enc_block_flags(
    u32 *__restrict__ flags, const u64 *__restrict__ offs,
    const u64 *__restrict__ partials, const u64 *__restrict__ run_start, u64 n,
    u32 bs) {
    u64 i = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (i >= n) return;
    if (flags[i]) return; /* already a boundary */
    u64 rid = d_off(offs, partials, i) + flags[i] - 1; /* inclusive rank - 1 */
    u64 rs = run_start[rid];
    u32 eff = bs ? bs : 1;
    flags[i] = (((i - rs) % eff) == 0);
}

__global__ __launch_bounds__(UA_BLOCK) void k_encode_blocks(
    const u64 *__restrict__ uids, const u64 *__restrict__ bstart, u64 nb,
    u64 *__restrict__ bases, u32 *__restrict__ nums, u32 *__restrict__ blk_bytes,
    u8 *__restrict__ stage) {
    __shared__ u8 sbytes[UA_PKW][UA_ENC_STRIDE];
    int wv = threadIdx.x >> 6;
    int lane = threadIdx.x & 63;
    u64 b = (u64)blockIdx.x * UA_PKW + wv;
    bool active = (b < nb);
    u64 s = 0, e = 0;
    u32 num = 0, ng = 0;
    if (active) {
        s = bstart[b];
        e = bstart[b + 1];
        num = (u32)(e - s);
        ng = (num > 1) ? ((num + 2) >> 2) : 1; /* >=1 group incl. pad-only (codec.go:76-96) */
        if (lane == 0) {
            bases[b] = uids[s];
            nums[b] = num;
        }
    }
    /* lane g: encode group g (deltas for uids[s+1+4g .. s+4+4g], zero-padded) */
    u32 glen = 0;
    u32 dl[4];
    u8 ln[4];
    if (active && lane < (int)ng) {
        u64 prev = uids[s + (u64)(4 * lane)];
        u32 tot = 1;
        for (int k = 0; k < 4; k++) {
            u64 idx = s + (u64)(4 * lane) + 1 + (u64)k;
            u32 d = (idx < e) ? (u32)(uids[idx] - prev) : 0;
            if (idx < e) prev = uids[idx];
            dl[k] = d;
            ln[k] = (u8)(1 + (d > 0xffu) + (d > 0xffffu) + (d > 0xffffffu));
            tot += ln[k];
        }
        glen = tot;
    }
    /* wave exclusive scan of group byte-lengths */
    u32 incl = glen;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        u32 x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    u32 goff = incl - glen;
    u32 total = (u32)__shfl(incl, 63);
    if (active && lane < (int)ng) {
        u8 *p = &sbytes[wv][goff];
        u8 tag = (u8)((ln[0] - 1) | ((ln[1] - 1) << 2) | ((ln[2] - 1) << 4) |
                      ((ln[3] - 1) << 6));
        *p++ = tag;
        for (int k = 0; k < 4; k++) {
            u32 d = dl[k];
            for (int bcount = 0; bcount < ln[k]; bcount++) {
                *p++ = (u8)(d & 0xff);
                d >>= 8;
            }
        }
    }
    __syncthreads(); /* cross-lane LDS visibility before the copy-out */
    if (!active) return;
    u8 *gdst = stage + b * UA_ENC_STRIDE;
    for (u32 i = lane; i < total; i += 64) gdst[i] = sbytes[wv][i];
    if (lane == 0) blk_bytes[b] = total;
}

__global__ __launch_bounds__(UA_BLOCK) void k_enc_finalize(
    const u8 *__restrict__ stage, const u32 *__restrict__ blk_bytes,
    const u64 *__restrict__ offs, const u64 *__restrict__ partials, u64 nb,
    u8 *__restrict__ deltas, u64 *__restrict__ delta_offs) {
    u64 b = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    int lane = threadIdx.x & 63;
    if (b > nb) return;
    u64 off = d_off(offs, partials, b);
    if (lane == 0) delta_offs[b] = off;
    if (b == nb) return;
    u32 bytes = blk_bytes[b];
    const u8 *src = stage + b * UA_ENC_STRIDE;
    u8 *dst = deltas + off;
    for (u32 i = lane; i < bytes; i += 64) dst[i] = src[i];
}


/* ---- device-chained merge tree helpers ---- */

/* fill a round's descriptor lengths from the previous round's device lens */
__global__ __launch_bounds__(UA_BLOCK) void k_make_descs(
    UaDesc *__restrict__ descs, const u64 *__restrict__ lens_prev, int nk_prev,
    int npair) {
    int j = blockIdx.x * UA_BLOCK + threadIdx.x;
    if (j >= npair) return;
    descs[j].n = lens_prev[2 * j];
    descs[j].m = (2 * j + 1 < nk_prev) ? lens_prev[2 * j + 1] : 0;
}

/* copy src[0..*len_ptr) to out without a host round-trip for the length */
__global__ __launch_bounds__(UA_BLOCK) void k_copy_len(
    u64 *__restrict__ out, const u64 *__restrict__ src, const u64 *__restrict__ len_ptr) {
    u64 n = *len_ptr;
    for (u64 i = (u64)blockIdx.x * UA_BLOCK + threadIdx.x; i < n;
         i += (u64)gridDim.x * UA_BLOCK)
        out[i] = src[i];
}

/* ==================== kernels: row-wise UID-matrix filter ====================
 * N rows x ONE shared sorted list (query/query.go:1425-1437 updateUidMatrix;
 * worker/task.go:1352,1617,1692,1778): a per-element membership filter over
 * the FLAT element array of a CSR matrix.  Search-based, not merge path: the
 * pair path streams the whole shared list once per row (8*(n_i+m) bytes per
 * row), this reads each element once and probes log2(m) times, the first
 * ~log2(P) probes in an LDS pivot table and the rest inside one stride-wide
 * bracket of the shared list (L2 / Infinity-Cache resident).  Rows exist only
 * as offsets: tiles are cut over the flat array, so row-length skew cannot
 * unbalance the grid, and k_rows_offs recovers each output offset from the
 * keep bits.  Nothing communicates across workgroups. */

#define UA_RTILE 2048                       /* flat elements per workgroup */
#define UA_RSTEPS (UA_RTILE / UA_BLOCK)     /* coalesced 256-wide steps per tile */
#define UA_RWORDS (UA_RTILE / 64)           /* u64 keep-words per tile */
#define UA_ROWS_P 1024                      /* pivot table entries (8 KB of LDS) */
static_assert(UA_RTILE % UA_BLOCK == 0 && UA_RWORDS == 32 && UA_RSTEPS <= 32,
              "one keep-word per wave-step; k_rows_write scans 32 words in one wave");
static_assert(UA_ROWS_P % UA_BLOCK == 0 && UA_ROWS_P % 2 == 0, "pivot table geometry");

/* piv[j] = shared[j * stride] for j < npiv; the pad keeps the table's 16-byte
 * loads defined.  With m <= P the stride is 1 and the table is the list. */
__global__ __launch_bounds__(UA_BLOCK) void k_rows_pivots(
    const u64 *__restrict__ shared, u64 stride, u32 npiv, u64 *__restrict__ piv) {
    u32 j = blockIdx.x * UA_BLOCK + threadIdx.x;
    if (j < UA_ROWS_P) piv[j] = (j < npiv) ? shared[(u64)j * stride] : ~0ull;
}

/* Pass 1: membership of every flat element, one ballot word per wave-step,
 * one keep count per tile.  Both searches look for the LAST entry <= key
 * (found iff that entry == key) with wave-uniform trip counts: the LDS one
 * runs over npiv, the global one gsteps times over a bracket of < stride
 * entries, idling (half == 0) once a lane's bracket is down to one entry.  The
 * 8 elements of a thread advance together so their probes overlap.  Every
 * index stays inside [0, npiv) / [0, m) whatever the data, so an unsorted
 * shared list gives wrong answers but no out-of-bounds access. */
template <int MODE>
__global__ __launch_bounds__(UA_BLOCK) void k_rows_probe(
    const u64 *__restrict__ vals, u64 total, const u64 *__restrict__ shared, u64 m,
    const u64 *__restrict__ piv_g, u32 npiv, u64 stride, int gsteps,
    u64 *__restrict__ kw, u32 *__restrict__ tile_cnt) {
    __shared__ __attribute__((aligned(16))) u64 piv[UA_ROWS_P];
    __shared__ u32 wsum[UA_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 tile = blockIdx.x;

    const ulonglong2 *src = (const ulonglong2 *)piv_g;
    ulonglong2 *dst = (ulonglong2 *)piv;
    for (u32 q = tid; q < (npiv + 1) / 2; q += UA_BLOCK) dst[q] = src[q];

    u64 key[UA_RSTEPS];
    u32 ok = 0;
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        u64 i = tile * UA_RTILE + (u64)s * UA_BLOCK + tid;
        bool in = i < total;
        key[s] = in ? vals[i] : 0;
        ok |= (u32)in << s;
    }
    __syncthreads();

    u32 j[UA_RSTEPS];
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) j[s] = 0;
    for (u32 n = npiv; n > 1; n -= n >> 1) {
        u32 half = n >> 1;
#pragma unroll
        for (int s = 0; s < UA_RSTEPS; s++)
            j[s] = (piv[j[s] + half] <= key[s]) ? j[s] + half : j[s];
    }

    u32 found = 0;
    u64 base[UA_RSTEPS];
    u32 len[UA_RSTEPS];
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        u64 pv = npiv ? piv[j[s]] : ~0ull;
        bool live = npiv && ((ok >> s) & 1);
        found |= (u32)(live && pv == key[s]) << s;
        /* pv < key: the key can only sit strictly between this pivot and the next */
        u64 lo = (u64)j[s] * stride + 1;
        u64 hi = (u64)(j[s] + 1) * stride;
        hi = hi < m ? hi : m;
        bool br = live && pv < key[s] && hi > lo;
        base[s] = br ? lo : 0;
        len[s] = br ? (u32)(hi - lo) : 0;
    }
    if (stride > 1) { /* m > P: shared[0] exists, so base == 0 is a safe idle probe */
        for (int k = 0; k < gsteps; k++) {
#pragma unroll
            for (int s = 0; s < UA_RSTEPS; s++) {
                u32 half = len[s] >> 1;
                u64 v = shared[base[s] + half];
                base[s] += (v <= key[s]) ? half : 0;
                len[s] -= half;
            }
        }
#pragma unroll
        for (int s = 0; s < UA_RSTEPS; s++) {
            u64 v = shared[base[s]];
            found |= (u32)(len[s] != 0 && v == key[s]) << s;
        }
    }

    u32 cnt = 0;
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        bool f = (found >> s) & 1;
        bool keep = ((ok >> s) & 1) && (MODE == UA_ROWS_DIFFERENCE ? !f : f);
        u64 w = __ballot(keep); /* lanes past total vote 0 */
        if (lane == 0) kw[tile * UA_RWORDS + s * (UA_BLOCK / 64) + wv] = w;
        cnt += (u32)__popcll(w);
    }
    if (lane == 0) wsum[wv] = cnt;
    __syncthreads();
    if (tid == 0) tile_cnt[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

/* Pass 2: same tile/element mapping; rank = tile offset + kept in earlier
 * wave-steps + kept lanes below.  No re-search: the keep-words are the answer. */
__global__ __launch_bounds__(UA_BLOCK) void k_rows_write(
    const u64 *__restrict__ vals, const u64 *__restrict__ kw,
    const u64 *__restrict__ offs, const u64 *__restrict__ partials,
    u64 *__restrict__ out_vals) {
    __shared__ u64 skw[UA_RWORDS];
    __shared__ u32 spre[UA_RWORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 tile = blockIdx.x;
    if (wv == 0) { /* wave-uniform: all 64 lanes take the shuffles */
        u64 w = lane < UA_RWORDS ? kw[tile * UA_RWORDS + lane] : 0;
        u32 c = (u32)__popcll(w), incl = c;
#pragma unroll
        for (int o = 1; o < UA_RWORDS; o <<= 1) {
            u32 x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        if (lane < UA_RWORDS) {
            skw[lane] = w;
            spre[lane] = incl - c;
        }
    }
    __syncthreads();
    const u64 tbase = d_off(offs, partials, tile);
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        int q = s * (UA_BLOCK / 64) + wv;
        u64 w = skw[q];
        if ((w >> lane) & 1) { /* a set bit implies i < total */
            u64 i = tile * UA_RTILE + (u64)s * UA_BLOCK + tid;
            out_vals[tbase + spre[q] + (u32)__popcll(w & ((1ull << lane) - 1))] = vals[i];
        }
    }
}

/* One thread per row boundary: the kept count before flat position pos is the
 * tile's scanned offset plus the popcount of the tile's keep bits below pos.
 * Needs no per-row descriptor or tile, and any number of boundaries (empty
 * rows included) may fall into one tile.  row_offs is clamped to total, so a
 * broken offsets array gives wrong offsets but in-bounds reads. */
__global__ __launch_bounds__(UA_BLOCK) void k_rows_offs(
    const u64 *__restrict__ row_offs, u64 n_rows, u64 total, const u64 *__restrict__ kw,
    const u64 *__restrict__ offs, const u64 *__restrict__ partials,
    u64 *__restrict__ out_row_offs) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r > n_rows) return;
    u64 pos = row_offs[r];
    pos = pos < total ? pos : total;
    u64 t = pos / UA_RTILE; /* == ntiles only with rem == 0: scan has that entry */
    u32 rem = (u32)(pos % UA_RTILE);
    u64 acc = d_off(offs, partials, t);
    const u64 *tw = kw + t * UA_RWORDS;
    for (u32 k = 0; k < rem / 64; k++) acc += (u64)__popcll(tw[k]);
    if (rem & 63) acc += (u64)__popcll(tw[rem / 64] & ((1ull << (rem & 63)) - 1));
    out_row_offs[r] = acc;
}

/* ==================== kernels: CSR UID matrix -> fan-out of UidPacks ====================
 * The inverse of the row decoders: every row of a CSR matrix
 * through codec.Encoder{BlockSize} (codec.go:57-136) in one call, into the flat
 * block arena the row decoders read.  The geometry is the row filter's: tiles
 * are cut over the FLAT element array, element e of a tile is lane e % 64 of
 * wave-step e / 64, so ballot word q covers elements [64q, 64q + 64) in order
 * and row lengths or block counts cannot unbalance the grid.
 *
 * Every element knows from O(1) state what it contributes:
 *   hard(i)  a row starts at i, or the upper 32 bits change from i - 1 to i;
 *   h(i)     the last hard index <= i (in the tile, else the tile's carry-in);
 *   p(i)     (i - h(i)) mod max(block_size, 1), its position in its block;
 *   start(i) p(i) == 0;  last(i) = start(i + 1) or i + 1 == total.
 * Bytes are attributed to elements so that a tile's bytes are one contiguous
 * range of the blob: element p >= 1 owns its delta (1-4 bytes), the control
 * byte of its group when (p - 1) % 4 == 0, and, when it is last, the group's
 * 3 - (p - 1) % 4 zero pads; a one-uid block's element owns the all-zero group
 * (5 bytes).  The count and the write pass are ONE template, so the write pass
 * stores exactly what the count pass counted. */

#define UA_RENC_LDS (5 * UA_RTILE + 3 + 16 + 13) /* tile bytes + alignment shift, 16-multiple */
/* Per element: 5 (one-uid block), or at most 4 + 1 + 3 = 8 (a 4-byte delta
 * that opens a group and ends the block).  A whole block of c >= 2 uids in g
 * groups is 5g + 3(c - 1) <= 4.25c bytes.  Only the tail of a block cut by the
 * tile's lower edge can exceed 5 per element: full groups cost 17 per 4, and
 * a last partial group of j elements 5 + 3j against 5j, +3 at j = 1.  So a
 * tile holds at most 5 * UA_RTILE + 3 bytes, placed behind a shift < 16. */
static_assert(UA_RENC_LDS >= 5 * UA_RTILE + 3 + 15 && UA_RENC_LDS % 16 == 0,
              "k_rowenc: LDS holds a tile's worst-case bytes behind the alignment shift");
static_assert(UA_RTILE == UA_RWORDS * 64 && UA_RSTEPS * (UA_BLOCK / 64) == UA_RWORDS,
              "k_rowenc: ballot word q covers elements [64q, 64q + 64)");

/* one thread per row: a non-empty row sets the bit of its (clamped) start.
 * The bitmap has one spare word past the last tile for the halo bit. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowenc_rowbits(
    const u64 *__restrict__ row_offs, u64 n_rows, u64 total,
    unsigned long long *__restrict__ rowbits) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    u64 a = row_offs[r], b = row_offs[r + 1];
    a = a < total ? a : total;
    b = b < total ? b : total;
    if (a < b) atomicOr(&rowbits[a >> 6], 1ull << (a & 63)); /* a < total */
}

template <bool WRITE>
__global__ __launch_bounds__(UA_BLOCK) void k_rowenc(
    const u64 *__restrict__ vals, u64 total, const u64 *__restrict__ row_offs, u64 n_rows,
    const u64 *__restrict__ rowbits, u32 eff, /* max(block_size, 1) */
    u64 *__restrict__ kw, u32 *__restrict__ tile_blocks, u32 *__restrict__ tile_bytes,
    const u64 *__restrict__ boffs, const u64 *__restrict__ bpart,
    const u64 *__restrict__ yoffs, const u64 *__restrict__ ypart,
    u64 *__restrict__ bases, u32 *__restrict__ num_uids, u64 *__restrict__ delta_offs,
    u64 cap_blocks, u8 *__restrict__ deltas, u64 cap_deltas) {
    __shared__ u64 s_hard[UA_RWORDS + 1];  /* [UA_RWORDS] bit 0: hard(t0 + UA_RTILE) */
    __shared__ u64 s_start[UA_RWORDS + 1]; /* [UA_RWORDS] bit 0: last(t0 + UA_RTILE - 1) */
    __shared__ int s_hprev[UA_RWORDS];     /* last hard element below word q, or -1 */
    __shared__ u32 s_bpre[UA_RWORDS], s_ypre[UA_RWORDS], s_ysum[UA_RWORDS];
    __shared__ u32 s_r0;                   /* (t0 - rs) mod eff: the carry-in position */
    __shared__ __attribute__((aligned(16))) u8 s_bytes[WRITE ? UA_RENC_LDS : 16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 tile = blockIdx.x;
    const u64 t0 = tile * UA_RTILE;

    /* ---- loads, hard flags ---- */
    u64 v[UA_RSTEPS], pv[UA_RSTEPS];
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int q = s * (UA_BLOCK / 64) + wv;
        u64 i = t0 + (u64)s * UA_BLOCK + tid;
        bool in = i < total;
        v[s] = in ? vals[i] : 0;
        pv[s] = (in && i > 0) ? vals[i - 1] : 0;
        u64 rb = rowbits[tile * UA_RWORDS + q]; /* wave-uniform address */
        bool hard = in && (i == 0 || ((rb >> lane) & 1) || ((v[s] ^ pv[s]) >> 32) != 0);
        u64 w = __ballot(hard);
        if (lane == 0) s_hard[q] = w;
    }
    if (tid == 0) { /* the element after the tile: its hard flag ends a block here */
        u64 i = t0 + UA_RTILE;
        bool hard = false;
        if (i < total)
            hard = (rowbits[(tile + 1) * UA_RWORDS] & 1) || ((vals[i] ^ vals[i - 1]) >> 32) != 0;
        s_hard[UA_RWORDS] = hard ? 1 : 0;
    }

    /* ---- carry-in (wave 0, wave-uniform): the run start of element t0 ----
     * The row holding t0 starts at the last row_offs entry <= t0; inside it the
     * run starts at the first value with t0's upper 32 bits.  Both searches
     * stay inside their arrays whatever the data; rs is clamped into [0, t0]. */
    if (wv == 0) {
        u64 idx = d_wave_lower_bound(row_offs, n_rows + 1, t0 + 1, lane); /* first > t0 */
        u64 rstart = idx ? row_offs[idx - 1] : 0;
        rstart = rstart < t0 ? rstart : t0;
        u64 key = (vals[t0] >> 32) << 32; /* t0 < total: the grid has no empty tile */
        u64 rs = rstart + d_wave_lower_bound(vals + rstart, t0 - rstart, key, lane);
        rs = __builtin_amdgcn_readfirstlane((u32)rs) |
             ((u64)__builtin_amdgcn_readfirstlane((u32)(rs >> 32)) << 32);
        if (lane == 0) s_r0 = (u32)((t0 - rs) % eff);
    }
    __syncthreads();

    /* ---- last hard element below each word (wave 0) ---- */
    if (wv == 0) {
        u64 w = lane < UA_RWORDS ? s_hard[lane] : 0;
        int last = w ? lane * 64 + 63 - __clzll((long long)w) : -1;
        int run = last; /* inclusive prefix max */
#pragma unroll
        for (int o = 1; o < UA_RWORDS; o <<= 1) {
            int x = __shfl_up(run, o);
            if (lane >= o) run = run > x ? run : x;
        }
        int excl = __shfl_up(run, 1);
        if (lane < UA_RWORDS) s_hprev[lane] = lane ? excl : -1;
    }
    __syncthreads();

    /* ---- positions, block starts ---- */
    const u32 r0 = s_r0;
    u32 pos[UA_RSTEPS];
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int q = s * (UA_BLOCK / 64) + wv;
        const int e = q * 64 + lane;
        u64 below = s_hard[q] & ((lane == 63) ? ~0ull : ((2ull << lane) - 1)); /* <= lane */
        int h = below ? q * 64 + 63 - __clzll((long long)below) : s_hprev[q];
        pos[s] = (h >= 0) ? (u32)(e - h) % eff : (r0 + (u32)e) % eff;
        bool in = t0 + (u64)e < total;
        u64 w = __ballot(in && pos[s] == 0);
        if (lane == 0) s_start[q] = w;
    }
    __syncthreads();
    if (tid == 0) {
        /* does a block start right after the tile?  Then element UA_RTILE - 1 is last. */
        u64 i = t0 + UA_RTILE;
        bool st = true; /* i >= total: the final element is last */
        if (i < total && !(s_hard[UA_RWORDS] & 1)) {
            int hl = s_hard[UA_RWORDS - 1]
                         ? (UA_RWORDS - 1) * 64 + 63 - __clzll((long long)s_hard[UA_RWORDS - 1])
                         : s_hprev[UA_RWORDS - 1];
            u32 p = (hl >= 0) ? (u32)(UA_RTILE - hl) % eff : (r0 + (u32)UA_RTILE) % eff;
            st = (p == 0);
        }
        s_start[UA_RWORDS] = st ? 1 : 0;
    }
    __syncthreads();

    /* ---- bytes per element, in-word prefix ---- */
    u32 blen[UA_RSTEPS], yin[UA_RSTEPS]; /* own bytes; exclusive prefix in the word */
    u32 dl[UA_RSTEPS];
    u32 meta[UA_RSTEPS]; /* bit0 in, bit1 start, bit2 last */
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int q = s * (UA_BLOCK / 64) + wv;
        const int e = q * 64 + lane;
        const u64 i = t0 + (u64)e;
        const bool in = i < total;
        const bool st = (s_start[q] >> lane) & 1;
        /* the next element's start bit; past total every bit is 0, so test the index */
        bool nx = (lane == 63) ? (s_start[q + 1] & 1) : ((s_start[q] >> (lane + 1)) & 1);
        const bool last = in && (nx || i + 1 >= total);
        const u32 p = pos[s];
        u32 d = (u32)(v[s] - pv[s]);
        u32 n = 0;
        if (in) {
            if (p == 0) {
                n = last ? 5 : 0;
            } else {
                u32 k = (p - 1) & 3;
                n = 1 + (d > 0xffu) + (d > 0xffffu) + (d > 0xffffffu) + (k == 0 ? 1 : 0) +
                    (last ? 3 - k : 0);
            }
        }
        dl[s] = d;
        blen[s] = n;
        meta[s] = (u32)in | ((u32)st << 1) | ((u32)last << 2);
        u32 incl = n;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            u32 x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        yin[s] = incl - n;
        if (lane == 63) s_ysum[q] = incl;
    }
    __syncthreads();

    /* ---- per-word prefixes of block starts and bytes (wave 0) ---- */
    if (wv == 0) {
        u32 cb = lane < UA_RWORDS ? (u32)__popcll(s_start[lane]) : 0;
        u32 cy = lane < UA_RWORDS ? s_ysum[lane] : 0;
        u32 ib = cb, iy = cy;
#pragma unroll
        for (int o = 1; o < UA_RWORDS; o <<= 1) {
            u32 x = __shfl_up(ib, o), y = __shfl_up(iy, o);
            if (lane >= o) {
                ib += x;
                iy += y;
            }
        }
        if (lane < UA_RWORDS) {
            s_bpre[lane] = ib - cb;
            s_ypre[lane] = iy - cy;
        }
        if (!WRITE) {
            if (lane < UA_RWORDS) kw[tile * UA_RWORDS + lane] = s_start[lane];
            if (lane == UA_RWORDS - 1) {
                tile_blocks[tile] = ib;
                tile_bytes[tile] = iy;
            }
        }
    }
    if (!WRITE) return;
    __syncthreads();

    /* ---- write pass: headers from the elements, bytes through LDS ---- */
    const u64 bbase = d_off(boffs, bpart, tile);
    const u64 ybase = d_off(yoffs, ypart, tile);
    const u32 ytot = s_ypre[UA_RWORDS - 1] + s_ysum[UA_RWORDS - 1];
    const u32 shift = (u32)(((uintptr_t)deltas + ybase) & 15);
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int q = s * (UA_BLOCK / 64) + wv;
        const bool in = meta[s] & 1, st = (meta[s] >> 1) & 1, last = (meta[s] >> 2) & 1;
        const u32 p = pos[s];
        const u32 yo = s_ypre[q] + yin[s];
        /* inclusive block rank: a block begun in an earlier tile is bbase - 1 */
        u32 rk = s_bpre[q] + (u32)__popcll(s_start[q] & ((lane == 63) ? ~0ull : ((2ull << lane) - 1)));
        u64 b = bbase + rk - 1; /* wraps past cap_blocks only on malformed input */
        if (in && b < cap_blocks) {
            if (st) {
                bases[b] = v[s];
                delta_offs[b] = ybase + yo;
            }
            if (last) num_uids[b] = p + 1;
        }
        if (in && blen[s] && shift + yo + blen[s] <= UA_RENC_LDS) {
            u8 *o = s_bytes + shift + yo;
            if (p == 0) { /* one-uid block: the all-zero group */
#pragma unroll
                for (int k = 0; k < 5; k++) o[k] = 0;
            } else {
                const u32 k = (p - 1) & 3;
                if (k == 0) o++; /* the control byte is assembled below */
                u32 d = dl[s];
                *o++ = (u8)d;
                if (d > 0xffu) *o++ = (u8)(d >> 8);
                if (d > 0xffffu) *o++ = (u8)(d >> 16);
                if (d > 0xffffffu) *o++ = (u8)(d >> 24);
                if (last)
                    for (u32 z = k; z < 3; z++) *o++ = 0;
            }
        }
    }
    __syncthreads();
    /* control bytes: the group's opener ORs in its followers' length codes.
     * Followers are the next up-to-3 elements of the same block; they may lie
     * in the next tile, which is why the opener reads them from global. */
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int q = s * (UA_BLOCK / 64) + wv;
        const int e = q * 64 + lane;
        const u64 i = t0 + (u64)e;
        const bool in = meta[s] & 1, last = (meta[s] >> 2) & 1;
        const u32 p = pos[s];
        const u32 yo = s_ypre[q] + yin[s];
        if (in && p != 0 && ((p - 1) & 3) == 0 && shift + yo < UA_RENC_LDS) {
            u32 d = dl[s];
            u32 tag = (d > 0xffu) + (d > 0xffffu) + (d > 0xffffffu);
            /* followers j = 1..3 exist while the block goes on: no start bit at
             * i + j, i + j < total, and p + j < eff */
            bool go = !last;
            u64 prev = v[s];
            for (u32 j = 1; j < 4 && go; j++) {
                u64 ij = i + j;
                if (ij >= total || p + j >= eff) break;
                u64 x = vals[ij];
                bool hardj;
                if (e + (int)j < UA_RTILE) {
                    hardj = (s_start[(e + j) >> 6] >> ((e + j) & 63)) & 1;
                } else { /* past the tile: its row bit and 32-MSB test */
                    hardj = ((rowbits[ij >> 6] >> (ij & 63)) & 1) || ((x ^ prev) >> 32) != 0;
                }
                if (hardj) break;
                u32 dj = (u32)(x - prev);
                tag |= (u32)((dj > 0xffu) + (dj > 0xffffu) + (dj > 0xffffffu)) << (2 * j);
                prev = x;
            }
            s_bytes[shift + yo] = (u8)tag;
        }
    }
    __syncthreads();
    /* copy-out: [ybase, ybase + ytot) clipped to cap_deltas; 16-byte stores
     * for the chunks that lie whole inside the range, bytes for the edges */
    u64 yend = ybase + ytot;
    if (yend > cap_deltas) yend = cap_deltas;
    if (ybase >= yend) return;
    const u32 nby = (u32)(yend - ybase);
    u32 nlds = shift + nby;
    if (nlds > UA_RENC_LDS) nlds = UA_RENC_LDS;
    u8 *gbase = deltas + ybase - shift; /* 16-byte aligned; [shift, nlds) is ours */
    const u32 c0 = shift ? 1 : 0, c1 = nlds / 16; /* whole chunks [c0, c1) */
    for (u32 cidx = c0 + tid; cidx < c1; cidx += UA_BLOCK)
        *(uint4 *)(gbase + 16 * cidx) = *(const uint4 *)(s_bytes + 16 * cidx);
    if (shift) {
        u32 hend = nlds < 16 ? nlds : 16;
        for (u32 k = shift + tid; k < hend; k += UA_BLOCK) gbase[k] = s_bytes[k];
    }
    if (16 * c1 < nlds && !(shift && c1 == 0)) /* c1 == 0 behind a shift: the head was all */
        for (u32 k = 16 * c1 + tid; k < nlds; k += UA_BLOCK) gbase[k] = s_bytes[k];
}

/* One thread per row boundary, k_rows_offs' arithmetic over the block-start
 * words: the blocks before flat position pos are the tile's scanned base plus
 * the start bits below pos.  Thread n_rows takes pos = total whatever
 * row_offs says, so row_block_base[n_rows] is the block count; it also
 * publishes both sizes and closes delta_offs. */
__global__ __launch_bounds__(UA_BLOCK) void k_rowenc_rows(
    const u64 *__restrict__ row_offs, u64 n_rows, u64 total, u64 ntiles,
    const u64 *__restrict__ kw, const u64 *__restrict__ boffs, const u64 *__restrict__ bpart,
    const u64 *__restrict__ yoffs, const u64 *__restrict__ ypart,
    u64 *__restrict__ row_block_base, u64 *__restrict__ delta_offs, u64 cap_blocks,
    u64 *__restrict__ sizes) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r > n_rows) return;
    u64 pos = (r == n_rows) ? total : row_offs[r];
    pos = pos < total ? pos : total;
    u64 t = pos / UA_RTILE; /* == ntiles only with rem == 0: the scans have that entry */
    u32 rem = (u32)(pos % UA_RTILE);
    u64 acc = d_off(boffs, bpart, t);
    const u64 *tw = kw + t * UA_RWORDS;
    for (u32 k = 0; k < rem / 64; k++) acc += (u64)__popcll(tw[k]);
    if (rem & 63) acc += (u64)__popcll(tw[rem / 64] & ((1ull << (rem & 63)) - 1));
    row_block_base[r] = acc;
    if (r == n_rows) {
        u64 db = d_off(yoffs, ypart, ntiles);
        sizes[0] = acc;
        sizes[1] = db;
        if (delta_offs && acc <= cap_blocks) delta_offs[acc] = db;
    }
}

/* ==================== kernels: sort and paginate a CSR UID matrix ====================
 * Order and pagination of every row of a CSR matrix in one call (DESIGN.md
 * §4.11): applyPagination (query/query.go:2493-2507), sortWithoutIndex
 * (worker/sort.go:139-187: sortByValue :775-821, paginate :740-772),
 * sortAndPaginateUsingVar (query/query.go:2697-2738) and the cascade
 * paginations (query/query.go:1483-1487, 3006-3010), with x.PageRange
 * (x/x.go:815-844) word for word.
 *
 * A record is (key', tag): key' = key, ~key under UA_SORT_DESC, 0 for an
 * element without a key; tag = null << 31 | flat input index.  Inside a row
 * records are ordered by (null, key', index), which is a total order, so every
 * merge below is deterministic and ties keep input order in both directions.
 * Tiles are cut over the FLAT element array; a row's segments are its
 * intersections with the tile grid.  k_rsort_tiles sorts each tile by (row,
 * record), which finishes every row inside one tile; round k of k_rsort_round
 * merges a row's groups of 2^k segments pairwise, aligned to the ROW's first
 * tile, between two record buffers.  A row of s segments is final after
 * ceil(log2 s) rounds, so the buffer it ends in follows from s alone. */

#define UA_RS_IDX 0x7fffffffu /* tag: flat input index */
#define UA_RS_NULL 0x80000000u /* tag: the element has no key */
static_assert(UA_RTILE == 2048 && UA_RWORDS == 32,
              "k_rsort_tiles packs (row in tile, null, position in tile) into 11+1+11 bits");

__device__ __forceinline__ bool d_rs_less(u64 kx, u32 tx, u64 ky, u32 ty) {
    const u32 nx = tx >> 31, ny = ty >> 31;
    if (nx != ny) return nx < ny;
    if (kx != ky) return kx < ky;
    return tx < ty;
}

__device__ __forceinline__ u32 d_rs_ceil_log2(u32 s) { /* s >= 1 */
    return s <= 1 ? 0u : 32u - (u32)__clz(s - 1);
}

/* row r's clamped range [a, b) and its segment count (0 for an empty row) */
__device__ __forceinline__ void d_rs_row(const u64 *__restrict__ row_offs, u64 r, u64 total,
                                         u32 &a, u32 &b, u32 &nseg) {
    u64 x = row_offs[r], y = row_offs[r + 1];
    x = x < total ? x : total;
    y = y < total ? y : total;
    if (y < x) y = x;
    a = (u32)x;
    b = (u32)y;
    nseg = (b > a) ? (b - 1) / UA_RTILE - a / UA_RTILE + 1 : 0;
}

/* one thread per row: a non-empty row sets the bit of its (clamped) start, as
 * k_rowenc_rowbits does, and the largest segment count goes to *maxseg */
__global__ __launch_bounds__(UA_BLOCK) void k_rsort_rowbits(
    const u64 *__restrict__ row_offs, u64 n_rows, u64 total,
    unsigned long long *__restrict__ rowbits, u32 *__restrict__ maxseg) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r >= n_rows) return;
    u32 a, b, nseg;
    d_rs_row(row_offs, r, total, a, b, nseg);
    if (a < b) atomicOr(&rowbits[a >> 6], 1ull << (a & 63)); /* a < total */
    /* elements past the last row belong to no row: keep them out of its sort */
    if (r == n_rows - 1 && b < total) atomicOr(&rowbits[b >> 6], 1ull << (b & 63));
    if (nseg > 1) atomicMax(maxseg, nseg);
}

/* One workgroup per UA_RTILE flat elements: sort the tile in LDS by (row in
 * tile, null, key', position) and store the records at the tile's own flat
 * positions.  The row number of an element is the count of row-start bits at
 * or below it, so no row descriptor is read.  Padding past total carries the
 * largest local tag and sorts last.  tile_rows[2t], [2t + 1]: the rows holding
 * the tile's first and last element (upper bounds over row_offs; a broken
 * row_offs gives some row, which k_rsort_round checks before it trusts it). */
__global__ __launch_bounds__(UA_BLOCK) void k_rsort_tiles(
    const u64 *__restrict__ keys, const u8 *__restrict__ has, u64 total, u32 desc,
    const u64 *__restrict__ rowbits, const u64 *__restrict__ row_offs, u64 n_rows,
    u64 *__restrict__ rkey, u32 *__restrict__ rtag, u32 *__restrict__ tile_rows) {
    __shared__ u64 s_key[UA_RTILE];
    __shared__ u32 s_tag[UA_RTILE];
    __shared__ u32 s_wpre[UA_RWORDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 tile = blockIdx.x;
    const u64 t0 = tile * UA_RTILE;
    const int len = (int)((total - t0 < UA_RTILE) ? total - t0 : UA_RTILE); /* t0 < total */

    if (wv == 0) { /* exclusive scan of the 32 words' start-bit counts; the bit
                    * of the tile's first element does not count, so rows number
                    * 0 .. UA_RTILE - 1 whether or not a row starts at t0 */
        u64 w = lane < UA_RWORDS ? rowbits[tile * UA_RWORDS + lane] : 0;
        if (lane == 0) w &= ~1ull;
        u32 cw = (u32)__popcll(w);
        u32 incl = cw;
#pragma unroll
        for (int o = 1; o < UA_RWORDS; o <<= 1) {
            u32 x = __shfl_up(incl, o);
            if (lane >= o) incl += x;
        }
        if (lane < UA_RWORDS) s_wpre[lane] = incl - cw;
    } else if (wv <= 2) { /* waves 1, 2: the rows of the first and the last element */
        u64 p = (wv == 1) ? t0 : t0 + (u64)len - 1;
        u64 idx = d_wave_lower_bound(row_offs, n_rows + 1, p + 1, lane); /* first > p */
        u64 r = idx ? idx - 1 : 0;
        if (r >= n_rows) r = n_rows - 1; /* n_rows >= 1: total > 0 */
        if (lane == 0) tile_rows[2 * tile + (wv - 1)] = (u32)r;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int i = s * UA_BLOCK + tid, q = i >> 6;
        u64 k = 0;
        u32 tg = 0xffffffffu;
        if (i < len) {
            bool hv = has ? has[t0 + i] != 0 : true;
            k = keys[t0 + i];
            k = hv ? (desc ? ~k : k) : 0;
            u64 w = rowbits[tile * UA_RWORDS + q]; /* wave-uniform address */
            if (q == 0) w &= ~1ull;
            u32 row = s_wpre[q] + (u32)__popcll(w & ((2ull << lane) - 1)); /* < UA_RTILE */
            tg = (row << 12) | ((hv ? 0u : 1u) << 11) | (u32)i;
        }
        s_key[i] = k;
        s_tag[i] = tg;
    }
    __syncthreads();
    /* the bitonic network of k_sort_chunks over (tag >> 11, key, tag) */
    for (int k = 2; k <= UA_RTILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < UA_RTILE; i += UA_BLOCK) {
                int p = i ^ j;
                if (p > i) {
                    bool up = ((i & k) == 0);
                    u64 kx = s_key[i], ky = s_key[p];
                    u32 tx = s_tag[i], ty = s_tag[p];
                    u32 hx = tx >> 11, hy = ty >> 11;
                    bool gt = hx != hy ? hx > hy : (kx != ky ? kx > ky : tx > ty);
                    if (gt == up) {
                        s_key[i] = ky;
                        s_key[p] = kx;
                        s_tag[i] = ty;
                        s_tag[p] = tx;
                    }
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int i = s * UA_BLOCK + tid;
        if (i < len) { /* the len real records sort before the padding */
            u32 tg = s_tag[i];
            rkey[t0 + i] = s_key[i];
            rtag[t0 + i] = (((tg >> 11) & 1u) << 31) | (u32)(t0 + (tg & (UA_RTILE - 1)));
        }
    }
}

/* merge-path split of diagonal d over A[0, na) and B[0, nb): the number of A
 * records among the first d of the merge.  The order is total, so one strict
 * comparison decides.  Every probe lies inside A or B. */
__device__ __forceinline__ u32 d_rs_split(const u64 *__restrict__ ak, const u32 *__restrict__ at,
                                          u32 na, const u64 *__restrict__ bk,
                                          const u32 *__restrict__ bt, u32 nb, u32 d) {
    u32 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        u32 m = (lo + hi) >> 1; /* m < na, d - 1 - m < nb */
        if (d_rs_less(ak[m], at[m], bk[d - 1 - m], bt[d - 1 - m])) lo = m + 1;
        else hi = m;
    }
    return lo;
}

/* Round k, one workgroup per flat tile: for the (at most two) rows that span
 * several tiles and touch this tile, produce the records of the tile's own
 * flat positions in the merge of the row's group pair, from src into dst.  A
 * group without a partner is copied.  Rows that are final (2^k >= segments)
 * and rows inside one tile are not touched.  Every value that decides a
 * barrier is workgroup-uniform: it comes from blockIdx, kernel arguments and
 * LDS words written before a barrier. */
__global__ __launch_bounds__(UA_BLOCK) void k_rsort_round(
    const u64 *__restrict__ row_offs, u64 n_rows, u64 total, const u32 *__restrict__ tile_rows,
    const u32 *__restrict__ maxseg, u32 k, const u64 *__restrict__ skey,
    const u32 *__restrict__ stag, u64 *__restrict__ dkey, u32 *__restrict__ dtag) {
    __shared__ u64 s_key[UA_RTILE];
    __shared__ u32 s_tag[UA_RTILE];
    __shared__ u32 s_sp[2];
    const int tid = threadIdx.x;
    if (((u64)1 << k) >= (u64)*maxseg) return; /* uniform: no row needs this round */
    const u32 t = blockIdx.x;
    const u32 t0 = t * UA_RTILE;
    const u32 tend = (total - t0 < UA_RTILE) ? (u32)total : t0 + UA_RTILE;
    u32 rows[2] = {tile_rows[2 * t], tile_rows[2 * t + 1]};
    const int nparts = rows[0] == rows[1] ? 1 : 2;
    for (int part = 0; part < nparts; part++) {
        u32 r = rows[part];
        if (r >= n_rows) continue; /* uniform */
        u32 a, b, nseg;
        d_rs_row(row_offs, r, total, a, b, nseg);
        /* the row must hold the tile's first (part 0) or last (part 1) element */
        const u32 probe = part == 0 ? t0 : tend - 1;
        if (!(a <= probe && probe < b) || nseg < 2 || ((u64)1 << k) >= nseg) continue;
        const u32 T0 = a / UA_RTILE, j = t - T0; /* j < nseg */
        const u32 s0 = (j >> (k + 1)) << (k + 1), smid = s0 + (1u << k);
        u64 s1w = (u64)s0 + ((u64)2 << k);
        const u32 s1 = s1w < nseg ? (u32)s1w : nseg;
        const u32 o0 = a > t0 ? a : t0, o1 = b < tend ? b : tend; /* o0 < o1 <= o0 + UA_RTILE */
        const u32 cnt = o1 - o0;
        if (smid >= nseg) { /* no partner: copy */
            for (u32 i = tid; i < cnt; i += UA_BLOCK) {
                dkey[o0 + i] = skey[o0 + i];
                dtag[o0 + i] = stag[o0 + i];
            }
            continue;
        }
        const u32 L0 = s0 == 0 ? a : (T0 + s0) * UA_RTILE;
        const u32 L1 = (T0 + smid) * UA_RTILE; /* smid < nseg: inside the row */
        const u32 R1 = s1 >= nseg ? b : (T0 + s1) * UA_RTILE;
        const u32 na = L1 - L0, nb = R1 - L1;
        __syncthreads(); /* the previous part's LDS reads are done */
        if (tid < 2)
            s_sp[tid] = d_rs_split(skey + L0, stag + L0, na, skey + L1, stag + L1, nb,
                                   (tid == 0 ? o0 : o1) - L0);
        __syncthreads();
        const u32 i0 = s_sp[0], i1 = s_sp[1];
        const u32 j0 = (o0 - L0) - i0;
        const u32 ca = i1 - i0; /* A records; the other cnt - ca come from B at j0 */
        for (u32 i = tid; i < cnt; i += UA_BLOCK) {
            u32 g = i < ca ? L0 + i0 + i : L1 + j0 + (i - ca);
            s_key[i] = skey[g];
            s_tag[i] = stag[g];
        }
        __syncthreads();
        u64 mk[UA_RSTEPS];
        u32 mt[UA_RSTEPS], mr[UA_RSTEPS];
#pragma unroll
        for (int s = 0; s < UA_RSTEPS; s++) {
            const u32 i = (u32)s * UA_BLOCK + tid;
            mr[s] = UA_RTILE;
            if (i < cnt) {
                mk[s] = s_key[i];
                mt[s] = s_tag[i];
                /* rank = own index in its part + records of the other part below it */
                u32 lo, hi, own;
                if (i < ca) { lo = ca; hi = cnt; own = i; }
                else { lo = 0; hi = ca; own = i - ca; }
                const u32 base = lo;
                while (lo < hi) {
                    u32 m = (lo + hi) >> 1;
                    if (d_rs_less(s_key[m], s_tag[m], mk[s], mt[s])) lo = m + 1;
                    else hi = m;
                }
                mr[s] = own + (lo - base);
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < UA_RSTEPS; s++)
            if (mr[s] < cnt) {
                s_key[mr[s]] = mk[s];
                s_tag[mr[s]] = mt[s];
            }
        __syncthreads();
        for (u32 i = tid; i < cnt; i += UA_BLOCK) {
            dkey[o0 + i] = s_key[i];
            dtag[o0 + i] = s_tag[i];
        }
    }
}

/* x.PageRange (x/x.go:815-844) */
__device__ __forceinline__ void d_page_range(long long count, long long offset, long long n,
                                             long long &start, long long &end) {
    if (n == 0) { start = 0; end = 0; return; }
    if (count == 0 && offset == 0) { start = 0; end = n; return; }
    if (count < 0) {
        if (-count > n) count = -n;
        start = (((n + count) % n) + n) % n;
        end = n;
        return;
    }
    start = offset < 0 ? 0 : offset;
    if (start > n) { start = n; end = n; return; }
    if (count == 0) { end = n; return; }
    end = start + count;
    if (end > n) end = n;
}

/* One thread per row: |V| from the sorted run, PageRange over S, the
 * UA_SORT_MULTI extension by binary search in the run's keys, then the row's
 * output length, the page's first rank and multiSortOffsets.  sorted == 0
 * (page only, or a count-only call whose lengths do not depend on the order)
 * reads no record.  Thread n_rows writes the zero count that closes the scan. */
__global__ __launch_bounds__(UA_BLOCK) void k_rsort_page(
    const u64 *__restrict__ row_offs, u64 n_rows, u64 total, const u64 *__restrict__ key0,
    const u32 *__restrict__ tag0, const u64 *__restrict__ key1, const u32 *__restrict__ tag1,
    u32 sorted, u32 flags, int count, int offset, u32 *__restrict__ row_len,
    u32 *__restrict__ row_start, int *__restrict__ out_ms_offs, u32 *__restrict__ bad) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r > n_rows) return;
    if (r == n_rows) {
        row_len[r] = 0;
        return;
    }
    u32 a, b, nseg;
    d_rs_row(row_offs, r, total, a, b, nseg);
    {   /* a clamped end below its start: rows may overlap, the lengths may sum
         * past total.  The later kernels then publish empty rows. */
        u64 y = row_offs[r + 1];
        if ((y < total ? y : total) < a) atomicOr(bad, 1u);
    }
    const u32 n = b - a;
    u32 nv = n, lenS = n;
    const u64 *rk = nullptr;
    if (sorted && n) {
        const bool odd = d_rs_ceil_log2(nseg) & 1;
        rk = (odd ? key1 : key0) + a;
        const u32 *rt = (odd ? tag1 : tag0) + a;
        u32 lo = 0, hi = n; /* first null of the run */
        while (lo < hi) {
            u32 m = (lo + hi) >> 1;
            if (rt[m] & UA_RS_NULL) hi = m;
            else lo = m + 1;
        }
        nv = lo;
        if ((flags & UA_SORT_DROP_NULLS) && nv) lenS = nv; /* nv == 0: the row stays */
    }
    long long start, end;
    d_page_range(count, offset, lenS, start, end);
    if ((flags & UA_SORT_MULTI) && rk) {
        if (start > 0 && start < nv) { /* first of the equal run holding S[start] */
            const u64 kk = rk[start];
            u32 lo = 0, hi = (u32)start;
            while (lo < hi) {
                u32 m = (lo + hi) >> 1;
                if (rk[m] < kk) lo = m + 1;
                else hi = m;
            }
            start = lo;
        }
        if (end > 0 && end < nv) { /* one past the equal run holding S[end - 1] */
            const u64 kk = rk[end - 1];
            u32 lo = (u32)end, hi = nv;
            while (lo < hi) {
                u32 m = (lo + hi) >> 1;
                if (rk[m] <= kk) lo = m + 1;
                else hi = m;
            }
            end = lo;
        }
    }
    if (end < start) end = start;
    row_len[r] = (u32)(end - start);
    row_start[r] = (u32)start;
    if (out_ms_offs) {
        long long off = offset; /* sort.go:170-178 */
        out_ms_offs[r] = start < off ? (int)(off - start) : 0;
    }
}

/* one thread per boundary: out_row_offs from the scan over the row lengths;
 * thread n_rows also publishes the total.  After a row_offs that descends
 * (*bad) every row is empty: disjoint rows are what keeps the total at or
 * below the input's. */
__global__ __launch_bounds__(UA_BLOCK) void k_rsort_offs(
    u64 n_rows, const u64 *__restrict__ offs, const u64 *__restrict__ part,
    const u32 *__restrict__ bad, u64 *__restrict__ out_row_offs, u64 *__restrict__ out_total) {
    u64 r = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (r > n_rows) return;
    u64 x = *bad ? 0 : d_off(offs, part, r);
    out_row_offs[r] = x;
    if (r == n_rows) *out_total = x;
}

/* last boundary <= o in the scanned lengths, searched inside [lo, hi] */
__device__ __forceinline__ u32 d_rs_row_of(const u64 *__restrict__ offs,
                                           const u64 *__restrict__ part, u32 lo, u32 hi,
                                           u64 o) {
    while (lo < hi) { /* invariant: boundary(lo) <= o */
        u32 m = lo + (hi - lo + 1) / 2;
        if (d_off(offs, part, m) <= o) lo = m;
        else hi = m - 1;
    }
    return lo;
}

/* Flat write pass, one thread per OUTPUT element below min(total, cap_vals):
 * the element's row is the last boundary at or below it in the scanned row
 * lengths (monotone by construction, whatever row_offs holds); the workgroup
 * first brackets the rows of its 256 elements, so a thread searches only
 * those.  The source index comes from the row's run (clamped below total:
 * with a broken row_offs a run may hold records no round wrote), or is the
 * input position itself when the call only pages. */
__global__ __launch_bounds__(UA_BLOCK) void k_rsort_write(
    const u64 *__restrict__ vals, const u64 *__restrict__ row_offs, u64 n_rows, u64 total,
    const u32 *__restrict__ tag0, const u32 *__restrict__ tag1, u32 sorted,
    const u64 *__restrict__ offs, const u64 *__restrict__ part,
    const u32 *__restrict__ row_start, const u32 *__restrict__ bad,
    u64 *__restrict__ out_vals, u64 *__restrict__ out_src, u64 cap_vals) {
    __shared__ u32 s_r[2];
    const int tid = threadIdx.x;
    if (*bad) return; /* uniform: every row was published empty */
    const u64 out_n = d_off(offs, part, n_rows);
    const u64 lim = out_n < cap_vals ? out_n : cap_vals;
    const u64 o_first = (u64)blockIdx.x * UA_BLOCK;
    if (o_first >= lim) return; /* uniform */
    const u64 o_last = (o_first + UA_BLOCK - 1 < lim) ? o_first + UA_BLOCK - 1 : lim - 1;
    if (tid < 2)
        s_r[tid] = d_rs_row_of(offs, part, 0, (u32)n_rows, tid == 0 ? o_first : o_last);
    __syncthreads();
    const u64 o = o_first + tid;
    if (o >= lim) return;
    /* boundary(r) <= o < out_n = boundary(n_rows), so r < n_rows */
    u32 r = d_rs_row_of(offs, part, s_r[0], s_r[1], o);
    if (r >= n_rows) return;
    u32 a, b, nseg;
    d_rs_row(row_offs, r, total, a, b, nseg);
    u64 p = (u64)a + row_start[r] + (o - d_off(offs, part, r)); /* < b by the page kernel */
    if (p >= total) return;
    u64 src = p;
    if (sorted) {
        const u32 *rt = (d_rs_ceil_log2(nseg) & 1) ? tag1 : tag0;
        src = rt[p] & UA_RS_IDX;
        if (src >= total) src = total - 1;
    }
    out_vals[o] = vals[src];
    if (out_src) out_src[o] = src;
}

/* ==================== kernels: transpose a CSR UID matrix ====================
 * src -> [dst...] into dst -> [src...] in one call: the
 * grouping of dedup.addValue (query/groupby.go:104-128) that formResult
 * (:195-260) and fillGroupedVars (:265-361) run per edge, and the reverse
 * postings of rebuildReverseEdges (posting/index.go:1759-1791, one
 * addReverseMutation :276-298 per posting).
 *
 * A record is (value, tag) with tag = dead << 31 | flat input index, in the row
 * sort's layout and under its order d_rs_less: live before dead, then value,
 * then flat index.  That is a total order over the FLAT array, so there is no
 * row segmentation: k_rtr_tiles sorts each tile, round k of k_rtr_round merges
 * groups of 2^k tiles pairwise between the two record buffers, and after
 * ceil(log2 ntiles) rounds the live records are one run ordered by (value,
 * flat index).  A group is a run of equal values, already in addValue's append
 * order.  k_rtr_groups<false> counts group heads and kept entries per tile of
 * that run, one scan runs over both count arrays, k_rtr_groups<true> is the
 * same code with the scanned bases and stores the four outputs. */

#define UA_TR_DEAD UA_RS_NULL /* tag: the element takes no part */

/* One workgroup per UA_RTILE flat elements.  Waves 0 and 1 bracket the rows of
 * the tile's first and last element (first row_offs entry above each); a
 * thread then searches only that bracket.  An element is live when its row r
 * holds it (row_offs[r] <= p < row_offs[r + 1], checked, so a row_offs that is
 * not monotone gives a dead element, never a wrong index), p lies below
 * min(row_offs[n_rows], total) and row_keep admits r.  Comparing the raw
 * row_offs entries against p < total is comparing the clamped ones.  erow[p]
 * gets the row (0 for a dead element), the sorted tile goes to the tile's own
 * flat positions.  Padding past total sorts last. */
__global__ __launch_bounds__(UA_BLOCK) void k_rtr_tiles(
    const u64 *__restrict__ vals, u64 total, const u64 *__restrict__ row_offs, u64 n_rows,
    const u8 *__restrict__ row_keep, u64 *__restrict__ rkey, u32 *__restrict__ rtag,
    u32 *__restrict__ erow) {
    __shared__ u64 s_key[UA_RTILE];
    __shared__ u32 s_tag[UA_RTILE];
    __shared__ u32 s_br[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u64 t0 = (u64)blockIdx.x * UA_RTILE;
    const int len = (int)((total - t0 < UA_RTILE) ? total - t0 : UA_RTILE); /* t0 < total */
    if (wv < 2) {
        const u64 p = (wv == 0) ? t0 : t0 + (u64)len - 1;
        u64 idx = d_wave_lower_bound(row_offs, n_rows + 1, p + 1, lane); /* first > p */
        if (idx > n_rows + 1) idx = n_rows + 1;
        if (lane == 0) s_br[wv] = (u32)idx; /* n_rows < 2^31 */
    }
    __syncthreads();
    const u32 br0 = s_br[0], br1 = s_br[1];
    u64 lim = row_offs[n_rows];
    lim = lim < total ? lim : total;
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int i = s * UA_BLOCK + tid;
        u64 k = ~(u64)0;
        u32 tg = 0xffffffffu;
        if (i < len) {
            const u64 p = t0 + i;
            u32 lo = br0, hi = br1; /* br0 > br1 (broken row_offs): no probe */
            while (lo < hi) {
                u32 m = lo + ((hi - lo) >> 1); /* m < br1 <= n_rows + 1 */
                if (row_offs[m] > p) hi = m;
                else lo = m + 1;
            }
            u32 r = 0;
            bool live = false;
            if (lo >= 1 && lo <= n_rows) {
                r = lo - 1;
                live = p < lim && row_offs[r] <= p && p < row_offs[r + 1] &&
                       (!row_keep || row_keep[r] != 0);
            }
            erow[p] = live ? r : 0;
            k = live ? vals[p] : 0;
            tg = (live ? 0u : UA_TR_DEAD) | (u32)p; /* p < 2^31 */
        }
        s_key[i] = k;
        s_tag[i] = tg;
    }
    __syncthreads();
    /* the bitonic network of k_sort_chunks under d_rs_less */
    for (int k = 2; k <= UA_RTILE; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < UA_RTILE; i += UA_BLOCK) {
                int p = i ^ j;
                if (p > i) {
                    bool up = ((i & k) == 0);
                    u64 kx = s_key[i], ky = s_key[p];
                    u32 tx = s_tag[i], ty = s_tag[p];
                    bool gt = d_rs_less(ky, ty, kx, tx);
                    if (gt == up) {
                        s_key[i] = ky;
                        s_key[p] = kx;
                        s_tag[i] = ty;
                        s_tag[p] = tx;
                    }
                }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const int i = s * UA_BLOCK + tid;
        if (i < len) { /* the len real records sort before the padding */
            rkey[t0 + i] = s_key[i];
            rtag[t0 + i] = s_tag[i];
        }
    }
}

/* Round k, one workgroup per flat tile: the records of the tile's own flat
 * positions in the merge of its group pair (2^k tiles each, the last group of
 * the array may be shorter), from src into dst: two diagonal splits in global
 * memory, at most UA_RTILE records into LDS, each ranked against the other
 * side, a coalesced store.  A group without a partner is copied.  The host
 * enqueues exactly ceil(log2 ntiles) rounds, so every round has work.  All
 * that decides a barrier comes from blockIdx and the kernel arguments. */
__global__ __launch_bounds__(UA_BLOCK) void k_rtr_round(
    u64 total, u32 ntiles, u32 k, const u64 *__restrict__ skey, const u32 *__restrict__ stag,
    u64 *__restrict__ dkey, u32 *__restrict__ dtag) {
    __shared__ u64 s_key[UA_RTILE];
    __shared__ u32 s_tag[UA_RTILE];
    __shared__ u32 s_sp[2];
    const int tid = threadIdx.x;
    const u32 t = blockIdx.x; /* t < ntiles <= 2^20 */
    const u32 o0 = t * UA_RTILE;
    const u32 o1 = (total - o0 < UA_RTILE) ? (u32)total : o0 + UA_RTILE;
    const u32 cnt = o1 - o0;
    const u32 s0 = (t >> (k + 1)) << (k + 1), smid = s0 + (1u << k);
    if (smid >= ntiles) { /* uniform: no partner */
        for (u32 i = tid; i < cnt; i += UA_BLOCK) {
            dkey[o0 + i] = skey[o0 + i];
            dtag[o0 + i] = stag[o0 + i];
        }
        return;
    }
    const u64 s1w = (u64)s0 + ((u64)2 << k);
    const u32 L0 = s0 * UA_RTILE, L1 = smid * UA_RTILE;
    const u32 R1 = s1w >= ntiles ? (u32)total : (u32)s1w * UA_RTILE;
    const u32 na = L1 - L0, nb = R1 - L1; /* L0 <= o0 < o1 <= R1 */
    if (tid < 2)
        s_sp[tid] = d_rs_split(skey + L0, stag + L0, na, skey + L1, stag + L1, nb,
                               (tid == 0 ? o0 : o1) - L0);
    __syncthreads();
    const u32 i0 = s_sp[0], i1 = s_sp[1];
    const u32 j0 = (o0 - L0) - i0;
    const u32 ca = i1 - i0; /* A records; the other cnt - ca come from B at j0 */
    for (u32 i = tid; i < cnt; i += UA_BLOCK) {
        u32 g = i < ca ? L0 + i0 + i : L1 + j0 + (i - ca);
        s_key[i] = skey[g];
        s_tag[i] = stag[g];
    }
    __syncthreads();
    u64 mk[UA_RSTEPS];
    u32 mt[UA_RSTEPS], mr[UA_RSTEPS];
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const u32 i = (u32)s * UA_BLOCK + tid;
        mr[s] = UA_RTILE;
        if (i < cnt) {
            mk[s] = s_key[i];
            mt[s] = s_tag[i];
            /* rank = own index in its part + records of the other part below it */
            u32 lo, hi, own;
            if (i < ca) { lo = ca; hi = cnt; own = i; }
            else { lo = 0; hi = ca; own = i - ca; }
            const u32 base = lo;
            while (lo < hi) {
                u32 m = (lo + hi) >> 1;
                if (d_rs_less(s_key[m], s_tag[m], mk[s], mt[s])) lo = m + 1;
                else hi = m;
            }
            mr[s] = own + (lo - base);
        }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++)
        if (mr[s] < cnt) {
            s_key[mr[s]] = mk[s];
            s_tag[mr[s]] = mt[s];
        }
    __syncthreads();
    for (u32 i = tid; i < cnt; i += UA_BLOCK) {
        dkey[o0 + i] = s_key[i];
        dtag[o0 + i] = s_tag[i];
    }
}

/* One workgroup per tile of the sorted run in UA_RSTEPS coalesced 256-wide
 * steps; a record's rank among the tile's heads (kept entries) is the count in
 * the steps and waves before its own plus the ballot bits of the lanes below
 * it.  head = live and (first or value != previous value);
 * keep = live and not (unique and same value and same row as the previous
 * record), so of equal (value, row) entries the lowest flat index stays.
 * WRITE == false leaves the tile's head count in cnt[tile] and its keep count
 * in cnt[ntiles + 1 + tile] (tile 0 also writes the two closing zeros) and
 * adds both to words[0], words[1].  One exclusive scan over the 2 * (ntiles +
 * 1) counts serves both: a head base is d_off(tile), a keep base d_off(ntiles
 * + 1 + tile) - words[0].  WRITE == true repeats the flags and stores keys and
 * group offsets below cap_keys (+ 1), entries below cap_vals.  Every flat
 * index read from a tag is clamped below total and every row below n_rows. */
template <bool WRITE>
__global__ __launch_bounds__(UA_BLOCK) void k_rtr_groups(
    const u64 *__restrict__ rkey, const u32 *__restrict__ rtag, const u32 *__restrict__ erow,
    u64 total, u64 n_rows, u32 ntiles, u32 unique, u32 *__restrict__ cnt,
    const u64 *__restrict__ offs, const u64 *__restrict__ part,
    unsigned long long *__restrict__ words, const u64 *__restrict__ row_uids,
    u64 *__restrict__ out_keys, u64 *__restrict__ out_offs, u64 cap_keys,
    u64 *__restrict__ out_vals, u64 *__restrict__ out_src, u64 cap_vals) {
    __shared__ u32 s_ch[UA_RSTEPS][UA_BLOCK / 64], s_ck[UA_RSTEPS][UA_BLOCK / 64];
    __shared__ u32 s_tot[2];
    static_assert(UA_RSTEPS * (UA_BLOCK / 64) == 32, "one half wave scans the counts");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const u32 tile = blockIdx.x;
    const u64 t0 = (u64)tile * UA_RTILE;
    const bool rows = unique || (WRITE && out_vals);
    const u64 below = ((u64)1 << lane) - 1;
    u64 ek[UA_RSTEPS];
    u32 es[UA_RSTEPS], er[UA_RSTEPS];
    u32 lh[UA_RSTEPS], lk[UA_RSTEPS]; /* heads and kept entries in the lanes below */
    u32 hm = 0, km = 0;
#pragma unroll
    for (int s = 0; s < UA_RSTEPS; s++) {
        const u64 p = t0 + (u64)s * UA_BLOCK + tid;
        const bool in = p < total;
        u32 tg = UA_TR_DEAD;
        u64 kk = 0;
        if (in) {
            tg = rtag[p];
            kk = rkey[p];
        }
        /* the previous record: the lane below holds it, lane 0 reads it */
        u64 pk = __shfl_up(kk, 1);
        u32 pt = __shfl_up(tg, 1);
        if (lane == 0) {
            pt = UA_TR_DEAD;
            pk = 0;
            if (in && p > 0) {
                pt = rtag[p - 1];
                pk = rkey[p - 1];
            }
        }
        const bool live = !(tg & UA_TR_DEAD);
        const bool same = !(pt & UA_TR_DEAD) && kk == pk;
        u64 src = tg & UA_RS_IDX;
        if (src >= total) src = total - 1; /* total > 0 */
        u32 row = 0;
        bool dup = false;
        if (live && rows) row = erow[src];
        if (live && unique && same) {
            u64 ps = pt & UA_RS_IDX;
            if (ps >= total) ps = total - 1;
            dup = erow[ps] == row;
        }
        const bool head = live && !same;
        const bool keep = live && !dup;
        const u64 bh = __ballot(head), bk = __ballot(keep);
        lh[s] = (u32)__popcll(bh & below);
        lk[s] = (u32)__popcll(bk & below);
        if (lane == 0) {
            s_ch[s][wv] = (u32)__popcll(bh);
            s_ck[s][wv] = (u32)__popcll(bk);
        }
        hm |= (head ? 1u : 0u) << s;
        km |= (keep ? 1u : 0u) << s;
        ek[s] = kk;
        es[s] = (u32)src;
        er[s] = row;
        /* keep the step's flags and counts in vector registers: as lane masks
         * sixteen ballots and conditions live to the stores outgrow the scalar file */
        asm volatile("" : "+v"(lh[s]), "+v"(lk[s]), "+v"(hm), "+v"(km));
    }
    __syncthreads();
    /* records run by (step, wave, lane): wave 0 scans the 32 head counts in its
     * lower half and the 32 keep counts in its upper half, exclusive, in place */
    if (wv == 0) {
        u32 *sc = lane < 32 ? &s_ch[0][0] : &s_ck[0][0];
        const int q = lane & 31;
        const u32 c = sc[q];
        u32 incl = c;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            u32 x = __shfl_up(incl, o);
            if (q >= o) incl += x;
        }
        sc[q] = incl - c;
        if (q == 31) s_tot[lane >> 5] = incl;
    }
    __syncthreads();
    const u32 M = ntiles + 1;
    if constexpr (!WRITE) {
        if (tid == 0) {
            const u32 toth = s_tot[0], totk = s_tot[1];
            cnt[tile] = toth;
            cnt[M + tile] = totk;
            if (tile == 0) {
                cnt[ntiles] = 0;
                cnt[M + ntiles] = 0;
            }
            atomicAdd(&words[0], (unsigned long long)toth);
            atomicAdd(&words[1], (unsigned long long)totk);
        }
    } else {
        const u64 ng = words[0], nt = words[1];
        const u64 gb = d_off(offs, part, tile);
        const u64 eb = d_off(offs, part, (u64)M + tile) - ng;
#pragma unroll
        for (int s = 0; s < UA_RSTEPS; s++) {
            if (!((km >> s) & 1u)) continue; /* a head is always kept */
            const u64 e = eb + s_ck[s][wv] + lk[s];
            if ((hm >> s) & 1u) {
                const u64 g = gb + s_ch[s][wv] + lh[s];
                if (g < cap_keys) out_keys[g] = ek[s];
                if (g <= cap_keys) out_offs[g] = e;
            }
            if (out_vals && e < cap_vals) {
                u64 r = er[s];
                if (r >= n_rows) r = n_rows - 1; /* n_rows >= 1: total > 0 */
                out_vals[e] = row_uids ? row_uids[r] : r;
                if (out_src) out_src[e] = es[s];
            }
        }
        if (tile == 0 && tid == 0 && ng <= cap_keys) out_offs[ng] = nt;
    }
}

/* ==================== host shim ==================== */

static thread_local hipError_t g_last_hip = hipSuccess;

#define HIP_TRY(x)                         \
    do {                                   \
        hipError_t _e = (x);               \
        if (_e != hipSuccess) {            \
            g_last_hip = _e;               \
            return UA_ERR_HIP;             \
        }                                  \
    } while (0)

enum {
    WS_DESC = 0, WS_TB, WS_TPAIR, WS_TA0, WS_TCNT, WS_TOFF, WS_PARTIAL,
    WS_STAGE, WS_STAGEP, WS_POUT, WS_HU, WS_HV, WS_HOUT, WS_PACK, WS_SCRATCH_A,
    WS_SCRATCH_B, WS_LOOK, WS_RPIV, WS_RKW, WS_KLEN, WS_MUT, WS_COUNT
};

struct ua_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    void *ws[WS_COUNT] = {};
    size_t ws_cap[WS_COUNT] = {};
    hipEvent_t ev[4] = {};
    hipStream_t stream_tail = nullptr; /* aux-tail overlap (run_n) */
    hipEvent_t oev[4] = {}; /* [0..1]=tile_done per set, [2..3]=tail_done */
    /* ApplyFilter's lookback flag array (WS_LOOK) bookkeeping */
    uint32_t look_gen = 0;
    size_t look_cleared = 0; /* bytes of the CURRENT WS_LOOK allocation zeroed */
    uint32_t *d_viol = nullptr; /* pack-limit validation flag (1 u32) */
    /* stats */
    uint64_t n_launches = 0;
    double kernel_ms = 0.0;
    uint64_t bytes_algo = 0;
    std::recursive_mutex mu; /* compound ops hold it across internal stages */
};

extern "C" const char *ua_strerror(int code) {
    switch (code) {
        case UA_OK: return "ok";
        case UA_ERR_HIP: return hipGetErrorString(g_last_hip);
        case UA_ERR_NOMEM: return "allocation failed";
        case UA_ERR_INVALID: return "invalid argument";
        case UA_ERR_NO_GPU: return "no HIP device visible";
        default: return "unknown error";
    }
}

extern "C" int ua_version(void) { return 20; }

/* streams and events; on failure the caller destroys c */
static int ctx_init(ua_ctx *c) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamCreate(&c->stream));
    for (int i = 0; i < 4; i++) {
        HIP_TRY(hipEventCreate(&c->ev[i]));
        /* record once eagerly: an event that has never been recorded cannot
         * be captured into a graph on this ROCm (invalid resource handle) */
        HIP_TRY(hipEventRecord(c->ev[i], c->stream));
    }
    HIP_TRY(hipStreamCreate(&c->stream_tail));
    for (int i = 0; i < 4; i++)
        HIP_TRY(hipEventCreateWithFlags(&c->oev[i], hipEventDisableTiming));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UA_OK;
}

extern "C" int ua_ctx_create(ua_ctx **out, int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) return UA_ERR_NO_GPU;
    if (device < 0 || device >= ndev) return UA_ERR_INVALID;
    ua_ctx *c = new ua_ctx();
    c->device = device;
    int rc = ctx_init(c);
    if (rc) {
        ua_ctx_destroy(c);
        return rc;
    }
    *out = c;
    return UA_OK;
}

extern "C" void ua_ctx_destroy(ua_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < WS_COUNT; i++)
        if (c->ws[i]) (void)hipFree(c->ws[i]);
    if (c->d_viol) (void)hipFree(c->d_viol);
    for (int i = 0; i < 4; i++)
        if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
    for (int i = 0; i < 4; i++)
        if (c->oev[i]) (void)hipEventDestroy(c->oev[i]);
    if (c->stream_tail) (void)hipStreamDestroy(c->stream_tail);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static int ws_reserve(ua_ctx *c, int slot, size_t bytes) {
    if (bytes <= c->ws_cap[slot]) return UA_OK;
    if (c->ws[slot]) (void)hipFree(c->ws[slot]);
    c->ws[slot] = nullptr;
    c->ws_cap[slot] = 0;
    size_t cap = bytes + bytes / 4; /* 25% headroom limits realloc churn */
    hipError_t e = hipMalloc(&c->ws[slot], cap);
    if (e != hipSuccess) {
        g_last_hip = e;
        /* retry exact */
        e = hipMalloc(&c->ws[slot], bytes);
        if (e != hipSuccess) return UA_ERR_NOMEM;
        cap = bytes;
    }
    c->ws_cap[slot] = cap;
    return UA_OK;
}

/* Acquire the ctx-level lookback flag array (k_filter) for T chunks with a
 * fresh generation.  The array must read as "stale" for the new generation:
 * guaranteed by zeroing on (re)allocation and re-zeroing when the 16-bit
 * generation wraps. */
static int lb_acquire_ws(ua_ctx *c, u64 T, u64 **flags, u64 *gen) {
    int rc = ws_reserve(c, WS_LOOK, (size_t)T * sizeof(u64));
    if (rc) return rc;
    u64 *f = (u64 *)c->ws[WS_LOOK];
    if (c->look_cleared < c->ws_cap[WS_LOOK] || c->look_gen >= UA_LB_GEN_MAX) {
        HIP_TRY(hipMemsetAsync(f, 0, c->ws_cap[WS_LOOK], c->stream));
        c->look_cleared = c->ws_cap[WS_LOOK];
        c->look_gen = 0;
    }
    c->look_gen += 1;
    *flags = f;
    *gen = c->look_gen;
    return UA_OK;
}

extern "C" int ua_dev_alloc(ua_ctx *c, uint64_t bytes, void **dptr) {
    HIP_TRY(hipSetDevice(c->device));
    hipError_t e = hipMalloc(dptr, bytes);
    if (e != hipSuccess) {
        g_last_hip = e;
        return UA_ERR_NOMEM;
    }
    return UA_OK;
}

extern "C" int ua_dev_free(ua_ctx *c, void *dptr) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipFree(dptr));
    return UA_OK;
}

extern "C" int ua_h2d(ua_ctx *c, void *dst, const void *src, uint64_t bytes) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UA_OK;
}

extern "C" int ua_d2h(ua_ctx *c, void *dst, const void *src, uint64_t bytes) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UA_OK;
}

extern "C" int ua_sync(ua_ctx *c) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UA_OK;
}

extern "C" int ua_stats_reset(ua_ctx *c) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    c->n_launches = 0;
    c->kernel_ms = 0.0;
    c->bytes_algo = 0;
    return UA_OK;
}

extern "C" int ua_stats_get(ua_ctx *c, uint64_t *n_launches, double *kernel_ms,
                            uint64_t *bytes_algorithmic) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (n_launches) *n_launches = c->n_launches;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    if (bytes_algorithmic) *bytes_algorithmic = c->bytes_algo;
    return UA_OK;
}

/* stats: one HIP-event pair -> kernel_ms, counted as n sampled launches */
static int stats_add(ua_ctx *c, hipEvent_t e0, hipEvent_t e1, u64 n = 1) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    c->kernel_ms += ms;
    c->n_launches += n;
    return UA_OK;
}

static u64 scan_chunks(u64 n) { return (n + UA_SCAN_CHUNK - 1) / UA_SCAN_CHUNK; }

/* Split flat scan: offs gets chunk-local exclusive offsets, part the scanned
 * chunk partials (nchunks + 1 u64); consumers combine via d_off(). */
static void enqueue_scan(const u32 *cnt, u64 n, u64 *offs, u64 *part, u64 nchunks,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_scan1, dim3((u32)nchunks), dim3(UA_BLOCK), 0, st, cnt, n, offs,
                       part);
    hipLaunchKernelGGL(k_scan2, dim3(1), dim3(UA_BLOCK), 0, st, part, nchunks);
}

/* the scan on the ctx stream with its partials in WS_PARTIAL */
static int ws_scan(ua_ctx *c, const u32 *cnt, u64 n, u64 *offs) {
    u64 nchunks = scan_chunks(n);
    int rc = ws_reserve(c, WS_PARTIAL, (nchunks + 1) * sizeof(u64));
    if (rc) return rc;
    enqueue_scan(cnt, n, offs, (u64 *)c->ws[WS_PARTIAL], nchunks, c->stream);
    return UA_OK;
}

/* ---- the pair pipeline: one view, one function per stage ----
 *
 * UaPipe is one pipeline instance as the kernels see it: plain pointers and
 * counts, owning nothing.  Three owners fill one: the one-shot path from the
 * ctx workspace, ua_batch from its own allocation (one view per buffer set)
 * and ua_merge_k_dev once per round.  The enqueue_* functions below are the
 * only place a pipeline kernel is launched and the only place the order
 * partition -> tiles -> tail is written. */
struct UaPipe {
    UaDesc *descs = nullptr;
    const u64 *tb = nullptr; /* per-pair first tile, n_pairs + 1 entries */
    int n_pairs = 0;
    u64 T = 0;               /* total tiles */
    u32 *tpair = nullptr;    /* k_partition's output: tile -> pair ... */
    u32 *ta0 = nullptr;      /* ... and tile -> first A index */
    u32 *tcnt = nullptr;     /* T + 1 counts; the owner zeroes [T] */
    u64 *toff = nullptr;     /* scanned tail: chunk-local offsets, T + 1 */
    u64 *part = nullptr;     /* scanned tail: chunk partials, nchunks + 1 */
    u64 nchunks = 0;         /* scan chunks over the T + 1 counts */
    u64 *stage = nullptr;    /* staged ops: stage_stride(op) u64 per tile */
    const u64 *prim = nullptr; /* dense primary staging (UA_STAGE_P/tile) or null */
    const UaTChunk *cmap = nullptr; /* fused tail's chunk map */
    u64 n_tchunks = 0;       /* 0 = this instance keeps the scanned tail */
    u64 *pout = nullptr;     /* per-pair output lengths */
    const u32 *slab = nullptr;   /* prepared batch: narrow records (k_narrow) ... */
    const u32 *tpairn = nullptr; /* ... and tpair with UA_NARROW_BIT, or both null */
};

/* staging u64 per tile; 0 = the op does not stage (union, merge-all) */
static u64 stage_stride(int op) {
    return op == OP_INTERSECT ? UA_TILE / 2 : op == OP_DIFF ? UA_TILE : 0;
}

/* the two k_partition passes (T > 0) */
static void enqueue_partition(const UaPipe &p, hipStream_t st) {
    u64 pblk = (p.T + UA_BLOCK - 1) / UA_BLOCK;
    for (int phase = 0; phase < 2; phase++)
        hipLaunchKernelGGL(k_partition, dim3((u32)pblk), dim3(UA_BLOCK), 0, st, p.descs,
                           p.tb, p.n_pairs, p.T, p.tpair, p.ta0, phase);
}

/* One workgroup per tile (T > 0).  STAGE passes the dense primary staging in
 * the otherwise unused offs slot; only WRITE reads offs/partials.  isin/isout
 * are the prepared batch's cached merge-path splits (see k_tiles). */
static int enqueue_tiles(const UaPipe &p, int op, int mode, const u32 *isin, u32 *isout,
                         hipStream_t st) {
    void (*k)(const UaDesc *, const u32 *, const u32 *, u64, u64 *, u64, u32 *,
              const u64 *, const u64 *, const u32 *, u32 *, const u32 *) = nullptr;
    if (op == OP_INTERSECT && mode == MODE_STAGE) k = k_tiles<OP_INTERSECT, MODE_STAGE>;
    else if (op == OP_DIFF && mode == MODE_STAGE) k = k_tiles<OP_DIFF, MODE_STAGE>;
    else if (op == OP_UNION && mode == MODE_COUNT) k = k_tiles<OP_UNION, MODE_COUNT>;
    else if (op == OP_UNION && mode == MODE_WRITE) k = k_tiles<OP_UNION, MODE_WRITE>;
    else if (op == OP_MERGE_ALL && mode == MODE_DIRECT) k = k_tiles<OP_MERGE_ALL, MODE_DIRECT>;
    else return UA_ERR_INVALID;
    const bool staged = (mode == MODE_STAGE), write = (mode == MODE_WRITE);
    const bool narrow = staged && p.slab && p.tpairn;
    hipLaunchKernelGGL(k, dim3((u32)p.T), dim3(UA_TBLOCK), 0, st, p.descs,
                       narrow ? p.tpairn : p.tpair, p.ta0,
                       p.T, staged ? p.stage : nullptr, stage_stride(op), p.tcnt,
                       staged ? p.prim : write ? p.toff : nullptr,
                       write ? p.part : nullptr, isin, isout, narrow ? p.slab : nullptr);
    return UA_OK;
}

/* the tile pass that opens each op's pipeline */
static int first_mode(int op) {
    return stage_stride(op) ? MODE_STAGE : op == OP_UNION ? MODE_COUNT : MODE_DIRECT;
}

/* The tail after the first tile pass, leaving the pair lengths in p.pout.
 * Staged ops with a chunk map: ONE k_tail_fused (pairs without tiles get no
 * chunk, so the owner zeroes pout).  Otherwise scan + (union: the WRITE tile
 * pass, timed by ev[2]/ev[3] when asked | staged: compact) + k_pair_out.  A
 * view without tiles (an all-empty round of the union tree) publishes zero
 * lengths.  write_isin: cached splits for union's WRITE pass, or null. */
static int enqueue_tail(ua_ctx *c, const UaPipe &p, int op, const u32 *write_isin,
                        bool timed, hipStream_t st) {
    const u64 stride = stage_stride(op);
    if (op == OP_MERGE_ALL) return UA_OK; /* output position == path position */
    if (stride && p.n_tchunks > 0) {
        hipLaunchKernelGGL(k_tail_fused, dim3((u32)p.n_tchunks), dim3(UA_BLOCK), 0, st,
                           p.descs, p.cmap, p.tcnt, p.stage, stride, p.prim, p.pout, op);
        return UA_OK;
    }
    if (p.T == 0) {
        HIP_TRY(hipMemsetAsync(p.toff, 0, sizeof(u64), st));
        HIP_TRY(hipMemsetAsync(p.part, 0, sizeof(u64), st));
    } else {
        enqueue_scan(p.tcnt, p.T + 1, p.toff, p.part, p.nchunks, st);
        if (op == OP_UNION) {
            if (timed) HIP_TRY(hipEventRecord(c->ev[2], st));
            int rc = enqueue_tiles(p, OP_UNION, MODE_WRITE, write_isin, nullptr, st);
            if (rc) return rc;
            if (timed) HIP_TRY(hipEventRecord(c->ev[3], st));
        } else {
            hipLaunchKernelGGL(k_compact, dim3((u32)((p.T + 15) / 16)), dim3(UA_BLOCK), 0,
                               st, p.descs, p.tpair, p.tb, p.tcnt, p.toff, p.part,
                               p.stage, stride, p.prim, p.T, op);
            hipLaunchKernelGGL(k_compact_small,
                               dim3((u32)((p.T + UA_BLOCK - 1) / UA_BLOCK)), dim3(UA_BLOCK),
                               0, st, p.descs, p.tpair, p.tb, p.tcnt, p.toff, p.part,
                               p.stage, stride, p.prim, p.T, op);
        }
    }
    u64 poutblk = ((u64)p.n_pairs + UA_BLOCK - 1) / UA_BLOCK;
    hipLaunchKernelGGL(k_pair_out, dim3((u32)poutblk), dim3(UA_BLOCK), 0, st, p.toff,
                       p.part, p.tb, p.n_pairs, p.pout);
    return UA_OK;
}

static size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

/* ---- fused tail (k_tail_fused): host-side chunk map ---- */

/* UA_FUSED_TAIL=0 keeps the scan/compact/pair_out tail (same-box A/B) */
static bool fused_tail_enabled() {
    const char *e = getenv("UA_FUSED_TAIL");
    return !(e && e[0] == '0');
}

/* Per-pair chunk limit.  A pair of Tp tiles re-reads Tp^2/(2C) counts (u32)
 * to rebuild its chunk bases, against Tp*UA_TILE*8 input bytes its tile
 * kernel streams from HBM: a ratio of Tp/(8192*C).  The cap of
 * UA_TAIL_MAX_TILES = 16384 tiles (33.5M path elements, 256 chunks) keeps
 * that at 3% — 8 MB of L2 hits on a 64 KB count array against 268 MB of HBM
 * stream; a 10Mx10M pair re-reads 3 MB.  n and m can reach 2^31 (2M tiles),
 * where the quadratic term would rival the tile kernel, so a batch holding a
 * larger pair keeps the scanned tail.  UA_TAIL_MAX_CHUNKS overrides; it is
 * read when the decision is taken (batch create / one-shot call). */
static u64 tail_chunk_limit() {
    const char *e = getenv("UA_TAIL_MAX_CHUNKS");
    if (e && e[0]) {
        long long v = atoll(e);
        if (v > 0) return (u64)v;
    }
    return UA_TAIL_MAX_TILES / UA_TAIL_C;
}

/* chunk -> (first tile, pair, tiles before) from the per-pair tile bases,
 * plus the sentinel entry.  false = some pair exceeds the chunk limit (the
 * caller keeps the scanned tail). */
static bool build_tail_chunks(const std::vector<u64> &tb, int n_pairs,
                              std::vector<UaTChunk> &cm) {
    const u64 limit = tail_chunk_limit();
    cm.clear();
    for (int p = 0; p < n_pairs; p++) {
        u64 tp = tb[p + 1] - tb[p];
        if ((tp + UA_TAIL_C - 1) / UA_TAIL_C > limit) return false;
        for (u64 f = 0; f < tp; f += UA_TAIL_C)
            cm.push_back({tb[p] + f, (u32)p, (u32)f});
    }
    cm.push_back({tb[n_pairs], 0xFFFFFFFFu, 0u});
    return true;
}

/* Host plan of one pair batch.  head is the upload image descs | tb | chunk
 * map (one allocation, one copy); n_tchunks == 0 means the scanned tail:
 * not asked for, toggled off, no tiles, or a pair over the chunk limit. */
struct UaPlan {
    std::vector<u8> head;
    size_t o_tb = 0, o_cmap = 0; /* byte offsets into head */
    u64 T = 0, in_bytes = 0, n_tchunks = 0;
};

static int plan_pairs(const ua_dpair *pairs, int n_pairs, bool want_fused, UaPlan &pl) {
    if (n_pairs < 0) return UA_ERR_INVALID;
    std::vector<UaDesc> descs((size_t)std::max(n_pairs, 1));
    std::vector<u64> tb((size_t)n_pairs + 1);
    for (int p = 0; p < n_pairs; p++) {
        const ua_dpair &pr = pairs[p];
        if (pr.n >= (1ull << 31) || pr.m >= (1ull << 31)) return UA_ERR_INVALID;
        descs[p] = {pr.u, pr.n, pr.v, pr.m, pr.out, pl.T};
        tb[p] = pl.T;
        pl.T += (pr.n + pr.m + UA_TILE - 1) / UA_TILE;
        pl.in_bytes += 8 * (pr.n + pr.m);
    }
    tb[n_pairs] = pl.T;
    std::vector<UaTChunk> cmap;
    if (want_fused && pl.T > 0 && fused_tail_enabled() &&
        build_tail_chunks(tb, n_pairs, cmap))
        pl.n_tchunks = cmap.size() - 1;
    else
        cmap.clear();
    pl.o_tb = descs.size() * sizeof(UaDesc);
    pl.o_cmap = align16(pl.o_tb + tb.size() * sizeof(u64));
    pl.head.resize(pl.o_cmap + cmap.size() * sizeof(UaTChunk));
    memcpy(pl.head.data(), descs.data(), pl.o_tb);
    memcpy(pl.head.data() + pl.o_tb, tb.data(), tb.size() * sizeof(u64));
    if (!cmap.empty())
        memcpy(pl.head.data() + pl.o_cmap, cmap.data(), cmap.size() * sizeof(UaTChunk));
    return UA_OK;
}

/* point a view at the device copy of a plan's head */
static void pipe_set_head(UaPipe &p, const UaPlan &pl, int n_pairs, void *d_head) {
    p.descs = (UaDesc *)d_head;
    p.tb = (const u64 *)((u8 *)d_head + pl.o_tb);
    p.cmap = (const UaTChunk *)((u8 *)d_head + pl.o_cmap);
    p.n_pairs = n_pairs;
    p.T = pl.T;
    p.nchunks = scan_chunks(pl.T + 1);
    p.n_tchunks = pl.n_tchunks;
}

/* ---- the batched set-algebra pipeline, one-shot on the ctx workspace ---- */
static int run_batch_locked(ua_ctx *c, const ua_dpair *pairs, int n_pairs,
                            uint64_t *out_lens, int op) {
    if (n_pairs <= 0) return UA_OK;
    HIP_TRY(hipSetDevice(c->device));
    const u64 stride = stage_stride(op);
    UaPlan pl;
    int rc = plan_pairs(pairs, n_pairs, stride != 0, pl);
    if (rc) return rc;
    const u64 T = pl.T;

    if ((rc = ws_reserve(c, WS_DESC, pl.head.size()))) return rc;
    if ((rc = ws_reserve(c, WS_TPAIR, (T + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TA0, (T + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TCNT, (T + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (T + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_POUT, (size_t)n_pairs * sizeof(u64)))) return rc;
    if (stride) {
        if ((rc = ws_reserve(c, WS_STAGE, T * stride * sizeof(u64)))) return rc;
        if ((rc = ws_reserve(c, WS_STAGEP, T * UA_STAGE_P * sizeof(u64)))) return rc;
    }
    UaPipe p;
    pipe_set_head(p, pl, n_pairs, c->ws[WS_DESC]);
    if (T > 0 && op != OP_MERGE_ALL && !p.n_tchunks &&
        (rc = ws_reserve(c, WS_PARTIAL, (p.nchunks + 1) * sizeof(u64))))
        return rc;
    p.tpair = (u32 *)c->ws[WS_TPAIR];
    p.ta0 = (u32 *)c->ws[WS_TA0];
    p.tcnt = (u32 *)c->ws[WS_TCNT];
    p.toff = (u64 *)c->ws[WS_TOFF];
    p.part = (u64 *)c->ws[WS_PARTIAL];
    p.pout = (u64 *)c->ws[WS_POUT];
    if (stride) {
        p.stage = (u64 *)c->ws[WS_STAGE];
        p.prim = (const u64 *)c->ws[WS_STAGEP];
    }

    HIP_TRY(hipMemcpyAsync(p.descs, pl.head.data(), pl.head.size(), hipMemcpyHostToDevice,
                           c->stream));
    /* zero sentinel so offs[T] = total output */
    HIP_TRY(hipMemsetAsync(p.tcnt + T, 0, sizeof(u32), c->stream));
    if (T == 0) {
        /* every pair is empty (n+m == 0) */
        HIP_TRY(hipStreamSynchronize(c->stream)); /* pl.head is scoped */
        for (int i = 0; i < n_pairs; i++) out_lens[i] = 0;
        return UA_OK;
    }
    enqueue_partition(p, c->stream);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if ((rc = enqueue_tiles(p, op, first_mode(op), nullptr, nullptr, c->stream))) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if (op != OP_MERGE_ALL) {
        /* WS_POUT is reused between calls and zero-tile pairs get no fused
         * chunk: their length must read 0 */
        if (p.n_tchunks)
            HIP_TRY(hipMemsetAsync(p.pout, 0, (size_t)n_pairs * sizeof(u64), c->stream));
        if ((rc = enqueue_tail(c, p, op, nullptr, true, c->stream))) return rc;
        HIP_TRY(hipMemcpyAsync(out_lens, p.pout, (size_t)n_pairs * sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());

    /* stats: HIP-event time of the dominant (tile) kernel(s) */
    if ((rc = stats_add(c, c->ev[0], c->ev[1]))) return rc;
    if (op == OP_UNION && (rc = stats_add(c, c->ev[2], c->ev[3]))) return rc;
    if (op == OP_MERGE_ALL) {
        /* duplicate-keeping merge: no scan / staging / compaction, lens are n+m */
        for (int i = 0; i < n_pairs; i++) out_lens[i] = pairs[i].n + pairs[i].m;
        c->bytes_algo += 2 * pl.in_bytes;
        return UA_OK;
    }
    u64 out_elems = 0;
    for (int i = 0; i < n_pairs; i++) out_elems += out_lens[i];
    c->bytes_algo += pl.in_bytes + 8 * out_elems;
    return UA_OK;
}

static int run_batch(ua_ctx *c, const ua_dpair *pairs, int n_pairs, uint64_t *out_lens, int op) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return run_batch_locked(c, pairs, n_pairs, out_lens, op);
}

extern "C" int ua_intersect_batch_dev(ua_ctx *c, const ua_dpair *pairs, int n_pairs,
                                      uint64_t *out_lens) {
    return run_batch(c, pairs, n_pairs, out_lens, OP_INTERSECT);
}

/* ==================== prepared batch (repeated-query path) ==================== */

struct ua_batch {
    /* view[0]: the batch's own buffers.  view[1]: the second set of the
     * overlapped run_n (UA_OVERLAP: the aux tail of step i runs on the tail
     * stream while step i+1's tile kernel fills the other set) — its own
     * tcnt/toff/part/stage, no primary staging (prim == nullptr), the rest
     * shared with view[0].  view[1].stage == nullptr until first needed.
     * A view's n_tchunks == 0 means this batch keeps the scanned tail. */
    UaPipe view[2];
    u64 in_bytes = 0;
    void *mem = nullptr;  /* one allocation for view[0]'s metadata arrays */
    void *mem1 = nullptr; /* view[1]'s tcnt + toff + part */
    /* view[0].stage (stride UA_TILE: fits intersect + diff), view[0].prim and
     * view[1].stage are separate lazy allocations owned by the batch.  prim
     * is allocated (or fails) once: captured tail graphs freeze it, so it
     * must never change after the first staged run */
    bool stage_p_tried = false;
    /* cached per-thread merge-path splits (valid because the prepared
     * batch's inputs are immutable — same contract as the cached tile
     * partition): one u32 per (tile, thread), T * UA_TBLOCK * 4 bytes;
     * written by the first run of any op, read by every later one */
    u32 *d_isplit = nullptr; /* packed lo16 = i0(s0), hi16 = i0b(smid) */
    bool i0_ready = false;
    /* third cache, on the same immutability promise: the narrow slab (see
     * k_narrow), T records of UA_NREC_W u32 + the marked tile-pair words in
     * ONE allocation, about 4 B per input element.  Built ahead of the first
     * intersect/difference run; the allocation is tried once (failure or
     * UA_NARROW=0: the batch runs the 64-bit fill on every tile), a
     * union-only batch never builds it */
    void *d_narrow = nullptr;
    size_t narrow_bytes = 0;
    bool narrow_tried = false;
    /* hipGraph capture of the staged pipeline (per op); out_lens land in the
     * pinned h_pout so the captured D2H copy has a fixed destination */
    hipGraphExec_t gexec[3][2] = {};
    bool no_graph = false; /* capture/replay failed on this box: stay eager */
    u64 *h_pout = nullptr;
};

/* allocate, upload and partition; on failure the caller destroys b */
static int batch_init(ua_ctx *c, ua_batch *b, const UaPlan &pl, int n_pairs) {
    UaPipe &p = b->view[0];
    const u64 T = pl.T;
    b->in_bytes = pl.in_bytes;
    u64 nchunks = scan_chunks(T + 1);
    size_t o_toff = align16(pl.head.size());
    size_t o_part = align16(o_toff + (T + 1) * sizeof(u64));
    size_t o_pout = align16(o_part + (nchunks + 1) * sizeof(u64));
    size_t o_tpair = align16(o_pout + (size_t)std::max(n_pairs, 1) * sizeof(u64));
    size_t o_ta0 = align16(o_tpair + (T + 1) * sizeof(u32));
    size_t o_tcnt = align16(o_ta0 + (T + 1) * sizeof(u32));
    size_t total_bytes = align16(o_tcnt + (T + 1) * sizeof(u32));
    hipError_t e = hipMalloc(&b->mem, total_bytes);
    if (e != hipSuccess) {
        g_last_hip = e;
        return UA_ERR_NOMEM;
    }
    u8 *base = (u8 *)b->mem;
    pipe_set_head(p, pl, n_pairs, base);
    p.toff = (u64 *)(base + o_toff);
    p.part = (u64 *)(base + o_part);
    p.pout = (u64 *)(base + o_pout);
    p.tpair = (u32 *)(base + o_tpair);
    p.ta0 = (u32 *)(base + o_ta0);
    p.tcnt = (u32 *)(base + o_tcnt);

    HIP_TRY(hipMemcpyAsync(b->mem, pl.head.data(), pl.head.size(), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipMemsetAsync(p.tcnt + T, 0, sizeof(u32), c->stream));
    HIP_TRY(hipMemsetAsync(p.toff, 0, sizeof(u64), c->stream));
    HIP_TRY(hipMemsetAsync(p.part, 0, sizeof(u64), c->stream));
    /* pout starts zeroed: zero-tile pairs get no fused-tail chunk, never
     * publish a length and stay 0 from here */
    HIP_TRY(hipMemsetAsync(p.pout, 0, (size_t)std::max(n_pairs, 1) * sizeof(u64),
                           c->stream));
    /* the partition depends only on the (immutable) pair contents:
     * computed once here, reused every run */
    if (T > 0) enqueue_partition(p, c->stream);
    HIP_TRY(hipStreamSynchronize(c->stream)); /* pl.head is the caller's */
    HIP_TRY(hipGetLastError());
    return UA_OK;
}

extern "C" int ua_batch_create(ua_ctx *c, const ua_dpair *pairs, int n_pairs,
                               ua_batch **out) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    UaPlan pl;
    int rc = plan_pairs(pairs, n_pairs, true, pl);
    if (rc) return rc;
    ua_batch *b = new ua_batch();
    if ((rc = batch_init(c, b, pl, n_pairs))) {
        ua_batch_destroy(c, b);
        return rc;
    }
    *out = b;
    return UA_OK;
}

extern "C" void ua_batch_destroy(ua_ctx *c, ua_batch *b) {
    if (!b) return;
    (void)hipSetDevice(c->device);
    for (int i = 0; i < 3; i++)
        for (int s = 0; s < 2; s++)
            if (b->gexec[i][s]) (void)hipGraphExecDestroy(b->gexec[i][s]);
    if (b->h_pout) (void)hipHostFree(b->h_pout);
    if (b->mem) (void)hipFree(b->mem);
    if (b->mem1) (void)hipFree(b->mem1);
    if (b->view[0].stage) (void)hipFree(b->view[0].stage);
    if (b->view[0].prim) (void)hipFree((void *)b->view[0].prim);
    if (b->view[1].stage) (void)hipFree(b->view[1].stage);
    if (b->d_isplit) (void)hipFree(b->d_isplit);
    if (b->d_narrow) (void)hipFree(b->d_narrow);
    delete b;
}

#ifndef UA_GRAPH
#define UA_GRAPH 1 /* hipGraph-capture the staged pipeline's AUX TAIL
                    * (k_tail_fused, or scan/compact/pair_out -> one replay;
                    * the D2H of the lengths is NOT captured — it is enqueued
                    * once after the last pass of a run_n).  The tile
                    * kernel stays an eager launch so its HIP-event timing
                    * (bench.py roofline leg) remains live — event-record
                    * nodes inside replayed graphs do not update events on
                    * this ROCm.  0 = eager launches */
#endif

/* lazy split-cache: returns (isin, isout) for this run and flips i0_ready */
static void batch_isplit(ua_batch *b, const u32 **isin, u32 **isout) {
    *isin = nullptr;
    *isout = nullptr;
    if (!b->d_isplit) {
        size_t bytes = (size_t)b->view[0].T * UA_TBLOCK * sizeof(u32);
        if (bytes == 0 || hipMalloc((void **)&b->d_isplit, bytes) != hipSuccess) {
            b->d_isplit = nullptr; /* cacheless fallback */
            (void)hipGetLastError();
            return;
        }
    }
    if (b->i0_ready) *isin = b->d_isplit;
    else {
        *isout = b->d_isplit;
        b->i0_ready = true; /* ordered: runs are stream-serialized */
    }
}

/* UA_NARROW=0 keeps every tile of a prepared batch on the 64-bit fill
 * (same-box A/B); read when the batch first runs a staged op */
static bool narrow_enabled() {
    const char *e = getenv("UA_NARROW");
    return !(e && e[0] == '0');
}

/* Build the narrow slab ahead of the batch's first staged run: one
 * allocation attempt per batch, one k_narrow on the engine's stream, outside
 * the tile kernel's event pair.  Never fatal: without the slab the batch
 * runs as it always has. */
static int batch_narrow(ua_ctx *c, ua_batch *b) {
    if (b->narrow_tried) return UA_OK;
    b->narrow_tried = true;
    UaPipe &v0 = b->view[0];
    if (!narrow_enabled() || v0.T == 0) return UA_OK;
    size_t o_tpn = align16((size_t)v0.T * UA_NREC_W * sizeof(u32));
    size_t bytes = align16(o_tpn + (size_t)(v0.T + 1) * sizeof(u32));
    if (hipMalloc(&b->d_narrow, bytes) != hipSuccess) {
        b->d_narrow = nullptr;
        (void)hipGetLastError();
        return UA_OK;
    }
    u8 *base = (u8 *)b->d_narrow;
    b->narrow_bytes = bytes;
    hipLaunchKernelGGL(k_narrow, dim3((u32)v0.T), dim3(UA_TBLOCK), 0, c->stream, v0.descs,
                       v0.tpair, v0.ta0, v0.T, (u32 *)base, (u32 *)(base + o_tpn));
    v0.slab = (const u32 *)base;
    v0.tpairn = (const u32 *)(base + o_tpn);
    if (b->mem1) { /* the overlap set shares the inputs' caches */
        b->view[1].slab = v0.slab;
        b->view[1].tpairn = v0.tpairn;
    }
    return UA_OK;
}

extern "C" int ua_batch_info(ua_ctx *c, ua_batch *b, uint64_t *tiles, uint64_t *narrow_tiles,
                             uint64_t *narrow_bytes) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (!b) return UA_ERR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    u64 nn = 0;
    if (b->view[0].tpairn) { /* count the marked tile-pair words */
        std::vector<u32> tp((size_t)b->view[0].T);
        HIP_TRY(hipMemcpyAsync(tp.data(), b->view[0].tpairn, tp.size() * sizeof(u32),
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (u32 w : tp) nn += (w >> 31);
    }
    if (tiles) *tiles = b->view[0].T;
    if (narrow_tiles) *narrow_tiles = nn;
    if (narrow_bytes) *narrow_bytes = b->d_narrow ? b->narrow_bytes : 0;
    return UA_OK;
}

/* How many tiles take the sentinel walk: the records' fast words, fetched on
 * demand with one strided copy (a narrow tile's alone can be 1). */
extern "C" int ua_batch_fast_tiles(ua_ctx *c, ua_batch *b, uint64_t *n) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (!b || !n) return UA_ERR_INVALID;
    HIP_TRY(hipSetDevice(c->device));
    u64 nf = 0;
    if (b->view[0].slab) {
        std::vector<u32> fw((size_t)b->view[0].T);
        HIP_TRY(hipMemcpy2DAsync(fw.data(), sizeof(u32), b->view[0].slab + UA_TILE + 3,
                                 UA_NREC_W * sizeof(u32), sizeof(u32), fw.size(),
                                 hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (u32 w : fw) nf += (w != 0);
    }
    *n = nf;
    return UA_OK;
}

/* the first tile pass of one run (eager; event-timed on the sampled pass) */
static int batch_tiles(ua_ctx *c, ua_batch *b, int kop, bool timed, int set) {
    const u32 *isin;
    u32 *isout;
    batch_isplit(b, &isin, &isout);
    if (timed) HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    int rc = enqueue_tiles(b->view[set], kop, first_mode(kop), isin, isout, c->stream);
    if (rc) return rc;
    if (timed) HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    return UA_OK;
}

/* one tail dispatch: graph replay when available, else eager enqueue.
 * Returns UA_OK with the tail enqueued (or already executed, for the one
 * capture-validation run). */
static int batch_tail_dispatch(ua_ctx *c, ua_batch *b, int kop, bool timed, int set,
                               hipStream_t st) {
    const UaPipe &p = b->view[set];
    /* union's WRITE pass reuses the splits its count pass just stored */
    const u32 *isw = b->i0_ready ? b->d_isplit : nullptr;
#if UA_GRAPH
    if (getenv("UA_NO_TAILGRAPH")) b->no_graph = true;
    if (kop != OP_UNION) { /* union's tail holds an event-timed kernel */
        if (!b->gexec[kop][set] && !b->no_graph) {
            /* capture the tail once and VALIDATE with a launch+sync; any
             * failure makes this batch permanently eager — self-healing,
             * never fatal.  The one validation launch IS this run's tail
             * (capture itself executes nothing). */
            hipError_t ce = hipStreamBeginCapture(st,
                                                  hipStreamCaptureModeThreadLocal);
            if (ce == hipSuccess) {
                int rc = enqueue_tail(c, p, kop, isw, false, st);
                hipGraph_t gr = nullptr;
                hipError_t ee = hipStreamEndCapture(st, &gr);
                if (rc == UA_OK && ee == hipSuccess && gr) {
                    hipError_t ie = hipGraphInstantiate(&b->gexec[kop][set], gr,
                                                        nullptr, nullptr, 0);
                    if (ie == hipSuccess) {
                        hipError_t le = hipGraphLaunch(b->gexec[kop][set], st);
                        if (le == hipSuccess) le = hipStreamSynchronize(st);
                        if (le == hipSuccess) {
                            (void)hipGraphDestroy(gr);
                            return UA_OK; /* tail executed */
                        }
                        if (getenv("UA_DEBUG"))
                            fprintf(stderr, "[ua] graph launch failed: %s\n",
                                    hipGetErrorName(le));
                        (void)hipGraphExecDestroy(b->gexec[kop][set]);
                        b->gexec[kop][set] = nullptr;
                    } else if (getenv("UA_DEBUG")) {
                        fprintf(stderr, "[ua] graph instantiate failed: %s\n",
                                hipGetErrorName(ie));
                        b->gexec[kop][set] = nullptr;
                    }
                    (void)hipGraphDestroy(gr);
                } else {
                    if (getenv("UA_DEBUG"))
                        fprintf(stderr, "[ua] capture failed (rc=%d, end=%s)\n", rc,
                                hipGetErrorName(ee));
                    if (gr) (void)hipGraphDestroy(gr);
                }
                b->no_graph = true;
                (void)hipGetLastError();
            } else {
                b->no_graph = true;
                (void)hipGetLastError();
            }
        } else if (b->gexec[kop][set]) {
            hipError_t le = hipGraphLaunch(b->gexec[kop][set], st);
            if (le == hipSuccess) return UA_OK;
            (void)hipGraphExecDestroy(b->gexec[kop][set]);
            b->gexec[kop][set] = nullptr;
            b->no_graph = true;
            (void)hipGetLastError();
        }
    }
#endif
    return enqueue_tail(c, p, kop, isw, timed, st);
}

/* UA_OVERLAP's second buffer set, allocated on first use; false = no memory
 * (the caller stays serial) */
static bool batch_alloc_set1(ua_batch *b) {
    const UaPipe &v0 = b->view[0];
    size_t o_cnt1 = 0;
    size_t o_off1 = align16(o_cnt1 + (v0.T + 1) * sizeof(u32));
    size_t o_part1 = align16(o_off1 + (v0.T + 1) * sizeof(u64));
    size_t tot1 = align16(o_part1 + (v0.nchunks + 1) * sizeof(u64));
    u64 *stage1 = nullptr;
    hipError_t e = hipMalloc(&b->mem1, tot1);
    if (e == hipSuccess) e = hipMalloc((void **)&stage1, v0.T * UA_TILE * sizeof(u64));
    if (e != hipSuccess) {
        if (b->mem1) { (void)hipFree(b->mem1); b->mem1 = nullptr; }
        return false;
    }
    u8 *m1 = (u8 *)b->mem1;
    b->view[1] = v0;
    b->view[1].tcnt = (u32 *)(m1 + o_cnt1);
    b->view[1].toff = (u64 *)(m1 + o_off1);
    b->view[1].part = (u64 *)(m1 + o_part1);
    b->view[1].stage = stage1;
    b->view[1].prim = nullptr;
    return true;
}

/* n_runs passes of one op over the prepared batch, enqueued back-to-back
 * with ONE sync at the end (the repeated-query serving shape: no host
 * round-trip between runs).  Kernel events are sampled on the LAST pass
 * (stats count it as one sampled launch). */
static int batch_run_locked(ua_ctx *c, ua_batch *b, int op, int n_runs,
                            uint64_t *out_lens) {
    HIP_TRY(hipSetDevice(c->device));
    UaPipe &v0 = b->view[0];
    const int n_pairs = v0.n_pairs;
    if (n_pairs == 0 || n_runs <= 0) return UA_OK;
    int kop = (op == UA_OP_INTERSECT) ? OP_INTERSECT
              : (op == UA_OP_MERGE) ? OP_UNION
              : (op == UA_OP_DIFFERENCE) ? OP_DIFF
                                         : -1;
    if (kop < 0) return UA_ERR_INVALID;
    const u64 T = v0.T;
    if (T == 0) {
        for (int p = 0; p < n_pairs; p++) out_lens[p] = 0;
        return UA_OK;
    }
    int rc;
    if (kop != OP_UNION && !v0.stage) {
        hipError_t e = hipMalloc((void **)&v0.stage, T * UA_TILE * sizeof(u64));
        if (e != hipSuccess) {
            g_last_hip = e;
            return UA_ERR_NOMEM;
        }
    }
    /* dense primary staging, view[0] only.  One allocation attempt per
     * batch: a failure is recorded, not retried, so prim is the same on
     * every run and in every captured tail. */
    if (kop != OP_UNION && !b->stage_p_tried) {
        b->stage_p_tried = true;
        u64 *prim = nullptr;
        if (hipMalloc((void **)&prim, (size_t)T * UA_STAGE_P * sizeof(u64)) != hipSuccess) {
            prim = nullptr;
            (void)hipGetLastError();
        }
        v0.prim = prim;
    }
    if (kop != OP_UNION && (rc = batch_narrow(c, b))) return rc;
    if (!b->h_pout) {
        hipError_t e = hipHostMalloc((void **)&b->h_pout, (size_t)n_pairs * sizeof(u64));
        if (e != hipSuccess) {
            g_last_hip = e;
            return UA_ERR_NOMEM;
        }
    }
    /* overlapped serving shape (UA_OVERLAP=1, measured NEUTRAL and
     * default-off): the aux tail (scan/compact/pair_out) of run i
     * executes on the tail stream against buffer set i&1 while run
     * i+1's tile kernel fills the other set.  Parity-green, but
     * co-scheduling contention stretches the tile kernel (727->766 us)
     * and k_compact (64->90 us) by about what the overlap hides —
     * whole-step 0.813 vs 0.802 ms serial, with one box showing a
     * pathological 1.65 ms at long run counts.  Union always serial
     * (its WRITE pass is a second tile kernel with live stats
     * events). */
    const char *ovl_env = getenv("UA_OVERLAP");
    bool ovl = (kop != OP_UNION) && n_runs > 1 && c->stream_tail &&
               ovl_env && ovl_env[0] == '1';
    if (ovl && !b->mem1) {
        ovl = batch_alloc_set1(b);
        if (ovl)
            HIP_TRY(hipMemsetAsync(b->view[1].tcnt + T, 0, sizeof(u32), c->stream));
    }
    hipStream_t tail_st = ovl ? c->stream_tail : c->stream;
    for (int it = 0; it < n_runs; it++) {
        bool timed = (it == n_runs - 1);
        int s = ovl ? (it & 1) : 0;
        /* set s's tail from run it-2 must be done before refilling */
        if (ovl) HIP_TRY(hipStreamWaitEvent(c->stream, c->oev[2 + s], 0));
        if ((rc = batch_tiles(c, b, kop, timed, s))) return rc;
        if (ovl) {
            HIP_TRY(hipEventRecord(c->oev[s], c->stream));
            HIP_TRY(hipStreamWaitEvent(tail_st, c->oev[s], 0));
        }
        if ((rc = batch_tail_dispatch(c, b, kop, timed, s, tail_st))) return rc;
        if (ovl) HIP_TRY(hipEventRecord(c->oev[2 + s], tail_st));
    }
    /* lengths: one copy after the last pass (only the last pass's are
     * returned); tails are serialized on their stream */
    HIP_TRY(hipMemcpyAsync(b->h_pout, v0.pout, (size_t)n_pairs * sizeof(u64),
                           hipMemcpyDeviceToHost, tail_st));
    HIP_TRY(hipStreamSynchronize(tail_st));
    if (ovl) HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    memcpy(out_lens, b->h_pout, (size_t)n_pairs * sizeof(u64));

    if ((rc = stats_add(c, c->ev[0], c->ev[1]))) return rc;
    if (kop == OP_UNION && (rc = stats_add(c, c->ev[2], c->ev[3]))) return rc;
    u64 out_elems = 0;
    for (int p = 0; p < n_pairs; p++) out_elems += out_lens[p];
    c->bytes_algo += ((u64)n_runs) * b->in_bytes + ((u64)n_runs) * 8 * out_elems;
    return UA_OK;
}

extern "C" int ua_batch_run(ua_ctx *c, ua_batch *b, int op, uint64_t *out_lens) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return batch_run_locked(c, b, op, 1, out_lens);
}

/* pipelined repeated runs: one sync for n_runs passes */
extern "C" int ua_batch_run_n(ua_ctx *c, ua_batch *b, int op, int n_runs,
                              uint64_t *out_lens) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return batch_run_locked(c, b, op, n_runs, out_lens);
}

extern "C" int ua_merge_batch_dev(ua_ctx *c, const ua_dpair *pairs, int n_pairs,
                                  uint64_t *out_lens) {
    return run_batch(c, pairs, n_pairs, out_lens, OP_UNION);
}

extern "C" int ua_difference_batch_dev(ua_ctx *c, const ua_dpair *pairs, int n_pairs,
                                       uint64_t *out_lens) {
    return run_batch(c, pairs, n_pairs, out_lens, OP_DIFF);
}

/* duplicate-keeping batched merge (sorted-run merge; out capacity exactly n+m) */
extern "C" int ua_merge_all_batch_dev(ua_ctx *c, const ua_dpair *pairs, int n_pairs,
                                      uint64_t *out_lens) {
    return run_batch(c, pairs, n_pairs, out_lens, OP_MERGE_ALL);
}

/* ---- batched segmented sort: LDS bitonic chunks + OP_MERGE_ALL tree ---- */
extern "C" int ua_sort_segments_dev(ua_ctx *c, const ua_dseg *segs, int n_segs) {
    std::lock_guard<std::recursive_mutex> gop(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (n_segs <= 0) return UA_OK;

    u64 max_runs = 1;
    std::vector<UaChunk> chunks;
    std::vector<int> seg_rounds(n_segs);
    for (int sgi = 0; sgi < n_segs; sgi++) {
        u64 n = segs[sgi].n;
        u64 runs = (n + UA_SORT_N - 1) / UA_SORT_N;
        if (runs > max_runs) max_runs = runs;
        int r = 0;
        for (u64 w = 1; w < runs; w <<= 1) r++;
        seg_rounds[sgi] = r;
    }
    int rounds = 0;
    for (u64 w = 1; w < max_runs; w <<= 1) rounds++;
    /* per-segment start side: a segment with r merge rounds of its own flips
     * sides r times, so start it where it will END in data — finished
     * segments then never re-copy while bigger ones keep merging */
    for (int sgi = 0; sgi < n_segs; sgi++) {
        const ua_dseg &sg = segs[sgi];
        u64 *dst = (seg_rounds[sgi] & 1) ? sg.tmp : sg.data;
        for (u64 off = 0; off < sg.n; off += UA_SORT_N) {
            u32 len = (u32)std::min<u64>(UA_SORT_N, sg.n - off);
            chunks.push_back({sg.data + off, dst + off, len, 0});
        }
    }
    if (!chunks.empty()) {
        int rc;
        if ((rc = ws_reserve(c, WS_DESC, chunks.size() * sizeof(UaChunk)))) return rc;
        HIP_TRY(hipMemcpyAsync(c->ws[WS_DESC], chunks.data(),
                               chunks.size() * sizeof(UaChunk), hipMemcpyHostToDevice,
                               c->stream));
        hipLaunchKernelGGL(k_sort_chunks, dim3((u32)chunks.size()), dim3(UA_BLOCK), 0,
                           c->stream, (const UaChunk *)c->ws[WS_DESC],
                           (u64)chunks.size());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }

    u64 width = UA_SORT_N;
    for (int r = 0; r < rounds; r++) {
        std::vector<ua_dpair> prs;
        for (int sgi = 0; sgi < n_segs; sgi++) {
            if (r >= seg_rounds[sgi]) continue; /* segment already fully sorted */
            const ua_dseg &sg = segs[sgi];
            /* this segment has flipped r times from its start side */
            int side = (seg_rounds[sgi] - r) & 1; /* 1 = current runs in tmp */
            u64 *cur = side ? sg.tmp : sg.data;
            u64 *nxt = side ? sg.data : sg.tmp;
            for (u64 off = 0; off < sg.n; off += 2 * width) {
                u64 n1 = std::min<u64>(width, sg.n - off);
                u64 rem = sg.n - off - n1;
                u64 n2 = std::min<u64>(width, rem);
                /* odd trailing run pairs with an empty side = a copy */
                prs.push_back({cur + off, n1, cur + off + n1, n2, nxt + off});
            }
        }
        if (!prs.empty()) {
            std::vector<u64> lens(prs.size());
            int rc = run_batch_locked(c, prs.data(), (int)prs.size(), lens.data(),
                                      OP_MERGE_ALL);
            if (rc) return rc;
        }
        width <<= 1;
    }
    return UA_OK; /* every segment ends in data by start-side parity */
}

/* ---- batched algo.ApplyFilter (uidlist.go:21; callers worker/task.go:1403,
 * query/query.go:1431) ---- */
extern "C" int ua_apply_filter_batch_dev(ua_ctx *c, const ua_dfilter *tasks,
                                         int n_tasks, uint64_t *out_lens) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    if (n_tasks <= 0) return UA_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<UaFDesc> descs((size_t)n_tasks);
    std::vector<u64> tb((size_t)n_tasks + 1);
    u64 T = 0, in_bytes = 0;
    for (int p = 0; p < n_tasks; p++) {
        const ua_dfilter &f = tasks[p];
        if (f.n >= (1ull << 31)) return UA_ERR_INVALID;
        descs[p] = {f.u, f.n, f.mask, f.out, T};
        tb[p] = T;
        T += (f.n + UA_TILE - 1) / UA_TILE;
        in_bytes += 9 * f.n; /* 8 B uid + 1 B mask */
    }
    tb[n_tasks] = T;
    int rc;
    size_t descs_bytes = descs.size() * sizeof(UaFDesc);
    size_t tb_bytes = tb.size() * sizeof(u64);
    if ((rc = ws_reserve(c, WS_DESC, descs_bytes + tb_bytes))) return rc;
    if ((rc = ws_reserve(c, WS_POUT, (size_t)n_tasks * sizeof(u64)))) return rc;
    UaFDesc *d_descs = (UaFDesc *)c->ws[WS_DESC];
    u64 *d_tb = (u64 *)((u8 *)c->ws[WS_DESC] + descs_bytes);
    u64 *d_pout = (u64 *)c->ws[WS_POUT];
    std::vector<u8> hostbuf(descs_bytes + tb_bytes);
    memcpy(hostbuf.data(), descs.data(), descs_bytes);
    memcpy(hostbuf.data() + descs_bytes, tb.data(), tb_bytes);
    HIP_TRY(hipMemcpyAsync(d_descs, hostbuf.data(), hostbuf.size(),
                           hipMemcpyHostToDevice, c->stream));
    if (T > 0) {
        u64 *d_look;
        u64 gen;
        if ((rc = lb_acquire_ws(c, T, &d_look, &gen))) return rc;
        HIP_TRY(hipEventRecord(c->ev[0], c->stream));
        hipLaunchKernelGGL(k_filter, dim3((u32)T), dim3(UA_BLOCK), 0, c->stream,
                           d_descs, d_tb, n_tasks, T, d_look, gen, d_pout);
        HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    }
    HIP_TRY(hipMemcpyAsync(out_lens, d_pout, (size_t)n_tasks * sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    u64 out_elems = 0;
    for (int p = 0; p < n_tasks; p++) {
        if (tasks[p].n == 0) out_lens[p] = 0; /* no tiles -> never published */
        out_elems += out_lens[p];
    }
    if (T > 0 && (rc = stats_add(c, c->ev[0], c->ev[1]))) return rc;
    c->bytes_algo += in_bytes + 8 * out_elems;
    return UA_OK;
}

/* host-pointer algo.ApplyFilter: in-place like the reference (u is compacted
 * to *out_n kept elements); upload + device compaction + download */
extern "C" int ua_apply_filter(ua_ctx *c, uint64_t *u, uint64_t n,
                               const uint8_t *mask, uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (n == 0) {
        *out_n = 0;
        return UA_OK;
    }
    int rc;
    if ((rc = ws_reserve(c, WS_HU, n * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_HV, n))) return rc;
    u64 *d_u = (u64 *)c->ws[WS_HU];
    u8 *d_mask = (u8 *)c->ws[WS_HV];
    HIP_TRY(hipMemcpyAsync(d_u, u, n * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_mask, mask, n, hipMemcpyHostToDevice, c->stream));
    ua_dfilter task = {d_u, n, d_mask, d_u}; /* in-place on device too */
    if ((rc = ua_apply_filter_batch_dev(c, &task, 1, out_n))) return rc;
    HIP_TRY(hipMemcpyAsync(u, d_u, *out_n * sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UA_OK;
}

extern "C" int ua_index_of_batch_dev(ua_ctx *c, const uint64_t *u, uint64_t n,
                                     const uint64_t *queries, uint64_t nq, int64_t *out) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (nq == 0) return UA_OK;
    u64 nblk = (nq + UA_BLOCK - 1) / UA_BLOCK;
    hipLaunchKernelGGL(k_index_of, dim3((u32)nblk), dim3(UA_BLOCK), 0, c->stream,
                       u, n, queries, nq, out);
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    return UA_OK;
}

/* ---- row-wise UID-matrix filter against one shared list ----
 * query/query.go:1425-1437 updateUidMatrix (IntersectWith per row, or
 * ApplyFilter+IndexOf per row when ordered) and worker/task.go:1352,1617,
 * 1692,1778 (IntersectWith(UidMatrix[i], filtered, UidMatrix[i]) per row):
 * all rows in one call, five enqueues, one sync. */
static bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

extern "C" int ua_rows_filter_dev(ua_ctx *c, const ua_drows *d, int mode,
                                  uint64_t *out_total) {
    if (!c || !d || !out_total) return UA_ERR_INVALID;
    if (mode != UA_ROWS_INTERSECT && mode != UA_ROWS_DIFFERENCE) return UA_ERR_INVALID;
    const u64 total = d->total, n_rows = d->n_rows, m = d->m;
    /* tile and row-boundary grids are u32 block counts; stride * P >= m must
     * keep bracket lengths in u32 */
    if (total >= ((u64)UA_RTILE << 31) || n_rows >= ((u64)UA_BLOCK << 31) ||
        m >= ((u64)UA_ROWS_P << 31))
        return UA_ERR_INVALID;
    if (n_rows == 0 && total != 0) return UA_ERR_INVALID;
    /* a packed flat compaction cannot run in place: a tile's writes land in
     * earlier tiles' input range */
    if (ranges_overlap(d->vals, total * sizeof(u64), d->out_vals, total * sizeof(u64)) ||
        ranges_overlap(d->row_offs, (n_rows + 1) * sizeof(u64), d->out_row_offs,
                       (n_rows + 1) * sizeof(u64)))
        return UA_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const u64 ntiles = (total + UA_RTILE - 1) / UA_RTILE;
    const u64 stride = m > UA_ROWS_P ? (m + UA_ROWS_P - 1) / UA_ROWS_P : 1;
    const u32 npiv = (u32)((m + stride - 1) / stride);
    int gsteps = 0;
    while (((u64)1 << gsteps) < stride) gsteps++;
    int rc;
    if ((rc = ws_reserve(c, WS_RPIV, UA_ROWS_P * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_RKW, (size_t)(ntiles ? ntiles : 1) * UA_RWORDS * sizeof(u64))))
        return rc;
    /* one extra zero count: d_off(ntiles) is the kept total, which a row
     * boundary at pos == total reads when total is a multiple of the tile */
    if ((rc = ws_reserve(c, WS_TCNT, (size_t)(ntiles + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (size_t)(ntiles + 1) * sizeof(u64)))) return rc;
    u64 *d_piv = (u64 *)c->ws[WS_RPIV];
    u64 *d_kw = (u64 *)c->ws[WS_RKW];
    u32 *d_cnt = (u32 *)c->ws[WS_TCNT];
    u64 *d_offs = (u64 *)c->ws[WS_TOFF];
    HIP_TRY(hipMemsetAsync(d_cnt + ntiles, 0, sizeof(u32), c->stream));
    if (ntiles) {
        hipLaunchKernelGGL(k_rows_pivots, dim3(UA_ROWS_P / UA_BLOCK), dim3(UA_BLOCK), 0,
                           c->stream, d->shared, stride, npiv, d_piv);
        HIP_TRY(hipEventRecord(c->ev[0], c->stream));
        if (mode == UA_ROWS_INTERSECT)
            hipLaunchKernelGGL(k_rows_probe<UA_ROWS_INTERSECT>, dim3((u32)ntiles),
                               dim3(UA_BLOCK), 0, c->stream, d->vals, total, d->shared, m,
                               d_piv, npiv, stride, gsteps, d_kw, d_cnt);
        else
            hipLaunchKernelGGL(k_rows_probe<UA_ROWS_DIFFERENCE>, dim3((u32)ntiles),
                               dim3(UA_BLOCK), 0, c->stream, d->vals, total, d->shared, m,
                               d_piv, npiv, stride, gsteps, d_kw, d_cnt);
        HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    }
    if ((rc = ws_scan(c, d_cnt, ntiles + 1, d_offs))) return rc;
    const u64 *d_part = (const u64 *)c->ws[WS_PARTIAL];
    if (ntiles)
        hipLaunchKernelGGL(k_rows_write, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                           d->vals, d_kw, d_offs, d_part, d->out_vals);
    hipLaunchKernelGGL(k_rows_offs, dim3((u32)(n_rows / UA_BLOCK + 1)), dim3(UA_BLOCK), 0,
                       c->stream, d->row_offs, n_rows, total, d_kw, d_offs, d_part,
                       d->out_row_offs);
    u64 kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, d->out_row_offs + n_rows, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    if (ntiles && (rc = stats_add(c, c->ev[0], c->ev[1]))) return rc;
    c->bytes_algo += 8 * (total + kept);
    *out_total = kept;
    return UA_OK;
}

/* ---- IntersectSorted fold (uidlist.go:297): smallest-first pairwise ---- */
extern "C" int ua_intersect_k_dev(ua_ctx *c, const uint64_t *const *lists,
                                  const uint64_t *lens, int k, uint64_t *out,
                                  uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: scratch reuse */
    if (k <= 0) {
        *out_n = 0;
        return UA_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int> ord(k);
    for (int i = 0; i < k; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return lens[a] < lens[b]; });
    if (k == 1) {
        HIP_TRY(hipMemcpyAsync(out, lists[0], lens[0] * sizeof(u64),
                               hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *out_n = lens[0];
        return UA_OK;
    }
    u64 cap = lens[ord[0]];
    int rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_A, (cap ? cap : 1) * sizeof(u64)))) return rc;
    u64 *scratch = (u64 *)c->ws[WS_SCRATCH_A];
    ua_dpair pr;
    u64 len0 = 0;
    pr = {lists[ord[0]], lens[ord[0]], lists[ord[1]], lens[ord[1]], out};
    if ((rc = run_batch_locked(c, &pr, 1, &len0, OP_INTERSECT))) return rc;
    for (int j = 2; j < k && len0 > 0; j++) {
        pr = {out, len0, lists[ord[j]], lens[ord[j]], scratch};
        if ((rc = run_batch_locked(c, &pr, 1, &len0, OP_INTERSECT))) return rc;
        HIP_TRY(hipMemcpyAsync(out, scratch, len0 * sizeof(u64),
                               hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out_n = len0;
    return UA_OK;
}

/* ---- pairwise union tree over k sorted items (MergeSorted's engine) ----
 * Device-chained: positions and tile layouts are CAPACITY-based (host-known
 * up front), while each round's actual pair lengths are filled on-device
 * from the previous round's outputs (k_make_descs) — the whole log2(k)-round
 * tree enqueues with a single final sync.  Tail tiles past a pair's actual
 * path no-op in k_tiles.  Odd items pair with an empty side (a dedup copy),
 * so every item moves to the other ping-pong buffer each round.
 *
 * items/caps are host arrays (device pointers, capacities); d_len0 is a
 * device array of k u64 that ALREADY holds the items' actual lengths (<= the
 * capacities) — uploaded by ua_merge_k_dev, written by k_union_leaves for
 * ua_rows_union_dev — and serves as one half of the rounds' length
 * ping-pong.  Round r writes WS_SCRATCH_A when r is even and WS_SCRATCH_B
 * when odd, sum(caps) u64 each, reserved here: items may therefore live in
 * WS_SCRATCH_B (reserved by the caller at the same size, so this reserve
 * keeps it), which nothing writes before round 1, when round 0 has consumed
 * them.  k >= 1; with k == 1 there is no round and the item is copied out.
 * Books 2 launches per round and the capacity bound of the traffic. */
static int union_tree_locked(ua_ctx *c, const u64 *const *items, const u64 *item_caps, int k,
                             u64 *d_len0, u64 *out, u64 *out_n) {
    u64 total = 0;
    for (int i = 0; i < k; i++) total += item_caps[i];
    int rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_A, (total ? total : 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_B, (total ? total : 1) * sizeof(u64)))) return rc;
    u64 *bufs[2] = {(u64 *)c->ws[WS_SCRATCH_A], (u64 *)c->ws[WS_SCRATCH_B]};

    /* host planning over capacities */
    struct Round {
        int nk_prev, npair;
        u64 total_tiles;
        size_t desc_off, tb_off; /* element offsets into the concat uploads */
    };
    std::vector<Round> rounds;
    std::vector<UaDesc> all_descs;
    std::vector<u64> all_tb;
    std::vector<u64> caps(item_caps, item_caps + k);
    std::vector<const u64 *> ptrs(items, items + k);
    u64 max_tiles = 0, cap_work = 0;
    int which = 0;
    while ((int)caps.size() > 1) {
        int nk = (int)caps.size();
        int npair = (nk + 1) / 2;
        Round r;
        r.nk_prev = nk;
        r.npair = npair;
        r.desc_off = all_descs.size();
        r.tb_off = all_tb.size();
        u64 *buf = bufs[which];
        std::vector<u64> ncaps;
        std::vector<const u64 *> nptrs;
        u64 off = 0, tiles = 0;
        for (int pj = 0; pj < npair; pj++) {
            u64 ca = caps[2 * pj];
            u64 cb = (2 * pj + 1 < nk) ? caps[2 * pj + 1] : 0;
            const u64 *pa = ptrs[2 * pj];
            const u64 *pb = (2 * pj + 1 < nk) ? ptrs[2 * pj + 1] : ptrs[2 * pj];
            all_tb.push_back(tiles);
            /* n,m are placeholders; k_make_descs overwrites from device lens */
            all_descs.push_back({pa, ca, pb, cb, buf + off, tiles});
            tiles += (ca + cb + UA_TILE - 1) / UA_TILE;
            nptrs.push_back(buf + off);
            ncaps.push_back(ca + cb);
            off += ca + cb;
            cap_work += ca + cb;
        }
        all_tb.push_back(tiles);
        r.total_tiles = tiles;
        if (tiles > max_tiles) max_tiles = tiles;
        rounds.push_back(r);
        caps.swap(ncaps);
        ptrs.swap(nptrs);
        which ^= 1;
    }
    int R = (int)rounds.size();

    /* workspace: concat descs+tb and the other half of the lens ping-pong
     * in WS_DESC; tiles in the usual slots sized by the largest round */
    size_t descs_bytes = all_descs.size() * sizeof(UaDesc);
    size_t tb_bytes = all_tb.size() * sizeof(u64);
    size_t lens_bytes = (size_t)k * sizeof(u64);
    if ((rc = ws_reserve(c, WS_DESC, descs_bytes + tb_bytes + lens_bytes + 64)))
        return rc;
    u8 *wbase = (u8 *)c->ws[WS_DESC];
    UaDesc *d_descs_all = (UaDesc *)wbase;
    u64 *d_tb_all = (u64 *)(wbase + descs_bytes);
    u64 *d_lens[2] = {d_len0, (u64 *)(wbase + descs_bytes + tb_bytes)};
    if (descs_bytes + tb_bytes) {
        std::vector<u8> hostbuf(descs_bytes + tb_bytes);
        memcpy(hostbuf.data(), all_descs.data(), descs_bytes);
        memcpy(hostbuf.data() + descs_bytes, all_tb.data(), tb_bytes);
        HIP_TRY(hipMemcpyAsync(wbase, hostbuf.data(), hostbuf.size(),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream)); /* hostbuf is scoped */
    }
    if ((rc = ws_reserve(c, WS_TPAIR, (max_tiles + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TA0, (max_tiles + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TCNT, (max_tiles + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (max_tiles + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_PARTIAL, (scan_chunks(max_tiles + 1) + 1) * sizeof(u64))))
        return rc;
    /* one view per round: the round's slice of the concatenated uploads
     * over the shared tile slots; a round's pout is the next round's lens */
    UaPipe p;
    p.tpair = (u32 *)c->ws[WS_TPAIR];
    p.ta0 = (u32 *)c->ws[WS_TA0];
    p.tcnt = (u32 *)c->ws[WS_TCNT];
    p.toff = (u64 *)c->ws[WS_TOFF];
    p.part = (u64 *)c->ws[WS_PARTIAL];

    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    int lcur = 0;
    for (int r = 0; r < R; r++) {
        const Round &rd = rounds[r];
        p.descs = d_descs_all + rd.desc_off;
        p.tb = d_tb_all + rd.tb_off;
        p.n_pairs = rd.npair;
        p.T = rd.total_tiles;
        p.nchunks = scan_chunks(p.T + 1);
        p.pout = d_lens[lcur ^ 1];
        u64 mk = ((u64)rd.npair + UA_BLOCK - 1) / UA_BLOCK;
        hipLaunchKernelGGL(k_make_descs, dim3((u32)mk), dim3(UA_BLOCK), 0, c->stream,
                           p.descs, d_lens[lcur], rd.nk_prev, rd.npair);
        HIP_TRY(hipMemsetAsync(p.tcnt + p.T, 0, sizeof(u32), c->stream));
        if (p.T > 0) {
            enqueue_partition(p, c->stream);
            if ((rc = enqueue_tiles(p, OP_UNION, MODE_COUNT, nullptr, nullptr, c->stream)))
                return rc;
        }
        if ((rc = enqueue_tail(c, p, OP_UNION, nullptr, false, c->stream))) return rc;
        lcur ^= 1;
    }
    /* final item: data in ptrs[0] (capacity position), length in d_lens[lcur][0] */
    u64 copy_grid = ((total ? total : 1) + UA_BLOCK - 1) / UA_BLOCK;
    if (copy_grid > 2048) copy_grid = 2048;
    hipLaunchKernelGGL(k_copy_len, dim3((u32)copy_grid), dim3(UA_BLOCK), 0, c->stream,
                       out, ptrs[0], d_lens[lcur]);
    u64 final_len = 0;
    HIP_TRY(hipMemcpyAsync(&final_len, d_lens[lcur], sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = stats_add(c, c->ev[0], c->ev[1], 2 * R))) return rc;
    c->bytes_algo += 8 * 3 * cap_work; /* capacity upper bound (union count+write) */
    *out_n = final_len;
    return UA_OK;
}

/* ---- MergeSorted k-way (uidlist.go:448): pairwise union tree ---- */
extern "C" int ua_merge_k_dev(ua_ctx *c, const uint64_t *const *lists,
                              const uint64_t *lens, int k, uint64_t *out,
                              uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: scratch reuse */
    if (k <= 0) {
        *out_n = 0;
        return UA_OK;
    }
    if (k == 1) {
        /* the reference's heap merge dedups even a single list
         * (TestMergeSorted9: {1,1,1} -> {1}): union with the empty list */
        ua_dpair pr = {lists[0], lens[0], lists[0], 0, out};
        return run_batch_locked(c, &pr, 1, out_n, OP_UNION);
    }
    /* one leaf per list, capacity == length; the tree's sync after its own
     * upload covers this one, so the caller's lens need not outlive the call */
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ws_reserve(c, WS_KLEN, (size_t)k * sizeof(u64)))) return rc;
    HIP_TRY(hipMemcpyAsync(c->ws[WS_KLEN], lens, (size_t)k * sizeof(u64),
                           hipMemcpyHostToDevice, c->stream));
    return union_tree_locked(c, lists, lens, k, (u64 *)c->ws[WS_KLEN], out, out_n);
}

/* ---- DestUIDs of a CSR UID matrix: flat sort-unique (k_union_leaves) + the
 * union tree over ceil(total / 2048) fixed-size leaves ----
 * The leaves are written to WS_SCRATCH_B, the ping-pong half round 0 does not
 * write, and their lengths to WS_KLEN, both on the device: no per-row
 * descriptors, no offsets on the host.  vals is consumed by the leaf kernel
 * before anything writes out (k_copy_len, last), so out may be vals.
 * The argument checks come before c is touched. */
extern "C" int ua_rows_union_dev(ua_ctx *c, const uint64_t *vals, uint64_t total,
                                 uint64_t *out, uint64_t *out_n) {
    if (!out_n) return UA_ERR_INVALID;
    if (total && (!vals || !out)) return UA_ERR_INVALID;
    /* the tree counts items and pairs in int */
    if (total > (u64)INT32_MAX * UA_SORT_N) return UA_ERR_INVALID;
    if (out != vals && ranges_overlap(vals, total * sizeof(u64), out, total * sizeof(u64)))
        return UA_ERR_INVALID;
    if (!c) return UA_ERR_INVALID;
    if (total == 0) {
        *out_n = 0;
        return UA_OK;
    }
    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: scratch reuse */
    HIP_TRY(hipSetDevice(c->device));
    const int nleaf = (int)((total + UA_SORT_N - 1) / UA_SORT_N);
    int rc;
    /* the sizes union_tree_locked reserves: its own reserve must not move them */
    if ((rc = ws_reserve(c, WS_SCRATCH_A, total * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_B, total * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_KLEN, (size_t)nleaf * sizeof(u64)))) return rc;
    u64 *runs = (u64 *)c->ws[WS_SCRATCH_B];
    u64 *d_len = (u64 *)c->ws[WS_KLEN];
    std::vector<const u64 *> items(nleaf);
    std::vector<u64> caps(nleaf);
    for (int i = 0; i < nleaf; i++) {
        items[i] = runs + (u64)i * UA_SORT_N;
        caps[i] = std::min<u64>(UA_SORT_N, total - (u64)i * UA_SORT_N);
    }
    HIP_TRY(hipEventRecord(c->ev[2], c->stream));
    hipLaunchKernelGGL(k_union_leaves, dim3((u32)nleaf), dim3(UA_BLOCK), 0, c->stream, vals,
                       total, runs, d_len);
    HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    if ((rc = union_tree_locked(c, items.data(), caps.data(), nleaf, d_len, out, out_n)))
        return rc;
    /* the tree has synced the stream: both leaf events are complete */
    if ((rc = stats_add(c, c->ev[2], c->ev[3]))) return rc;
    c->bytes_algo += 16 * total; /* leaf pass: read vals, write runs (upper bound) */
    return UA_OK;
}

/* Pack-limit validation: k_packed decodes blocks only up to
 * num_uids <= UA_MAX_BLOCK_UIDS and deltas_len <= UA_MAX_DELTAS.  The
 * reference supports arbitrary BlockSize, so packs encoded elsewhere must be
 * REJECTED (UA_ERR_INVALID), not silently zeroed by the in-kernel guard
 * (ADVICE r01). */
__global__ __launch_bounds__(UA_BLOCK) void k_validate_pack(
    const u32 *__restrict__ num_uids, const u64 *__restrict__ delta_offs, u64 nb,
    u32 *__restrict__ viol) {
    u64 b = (u64)blockIdx.x * UA_BLOCK + threadIdx.x;
    if (b >= nb) return;
    if (num_uids[b] > UA_MAX_BLOCK_UIDS ||
        delta_offs[b + 1] - delta_offs[b] > UA_MAX_DELTAS)
        atomicOr(viol, 1u);
}

/* enqueue the validation on the ctx stream (read the flag after a sync) */
static int pack_validate_begin(ua_ctx *c, const u32 *num_uids, const u64 *delta_offs,
                               u64 nb) {
    if (!c->d_viol) {
        hipError_t e = hipMalloc((void **)&c->d_viol, sizeof(u32));
        if (e != hipSuccess) {
            g_last_hip = e;
            return UA_ERR_NOMEM;
        }
    }
    HIP_TRY(hipMemsetAsync(c->d_viol, 0, sizeof(u32), c->stream));
    if (nb) {
        u64 g = (nb + UA_BLOCK - 1) / UA_BLOCK;
        hipLaunchKernelGGL(k_validate_pack, dim3((u32)g), dim3(UA_BLOCK), 0, c->stream,
                           num_uids, delta_offs, nb, c->d_viol);
    }
    return UA_OK;
}

/* read the flag; stream must already be synchronized */
static int pack_validate_end(ua_ctx *c) {
    u32 viol = 0;
    HIP_TRY(hipMemcpy(&viol, c->d_viol, sizeof(u32), hipMemcpyDeviceToHost));
    return viol ? UA_ERR_INVALID : UA_OK;
}

/* ---- packed pipeline ---- */
static int run_packed_locked(ua_ctx *c, const ua_dpack *pk, u64 after, const u64 *v, u64 m,
                             u64 *out, u64 *out_n, int decode_only) {
    HIP_TRY(hipSetDevice(c->device));
    u64 nb = pk->n_blocks;
    if (nb == 0) {
        *out_n = 0;
        return UA_OK;
    }
    int rc;
    if ((rc = ws_reserve(c, WS_TCNT, (nb + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (nb + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_STAGE, nb * UA_MAX_BLOCK_UIDS * sizeof(u64)))) return rc;
    u32 *d_cnt = (u32 *)c->ws[WS_TCNT];
    u64 *d_off = (u64 *)c->ws[WS_TOFF];
    u64 *d_stage = (u64 *)c->ws[WS_STAGE];
    HIP_TRY(hipMemsetAsync(d_cnt + nb, 0, sizeof(u32), c->stream));

    if ((rc = pack_validate_begin(c, pk->num_uids, pk->delta_offs, nb))) return rc;
    u64 nwg = (nb + UA_PKW - 1) / UA_PKW;
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (decode_only) {
        hipLaunchKernelGGL(k_packed<1>, dim3((u32)nwg), dim3(UA_BLOCK), 0, c->stream,
                           pk->bases, pk->num_uids, pk->delta_offs, pk->deltas, nb, after,
                           v, m, d_stage, d_cnt, (const u64 *)nullptr, 0,
                           (const ua_ptask *)nullptr);
    } else {
        hipLaunchKernelGGL(k_packed<0>, dim3((u32)nwg), dim3(UA_BLOCK), 0, c->stream,
                           pk->bases, pk->num_uids, pk->delta_offs, pk->deltas, nb, after,
                           v, m, d_stage, d_cnt, (const u64 *)nullptr, 0,
                           (const ua_ptask *)nullptr);
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));

    if ((rc = ws_scan(c, d_cnt, nb + 1, d_off))) return rc;
    u64 *d_part = (u64 *)c->ws[WS_PARTIAL];
    hipLaunchKernelGGL(k_compact_flat, dim3((u32)((nb + 15) / 16)), dim3(UA_BLOCK), 0,
                       c->stream, out, d_cnt, d_off, d_part, d_stage,
                       (u64)UA_MAX_BLOCK_UIDS, nb);
    u64 off_nb = 0, part_nb = 0;
    HIP_TRY(hipMemcpyAsync(&off_nb, d_off + nb, sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(&part_nb, d_part + nb / UA_SCAN_CHUNK, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    *out_n = off_nb + part_nb;

    if ((rc = stats_add(c, c->ev[0], c->ev[1]))) return rc;
    /* algorithmic bytes: deltas + block headers + 8*(m + out) */
    u64 hdr = nb * (8 + 4 + 8);
    u64 dbytes = 0;
    HIP_TRY(hipMemcpyAsync(&dbytes, pk->delta_offs + nb, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((rc = pack_validate_end(c))) {
        *out_n = 0;
        return rc;
    }
    c->bytes_algo += hdr + dbytes + 8 * (m + *out_n);
    return UA_OK;
}

extern "C" int ua_intersect_packed_dev(ua_ctx *c, const ua_dpack *pk, uint64_t after_uid,
                                       const uint64_t *v, uint64_t m, uint64_t *out,
                                       uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return run_packed_locked(c, pk, after_uid, v, m, out, out_n, 0);
}

/* ---- multi-pack fan-out: one grid over every pack's blocks ---- */

/* one fan-out instance as the kernels see it (owns nothing): filled from the
 * ctx workspace by the one-shot call and from ua_pbatch's allocation */
struct UaFan {
    const u64 *bases = nullptr;
    const u32 *nums = nullptr;
    const u64 *doffs = nullptr;
    const u8 *deltas = nullptr;
    u64 nb = 0;               /* blocks over all packs */
    const u64 *pbb = nullptr; /* per-pack first block, n_packs + 1 */
    const ua_ptask *tasks = nullptr;
    int n_packs = 0;
    u32 *cnt = nullptr;       /* nb + 1 counts; the owner zeroes [nb] */
    u64 *offs = nullptr;
    u64 *part = nullptr;
    u64 nchunks = 0;          /* scan chunks over the nb + 1 counts */
    u64 *stage = nullptr;
    u64 *pout = nullptr;
};

/* k_packed -> scan -> k_compact_pack -> k_pair_out on the ctx stream */
static int enqueue_packed_fanout(ua_ctx *c, const UaFan &f) {
    if (f.nb > 0) {
        u64 nwg = (f.nb + UA_PKW - 1) / UA_PKW;
        HIP_TRY(hipEventRecord(c->ev[0], c->stream));
        hipLaunchKernelGGL(k_packed<0>, dim3((u32)nwg), dim3(UA_BLOCK), 0, c->stream,
                           f.bases, f.nums, f.doffs, f.deltas, f.nb, (u64)0,
                           (const u64 *)nullptr, (u64)0, f.stage, f.cnt, f.pbb, f.n_packs,
                           f.tasks);
        HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    }
    enqueue_scan(f.cnt, f.nb + 1, f.offs, f.part, f.nchunks, c->stream);
    if (f.nb > 0)
        hipLaunchKernelGGL(k_compact_pack, dim3((u32)((f.nb + 15) / 16)), dim3(UA_BLOCK),
                           0, c->stream, f.tasks, f.pbb, f.n_packs, f.cnt, f.offs, f.part,
                           f.stage, f.nb);
    u64 poutblk = ((u64)f.n_packs + UA_BLOCK - 1) / UA_BLOCK;
    hipLaunchKernelGGL(k_pair_out, dim3((u32)poutblk), dim3(UA_BLOCK), 0, c->stream,
                       f.offs, f.part, f.pbb, f.n_packs, f.pout);
    return UA_OK;
}

/* the fan-out's lengths to the host, and the call's one sync */
static int packed_fanout_lens(ua_ctx *c, const UaFan &f, uint64_t *out_lens) {
    HIP_TRY(hipMemcpyAsync(out_lens, f.pout, (size_t)f.n_packs * sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    return UA_OK;
}

/* algorithmic bytes: deltas + block headers + 8*(m + out) */
static int packed_fanout_stats(ua_ctx *c, const UaFan &f, const uint64_t *out_lens,
                               u64 deltas_bytes, u64 sum_m) {
    if (f.nb > 0) {
        int rc = stats_add(c, c->ev[0], c->ev[1]);
        if (rc) return rc;
    }
    u64 out_elems = 0;
    for (int p = 0; p < f.n_packs; p++) out_elems += out_lens[p];
    c->bytes_algo += deltas_bytes + f.nb * 20 + 8 * (sum_m + out_elems);
    return UA_OK;
}

extern "C" int ua_intersect_packed_batch_dev(ua_ctx *c, const uint64_t *bases,
                                             const uint32_t *num_uids,
                                             const uint64_t *delta_offs,
                                             const uint8_t *deltas,
                                             const uint64_t *pack_block_base,
                                             int n_packs, const ua_ptask *tasks,
                                             uint64_t *out_lens) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (n_packs <= 0) return UA_OK;
    UaFan f;
    f.bases = bases;
    f.nums = num_uids;
    f.doffs = delta_offs;
    f.deltas = deltas;
    f.n_packs = n_packs;
    f.nb = pack_block_base[n_packs];
    f.nchunks = scan_chunks(f.nb + 1);
    const u64 nb = f.nb;
    int rc;
    /* upload pbb + tasks in one copy (WS_DESC is free during this call) */
    size_t pbb_bytes = ((size_t)n_packs + 1) * sizeof(u64);
    size_t task_bytes = (size_t)n_packs * sizeof(ua_ptask);
    if ((rc = ws_reserve(c, WS_DESC, pbb_bytes + task_bytes))) return rc;
    if ((rc = ws_reserve(c, WS_TCNT, (nb + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (nb + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_PARTIAL, (f.nchunks + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_STAGE, (nb ? nb : 1) * UA_MAX_BLOCK_UIDS * sizeof(u64))))
        return rc;
    if ((rc = ws_reserve(c, WS_POUT, (size_t)n_packs * sizeof(u64)))) return rc;
    f.pbb = (const u64 *)c->ws[WS_DESC];
    f.tasks = (const ua_ptask *)((u8 *)c->ws[WS_DESC] + pbb_bytes);
    f.cnt = (u32 *)c->ws[WS_TCNT];
    f.offs = (u64 *)c->ws[WS_TOFF];
    f.part = (u64 *)c->ws[WS_PARTIAL];
    f.stage = (u64 *)c->ws[WS_STAGE];
    f.pout = (u64 *)c->ws[WS_POUT];

    std::vector<u8> hostbuf(pbb_bytes + task_bytes);
    memcpy(hostbuf.data(), pack_block_base, pbb_bytes);
    memcpy(hostbuf.data() + pbb_bytes, tasks, task_bytes);
    HIP_TRY(hipMemcpyAsync(c->ws[WS_DESC], hostbuf.data(), hostbuf.size(),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(f.cnt + nb, 0, sizeof(u32), c->stream));
    if (nb > 0 && (rc = pack_validate_begin(c, num_uids, delta_offs, nb))) return rc;
    if ((rc = enqueue_packed_fanout(c, f))) return rc;
    u64 dbytes = 0;
    HIP_TRY(hipMemcpyAsync(&dbytes, delta_offs + nb, sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    if ((rc = packed_fanout_lens(c, f, out_lens))) return rc;
    if (nb > 0 && (rc = pack_validate_end(c))) {
        for (int p = 0; p < n_packs; p++) out_lens[p] = 0;
        return rc;
    }
    u64 m_elems = 0;
    for (int p = 0; p < n_packs; p++) m_elems += tasks[p].m;
    return packed_fanout_stats(c, f, out_lens, dbytes, m_elems);
}

extern "C" int ua_decode_dev(ua_ctx *c, const ua_dpack *pk, uint64_t seek_uid, uint64_t *out,
                             uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    return run_packed_locked(c, pk, seek_uid, nullptr, 0, out, out_n, 1);
}

/* ---- one host path for the pack fan-out -> CSR matrix calls ----
 * ua_rows_decode_dev, ua_rows_intersect_packed_dev and ua_rows_decode_mut_dev
 * share one view of a call, ua_drowpacks itself: the block arena, the row
 * boundaries, after, first and the two outputs.  The other two descriptors are
 * those slots plus their own, and their entries build the view from them.
 * Each entry reads: check, lock, reserve, count kernels, offsets, write
 * kernels, finish.  The kernels, the event brackets and whatever differs
 * between the calls stay in the entries. */
#define UA_RD_MAX_BLOCKS (((u64)1 << 24) - 1) /* x 256 uids < 2^32: counts fit the u32 scan */

enum { RV_VALS = 1, RV_OFFS = 2, RV_BOTH = 3 }; /* the outputs an input must not overlap */
struct UaRowsIn {
    const void *p;
    size_t bytes;
    int vs;
};

/* Everything that is rejected before c is read or locked; writes nothing.
 * arena_vs is what the pack arrays, after and first are tested against;
 * row_block_base is always tested against both outputs, a call's own inputs as
 * `extras` says.  The blob's length lives on the device: deltas is held to its
 * first byte. */
static bool rows_args_ok(const ua_ctx *c, const ua_drowpacks &v, const uint64_t *out_total,
                         int arena_vs, std::initializer_list<UaRowsIn> extras) {
    if (!c || !out_total || !v.out_row_offs) return false;
    const u64 nb = v.n_blocks, n_rows = v.n_rows;
    if (nb && (!v.bases || !v.num_uids || !v.delta_offs || !v.deltas)) return false;
    if (n_rows && !v.row_block_base) return false;
    if (v.cap_vals && !v.out_vals) return false;
    if (n_rows == 0 && nb != 0) return false;
    /* the row grids are u32 block counts */
    if (nb > UA_RD_MAX_BLOCKS || n_rows >= ((u64)UA_BLOCK << 31)) return false;
    const size_t ro_bytes = (n_rows + 1) * sizeof(u64), ov_bytes = v.cap_vals * sizeof(u64);
    if (ranges_overlap(v.out_vals, ov_bytes, v.out_row_offs, ro_bytes)) return false;
    const UaRowsIn arena[] = {{v.bases, nb * sizeof(u64), arena_vs},
                              {v.num_uids, nb * sizeof(u32), arena_vs},
                              {v.delta_offs, nb ? (nb + 1) * sizeof(u64) : 0, arena_vs},
                              {v.deltas, (size_t)(nb ? 1 : 0), arena_vs},
                              {v.row_block_base, ro_bytes, RV_BOTH},
                              {v.after, n_rows * sizeof(u64), arena_vs},
                              {v.first, n_rows * sizeof(int32_t), arena_vs}};
    auto clear = [&](const UaRowsIn &in) {
        return !in.p ||
               !(((in.vs & RV_VALS) && ranges_overlap(v.out_vals, ov_bytes, in.p, in.bytes)) ||
                 ((in.vs & RV_OFFS) && ranges_overlap(v.out_row_offs, ro_bytes, in.p, in.bytes)));
    };
    return std::all_of(std::begin(arena), std::end(arena), clear) &&
           std::all_of(extras.begin(), extras.end(), clear);
}

/* every row is empty: no launch, nothing indexes an empty array */
static int rows_publish_empty(ua_ctx *c, const ua_drowpacks &v, uint64_t *out_total) {
    HIP_TRY(hipMemsetAsync(v.out_row_offs, 0, (v.n_rows + 1) * sizeof(u64), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->bytes_algo += 8 * (v.n_rows + 1);
    *out_total = 0;
    return UA_OK;
}

/* one call's scan workspace: a count and an offset per item (a block, or in
 * the mutation call a block or a row head), and first's window lengths per row */
struct UaRowsWs {
    u32 *cnt = nullptr;        /* WS_TCNT [n_items + 1] */
    u64 *offs = nullptr;       /* WS_TOFF [n_items + 1] */
    const u64 *part = nullptr; /* WS_PARTIAL, from rows_offsets on */
    u32 *kcnt = nullptr;       /* WS_KLEN, all three null without first */
    u64 *offs2 = nullptr, *part2 = nullptr;
};

static int rows_reserve_counts(ua_ctx *c, u64 n_items, UaRowsWs &w) {
    int rc;
    if ((rc = ws_reserve(c, WS_TCNT, (n_items + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (n_items + 1) * sizeof(u64)))) return rc;
    w.cnt = (u32 *)c->ws[WS_TCNT];
    w.offs = (u64 *)c->ws[WS_TOFF];
    return UA_OK;
}

static int rows_reserve_window(ua_ctx *c, const ua_drowpacks &v, UaRowsWs &w) {
    if (!v.first) return UA_OK;
    const size_t kcnt_bytes = align16((v.n_rows + 1) * sizeof(u32));
    const size_t offs2_bytes = align16((v.n_rows + 1) * sizeof(u64));
    int rc = ws_reserve(c, WS_KLEN, kcnt_bytes + offs2_bytes +
                                        (scan_chunks(v.n_rows + 1) + 1) * sizeof(u64));
    if (rc) return rc;
    w.kcnt = (u32 *)c->ws[WS_KLEN];
    w.offs2 = (u64 *)((u8 *)c->ws[WS_KLEN] + kcnt_bytes);
    w.part2 = (u64 *)((u8 *)c->ws[WS_KLEN] + kcnt_bytes + offs2_bytes);
    return UA_OK;
}

/* counts -> out_row_offs: the scan over the items, the rows' offsets from it
 * and, with first, the scan of the window lengths over them.  rbb is the rows'
 * boundaries in items.  Adds its launches to *launches. */
static int rows_offsets(ua_ctx *c, const ua_drowpacks &v, const u64 *rbb, u64 n_items,
                        UaRowsWs &w, u64 *launches) {
    int rc;
    const u32 rgrid = (u32)(v.n_rows / UA_BLOCK + 1); /* n_rows + 1 threads */
    if ((rc = ws_scan(c, w.cnt, n_items + 1, w.offs))) return rc;
    w.part = (const u64 *)c->ws[WS_PARTIAL];
    hipLaunchKernelGGL(k_rowdec_rows, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream, rbb, v.n_rows,
                       n_items, w.offs, w.part, v.first, w.kcnt, v.out_row_offs);
    *launches += 3;
    if (v.first) {
        enqueue_scan(w.kcnt, v.n_rows + 1, w.offs2, w.part2, scan_chunks(v.n_rows + 1),
                     c->stream);
        hipLaunchKernelGGL(k_rowdec_offs, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream, w.offs2,
                           w.part2, v.n_rows, v.out_row_offs);
        *launches += 3;
    }
    return UA_OK;
}

/* The one sync of a call.  out_row_offs[n_rows] is the published total; with
 * blocks, the blob length rides along for the byte count and the validation
 * flag is read.  in_bytes is the call's input apart from the blob. */
static int rows_finish(ua_ctx *c, const ua_drowpacks &v, u64 launches, u64 in_bytes,
                       uint64_t *out_total) {
    const bool count_only = (v.out_vals == nullptr);
    int rc;
    u64 total = 0, dbytes = 0;
    HIP_TRY(hipMemcpyAsync(&total, v.out_row_offs + v.n_rows, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    if (v.n_blocks)
        HIP_TRY(hipMemcpyAsync(&dbytes, v.delta_offs + v.n_blocks, sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    if ((rc = stats_add(c, c->ev[0], c->ev[1], launches))) return rc;
    if (!count_only && (rc = stats_add(c, c->ev[2], c->ev[3]))) return rc;
    if (v.n_blocks && (rc = pack_validate_end(c))) {
        *out_total = 0;
        return rc;
    }
    /* the call's input plus its output, not its traffic: a dropped block's
     * deltas are never read, and a probed shared value is read more than once */
    c->bytes_algo += dbytes + in_bytes + 8 * total;
    *out_total = total;
    return (!count_only && total > v.cap_vals) ? UA_ERR_INVALID : UA_OK;
}

/* ---- fan-out decode into a CSR UID matrix ----
 * handleUidPostings' per-key pl.Uids(opts) loop with opts.Intersect == nil
 * (worker/task.go:834-971, posting/list.go:1786-1902) as one call: count ->
 * scan -> (window lengths -> scan ->) write, one sync, three u64 and the
 * validation flag back to the host.  The argument checks come before c is
 * touched. */
extern "C" int ua_rows_decode_dev(ua_ctx *c, const ua_drowpacks *d, uint64_t *out_total) {
    if (!d || !rows_args_ok(c, *d, out_total, RV_VALS, {})) return UA_ERR_INVALID;
    const ua_drowpacks &v = *d;
    const u64 nb = v.n_blocks, n_rows = v.n_rows;

    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (nb == 0) return rows_publish_empty(c, v, out_total);
    int rc;
    UaRowsWs w;
    if ((rc = rows_reserve_counts(c, nb, w))) return rc;
    if ((rc = rows_reserve_window(c, v, w))) return rc;
    HIP_TRY(hipMemsetAsync(w.cnt + nb, 0, sizeof(u32), c->stream));
    if ((rc = pack_validate_begin(c, v.num_uids, v.delta_offs, nb))) return rc;
    u64 launches = 2; /* the validation and the count */

    const u32 nwg = (u32)((nb + UA_PKW - 1) / UA_PKW);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    if (v.after)
        hipLaunchKernelGGL(k_rowdec_count, dim3(nwg), dim3(UA_BLOCK), 0, c->stream, v.bases,
                           v.num_uids, v.delta_offs, v.deltas, nb, v.row_block_base, n_rows,
                           v.after, w.cnt);
    else
        hipLaunchKernelGGL(k_rowdec_count_hdr, dim3((u32)((nb + UA_BLOCK - 1) / UA_BLOCK)),
                           dim3(UA_BLOCK), 0, c->stream, v.bases, v.num_uids, v.delta_offs, nb,
                           w.cnt);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if ((rc = rows_offsets(c, v, v.row_block_base, nb, w, &launches))) return rc;
    if (v.out_vals) {
        HIP_TRY(hipEventRecord(c->ev[2], c->stream));
        hipLaunchKernelGGL(k_rowdec_write, dim3(nwg), dim3(UA_BLOCK), 0, c->stream, v.bases,
                           v.num_uids, v.delta_offs, v.deltas, nb, v.row_block_base, n_rows,
                           v.after, v.first, w.cnt, w.offs, w.part, v.out_row_offs, v.out_vals,
                           v.cap_vals);
        HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    }
    return rows_finish(c, v, launches, 20 * nb + 8 * (n_rows + 1), out_total);
}

/* ---- fan-out intersect into a CSR UID matrix ----
 * handleUidPostings' per-key pl.Uids(opts) loop with opts.Intersect != nil
 * (posting/list.go:1823-1829 -> algo.IntersectCompressedWith, uidlist.go:33)
 * as one call: count -> scan -> write, one sync, two u64 and the validation
 * flag back to the host.  There is no first, so the block scan is the output
 * position and k_rowdec_rows publishes the offsets.  The argument checks come
 * before c is touched. */
extern "C" int ua_rows_intersect_packed_dev(ua_ctx *c, const ua_drowisect *d,
                                            uint64_t *out_total) {
    if (!d) return UA_ERR_INVALID;
    const ua_drowpacks v = {d->bases, d->num_uids, d->delta_offs, d->deltas, d->n_blocks,
                            d->row_block_base, d->n_rows, d->after, nullptr,
                            d->out_vals, d->cap_vals, d->out_row_offs};
    const u64 nb = v.n_blocks, n_rows = v.n_rows, m = d->m;
    if (m && !d->shared) return UA_ERR_INVALID;
    if (d->reserved) return UA_ERR_INVALID; /* ua_drowpacks' first: none here */
    if (m > (UINT64_MAX >> 3)) return UA_ERR_INVALID; /* 8 * m is a byte count below */
    if (!rows_args_ok(c, v, out_total, RV_BOTH, {{d->shared, m * sizeof(u64), RV_BOTH}}))
        return UA_ERR_INVALID;

    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (nb == 0 || m == 0) return rows_publish_empty(c, v, out_total); /* no pack is read */
    int rc;
    UaRowsWs w;
    if ((rc = rows_reserve_counts(c, nb, w))) return rc;
    u64 *d_keep = nullptr; /* (lo, mask) per block, count pass -> write pass */
    if (UA_RI_KEEP && v.out_vals) {
        if ((rc = ws_reserve(c, WS_KLEN, nb * 2 * sizeof(u64)))) return rc;
        d_keep = (u64 *)c->ws[WS_KLEN];
    }
    HIP_TRY(hipMemsetAsync(w.cnt + nb, 0, sizeof(u32), c->stream));
    if ((rc = pack_validate_begin(c, v.num_uids, v.delta_offs, nb))) return rc;
    u64 launches = 2; /* the validation and the count */

    const u32 nwg = (u32)((nb + UA_PKW - 1) / UA_PKW);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_rowisect<false>, dim3(nwg), dim3(UA_BLOCK), 0, c->stream, v.bases,
                       v.num_uids, v.delta_offs, v.deltas, nb, v.row_block_base, n_rows,
                       v.after, d->shared, m, w.cnt, (const u64 *)nullptr,
                       (const u64 *)nullptr, (u64 *)nullptr, (u64)0, d_keep);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if ((rc = rows_offsets(c, v, v.row_block_base, nb, w, &launches))) return rc;
    if (v.out_vals) {
        HIP_TRY(hipEventRecord(c->ev[2], c->stream));
        hipLaunchKernelGGL(k_rowisect<true>, dim3(nwg), dim3(UA_BLOCK), 0, c->stream, v.bases,
                           v.num_uids, v.delta_offs, v.deltas, nb, v.row_block_base, n_rows,
                           v.after, d->shared, m, w.cnt, (const u64 *)w.offs, w.part,
                           v.out_vals, v.cap_vals, d_keep);
        HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    }
    return rows_finish(c, v, launches, 20 * nb + 8 * (n_rows + 1) + 8 * m, out_total);
}

/* ---- fan-out decode with mutation layers into a CSR UID matrix ----
 * handleUidPostings' per-key pl.Uids(opts) loop on lists with a mutable layer
 * (List.iterate, posting/list.go:1135-1251) as one call: flags -> scan ->
 * counts -> scan -> rows (-> window lengths -> scan) -> write, one sync.
 * n_mut == 0 IS ua_rows_decode_dev.  The argument checks come before c is
 * touched.
 *
 * The bound on n_mut: every count goes through the u32 scan, and the largest
 * is a row's window length (k_rowdec_rows' kcnt), at most the call's total
 * 256 * n_blocks + n_mut.  That must stay below UA_MUT_WAVE = 2^32 - 1. */
extern "C" int ua_rows_decode_mut_dev(ua_ctx *c, const ua_drowmut *d, uint64_t *out_total) {
    if (!d) return UA_ERR_INVALID;
    const ua_drowpacks v = {d->bases, d->num_uids, d->delta_offs, d->deltas, d->n_blocks,
                            d->row_block_base, d->n_rows, d->after, d->first,
                            d->out_vals, d->cap_vals, d->out_row_offs};
    const u64 nb = v.n_blocks, n_rows = v.n_rows, cap = v.cap_vals, n_mut = d->n_mut;
    /* the same checks, kernels, launches and stats as the plain call */
    if (n_mut == 0) return ua_rows_decode_dev(c, &v, out_total);
    if (!d->mut_uids || !d->mut_ops || !d->row_mut_base || n_rows == 0) return UA_ERR_INVALID;
    const size_t ro_bytes = (n_rows + 1) * sizeof(u64);
    if (!rows_args_ok(c, v, out_total, RV_VALS,
                      {{d->mut_uids, n_mut * sizeof(u64), RV_BOTH},
                       {d->mut_ops, n_mut, RV_BOTH},
                       {d->row_mut_base, ro_bytes, RV_BOTH}}))
        return UA_ERR_INVALID;
    if (n_mut >= (u64)UINT32_MAX - 256 * nb) return UA_ERR_INVALID;

    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    const u64 n_items = nb + n_rows;
    const u64 nchunksm = scan_chunks(n_mut + 1);
    const size_t flag_bytes = align16((n_mut + 1) * sizeof(u32));
    const size_t poffs_bytes = align16((n_mut + 1) * sizeof(u64));
    const size_t ppart_bytes = align16((nchunksm + 1) * sizeof(u64));
    UaRowsWs w;
    if ((rc = rows_reserve_counts(c, n_items, w))) return rc;
    if ((rc = ws_reserve(c, WS_MUT, flag_bytes + poffs_bytes + ppart_bytes + align16(ro_bytes) +
                                        nb * sizeof(u64) + (2 * nb + 4) * sizeof(u32))))
        return rc;
    if ((rc = rows_reserve_window(c, v, w))) return rc;
    u32 *d_cnt = w.cnt;
    u32 *d_flag = (u32 *)c->ws[WS_MUT];
    u64 *d_poffs = (u64 *)((u8 *)c->ws[WS_MUT] + flag_bytes);
    u64 *d_ppart = (u64 *)((u8 *)d_poffs + poffs_bytes);
    u64 *d_ribb = (u64 *)((u8 *)d_ppart + ppart_bytes);
    u64 *d_brow = (u64 *)((u8 *)d_ribb + align16(ro_bytes)); /* [nb] */
    u32 *d_listn = (u32 *)(d_brow + nb);                     /* [4]: two used */
    u32 *d_wlist = d_listn + 4, *d_olist = d_wlist + nb;     /* [nb] each */
    /* every item's count starts at 0: a malformed row_block_base leaves some unwritten */
    HIP_TRY(hipMemsetAsync(d_cnt, 0, (n_items + 1) * sizeof(u32), c->stream));
    HIP_TRY(hipMemsetAsync(d_listn, 0, 4 * sizeof(u32), c->stream));
    u64 launches = 0;
    if (nb) {
        if ((rc = pack_validate_begin(c, d->num_uids, d->delta_offs, nb))) return rc;
        launches++;
    }
    const UaMutView M = {d->mut_uids, d->mut_ops, d->row_mut_base, n_mut, d_poffs, d_ppart};
    const u32 nwg = (u32)((nb + UA_PKW - 1) / UA_PKW);
    const u32 rgrid = (u32)(n_rows / UA_BLOCK + 1); /* n_rows + 1 threads */
    const u32 hgrid = (u32)std::min<u64>((n_rows + UA_PKW - 1) / UA_PKW, (u64)1 << 20);
    const u32 lgrid = std::min<u32>(nwg, 1u << 14); /* the listed blocks, in steps */
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_rowmut_flags, dim3((u32)(n_mut / UA_BLOCK + 1)), dim3(UA_BLOCK), 0,
                       c->stream, M, n_rows, d->after, d_flag);
    enqueue_scan(d_flag, n_mut + 1, d_poffs, d_ppart, nchunksm, c->stream);
    hipLaunchKernelGGL(k_rowmut_head, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream,
                       d->row_block_base, n_rows, nb, d->bases, M, d_cnt, d_ribb);
    launches += 4;
    if (nb) {
        hipLaunchKernelGGL(k_rowmut_blocks, dim3((u32)((nb + UA_BLOCK - 1) / UA_BLOCK)),
                           dim3(UA_BLOCK), 0, c->stream, d->bases, d->num_uids, d->delta_offs,
                           nb, d->row_block_base, n_rows, d->after, M, d_cnt, d_brow, d_listn, d_wlist,
                           d_olist);
        hipLaunchKernelGGL(k_rowmut<false>, dim3(lgrid), dim3(UA_BLOCK), 0, c->stream, d->bases,
                           d->num_uids, d->delta_offs, d->deltas, nb, d->row_block_base,
                           n_rows, d->after, d->first, M, (const u64 *)d_brow,
                           (const u32 *)d_wlist, (const u32 *)d_listn, (const u64 *)d_ribb,
                           d_cnt, (const u64 *)nullptr, (const u64 *)nullptr,
                           (const u64 *)nullptr, (u64 *)nullptr, (u64)0);
        launches += 2;
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if ((rc = rows_offsets(c, v, d_ribb, n_items, w, &launches))) return rc;
    const u64 *d_offs = w.offs, *d_part = w.part;
    if (v.out_vals) {
        HIP_TRY(hipEventRecord(c->ev[2], c->stream));
        if (nb) {
            hipLaunchKernelGGL(k_rowmut_plain_write, dim3(nwg), dim3(UA_BLOCK), 0, c->stream,
                               d->bases, d->num_uids, d->delta_offs, d->deltas, nb,
                               d->row_block_base, n_rows, d->after, d->first, M,
                               (const u64 *)d_brow, (const u64 *)d_ribb, (const u32 *)d_cnt,
                               d_offs, d_part, (const u64 *)d->out_row_offs, d->out_vals, cap);
            hipLaunchKernelGGL(k_rowmut<true>, dim3(lgrid), dim3(UA_BLOCK), 0, c->stream,
                               d->bases, d->num_uids, d->delta_offs, d->deltas, nb,
                               d->row_block_base, n_rows, d->after, d->first, M,
                               (const u64 *)d_brow, (const u32 *)d_olist,
                               (const u32 *)(d_listn + 1), (const u64 *)d_ribb, d_cnt, d_offs,
                               d_part, (const u64 *)d->out_row_offs, d->out_vals, cap);
            launches += 2;
        }
        hipLaunchKernelGGL(k_rowmut_head_write, dim3(hgrid), dim3(UA_BLOCK), 0, c->stream,
                           d->row_block_base, n_rows, nb, d->after, d->first, M,
                           (const u64 *)d_ribb, (const u32 *)d_cnt, d_offs, d_part,
                           (const u64 *)d->out_row_offs, d->out_vals, cap);
        HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    }
    /* the call's input plus its output, as for the plain call */
    return rows_finish(c, v, launches, 20 * nb + 16 * (n_rows + 1) + 9 * n_mut, out_total);
}

/* ---- prepared pack fan-out (standing query plan) ---- */

struct ua_pbatch {
    UaFan fan; /* over mem: pbb + tasks + cnt + offs + partials + pout + staging */
    void *mem = nullptr;
    u64 deltas_bytes = 0;
    u64 sum_m = 0;
};

extern "C" int ua_pbatch_create(ua_ctx *c, const uint64_t *bases, const uint32_t *num_uids,
                                const uint64_t *delta_offs, const uint8_t *deltas,
                                const uint64_t *pack_block_base, int n_packs,
                                const ua_ptask *tasks, ua_pbatch **out) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (n_packs <= 0) return UA_ERR_INVALID;
    ua_pbatch *b = new ua_pbatch();
    UaFan &f = b->fan;
    f.n_packs = n_packs;
    f.nb = pack_block_base[n_packs];
    f.bases = bases;
    f.nums = num_uids;
    f.doffs = delta_offs;
    f.deltas = deltas;
    for (int p = 0; p < n_packs; p++) b->sum_m += tasks[p].m;
    f.nchunks = scan_chunks(f.nb + 1);

    size_t o_pbb = 0;
    size_t o_tasks = align16(o_pbb + ((size_t)n_packs + 1) * sizeof(u64));
    size_t o_cnt = align16(o_tasks + (size_t)n_packs * sizeof(ua_ptask));
    size_t o_offs = align16(o_cnt + (f.nb + 1) * sizeof(u32));
    size_t o_part = align16(o_offs + (f.nb + 1) * sizeof(u64));
    size_t o_pout = align16(o_part + (f.nchunks + 1) * sizeof(u64));
    size_t o_stage = align16(o_pout + (size_t)n_packs * sizeof(u64));
    size_t total = align16(o_stage + (f.nb ? f.nb : 1) * UA_MAX_BLOCK_UIDS * sizeof(u64));
    hipError_t e = hipMalloc(&b->mem, total);
    if (e != hipSuccess) {
        g_last_hip = e;
        delete b;
        return UA_ERR_NOMEM;
    }
    u8 *base8 = (u8 *)b->mem;
    f.pbb = (const u64 *)(base8 + o_pbb);
    f.tasks = (const ua_ptask *)(base8 + o_tasks);
    f.cnt = (u32 *)(base8 + o_cnt);
    f.offs = (u64 *)(base8 + o_offs);
    f.part = (u64 *)(base8 + o_part);
    f.pout = (u64 *)(base8 + o_pout);
    f.stage = (u64 *)(base8 + o_stage);

    std::vector<u8> hostbuf(o_cnt);
    memcpy(hostbuf.data(), pack_block_base, ((size_t)n_packs + 1) * sizeof(u64));
    memcpy(hostbuf.data() + o_tasks, tasks, (size_t)n_packs * sizeof(ua_ptask));
    HIP_TRY(hipMemcpyAsync(b->mem, hostbuf.data(), hostbuf.size(),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(f.cnt + f.nb, 0, sizeof(u32), c->stream));
    u64 db = 0;
    HIP_TRY(hipMemcpyAsync(&db, delta_offs + f.nb, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    int vrc = (f.nb > 0) ? pack_validate_begin(c, num_uids, delta_offs, f.nb) : UA_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (vrc == UA_OK && f.nb > 0) vrc = pack_validate_end(c);
    if (vrc != UA_OK) {
        ua_pbatch_destroy(c, b);
        return vrc;
    }
    b->deltas_bytes = db;
    *out = b;
    return UA_OK;
}

extern "C" void ua_pbatch_destroy(ua_ctx *c, ua_pbatch *b) {
    if (!b) return;
    (void)hipSetDevice(c->device);
    if (b->mem) (void)hipFree(b->mem);
    delete b;
}

extern "C" int ua_pbatch_run(ua_ctx *c, ua_pbatch *b, uint64_t *out_lens) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = enqueue_packed_fanout(c, b->fan))) return rc;
    if ((rc = packed_fanout_lens(c, b->fan, out_lens))) return rc;
    return packed_fanout_stats(c, b->fan, out_lens, b->deltas_bytes, b->sum_m);
}

/* ---- GPU codec.Encode pipeline (codec.go:393 semantics, engine layout) ---- */
extern "C" int ua_encode_dev(ua_ctx *c, const uint64_t *uids, uint64_t n,
                             uint32_t block_size, uint64_t *bases, uint32_t *num_uids,
                             uint64_t *delta_offs, uint8_t *deltas,
                             uint64_t *n_blocks_out, uint64_t *deltas_bytes_out) {
    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (block_size > UA_MAX_BLOCK_UIDS) return UA_ERR_INVALID;
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(delta_offs, 0, sizeof(u64), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *n_blocks_out = 0;
        *deltas_bytes_out = 0;
        return UA_OK;
    }
    int rc;
    if ((rc = ws_reserve(c, WS_TCNT, (n + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (n + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_A, (n + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_B, (n + 1) * sizeof(u64)))) return rc;
    u32 *d_flags = (u32 *)c->ws[WS_TCNT];
    u64 *d_offs = (u64 *)c->ws[WS_TOFF];
    u64 *d_run = (u64 *)c->ws[WS_SCRATCH_A];
    u64 *d_bstart = (u64 *)c->ws[WS_SCRATCH_B];

    u64 nblk = (n + UA_BLOCK - 1) / UA_BLOCK;
    u64 nblk1 = (n + 1 + UA_BLOCK - 1) / UA_BLOCK;
    HIP_TRY(hipMemsetAsync(d_flags + n, 0, sizeof(u32), c->stream));
    hipLaunchKernelGGL(k_enc_msb_flags, dim3((u32)nblk), dim3(UA_BLOCK), 0, c->stream,
                       uids, n, d_flags);
    if ((rc = ws_scan(c, d_flags, n + 1, d_offs))) return rc;
    u64 *d_part = (u64 *)c->ws[WS_PARTIAL];
    hipLaunchKernelGGL(k_enc_mark_start, dim3((u32)nblk1), dim3(UA_BLOCK), 0, c->stream,
                       d_flags, d_offs, d_part, n, d_run);
    hipLaunchKernelGGL(k_enc_block_flags, dim3((u32)nblk), dim3(UA_BLOCK), 0, c->stream,
                       d_flags, d_offs, d_part, d_run, n, block_size);
    if ((rc = ws_scan(c, d_flags, n + 1, d_offs))) return rc;
    d_part = (u64 *)c->ws[WS_PARTIAL];
    hipLaunchKernelGGL(k_enc_mark_start, dim3((u32)nblk1), dim3(UA_BLOCK), 0, c->stream,
                       d_flags, d_offs, d_part, n, d_bstart);
    u64 off_n = 0, part_n = 0;
    HIP_TRY(hipMemcpyAsync(&off_n, d_offs + n, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&part_n, d_part + n / UA_SCAN_CHUNK, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    u64 nb = off_n + part_n;

    if ((rc = ws_reserve(c, WS_STAGE, (nb ? nb : 1) * UA_ENC_STRIDE))) return rc;
    u8 *d_stage = (u8 *)c->ws[WS_STAGE];
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_encode_blocks, dim3((u32)((nb + UA_PKW - 1) / UA_PKW)),
                       dim3(UA_BLOCK), 0, c->stream, uids, d_bstart, nb, bases, num_uids,
                       d_flags, d_stage);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    HIP_TRY(hipMemsetAsync(d_flags + nb, 0, sizeof(u32), c->stream));
    if ((rc = ws_scan(c, d_flags, nb + 1, d_offs))) return rc;
    d_part = (u64 *)c->ws[WS_PARTIAL];
    hipLaunchKernelGGL(k_enc_finalize, dim3((u32)((nb + 1 + 3) / 4)), dim3(UA_BLOCK), 0,
                       c->stream, d_stage, d_flags, d_offs, d_part, nb, deltas, delta_offs);
    u64 db_off = 0, db_part = 0;
    HIP_TRY(hipMemcpyAsync(&db_off, d_offs + nb, sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipMemcpyAsync(&db_part, d_part + nb / UA_SCAN_CHUNK, sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    *n_blocks_out = nb;
    *deltas_bytes_out = db_off + db_part;

    if ((rc = stats_add(c, c->ev[0], c->ev[1]))) return rc;
    c->bytes_algo += 8 * n + (db_off + db_part) + nb * 20;
    return UA_OK;
}

/* ---- CSR UID matrix -> fan-out of UidPacks ----
 * One codec.Encoder{BlockSize} per row (codec.go:57-136, codec.Encode
 * codec.go:393) for a whole population of lists, as the bulk reducer
 * (dgraph/cmd/bulk/reduce.go:811-861, count_index.go:133-154) and the rollup
 * (posting/list.go:1609-1664) run it one key after another: row bits -> count
 * -> two tile scans -> row bases (-> write), one sync, two u64 back to the
 * host.  The argument checks come before c is touched. */
extern "C" int ua_rows_encode_dev(ua_ctx *c, const ua_drowenc *d, uint64_t *n_blocks,
                                  uint64_t *deltas_bytes) {
    if (!c || !d || !n_blocks || !deltas_bytes || !d->row_block_base) return UA_ERR_INVALID;
    const u64 total = d->total, n_rows = d->n_rows;
    if (total && !d->vals) return UA_ERR_INVALID;
    if (n_rows && !d->row_offs) return UA_ERR_INVALID;
    if (n_rows == 0 && total != 0) return UA_ERR_INVALID;
    if (d->block_size > UA_MAX_BLOCK_UIDS) return UA_ERR_INVALID;
    /* the tile grid and the row grids are u32 block counts; a tile's counts
     * (<= UA_RTILE blocks, <= 5 * UA_RTILE + 3 bytes) always fit the u32 scan */
    if (total >= ((u64)UA_RTILE << 31) || n_rows >= ((u64)UA_BLOCK << 31))
        return UA_ERR_INVALID;
    const int n_null = !d->bases + !d->num_uids + !d->delta_offs + !d->deltas;
    if (n_null != 0 && n_null != 4) return UA_ERR_INVALID;
    const bool count_only = (n_null == 4);
    if (count_only && (d->cap_blocks || d->cap_deltas)) return UA_ERR_INVALID;
    if (d->cap_blocks >= ((u64)1 << 60)) return UA_ERR_INVALID; /* byte sizes below stay in u64 */
    const size_t ro_bytes = (n_rows + 1) * sizeof(u64);
    const struct {
        const void *p;
        size_t bytes;
    } rg[] = {{d->vals, total * sizeof(u64)},
              {d->row_offs, d->row_offs ? ro_bytes : 0},
              {d->row_block_base, ro_bytes},
              {d->bases, d->cap_blocks * sizeof(u64)},
              {d->num_uids, d->cap_blocks * sizeof(u32)},
              {d->delta_offs, count_only ? 0 : (d->cap_blocks + 1) * sizeof(u64)},
              {d->deltas, d->cap_deltas}};
    const int n_rg = (int)(sizeof(rg) / sizeof(rg[0]));
    for (int a = 2; a < n_rg; a++) /* every output against the inputs and the other outputs */
        for (int b = 0; b < a; b++)
            if (rg[a].p && rg[b].p && ranges_overlap(rg[a].p, rg[a].bytes, rg[b].p, rg[b].bytes))
                return UA_ERR_INVALID;

    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    if (total == 0) { /* every row is empty: zero offsets, no launch */
        HIP_TRY(hipMemsetAsync(d->row_block_base, 0, ro_bytes, c->stream));
        if (!count_only) HIP_TRY(hipMemsetAsync(d->delta_offs, 0, sizeof(u64), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->bytes_algo += 16 * (n_rows + 1);
        *n_blocks = 0;
        *deltas_bytes = 0;
        return UA_OK;
    }
    const u64 ntiles = (total + UA_RTILE - 1) / UA_RTILE;
    const u64 nchunks = scan_chunks(ntiles + 1);
    const size_t ycnt_bytes = align16((ntiles + 1) * sizeof(u32));
    const size_t yoffs_bytes = align16((ntiles + 1) * sizeof(u64));
    const size_t ypart_bytes = align16((nchunks + 1) * sizeof(u64));
    const size_t bits_bytes = (size_t)(ntiles * UA_RWORDS + 1) * sizeof(u64);
    int rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_A, bits_bytes))) return rc;
    if ((rc = ws_reserve(c, WS_RKW, (size_t)ntiles * UA_RWORDS * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_TCNT, (size_t)(ntiles + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (size_t)(ntiles + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_KLEN, ycnt_bytes + yoffs_bytes + ypart_bytes + 2 * sizeof(u64))))
        return rc;
    u64 *d_bits = (u64 *)c->ws[WS_SCRATCH_A];
    u64 *d_kw = (u64 *)c->ws[WS_RKW];
    u32 *d_bcnt = (u32 *)c->ws[WS_TCNT];
    u64 *d_boffs = (u64 *)c->ws[WS_TOFF];
    u32 *d_ycnt = (u32 *)c->ws[WS_KLEN];
    u64 *d_yoffs = (u64 *)((u8 *)c->ws[WS_KLEN] + ycnt_bytes);
    u64 *d_ypart = (u64 *)((u8 *)d_yoffs + yoffs_bytes);
    u64 *d_sizes = (u64 *)((u8 *)d_ypart + ypart_bytes);
    const u32 eff = d->block_size ? (u32)d->block_size : 1;
    const u32 rgrid = (u32)(n_rows / UA_BLOCK + 1); /* n_rows + 1 threads */

    HIP_TRY(hipMemsetAsync(d_bits, 0, bits_bytes, c->stream));
    /* one extra zero count each: d_off(ntiles) is the grand total */
    HIP_TRY(hipMemsetAsync(d_bcnt + ntiles, 0, sizeof(u32), c->stream));
    HIP_TRY(hipMemsetAsync(d_ycnt + ntiles, 0, sizeof(u32), c->stream));
    hipLaunchKernelGGL(k_rowenc_rowbits, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream,
                       d->row_offs, n_rows, total, (unsigned long long *)d_bits);
    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    hipLaunchKernelGGL(k_rowenc<false>, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                       d->vals, total, d->row_offs, n_rows, d_bits, eff, d_kw, d_bcnt, d_ycnt,
                       nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (u64)0,
                       nullptr, (u64)0);
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    if ((rc = ws_scan(c, d_bcnt, ntiles + 1, d_boffs))) return rc;
    const u64 *d_bpart = (const u64 *)c->ws[WS_PARTIAL];
    enqueue_scan(d_ycnt, ntiles + 1, d_yoffs, d_ypart, nchunks, c->stream);
    hipLaunchKernelGGL(k_rowenc_rows, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream, d->row_offs,
                       n_rows, total, ntiles, d_kw, d_boffs, d_bpart, d_yoffs, d_ypart,
                       d->row_block_base, d->delta_offs, d->cap_blocks, d_sizes);
    if (!count_only) {
        HIP_TRY(hipEventRecord(c->ev[2], c->stream));
        hipLaunchKernelGGL(k_rowenc<true>, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                           d->vals, total, d->row_offs, n_rows, d_bits, eff, d_kw, d_bcnt,
                           d_ycnt, d_boffs, d_bpart, d_yoffs, d_ypart, d->bases, d->num_uids,
                           d->delta_offs, d->cap_blocks, d->deltas, d->cap_deltas);
        HIP_TRY(hipEventRecord(c->ev[3], c->stream));
    }
    u64 sizes[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(sizes, d_sizes, sizeof(sizes), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    if ((rc = stats_add(c, c->ev[0], c->ev[1], 7))) return rc;
    if (!count_only && (rc = stats_add(c, c->ev[2], c->ev[3]))) return rc;
    c->bytes_algo += 8 * total + 8 * (n_rows + 1) + sizes[1] + 20 * sizes[0] + 8 * (n_rows + 1);
    *n_blocks = sizes[0];
    *deltas_bytes = sizes[1];
    return (!count_only && (sizes[0] > d->cap_blocks || sizes[1] > d->cap_deltas))
               ? UA_ERR_INVALID
               : UA_OK;
}

/* host-pointer form of ua_rows_encode_dev: total is row_offs[n_rows].  Upload,
 * one device call, download what fits the capacities; count-only with all
 * four pack outputs NULL. */
extern "C" int ua_rows_encode(ua_ctx *c, const uint64_t *vals, const uint64_t *row_offs,
                              uint64_t n_rows, uint64_t block_size, uint64_t *bases,
                              uint32_t *num_uids, uint64_t *delta_offs, uint64_t cap_blocks,
                              uint8_t *deltas, uint64_t cap_deltas, uint64_t *row_block_base,
                              uint64_t *n_blocks, uint64_t *deltas_bytes) {
    if (!c || !n_blocks || !deltas_bytes || !row_block_base) return UA_ERR_INVALID;
    if (n_rows && !row_offs) return UA_ERR_INVALID;
    const u64 total = n_rows ? row_offs[n_rows] : 0;
    if (total && !vals) return UA_ERR_INVALID;
    if (block_size > UA_MAX_BLOCK_UIDS) return UA_ERR_INVALID;
    if (total >= ((u64)UA_RTILE << 31) || n_rows >= ((u64)UA_BLOCK << 31))
        return UA_ERR_INVALID;
    const int n_null = !bases + !num_uids + !delta_offs + !deltas;
    if (n_null != 0 && n_null != 4) return UA_ERR_INVALID;
    const bool count_only = (n_null == 4);
    if (count_only && (cap_blocks || cap_deltas)) return UA_ERR_INVALID;
    if (cap_blocks >= ((u64)1 << 60)) return UA_ERR_INVALID;
    /* the device never needs more than one block per uid and 5 bytes + 3 per uid */
    const u64 cb = std::min(cap_blocks, total), cd = std::min(cap_deltas, 5 * total + 3);

    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_H* reuse */
    HIP_TRY(hipSetDevice(c->device));
    const u64 nro = n_rows + 1;
    int rc;
    if ((rc = ws_reserve(c, WS_HU, (total + nro) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_HOUT, (nro + cb + cb + 1) * sizeof(u64) + cb * sizeof(u32) + 16)))
        return rc;
    if ((rc = ws_reserve(c, WS_HV, cd + 16))) return rc;
    u64 *d_vals = (u64 *)c->ws[WS_HU], *d_ro = d_vals + total;
    u64 *d_rbb = (u64 *)c->ws[WS_HOUT], *d_bases = d_rbb + nro, *d_doffs = d_bases + cb;
    u32 *d_nums = (u32 *)(d_doffs + cb + 1);
    u8 *d_blob = (u8 *)c->ws[WS_HV];
    if (total)
        HIP_TRY(hipMemcpyAsync(d_vals, vals, total * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    if (n_rows)
        HIP_TRY(hipMemcpyAsync(d_ro, row_offs, nro * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    else
        HIP_TRY(hipMemsetAsync(d_ro, 0, sizeof(u64), c->stream));
    ua_drowenc d = {d_vals, d_ro, n_rows, total, block_size,
                    count_only ? nullptr : d_bases, count_only ? nullptr : d_nums,
                    count_only ? nullptr : d_doffs, count_only ? 0 : cb,
                    count_only ? nullptr : d_blob, count_only ? 0 : cd, d_rbb};
    u64 nb = 0, db = 0;
    rc = ua_rows_encode_dev(c, &d, &nb, &db);
    if (rc && rc != UA_ERR_INVALID) return rc;
    if (rc == UA_ERR_INVALID && nb == 0 && db == 0 && total) return rc; /* rejected */
    *n_blocks = nb;
    *deltas_bytes = db;
    HIP_TRY(hipMemcpyAsync(row_block_base, d_rbb, nro * sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    if (!count_only && rc == UA_OK && nb <= cap_blocks && db <= cap_deltas) {
        if (nb) {
            HIP_TRY(hipMemcpyAsync(bases, d_bases, nb * sizeof(u64), hipMemcpyDeviceToHost,
                                   c->stream));
            HIP_TRY(hipMemcpyAsync(num_uids, d_nums, nb * sizeof(u32), hipMemcpyDeviceToHost,
                                   c->stream));
        }
        HIP_TRY(hipMemcpyAsync(delta_offs, d_doffs, (nb + 1) * sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
        if (db)
            HIP_TRY(hipMemcpyAsync(deltas, d_blob, db, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!count_only && (nb > cap_blocks || db > cap_deltas)) return UA_ERR_INVALID;
    return UA_OK;
}

/* ==================== host-side codec (codec.Encode restated) ==================== */

/* ---- sort and paginate a CSR UID matrix ----
 * applyPagination (query/query.go:2493-2507), sortWithoutIndex
 * (worker/sort.go:139-187), sortAndPaginateUsingVar (query/query.go:2697-2738)
 * and the cascade paginations (query/query.go:1483-1487, 3006-3010) for every
 * row in one call: row bits -> tile sort -> merge rounds -> page -> scan ->
 * offsets (-> write), one sync, one u64 back to the host.  The argument checks
 * come before c is touched. */
static u32 rsort_rounds(u64 ntiles) { /* ceil(log2(ntiles)) */
    u32 k = 0;
    while (((u64)1 << k) < ntiles) k++;
    return k;
}

extern "C" int ua_rows_sort_dev(ua_ctx *c, const ua_drowsort *d, uint64_t *out_total) {
    if (!c || !d || !out_total || !d->out_row_offs) return UA_ERR_INVALID;
    const u64 total = d->total, n_rows = d->n_rows, flags = d->flags;
    if (total && !d->vals) return UA_ERR_INVALID;
    if (n_rows && !d->row_offs) return UA_ERR_INVALID;
    if (n_rows == 0 && total != 0) return UA_ERR_INVALID;
    if (!d->keys && (flags || d->has)) return UA_ERR_INVALID;
    if (flags & ~(u64)(UA_SORT_DESC | UA_SORT_MULTI | UA_SORT_DROP_NULLS)) return UA_ERR_INVALID;
    if ((flags & UA_SORT_MULTI) && (flags & UA_SORT_DROP_NULLS)) return UA_ERR_INVALID;
    if (d->out_ms_offs && !(flags & UA_SORT_MULTI)) return UA_ERR_INVALID;
    if (d->out_src && !d->out_vals) return UA_ERR_INVALID;
    if (!d->out_vals && d->cap_vals) return UA_ERR_INVALID;
    /* a flat index and the null bit share a 32-bit tag */
    if (total >= ((u64)1 << 31) || n_rows >= ((u64)1 << 31)) return UA_ERR_INVALID;
    if (d->cap_vals >= ((u64)1 << 60)) return UA_ERR_INVALID; /* byte sizes below stay in u64 */
    const bool count_only = !d->out_vals;
    const size_t ro_bytes = (n_rows + 1) * sizeof(u64);
    const struct {
        const void *p;
        size_t bytes;
    } rg[] = {{d->vals, total * sizeof(u64)},
              {d->row_offs, d->row_offs ? ro_bytes : 0},
              {d->keys, total * sizeof(u64)},
              {d->has, total},
              {d->out_row_offs, ro_bytes},
              {d->out_vals, d->cap_vals * sizeof(u64)},
              {d->out_src, d->cap_vals * sizeof(u64)},
              {d->out_ms_offs, n_rows * sizeof(int32_t)}};
    const int n_rg = (int)(sizeof(rg) / sizeof(rg[0]));
    for (int a = 4; a < n_rg; a++) /* every output against the inputs and the other outputs */
        for (int b = 0; b < a; b++)
            if (rg[a].p && rg[b].p && ranges_overlap(rg[a].p, rg[a].bytes, rg[b].p, rg[b].bytes))
                return UA_ERR_INVALID;

    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const u64 in_bytes = 8 * total + (d->keys ? 8 * total : 0) + (d->has ? total : 0) +
                         8 * (n_rows + 1);
    /* The lengths depend on the order only through the MULTI extension and |V|.
     * total == 0 takes the page-only path: every row is empty, but out_ms_offs
     * still receives max(offset, 0) per row (sort.go:170-178 with start == 0). */
    const bool sorted = d->keys && total &&
                        !(count_only && !(flags & (UA_SORT_MULTI | UA_SORT_DROP_NULLS)));
    const u64 ntiles = (total + UA_RTILE - 1) / UA_RTILE;
    const u32 rounds = sorted ? rsort_rounds(ntiles) : 0;
    const size_t bits_bytes = (size_t)(ntiles * UA_RWORDS + 1) * sizeof(u64);
    const size_t rs_bytes = align16(n_rows * sizeof(u32));
    int rc;
    if (sorted) {
        if ((rc = ws_reserve(c, WS_SCRATCH_A, bits_bytes))) return rc;
        if ((rc = ws_reserve(c, WS_SCRATCH_B, (size_t)total * 24))) return rc;
        if ((rc = ws_reserve(c, WS_RKW, (size_t)ntiles * 2 * sizeof(u32)))) return rc;
    }
    if ((rc = ws_reserve(c, WS_TCNT, (size_t)(n_rows + 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (size_t)(n_rows + 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_KLEN, rs_bytes + 2 * sizeof(u64)))) return rc;
    u64 *d_bits = (u64 *)c->ws[WS_SCRATCH_A];
    u64 *d_key[2] = {nullptr, nullptr};
    u32 *d_tag[2] = {nullptr, nullptr};
    if (sorted) {
        d_key[0] = (u64 *)c->ws[WS_SCRATCH_B];
        d_key[1] = d_key[0] + total;
        d_tag[0] = (u32 *)(d_key[1] + total);
        d_tag[1] = d_tag[0] + total;
    }
    u32 *d_trows = (u32 *)c->ws[WS_RKW];
    u32 *d_len = (u32 *)c->ws[WS_TCNT];
    u64 *d_offs = (u64 *)c->ws[WS_TOFF];
    u32 *d_rstart = (u32 *)c->ws[WS_KLEN];
    /* word 0: u32 max segments, u32 "row_offs descends"; word 1: the total */
    u64 *d_words = (u64 *)((u8 *)c->ws[WS_KLEN] + rs_bytes);
    u32 *d_bad = (u32 *)d_words + 1;
    const u32 rgrid = (u32)(n_rows / UA_BLOCK + 1); /* n_rows + 1 threads */
    u64 launches = 0;

    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(hipMemsetAsync(d_words, 0, sizeof(u64), c->stream));
    if (sorted) {
        HIP_TRY(hipMemsetAsync(d_bits, 0, bits_bytes, c->stream));
        hipLaunchKernelGGL(k_rsort_rowbits, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream,
                           d->row_offs, n_rows, total, (unsigned long long *)d_bits,
                           (u32 *)d_words);
        hipLaunchKernelGGL(k_rsort_tiles, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                           d->keys, d->has, total, (u32)((flags & UA_SORT_DESC) != 0), d_bits,
                           d->row_offs, n_rows, d_key[0], d_tag[0], d_trows);
        /* the host knows only total: a round past the longest row's returns at once */
        for (u32 k = 0; k < rounds; k++)
            hipLaunchKernelGGL(k_rsort_round, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                               d->row_offs, n_rows, total, d_trows, (const u32 *)d_words, k,
                               d_key[k & 1], d_tag[k & 1], d_key[(k + 1) & 1],
                               d_tag[(k + 1) & 1]);
        launches += 2 + rounds;
    }
    hipLaunchKernelGGL(k_rsort_page, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream, d->row_offs,
                       n_rows, total, d_key[0], d_tag[0], d_key[1], d_tag[1], (u32)sorted,
                       (u32)flags, (int)d->count, (int)d->offset, d_len, d_rstart,
                       d->out_ms_offs, d_bad);
    if ((rc = ws_scan(c, d_len, n_rows + 1, d_offs))) return rc;
    const u64 *d_part = (const u64 *)c->ws[WS_PARTIAL];
    hipLaunchKernelGGL(k_rsort_offs, dim3(rgrid), dim3(UA_BLOCK), 0, c->stream, n_rows, d_offs,
                       d_part, d_bad, d->out_row_offs, d_words + 1);
    launches += 4;
    const u64 wcap = d->cap_vals < total ? d->cap_vals : total; /* a page never grows a row */
    if (!count_only && wcap) {
        hipLaunchKernelGGL(k_rsort_write, dim3((u32)((wcap + UA_BLOCK - 1) / UA_BLOCK)),
                           dim3(UA_BLOCK), 0, c->stream, d->vals, d->row_offs, n_rows, total,
                           d_tag[0], d_tag[1], (u32)sorted, d_offs, d_part, d_rstart, d_bad,
                           d->out_vals, d->out_src, wcap);
        launches += 1;
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    u64 need = 0;
    HIP_TRY(hipMemcpyAsync(&need, d_words + 1, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    if ((rc = stats_add(c, c->ev[0], c->ev[1], launches))) return rc;
    const u64 written = count_only ? 0 : (need < d->cap_vals ? need : d->cap_vals);
    c->bytes_algo += in_bytes + 8 * (n_rows + 1) + 8 * written + (d->out_src ? 8 * written : 0);
    *out_total = need;
    return (!count_only && need > d->cap_vals) ? UA_ERR_INVALID : UA_OK;
}

/* host-pointer form of ua_rows_sort_dev: total is row_offs[n_rows].  Upload,
 * one device call, download the offsets and what fits the capacity. */
extern "C" int ua_rows_sort(ua_ctx *c, const uint64_t *vals, const uint64_t *row_offs,
                            uint64_t n_rows, const uint64_t *keys, const uint8_t *has,
                            uint64_t flags, int32_t count, int32_t offset, uint64_t *out_vals,
                            uint64_t cap_vals, uint64_t *out_row_offs, uint64_t *out_src,
                            int32_t *out_ms_offs, uint64_t *out_total) {
    if (!c || !out_total || !out_row_offs) return UA_ERR_INVALID;
    if (n_rows && !row_offs) return UA_ERR_INVALID;
    if (n_rows >= ((u64)1 << 31)) return UA_ERR_INVALID;
    const u64 total = n_rows ? row_offs[n_rows] : 0;
    if (total && !vals) return UA_ERR_INVALID;
    if (total >= ((u64)1 << 31)) return UA_ERR_INVALID;
    if (!keys && (flags || has)) return UA_ERR_INVALID;
    if (flags & ~(u64)(UA_SORT_DESC | UA_SORT_MULTI | UA_SORT_DROP_NULLS)) return UA_ERR_INVALID;
    if ((flags & UA_SORT_MULTI) && (flags & UA_SORT_DROP_NULLS)) return UA_ERR_INVALID;
    if (out_ms_offs && !(flags & UA_SORT_MULTI)) return UA_ERR_INVALID;
    if (out_src && !out_vals) return UA_ERR_INVALID;
    if (!out_vals && cap_vals) return UA_ERR_INVALID;
    if (cap_vals >= ((u64)1 << 60)) return UA_ERR_INVALID;
    const bool count_only = !out_vals;
    const u64 cb = std::min(cap_vals, total); /* the device never needs more */

    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_H* reuse */
    HIP_TRY(hipSetDevice(c->device));
    const u64 nro = n_rows + 1;
    int rc;
    if ((rc = ws_reserve(c, WS_HU, (2 * total + nro) * sizeof(u64) + 16))) return rc;
    if ((rc = ws_reserve(c, WS_HV, total + 16))) return rc;
    if ((rc = ws_reserve(c, WS_HOUT, (nro + 2 * cb) * sizeof(u64) + n_rows * sizeof(int32_t) + 16)))
        return rc;
    u64 *d_vals = (u64 *)c->ws[WS_HU], *d_keys = d_vals + total, *d_ro = d_keys + total;
    u8 *d_has = (u8 *)c->ws[WS_HV];
    u64 *d_oro = (u64 *)c->ws[WS_HOUT], *d_ov = d_oro + nro, *d_os = d_ov + cb;
    int32_t *d_ms = (int32_t *)(d_os + cb);
    if (total) {
        HIP_TRY(hipMemcpyAsync(d_vals, vals, total * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
        if (keys)
            HIP_TRY(hipMemcpyAsync(d_keys, keys, total * sizeof(u64), hipMemcpyHostToDevice,
                                   c->stream));
        if (has) HIP_TRY(hipMemcpyAsync(d_has, has, total, hipMemcpyHostToDevice, c->stream));
    }
    if (n_rows)
        HIP_TRY(hipMemcpyAsync(d_ro, row_offs, nro * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    else
        HIP_TRY(hipMemsetAsync(d_ro, 0, sizeof(u64), c->stream));
    ua_drowsort d = {};
    d.vals = d_vals;
    d.row_offs = d_ro;
    d.n_rows = n_rows;
    d.total = total;
    d.keys = keys ? d_keys : nullptr;
    d.has = has ? d_has : nullptr;
    d.flags = flags;
    d.count = count;
    d.offset = offset;
    d.out_vals = count_only ? nullptr : d_ov;
    d.cap_vals = count_only ? 0 : cb;
    d.out_row_offs = d_oro;
    d.out_src = out_src ? d_os : nullptr;
    d.out_ms_offs = out_ms_offs ? d_ms : nullptr;
    u64 need = 0;
    rc = ua_rows_sort_dev(c, &d, &need);
    if (rc && rc != UA_ERR_INVALID) return rc;
    if (rc == UA_ERR_INVALID && need == 0) return rc; /* rejected */
    *out_total = need;
    HIP_TRY(hipMemcpyAsync(out_row_offs, d_oro, nro * sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    if (out_ms_offs && n_rows)
        HIP_TRY(hipMemcpyAsync(out_ms_offs, d_ms, n_rows * sizeof(int32_t),
                               hipMemcpyDeviceToHost, c->stream));
    if (!count_only && need <= cap_vals && need) {
        HIP_TRY(hipMemcpyAsync(out_vals, d_ov, need * sizeof(u64), hipMemcpyDeviceToHost,
                               c->stream));
        if (out_src)
            HIP_TRY(hipMemcpyAsync(out_src, d_os, need * sizeof(u64), hipMemcpyDeviceToHost,
                                   c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return (!count_only && need > cap_vals) ? UA_ERR_INVALID : UA_OK;
}

/* ---- transpose a CSR UID matrix ----
 * dedup.addValue's grouping (query/groupby.go:104-128, formResult :195-260,
 * fillGroupedVars :265-361) and rebuildReverseEdges (posting/index.go:1759-1791)
 * over a whole matrix in one call: tile sort -> merge rounds -> flags -> scan
 * (-> write), one sync, two u64 back to the host.  The argument checks come
 * before c is touched. */
extern "C" int ua_rows_transpose_dev(ua_ctx *c, const ua_drowtr *d, uint64_t *n_groups,
                                     uint64_t *out_total) {
    if (!c || !d || !n_groups || !out_total) return UA_ERR_INVALID;
    const u64 total = d->total, n_rows = d->n_rows, flags = d->flags;
    if (total && !d->vals) return UA_ERR_INVALID;
    if (n_rows && !d->row_offs) return UA_ERR_INVALID;
    if (n_rows == 0 && total != 0) return UA_ERR_INVALID;
    if (flags & ~(u64)UA_TR_UNIQUE) return UA_ERR_INVALID;
    if (!d->out_keys != !d->out_offs) return UA_ERR_INVALID;
    if (!d->out_keys && d->cap_keys) return UA_ERR_INVALID;
    if (!d->out_vals && d->cap_vals) return UA_ERR_INVALID;
    if (d->out_src && !d->out_vals) return UA_ERR_INVALID;
    if (d->out_vals && !d->out_keys) return UA_ERR_INVALID;
    /* a flat index and the dead bit share a 32-bit tag */
    if (total >= ((u64)1 << 31) || n_rows >= ((u64)1 << 31)) return UA_ERR_INVALID;
    if (d->cap_keys >= ((u64)1 << 60) || d->cap_vals >= ((u64)1 << 60))
        return UA_ERR_INVALID; /* byte sizes below stay in u64 */
    const struct {
        const void *p;
        size_t bytes;
    } rg[] = {{d->vals, total * sizeof(u64)},
              {d->row_offs, d->row_offs ? (n_rows + 1) * sizeof(u64) : 0},
              {d->row_uids, n_rows * sizeof(u64)},
              {d->row_keep, n_rows},
              {d->out_keys, d->cap_keys * sizeof(u64)},
              {d->out_offs, (d->cap_keys + 1) * sizeof(u64)},
              {d->out_vals, d->cap_vals * sizeof(u64)},
              {d->out_src, d->cap_vals * sizeof(u64)}};
    const int n_rg = (int)(sizeof(rg) / sizeof(rg[0]));
    for (int a = 4; a < n_rg; a++) /* every output against the inputs and the other outputs */
        for (int b = 0; b < a; b++)
            if (rg[a].p && rg[b].p && ranges_overlap(rg[a].p, rg[a].bytes, rg[b].p, rg[b].bytes))
                return UA_ERR_INVALID;

    std::lock_guard<std::recursive_mutex> g(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    const bool groups = d->out_keys != nullptr; /* the full and the groups-only form */
    const u64 ntiles = (total + UA_RTILE - 1) / UA_RTILE;
    const u32 rounds = rsort_rounds(ntiles);
    const u64 M = ntiles + 1;
    int rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_A, (size_t)(total ? total : 1) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_SCRATCH_B, (size_t)(total ? total : 1) * 24))) return rc;
    if ((rc = ws_reserve(c, WS_TCNT, (size_t)(2 * M) * sizeof(u32)))) return rc;
    if ((rc = ws_reserve(c, WS_TOFF, (size_t)(2 * M) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_KLEN, 2 * sizeof(u64)))) return rc;
    u32 *d_erow = (u32 *)c->ws[WS_SCRATCH_A];
    u64 *d_key[2];
    u32 *d_tag[2];
    d_key[0] = (u64 *)c->ws[WS_SCRATCH_B];
    d_key[1] = d_key[0] + total;
    d_tag[0] = (u32 *)(d_key[1] + total);
    d_tag[1] = d_tag[0] + total;
    u32 *d_cnt = (u32 *)c->ws[WS_TCNT];
    u64 *d_offs = (u64 *)c->ws[WS_TOFF];
    unsigned long long *d_words = (unsigned long long *)c->ws[WS_KLEN]; /* groups, entries */
    u64 launches = 0;

    HIP_TRY(hipEventRecord(c->ev[0], c->stream));
    HIP_TRY(hipMemsetAsync(d_words, 0, 2 * sizeof(u64), c->stream));
    if (total == 0) {
        if (groups) HIP_TRY(hipMemsetAsync(d->out_offs, 0, sizeof(u64), c->stream));
    } else {
        const u32 unique = (u32)((flags & UA_TR_UNIQUE) != 0);
        hipLaunchKernelGGL(k_rtr_tiles, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream, d->vals,
                           total, d->row_offs, n_rows, d->row_keep, d_key[0], d_tag[0], d_erow);
        for (u32 k = 0; k < rounds; k++)
            hipLaunchKernelGGL(k_rtr_round, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                               total, (u32)ntiles, k, d_key[k & 1], d_tag[k & 1],
                               d_key[(k + 1) & 1], d_tag[(k + 1) & 1]);
        const u64 *fkey = d_key[rounds & 1];
        const u32 *ftag = d_tag[rounds & 1];
        hipLaunchKernelGGL(k_rtr_groups<false>, dim3((u32)ntiles), dim3(UA_BLOCK), 0, c->stream,
                           fkey, ftag, d_erow, total, n_rows, (u32)ntiles, unique, d_cnt,
                           (const u64 *)nullptr, (const u64 *)nullptr, d_words,
                           (const u64 *)nullptr, (u64 *)nullptr, (u64 *)nullptr, (u64)0,
                           (u64 *)nullptr, (u64 *)nullptr, (u64)0);
        launches += 2 + rounds;
        if (groups) {
            if ((rc = ws_scan(c, d_cnt, 2 * M, d_offs))) return rc;
            const u64 *d_part = (const u64 *)c->ws[WS_PARTIAL];
            hipLaunchKernelGGL(k_rtr_groups<true>, dim3((u32)ntiles), dim3(UA_BLOCK), 0,
                               c->stream, fkey, ftag, d_erow, total, n_rows, (u32)ntiles, unique,
                               d_cnt, d_offs, d_part, d_words, d->row_uids, d->out_keys,
                               d->out_offs, d->cap_keys, d->out_vals, d->out_src, d->cap_vals);
            launches += 3;
        }
    }
    HIP_TRY(hipEventRecord(c->ev[1], c->stream));
    u64 need[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(need, d_words, 2 * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipGetLastError());
    if ((rc = stats_add(c, c->ev[0], c->ev[1], launches))) return rc;
    const u64 wk = groups ? std::min(need[0], d->cap_keys) : 0;
    const u64 wv = d->out_vals ? std::min(need[1], d->cap_vals) : 0;
    c->bytes_algo += 8 * total + 8 * (n_rows + 1) + (d->row_uids ? 8 * n_rows : 0) +
                     (d->row_keep ? n_rows : 0) + (groups ? 8 * wk + 8 * (wk + 1) : 0) +
                     8 * wv + (d->out_src ? 8 * wv : 0);
    *n_groups = need[0];
    *out_total = need[1];
    const bool is_short = (groups && need[0] > d->cap_keys) ||
                          (d->out_vals && need[1] > d->cap_vals);
    return is_short ? UA_ERR_INVALID : UA_OK;
}

/* host-pointer form of ua_rows_transpose_dev: total is row_offs[n_rows].
 * Upload, one device call, download what fits the capacities. */
extern "C" int ua_rows_transpose(ua_ctx *c, const uint64_t *vals, const uint64_t *row_offs,
                                 uint64_t n_rows, const uint64_t *row_uids,
                                 const uint8_t *row_keep, uint64_t flags, uint64_t *out_keys,
                                 uint64_t *out_offs, uint64_t cap_keys, uint64_t *out_vals,
                                 uint64_t *out_src, uint64_t cap_vals, uint64_t *n_groups,
                                 uint64_t *out_total) {
    if (!c || !n_groups || !out_total) return UA_ERR_INVALID;
    if (n_rows && !row_offs) return UA_ERR_INVALID;
    if (n_rows >= ((u64)1 << 31)) return UA_ERR_INVALID;
    const u64 total = n_rows ? row_offs[n_rows] : 0;
    if (total && !vals) return UA_ERR_INVALID;
    if (total >= ((u64)1 << 31)) return UA_ERR_INVALID;
    if (flags & ~(u64)UA_TR_UNIQUE) return UA_ERR_INVALID;
    if (!out_keys != !out_offs) return UA_ERR_INVALID;
    if (!out_keys && cap_keys) return UA_ERR_INVALID;
    if (!out_vals && cap_vals) return UA_ERR_INVALID;
    if (out_src && !out_vals) return UA_ERR_INVALID;
    if (out_vals && !out_keys) return UA_ERR_INVALID;
    if (cap_keys >= ((u64)1 << 60) || cap_vals >= ((u64)1 << 60)) return UA_ERR_INVALID;
    const u64 ck = std::min(cap_keys, total), cv = std::min(cap_vals, total);

    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_H* reuse */
    HIP_TRY(hipSetDevice(c->device));
    const u64 nro = n_rows + 1;
    int rc;
    if ((rc = ws_reserve(c, WS_HU, (total + nro + n_rows) * sizeof(u64) + 16))) return rc;
    if ((rc = ws_reserve(c, WS_HV, n_rows + 16))) return rc;
    if ((rc = ws_reserve(c, WS_HOUT, (2 * ck + 1 + 2 * cv) * sizeof(u64) + 16))) return rc;
    u64 *d_vals = (u64 *)c->ws[WS_HU], *d_ro = d_vals + total, *d_ru = d_ro + nro;
    u8 *d_keep = (u8 *)c->ws[WS_HV];
    u64 *d_ok = (u64 *)c->ws[WS_HOUT], *d_oo = d_ok + ck, *d_ov = d_oo + ck + 1, *d_os = d_ov + cv;
    if (total)
        HIP_TRY(hipMemcpyAsync(d_vals, vals, total * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    if (n_rows) {
        HIP_TRY(hipMemcpyAsync(d_ro, row_offs, nro * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
        if (row_uids)
            HIP_TRY(hipMemcpyAsync(d_ru, row_uids, n_rows * sizeof(u64), hipMemcpyHostToDevice,
                                   c->stream));
        if (row_keep)
            HIP_TRY(hipMemcpyAsync(d_keep, row_keep, n_rows, hipMemcpyHostToDevice, c->stream));
    } else {
        HIP_TRY(hipMemsetAsync(d_ro, 0, sizeof(u64), c->stream));
    }
    ua_drowtr d = {};
    d.vals = d_vals;
    d.row_offs = d_ro;
    d.n_rows = n_rows;
    d.total = total;
    d.row_uids = (row_uids && n_rows) ? d_ru : nullptr;
    d.row_keep = (row_keep && n_rows) ? d_keep : nullptr;
    d.flags = flags;
    d.out_keys = out_keys ? d_ok : nullptr;
    d.out_offs = out_keys ? d_oo : nullptr;
    d.cap_keys = out_keys ? ck : 0;
    d.out_vals = out_vals ? d_ov : nullptr;
    d.out_src = out_src ? d_os : nullptr;
    d.cap_vals = out_vals ? cv : 0;
    u64 ng = UINT64_MAX, nt = UINT64_MAX;
    rc = ua_rows_transpose_dev(c, &d, &ng, &nt);
    if (rc && rc != UA_ERR_INVALID) return rc;
    if (rc == UA_ERR_INVALID && ng == UINT64_MAX) return rc; /* rejected */
    *n_groups = ng;
    *out_total = nt;
    const bool is_short = (out_keys && ng > cap_keys) || (out_vals && nt > cap_vals);
    if (!is_short && out_keys) {
        if (ng) HIP_TRY(hipMemcpyAsync(out_keys, d_ok, ng * sizeof(u64), hipMemcpyDeviceToHost,
                                       c->stream));
        HIP_TRY(hipMemcpyAsync(out_offs, d_oo, (ng + 1) * sizeof(u64), hipMemcpyDeviceToHost,
                               c->stream));
        if (out_vals && nt) {
            HIP_TRY(hipMemcpyAsync(out_vals, d_ov, nt * sizeof(u64), hipMemcpyDeviceToHost,
                                   c->stream));
            if (out_src)
                HIP_TRY(hipMemcpyAsync(out_src, d_os, nt * sizeof(u64), hipMemcpyDeviceToHost,
                                       c->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return is_short ? UA_ERR_INVALID : UA_OK;
}

struct ua_owned_pack {
    std::vector<ua_block> blocks;
    std::vector<u8> blob; /* all deltas, contiguous */
    std::vector<size_t> blob_off;
    ua_pack view;
};

static size_t gv_encode4_cc(u8 *buf, const u32 v[4]) {
    u8 *p = buf + 1;
    u8 tag = 0;
    for (int i = 0; i < 4; i++) {
        u32 x = v[i];
        int len = 1 + (x > 0xffu) + (x > 0xffffu) + (x > 0xffffffu);
        tag = (u8)(tag | ((len - 1) << (2 * i)));
        for (int b = 0; b < len; b++) {
            *p++ = (u8)(x & 0xff);
            x >>= 8;
        }
    }
    buf[0] = tag;
    return (size_t)(p - buf);
}

/* codec.go:57 packBlock + :107 Add + :117 32-MSB/blockSize split rules */
extern "C" int ua_encode(const uint64_t *uids, uint64_t n, uint32_t block_size,
                         ua_owned_pack **out) {
    ua_owned_pack *pk = new ua_owned_pack();
    u64 i = 0;
    while (i < n) {
        /* collect one block: stop at block_size or 32-MSB change */
        u64 start = i;
        u64 base = uids[i];
        i++;
        while (i < n && (i - start) < (u64)(block_size ? block_size : 1) &&
               ((uids[i] ^ uids[i - 1]) >> 32) == 0) {
            i++;
        }
        /* blockSize==0 in Go packs after every Add -> 1-uid blocks */
        u64 cnt = i - start;
        ua_block blk;
        blk.base = base;
        blk.num_uids = (u32)cnt;
        size_t blob_start = pk->blob.size();
        u64 last = base;
        u64 off = start + 1, rem = cnt - 1;
        u8 gbuf[17];
        u32 tmp[4];
        for (;;) {
            for (int j = 0; j < 4; j++) {
                if ((u64)j >= rem) {
                    tmp[j] = 0;
                } else {
                    tmp[j] = (u32)(uids[off + (u64)j] - last);
                    last = uids[off + (u64)j];
                }
            }
            size_t sz = gv_encode4_cc(gbuf, tmp);
            pk->blob.insert(pk->blob.end(), gbuf, gbuf + sz);
            if (rem <= 4) break;
            off += 4;
            rem -= 4;
        }
        blk.deltas_len = (u32)(pk->blob.size() - blob_start);
        blk.deltas = nullptr; /* fixed up below (blob may reallocate) */
        pk->blob_off.push_back(blob_start);
        pk->blocks.push_back(blk);
    }
    for (size_t b = 0; b < pk->blocks.size(); b++)
        pk->blocks[b].deltas = pk->blob.data() + pk->blob_off[b];
    pk->view.block_size = block_size;
    pk->view.n_blocks = pk->blocks.size();
    pk->view.blocks = pk->blocks.data();
    *out = pk;
    return UA_OK;
}

extern "C" const ua_pack *ua_owned_pack_view(ua_owned_pack *pk) { return &pk->view; }
extern "C" void ua_owned_pack_free(ua_owned_pack *pk) { delete pk; }

extern "C" uint64_t ua_pack_exact_len(const ua_pack *p) {
    if (!p) return 0;
    u64 n = 0;
    for (u64 i = 0; i < p->n_blocks; i++) n += p->blocks[i].num_uids;
    return n;
}

extern "C" uint64_t ua_pack_approx_len(const ua_pack *p) {
    if (!p) return 0;
    return p->n_blocks * (u64)p->block_size;
}

extern "C" int ua_pack_flat_sizes(const ua_pack *p, uint64_t *n_blocks,
                                  uint64_t *deltas_bytes, uint64_t *total_uids) {
    if (!p) return UA_ERR_INVALID;
    u64 db = 0, tu = 0;
    for (u64 i = 0; i < p->n_blocks; i++) {
        db += p->blocks[i].deltas_len;
        tu += p->blocks[i].num_uids;
    }
    *n_blocks = p->n_blocks;
    *deltas_bytes = db;
    *total_uids = tu;
    return UA_OK;
}

extern "C" int ua_pack_flatten(const ua_pack *p, uint64_t *bases, uint32_t *num_uids,
                               uint64_t *delta_offs, uint8_t *deltas_blob) {
    if (!p) return UA_ERR_INVALID;
    u64 off = 0;
    for (u64 i = 0; i < p->n_blocks; i++) {
        const ua_block &b = p->blocks[i];
        if (b.num_uids > UA_MAX_BLOCK_UIDS || b.deltas_len > UA_MAX_DELTAS)
            return UA_ERR_INVALID;
        bases[i] = b.base;
        num_uids[i] = b.num_uids;
        delta_offs[i] = off;
        memcpy(deltas_blob + off, b.deltas, b.deltas_len);
        off += b.deltas_len;
    }
    delta_offs[p->n_blocks] = off;
    return UA_OK;
}

/* ==================== host-pointer convenience (mirrors algo signatures) ==================== */

extern "C" int64_t ua_index_of(const uint64_t *u, uint64_t n, uint64_t uid) {
    /* algo.IndexOf (uidlist.go:546): one binary search — host-side, like the
     * reference; batched GPU form is ua_index_of_batch_dev. */
    u64 lo = 0, hi = n;
    while (lo < hi) {
        u64 mid = (lo + hi) >> 1;
        if (u[mid] >= uid) hi = mid;
        else lo = mid + 1;
    }
    return (lo < n && u[lo] == uid) ? (int64_t)lo : -1;
}

static int host_pair_op(ua_ctx *c, const u64 *u, u64 n, const u64 *v, u64 m, u64 *out,
                        u64 *out_n, int op) {
    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_H* reuse */
    int rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = ws_reserve(c, WS_HU, (n ? n : 1) * sizeof(u64)))) return rc;
        if ((rc = ws_reserve(c, WS_HV, (m ? m : 1) * sizeof(u64)))) return rc;
        u64 cap = (op == OP_UNION) ? n + m : (op == OP_DIFF ? n : (n < m ? n : m));
        if ((rc = ws_reserve(c, WS_HOUT, (cap ? cap : 1) * sizeof(u64)))) return rc;
        HIP_TRY(hipMemcpyAsync(c->ws[WS_HU], u, n * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMemcpyAsync(c->ws[WS_HV], v, m * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    }
    ua_dpair pr = {(const u64 *)c->ws[WS_HU], n, (const u64 *)c->ws[WS_HV], m,
                   (u64 *)c->ws[WS_HOUT]};
    u64 len = 0;
    if ((rc = run_batch(c, &pr, 1, &len, op))) return rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipMemcpyAsync(out, c->ws[WS_HOUT], len * sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out_n = len;
    return UA_OK;
}

extern "C" int ua_intersect(ua_ctx *c, const uint64_t *u, uint64_t n, const uint64_t *v,
                            uint64_t m, uint64_t *out, uint64_t *out_n) {
    return host_pair_op(c, u, n, v, m, out, out_n, OP_INTERSECT);
}

extern "C" int ua_difference(ua_ctx *c, const uint64_t *u, uint64_t n, const uint64_t *v,
                             uint64_t m, uint64_t *out, uint64_t *out_n) {
    return host_pair_op(c, u, n, v, m, out, out_n, OP_DIFF);
}

static int host_upload_lists(ua_ctx *c, const uint64_t *const *lists, const uint64_t *lens,
                             int k, std::vector<const u64 *> &dptrs, u64 &total) {
    total = 0;
    for (int i = 0; i < k; i++) total += lens[i];
    int rc;
    if ((rc = ws_reserve(c, WS_HU, (total ? total : 1) * sizeof(u64)))) return rc;
    u64 *base = (u64 *)c->ws[WS_HU];
    u64 off = 0;
    dptrs.resize(k);
    for (int i = 0; i < k; i++) {
        HIP_TRY(hipMemcpyAsync(base + off, lists[i], lens[i] * sizeof(u64),
                               hipMemcpyHostToDevice, c->stream));
        dptrs[i] = base + off;
        off += lens[i];
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UA_OK;
}

extern "C" int ua_intersect_k(ua_ctx *c, const uint64_t *const *lists, const uint64_t *lens,
                              int k, uint64_t *out, uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> gop(c->mu);
    if (k <= 0) {
        *out_n = 0;
        return UA_OK;
    }
    std::vector<const u64 *> dptrs;
    u64 total;
    int rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = host_upload_lists(c, lists, lens, k, dptrs, total))) return rc;
        u64 cap = lens[0];
        for (int i = 1; i < k; i++) cap = std::min(cap, lens[i]);
        if ((rc = ws_reserve(c, WS_HOUT, (cap ? cap : 1) * sizeof(u64)))) return rc;
    }
    u64 len = 0;
    if ((rc = ua_intersect_k_dev(c, dptrs.data(), lens, k, (u64 *)c->ws[WS_HOUT], &len)))
        return rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipMemcpyAsync(out, c->ws[WS_HOUT], len * sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out_n = len;
    return UA_OK;
}

extern "C" int ua_merge_k(ua_ctx *c, const uint64_t *const *lists, const uint64_t *lens,
                          int k, uint64_t *out, uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> gop(c->mu);
    if (k <= 0) {
        *out_n = 0;
        return UA_OK;
    }
    std::vector<const u64 *> dptrs;
    u64 total;
    int rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipSetDevice(c->device));
        if ((rc = host_upload_lists(c, lists, lens, k, dptrs, total))) return rc;
        if ((rc = ws_reserve(c, WS_HOUT, (total ? total : 1) * sizeof(u64)))) return rc;
    }
    u64 len = 0;
    if ((rc = ua_merge_k_dev(c, dptrs.data(), lens, k, (u64 *)c->ws[WS_HOUT], &len)))
        return rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipMemcpyAsync(out, c->ws[WS_HOUT], len * sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out_n = len;
    return UA_OK;
}

extern "C" int ua_intersect_packed(ua_ctx *c, const ua_pack *pack, uint64_t after_uid,
                                   const uint64_t *v, uint64_t m, uint64_t *out,
                                   uint64_t *out_n) {
    std::lock_guard<std::recursive_mutex> gop(c->mu);
    if (!pack || pack->n_blocks == 0) {
        *out_n = 0;
        return UA_OK;
    }
    u64 nb, db, tu;
    int rc = ua_pack_flat_sizes(pack, &nb, &db, &tu);
    if (rc) return rc;
    std::vector<u64> bases(nb), doffs(nb + 1);
    std::vector<u32> nums(nb);
    std::vector<u8> blob(db ? db : 1);
    if ((rc = ua_pack_flatten(pack, bases.data(), nums.data(), doffs.data(), blob.data())))
        return rc;
    ua_dpack dpk;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipSetDevice(c->device));
        size_t need = nb * 8 + (nb + 1) * 8 + nb * 4 + blob.size() + 64;
        if ((rc = ws_reserve(c, WS_PACK, need))) return rc;
        u8 *w = (u8 *)c->ws[WS_PACK];
        u64 *d_bases = (u64 *)w;
        u64 *d_doffs = (u64 *)(w + nb * 8);
        u32 *d_nums = (u32 *)(w + nb * 8 + (nb + 1) * 8);
        u8 *d_blob = w + nb * 8 + (nb + 1) * 8 + nb * 4;
        HIP_TRY(hipMemcpyAsync(d_bases, bases.data(), nb * 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_doffs, doffs.data(), (nb + 1) * 8, hipMemcpyHostToDevice,
                               c->stream));
        HIP_TRY(hipMemcpyAsync(d_nums, nums.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_blob, blob.data(), blob.size(), hipMemcpyHostToDevice,
                               c->stream));
        if ((rc = ws_reserve(c, WS_HV, (m ? m : 1) * sizeof(u64)))) return rc;
        HIP_TRY(hipMemcpyAsync(c->ws[WS_HV], v, m * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
        u64 cap = std::min(tu, m);
        if ((rc = ws_reserve(c, WS_HOUT, (cap ? cap : 1) * sizeof(u64)))) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        dpk = {pack->block_size, nb, d_bases, d_nums, d_doffs, d_blob, tu};
    }
    u64 len = 0;
    if ((rc = ua_intersect_packed_dev(c, &dpk, after_uid, (const u64 *)c->ws[WS_HV], m,
                                      (u64 *)c->ws[WS_HOUT], &len)))
        return rc;
    {
        std::lock_guard<std::recursive_mutex> g(c->mu);
        HIP_TRY(hipMemcpyAsync(out, c->ws[WS_HOUT], len * sizeof(u64),
                               hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *out_n = len;
    return UA_OK;
}

/* host-pointer form of ua_rows_filter_dev: what the cgo shim's
 * updateUidMatrix loop (query/query.go:1425-1437) and the worker/task.go:1352,
 * 1617,1692,1778 loops call ONCE instead of once per row.  total is
 * row_offs[n_rows]; out_vals may be vals and out_row_offs may be row_offs
 * (the device works on its own buffers). */
extern "C" int ua_rows_filter(ua_ctx *c, const uint64_t *vals, const uint64_t *row_offs,
                              uint64_t n_rows, const uint64_t *shared, uint64_t m, int mode,
                              uint64_t *out_vals, uint64_t *out_row_offs,
                              uint64_t *out_total) {
    if (!c || !row_offs || !out_row_offs || !out_total) return UA_ERR_INVALID;
    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_H* reuse */
    HIP_TRY(hipSetDevice(c->device));
    const u64 total = row_offs[n_rows];
    const u64 nro = n_rows + 1;
    int rc;
    if ((rc = ws_reserve(c, WS_HU, (total + nro) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_HV, (m ? m : 1) * sizeof(u64)))) return rc;
    if ((rc = ws_reserve(c, WS_HOUT, (total + nro) * sizeof(u64)))) return rc;
    u64 *d_vals = (u64 *)c->ws[WS_HU], *d_ro = d_vals + total;
    u64 *d_ov = (u64 *)c->ws[WS_HOUT], *d_oro = d_ov + total;
    if (total)
        HIP_TRY(hipMemcpyAsync(d_vals, vals, total * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    HIP_TRY(hipMemcpyAsync(d_ro, row_offs, nro * sizeof(u64), hipMemcpyHostToDevice,
                           c->stream));
    if (m)
        HIP_TRY(hipMemcpyAsync(c->ws[WS_HV], shared, m * sizeof(u64), hipMemcpyHostToDevice,
                               c->stream));
    ua_drows d = {d_vals, d_ro, n_rows, total, (const u64 *)c->ws[WS_HV], m, d_ov, d_oro};
    u64 kept = 0;
    if ((rc = ua_rows_filter_dev(c, &d, mode, &kept))) return rc;
    if (kept)
        HIP_TRY(hipMemcpyAsync(out_vals, d_ov, kept * sizeof(u64), hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipMemcpyAsync(out_row_offs, d_oro, nro * sizeof(u64), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_total = kept;
    return UA_OK;
}

/* host-pointer form of ua_rows_union_dev: DestUIDs = MergeSorted(UidMatrix)
 * (query/query.go:1874,2290,2505) over the rows' concatenation, sorted or
 * not.  The device works in place on its own copy, so out may overlap vals
 * in any way. */
extern "C" int ua_rows_union(ua_ctx *c, const uint64_t *vals, uint64_t total, uint64_t *out,
                             uint64_t *out_n) {
    if (!out_n) return UA_ERR_INVALID;
    if (total && (!vals || !out)) return UA_ERR_INVALID;
    if (!c) return UA_ERR_INVALID;
    if (total == 0) {
        *out_n = 0;
        return UA_OK;
    }
    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_H* reuse */
    HIP_TRY(hipSetDevice(c->device));
    int rc;
    if ((rc = ws_reserve(c, WS_HU, total * sizeof(u64)))) return rc;
    u64 *d_vals = (u64 *)c->ws[WS_HU];
    HIP_TRY(hipMemcpyAsync(d_vals, vals, total * sizeof(u64), hipMemcpyHostToDevice,
                           c->stream));
    u64 len = 0;
    if ((rc = ua_rows_union_dev(c, d_vals, total, d_vals, &len))) return rc;
    if (len)
        HIP_TRY(hipMemcpyAsync(out, d_vals, len * sizeof(u64), hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *out_n = len;
    return UA_OK;
}

/* ---- host-pointer forms of the pack fan-out -> CSR matrix calls ----
 * Flatten, upload, one device call, download.  The three forms share the
 * three helpers below and keep their own null checks, their extra inputs,
 * their descriptor and the device call. */
struct UaHostArena { /* packs[0..n_rows) as one block arena, a null pack an empty row */
    std::vector<u64> bases, doffs, rbb;
    std::vector<u32> nums;
    std::vector<u8> blob;
    u64 nb = 0;
};

/* n_mut is the mutation call's (0 elsewhere): both limits on the block count
 * reject before anything is allocated */
static int rows_flatten(const ua_pack *const *packs, u64 n_rows, u64 n_mut, UaHostArena &a) {
    u64 nb = 0, db = 0;
    for (u64 r = 0; r < n_rows; r++) {
        if (!packs[r]) continue;
        u64 pnb, pdb, ptu;
        int prc = ua_pack_flat_sizes(packs[r], &pnb, &pdb, &ptu);
        if (prc) return prc;
        nb += pnb;
        db += pdb;
    }
    if (nb > UA_RD_MAX_BLOCKS || n_mut >= (u64)UINT32_MAX - 256 * nb) return UA_ERR_INVALID;
    a.nb = nb;
    a.bases.resize(nb);
    a.doffs.resize(nb + 1);
    a.rbb.resize(n_rows + 1);
    a.nums.resize(nb);
    a.blob.resize(db ? db : 1);
    u64 b0 = 0, off0 = 0;
    for (u64 r = 0; r < n_rows; r++) {
        a.rbb[r] = b0;
        if (!packs[r] || packs[r]->n_blocks == 0) continue;
        int prc = ua_pack_flatten(packs[r], a.bases.data() + b0, a.nums.data() + b0,
                                  a.doffs.data() + b0, a.blob.data() + off0);
        if (prc) return prc;
        const u64 pnb = packs[r]->n_blocks, pdb = a.doffs[b0 + pnb];
        for (u64 i = 0; i <= pnb; i++) a.doffs[b0 + i] += off0; /* pack-local -> arena */
        b0 += pnb;
        off0 += pdb;
    }
    a.rbb[n_rows] = nb;
    a.doffs[nb] = off0;
    return UA_OK;
}

struct UaHostIn { /* one host array to upload */
    const void *src;
    size_t bytes, align; /* align: the element size */
    void *dev;           /* out: where it went; null for a null src or no bytes */
};

static size_t rows_place(size_t &end, const UaHostIn &x) {
    const size_t off = (end + x.align - 1) & ~(x.align - 1);
    end = off + x.bytes;
    return off;
}

/* WS_PACK takes the arena and the call's extra inputs, one after the other,
 * every array at its natural alignment; WS_HOUT the values and then the
 * offsets.  v gets the arena and the outputs as device pointers.  Nothing is
 * synced: the device call's sync covers the uploads, so the host arrays must
 * live past it. */
static int rows_upload(ua_ctx *c, const UaHostArena &a, u64 n_rows, bool want_vals,
                       u64 cap_vals, std::initializer_list<UaHostIn *> extras,
                       ua_drowpacks &v) {
    const u64 nb = a.nb, nro = n_rows + 1;
    UaHostIn arena[] = {{a.bases.data(), nb * 8, 8, nullptr},
                        {a.doffs.data(), (nb + 1) * 8, 8, nullptr},
                        {a.rbb.data(), nro * 8, 8, nullptr},
                        {a.nums.data(), nb * 4, 4, nullptr},
                        {a.blob.data(), a.blob.size(), 1, nullptr}};
    std::vector<UaHostIn *> all;
    for (UaHostIn &x : arena) all.push_back(&x);
    for (UaHostIn *x : extras)
        if (x->src && x->bytes) all.push_back(x);
    size_t need = 0;
    for (const UaHostIn *x : all) rows_place(need, *x);
    int rc;
    if ((rc = ws_reserve(c, WS_PACK, need))) return rc;
    if ((rc = ws_reserve(c, WS_HOUT, (cap_vals + nro) * sizeof(u64)))) return rc;
    size_t end = 0;
    for (UaHostIn *x : all) {
        x->dev = (u8 *)c->ws[WS_PACK] + rows_place(end, *x);
        if (x->bytes)
            HIP_TRY(hipMemcpyAsync(x->dev, x->src, x->bytes, hipMemcpyHostToDevice, c->stream));
    }
    u64 *d_ov = (u64 *)c->ws[WS_HOUT];
    v = {(const u64 *)arena[0].dev, (const u32 *)arena[3].dev, (const u64 *)arena[1].dev,
         (const u8 *)arena[4].dev, nb, (const u64 *)arena[2].dev, n_rows, nullptr, nullptr,
         want_vals ? d_ov : nullptr, cap_vals, d_ov + cap_vals};
    return UA_OK;
}

/* After the device call.  Short capacity: the offsets are complete and still
 * go back; the values only after UA_OK. */
static int rows_download(ua_ctx *c, const ua_drowpacks &v, int rc, u64 total,
                         uint64_t *out_vals, uint64_t *out_row_offs) {
    if (rc && !(rc == UA_ERR_INVALID && total > v.cap_vals)) return rc;
    const u64 nv = out_vals ? std::min<u64>(total, v.cap_vals) : 0;
    if (nv && rc == UA_OK)
        HIP_TRY(hipMemcpyAsync(out_vals, v.out_vals, nv * sizeof(u64), hipMemcpyDeviceToHost,
                               c->stream));
    HIP_TRY(hipMemcpyAsync(out_row_offs, v.out_row_offs, (v.n_rows + 1) * sizeof(u64),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return rc;
}

/* host-pointer form of ua_rows_decode_dev: the UidMatrix of a per-key fan-out
 * (worker/task.go:834-971, one pl.Uids(opts) per key with opts.Intersect ==
 * nil) from host packs; a null packs[r] is an empty row. */
extern "C" int ua_rows_decode(ua_ctx *c, const ua_pack *const *packs, uint64_t n_rows,
                              const uint64_t *after, const int32_t *first,
                              uint64_t *out_vals, uint64_t cap_vals, uint64_t *out_row_offs,
                              uint64_t *out_total) {
    if (!c || !out_total || !out_row_offs) return UA_ERR_INVALID;
    if (n_rows && !packs) return UA_ERR_INVALID;
    if (cap_vals && !out_vals) return UA_ERR_INVALID;
    UaHostArena a;
    int rc;
    if ((rc = rows_flatten(packs, n_rows, 0, a))) return rc;

    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_PACK/WS_HOUT reuse */
    HIP_TRY(hipSetDevice(c->device));
    UaHostIn h_after = {after, n_rows * 8, 8, nullptr}, h_first = {first, n_rows * 4, 4, nullptr};
    ua_drowpacks d;
    if ((rc = rows_upload(c, a, n_rows, out_vals != nullptr, cap_vals, {&h_after, &h_first}, d)))
        return rc;
    d.after = (const u64 *)h_after.dev;
    d.first = (const int32_t *)h_first.dev;
    u64 total = 0;
    rc = ua_rows_decode_dev(c, &d, &total);
    *out_total = total;
    return rows_download(c, d, rc, total, out_vals, out_row_offs);
}

/* host-pointer form of ua_rows_decode_mut_dev: the UidMatrix of a per-key
 * fan-out over lists with mutable layers (one pl.Uids(opts) per key through
 * List.iterate, posting/list.go:1135-1251) from host packs and host mutation
 * slices; a null packs[r] is a row without blocks. */
extern "C" int ua_rows_decode_mut(ua_ctx *c, const ua_pack *const *packs, uint64_t n_rows,
                                  const uint64_t *mut_uids, const uint8_t *mut_ops,
                                  const uint64_t *row_mut_base, const uint64_t *after,
                                  const int32_t *first, uint64_t *out_vals, uint64_t cap_vals,
                                  uint64_t *out_row_offs, uint64_t *out_total) {
    if (!c || !out_total || !out_row_offs) return UA_ERR_INVALID;
    if (n_rows && !packs) return UA_ERR_INVALID;
    if (cap_vals && !out_vals) return UA_ERR_INVALID;
    const u64 n_mut = (row_mut_base && n_rows) ? row_mut_base[n_rows] : 0;
    if (n_mut == 0)
        return ua_rows_decode(c, packs, n_rows, after, first, out_vals, cap_vals,
                              out_row_offs, out_total);
    if (!mut_uids || !mut_ops || n_mut > UINT32_MAX) return UA_ERR_INVALID;
    UaHostArena a;
    int rc;
    if ((rc = rows_flatten(packs, n_rows, n_mut, a))) return rc;

    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_PACK/WS_HOUT reuse */
    HIP_TRY(hipSetDevice(c->device));
    UaHostIn h_rmb = {row_mut_base, (n_rows + 1) * 8, 8, nullptr},
             h_muids = {mut_uids, n_mut * 8, 8, nullptr}, h_mops = {mut_ops, n_mut, 1, nullptr},
             h_after = {after, n_rows * 8, 8, nullptr}, h_first = {first, n_rows * 4, 4, nullptr};
    ua_drowpacks p;
    if ((rc = rows_upload(c, a, n_rows, out_vals != nullptr, cap_vals,
                          {&h_rmb, &h_muids, &h_mops, &h_after, &h_first}, p)))
        return rc;
    ua_drowmut d = {p.bases, p.num_uids, p.delta_offs, p.deltas, p.n_blocks, p.row_block_base,
                    n_rows, (const u64 *)h_after.dev, (const int32_t *)h_first.dev,
                    (const u64 *)h_muids.dev, (const u8 *)h_mops.dev, (const u64 *)h_rmb.dev,
                    n_mut, p.out_vals, cap_vals, p.out_row_offs};
    u64 total = 0;
    rc = ua_rows_decode_mut_dev(c, &d, &total);
    *out_total = total;
    return rows_download(c, p, rc, total, out_vals, out_row_offs);
}

/* host-pointer form of ua_rows_intersect_packed_dev: the UidMatrix of a
 * per-key fan-out with opts.Intersect != nil (posting/list.go:1823-1829, one
 * algo.IntersectCompressedWith per key, all against q.UidList) from host
 * packs; a null packs[r] is an empty row. */
extern "C" int ua_rows_intersect_packed(ua_ctx *c, const ua_pack *const *packs,
                                        uint64_t n_rows, const uint64_t *after,
                                        const uint64_t *shared, uint64_t m,
                                        uint64_t *out_vals, uint64_t cap_vals,
                                        uint64_t *out_row_offs, uint64_t *out_total) {
    if (!c || !out_total || !out_row_offs) return UA_ERR_INVALID;
    if (n_rows && !packs) return UA_ERR_INVALID;
    if (m && !shared) return UA_ERR_INVALID;
    if (cap_vals && !out_vals) return UA_ERR_INVALID;
    if (m > (UINT64_MAX >> 3)) return UA_ERR_INVALID;
    UaHostArena a;
    int rc;
    if ((rc = rows_flatten(packs, n_rows, 0, a))) return rc;

    std::lock_guard<std::recursive_mutex> gop(c->mu); /* whole-op: WS_PACK/WS_HOUT reuse */
    HIP_TRY(hipSetDevice(c->device));
    UaHostIn h_after = {after, n_rows * 8, 8, nullptr}, h_shared = {shared, m * 8, 8, nullptr};
    ua_drowpacks p;
    if ((rc = rows_upload(c, a, n_rows, out_vals != nullptr, cap_vals, {&h_after, &h_shared}, p)))
        return rc;
    ua_drowisect d = {p.bases, p.num_uids, p.delta_offs, p.deltas, p.n_blocks,
                      p.row_block_base, n_rows, (const u64 *)h_after.dev, nullptr,
                      (const u64 *)h_shared.dev, m, p.out_vals, cap_vals, p.out_row_offs};
    u64 total = 0;
    rc = ua_rows_intersect_packed_dev(c, &d, &total);
    *out_total = total;
    return rows_download(c, p, rc, total, out_vals, out_row_offs);
}

