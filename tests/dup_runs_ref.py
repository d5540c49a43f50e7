"""Inputs WITH duplicates: case builders and a host model of the union walk (a
helper, not a test).  The half of the contract these cases pin:

  - MergeSorted collapses all duplicates, those inside one list included
    (uidlist.go:417; TestMergeSorted6/9/10): union = np.unique(concat);
  - the keep-all merge (ua_merge_all_batch_dev) and the segmented sort
    (ua_sort_segments_dev) keep them: np.sort(concat);
  - IndexOf is sort.Search, the FIRST index of a run (uidlist.go:546).

A list is written as runs [(value, count), ...], non-decreasing.  Every list
has at most about 8 200 elements (four 2048-element tiles); the k-way cases use
at most 33 lists of 5 000 (the IntersectSorted fold takes the random lists of
test_parity_gpu.py::test_kway_vs_oracle, at most 20 300 each).

model_union restates how k_tiles<OP_UNION> decides what to emit: the merge path
with A (u) first on ties, cut into 2048-element tiles and 8-element thread
segments, each segment seeded as tile_walk2 seeds it.  One ablation at a time
breaks the seed the way a plausible kernel bug would; test_dup_runs_ref.py
holds that every ablation changes the output of a named case, which is the
evidence that the GPU cases can fail.
"""
import functools

import numpy as np

from dgraph_amd import synth

TILE = 2048  # UA_TILE: merge-path elements per tile
WPT = 8      # UA_WPT: path elements per thread
U64_MAX = 2**64 - 1
X = 1_000_000          # the repeated value of most cases
RUN_START = 39         # run_u_L*: 39 = 7 mod 8, so even L = 2 straddles a thread edge
RUN_LENS = (2, 8, 9, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
BOTH_COPIES = ((1, 2048), (2048, 1), (2048, 2048), (1000, 3000), (3000, 1000))
BEFORES = (TILE - 1, TILE, TILE + 1)
PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))
SEED = synth.SEED + 417


def arr(x):
    return np.asarray(x, dtype=np.uint64)


def runs(spec):
    """[(value, count), ...] -> the uint64 list it spells."""
    vals = [int(v) for v, _ in spec]
    assert all(a <= b for a, b in zip(vals, vals[1:])), "runs must be non-decreasing"
    assert all(0 <= v <= U64_MAX for v in vals) and all(c >= 0 for _, c in spec)
    return np.repeat(arr(vals), np.asarray([c for _, c in spec], dtype=np.int64))


def distinct(lo, n, step=3):
    """n single-element runs lo, lo + step, ..."""
    return [(lo + step * i, 1) for i in range(n)]


# ---- expected values ----

def want_union(*lists):
    return np.unique(np.concatenate([arr([])] + [arr(x) for x in lists]))


def want_all(*lists):
    return np.sort(np.concatenate([arr([])] + [arr(x) for x in lists]))


def want_index_of(u, q):
    """sort.Search: the first index of q in u, -1 when absent."""
    u, q = arr(u), arr(q)
    if u.size == 0:
        return np.full(q.size, -1, dtype=np.int64)
    pos = np.searchsorted(u, q, "left")
    hit = (pos < u.size) & (u[np.minimum(pos, u.size - 1)] == q)
    return np.where(hit, pos, -1).astype(np.int64)


def want_fold(lists):
    return functools.reduce(np.intersect1d, [arr(x) for x in lists])


# ---- the merge path and its tiles ----

def merge_path(u, v):
    """(merged, from_a): the path's values and which come from u, A first on
    ties (d_merge_path_tile / k_partition: A[mid] <= B[diag - 1 - mid])."""
    cat = np.concatenate([arr(u), arr(v)])
    order = np.argsort(cat, kind="stable")
    return cat[order], order < len(u)


def tile_geometry(u, v):
    """Per tile (a0, alen, b0, blen), as d_tile_geom derives them."""
    _, from_a = merge_path(u, v)
    ca = np.concatenate([[0], np.cumsum(from_a)])
    path = from_a.size
    out = []
    for d0 in range(0, path, TILE):
        d1 = min(d0 + TILE, path)
        a0, a1 = int(ca[d0]), int(ca[d1])
        out.append((a0, a1 - a0, d0 - a0, (d1 - a1) - (d0 - a0)))
    return out


def run_span(u, v, x):
    """First and last path position holding x."""
    merged, _ = merge_path(u, v)
    pos = np.flatnonzero(merged == np.uint64(x))
    return int(pos[0]), int(pos[-1])


# ---- host model of the union walk ----

ABLATIONS = {
    0: "none: the walk as k_tiles<OP_UNION> does it",
    1: "ignore a_before: a range head (i == 0) has no previous A",
    2: "ignore b_before: a range head (j == 0) has no previous B",
    3: "min instead of max of the two previous values",
    4: "no seed at a thread head inside a tile",
    5: "prev_out == 0 read as 'no previous'",
}


def model_union(u, v, ablation=0):
    """What the union tiles emit, tile by tile and thread by thread.  A
    thread's segment [s0, s1) starts with i A-elements and j B-elements of the
    tile consumed; its previous value is max(last A before, last B before),
    the tile's a_before / b_before standing in at a range head, and there is
    no previous value only at the very head of the pair."""
    u, v = arr(u), arr(v)
    merged, from_a = merge_path(u, v)
    ca = np.concatenate([[0], np.cumsum(from_a)]).tolist()
    ul, vl, ml = u.tolist(), v.tolist(), merged.tolist()
    path = len(ml)
    out = []
    for d0 in range(0, path, TILE):
        d1 = min(d0 + TILE, path)
        a0 = ca[d0]
        b0 = d0 - a0
        has_ab, has_bb = a0 > 0, b0 > 0
        a_before = ul[a0 - 1] if has_ab else 0
        b_before = vl[b0 - 1] if has_bb else 0
        for s0 in range(d0, d1, WPT):
            s1 = min(s0 + WPT, d1)
            i = ca[s0] - a0
            j = (s0 - d0) - i
            pa = ul[a0 + i - 1] if i > 0 else a_before
            hpa = i > 0 or has_ab
            pb = vl[b0 + j - 1] if j > 0 else b_before
            hpb = j > 0 or has_bb
            if ablation == 1 and i == 0:
                hpa = False
            if ablation == 2 and j == 0:
                hpb = False
            has_prev = hpa or hpb
            if not hpa:
                prev = pb
            elif not hpb:
                prev = pa
            else:
                prev = min(pa, pb) if ablation == 3 else max(pa, pb)
            if ablation == 4 and s0 > d0:
                has_prev = False
            for p in range(s0, s1):
                val = ml[p]
                if ablation == 5:
                    has_prev = prev != 0
                if not has_prev or val != prev:
                    out.append(val)
                prev = val
                has_prev = True
    return arr(out)


# ---- union cases ----

class Case:
    """One (u, v) pair; pu / pv: the u64 parity of the device slices."""

    def __init__(self, name, u, v, pu=0, pv=0):
        self.name, self.u, self.v, self.pu, self.pv = name, arr(u), arr(v), pu, pv
        for a in (self.u, self.v):
            assert a.size < 2 or np.all(a[1:] >= a[:-1]), name
        assert max(self.u.size, self.v.size) <= 4 * TILE + 8, name
        self.want = {"merge": want_union(self.u, self.v),
                     "merge_all": want_all(self.u, self.v)}

    def mirrored(self):
        return Case(self.name + "_mirror", self.v, self.u, self.pv, self.pu)

    def sliced(self, pu, pv):
        return Case(f"{self.name}_p{pu}{pv}", self.u, self.v, pu, pv)


def first_above(src, floor, avoid):
    for x in src:
        if x > floor and x not in avoid:
            return int(x)
    return None


def guarded(own, other, parity):
    """Host array [guards | own | guards] and the offset of `own` in it, as in
    test_tile_prologue_gpu.py.  Before: own[0] again.  After: a value the other
    list has and own lacks, above own's last, else the other list's last."""
    own_set = set(own.tolist())
    before = int(own[0]) if own.size else (int(other[0]) if other.size else 7)
    floor = int(own[-1]) if own.size else -1
    after = first_above(other.tolist(), floor, own_set)
    if after is None:
        after = int(other[-1]) if other.size else before
    off = 2 - parity  # even offset -> 16B aligned slice, odd -> not
    big = np.concatenate([arr([before] * off), own, arr([after] * 2)])
    return big, off


def run_u_case(L):
    """One run of X in u only, at path positions [RUN_START, RUN_START + L);
    v is distinct and lacks X; distinct values on both sides of the run."""
    u = runs(distinct(1, 20) + [(X, L)] + distinct(X + 1, 30))
    v = runs(distinct(2, 19) + distinct(X + 2, 40))
    return Case(f"run_u_L{L}", u, v)


def both_case(a, b, before):
    """X a times in u and b times in v, behind `before` distinct values: the
    run covers path positions [before, before + a + b), u's copies first."""
    nu = before // 2
    u = runs(distinct(1, nu) + [(X, a)] + distinct(X + 1, 20))
    v = runs(distinct(2, before - nu) + [(X, b)] + distinct(X + 2, 25))
    return Case(f"both_a{a}_b{b}_before{before}", u, v)


def all_b_case(nlow, name):
    """u = nlow distinct values and X, v = X x 3000: behind u's X every tile is
    all-B, with alen == 0 and has_ab; v has no value below X."""
    return Case(name, runs(distinct(1, nlow) + [(X, 1)]), runs([(X, 3000)]))


def build_union_cases():
    base = [run_u_case(L) for L in RUN_LENS]
    sliced = [both_case(a, b, before) for a, b in BOTH_COPIES for before in BEFORES]
    # tile 1 starts right behind u's X and has no B before it: a_before alone
    # keeps v's first X out (b_before in the mirrored case)
    sliced.append(all_b_case(TILE - 1, "allB_after_ua"))
    sliced.append(all_b_case(100, "allB_after_ua_short"))
    base += sliced
    # has_prev == false with prev_out == 0: only at the very head
    base.append(Case("zero_head_u", runs([(0, 20)] + distinct(5, 60)), runs(distinct(7, 50))))
    base.append(Case("zero_head_both", runs([(0, TILE + 52)] + distinct(5, 60)),
                     runs([(0, 10)] + distinct(7, 50))))
    # UINT64_MAX: the last partial tile is nothing but the run (it begins on
    # the tile edge / 48 elements before it)
    for nlow, name in ((1024, "max_tail_fill"), (1000, "max_tail_over")):
        base.append(Case(name, runs(distinct(1, nlow) + [(U64_MAX, 600)]),
                         runs(distinct(2, nlow) + [(U64_MAX, 400)])))
    base.append(Case("sign_edge",
                     runs(distinct(1, 30) + [(2**63 - 1, 1500), (2**63, 1500), (2**63 + 1, 1)]),
                     runs([(2**63 - 1, 700), (2**63, 900)] + distinct(2**63 + 5, 33))))
    for n, m in ((1, 1), (5000, 0), (0, 5000), (5000, 5000)):
        base.append(Case(f"equal_n{n}_m{m}", runs([(X, n)]), runs([(X, m)])))
    # three tiles of doubles and triples: u holds i two or three times, v holds
    # every other value three or two times
    base.append(Case("doubles_triples",
                     runs([(10 + i, 2 + i % 2) for i in range(1230)]),
                     runs([(10 + 2 * i, 3 - i % 2) for i in range(1230)])))
    cases = []
    for c in base:
        cases += [c, c.mirrored()]
    for c in sliced:
        for pu, pv in PARITIES[1:]:
            s = c.sliced(pu, pv)
            cases += [s, s.mirrored()]
    return cases


UNION_CASES = build_union_cases()
UNION_BY_NAME = {c.name: c for c in UNION_CASES}
assert len(UNION_BY_NAME) == len(UNION_CASES)
# the distinct (u, v) contents: the parity variants repeat their base case
UNION_CONTENT_CASES = [c for c in UNION_CASES if (c.pu, c.pv) == (0, 0)]


# ---- k-way union tree: heavy duplicates, so lengths collapse after round 0 ----

TREE_KS = (2, 3, 5, 9, 33)
TREE_N = 5000


def _draw(rng, pool, n):
    """n sorted draws from pool, every pool value present."""
    pool = arr(pool)
    assert n >= pool.size
    extra = rng.choice(pool, size=n - pool.size)
    return np.sort(np.concatenate([pool, extra]))


@functools.lru_cache(maxsize=None)
def tree_cases():
    """name -> list of lists.  three: every list drawn from {3, 2^40,
    UINT64_MAX}.  ragged: list i holds i + 1 distinct values, so round-0
    lengths differ.  gaps: ragged with every odd list empty."""
    rng = np.random.default_rng(SEED)
    pool = [3, 2**40, U64_MAX] + [2**40 + 17 * i for i in range(1, 31)]
    assert len(pool) == max(TREE_KS)
    out = {}
    for k in TREE_KS:
        out[f"three_k{k}"] = [_draw(rng, pool[:3], TREE_N) for _ in range(k)]
        ragged = [_draw(rng, sorted(pool[:i + 1]), TREE_N) for i in range(k)]
        out[f"ragged_k{k}"] = ragged
        out[f"gaps_k{k}"] = [arr([]) if i % 2 else x for i, x in enumerate(ragged)]
    return out


# ---- segmented sort ----

SORT_NS = (2047, 2048, 2049, 4097, 3 * 2048, 5 * 2048 + 1)  # 0, 0, 1, 2, 2, 3 merge rounds
SORT_VALUES = (U64_MAX, 2**63, 5)  # UINT64_MAX is also the chunk padding


def sort_rounds(n):
    r, w = 0, 1
    while w < (n + 2047) // 2048:
        w, r = w * 2, r + 1
    return r


@functools.lru_cache(maxsize=None)
def sort_segments():
    """(n, d) -> unsorted segment of n draws from d distinct values."""
    rng = np.random.default_rng(SEED + 1)
    return {(n, d): rng.choice(arr(SORT_VALUES[:d]), size=n) for n in SORT_NS for d in (1, 2, 3)}


@functools.lru_cache(maxsize=None)
def packed_segments():
    """The words sortpath.sort_without_index sorts: key << 32 | pos, keys at or
    above 2^31, ascending and with the descending flip 0xFFFFFFFF - key."""
    rng = np.random.default_rng(SEED + 2)
    keys = arr([2**31, 2**31 + 1, 2**32 - 1, 2**32 - 2, 3 * 2**30])
    out = []
    for n, desc in ((3000, False), (5000, True), (2500, True), (4097, False)):
        k = rng.choice(keys, size=n)
        if desc:
            k = np.uint64(0xFFFFFFFF) - k
        out.append((k << np.uint64(32)) | np.arange(n, dtype=np.uint64))
    return out


# ---- IndexOf ----

INDEX_NQ = (0, 1, 255, 256, 257)


def _fit(q, nq):
    q = arr(q)
    return np.resize(q, nq) if q.size else np.zeros(nq, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def index_cases():
    """[(name, u, q)]: u with duplicate runs on both sides of 2^63; n in
    {0, 1, 2}; nq on both sides of a 256-thread block.  Queries: every value
    of u and its two neighbours, 0, UINT64_MAX, u[0] - 1 and u[-1] + 1."""
    dup = runs([(5, 3), (9, 1), (2**40, 700), (2**63 - 1, 4), (2**63, 2000), (2**63 + 7, 1),
                (U64_MAX - 1, 300)])
    top = runs([(0, 2), (1, 1), (U64_MAX, 5)])
    out = []
    for uname, u in (("dup", dup), ("top", top), ("n0", arr([])), ("n1", arr([7])),
                     ("n1_max", arr([U64_MAX])), ("n2_same", arr([7, 7])),
                     ("n2", arr([0, U64_MAX]))):
        q = {0, U64_MAX, 2**63 - 2, 2**63 - 1, 2**63, 2**63 + 1}
        for x in set(u.tolist()):
            q |= {x, max(x - 1, 0), min(x + 1, U64_MAX)}
        q = arr(sorted(q))
        np.random.default_rng(SEED + 3).shuffle(q)
        for nq in INDEX_NQ:
            out.append((f"{uname}_nq{nq}", u, _fit(q, nq)))
    return out


# ---- IntersectSorted fold with a non-empty result ----

def _random_lists(seed, k):
    """The lists of test_parity_gpu.py::test_kway_vs_oracle."""
    rng = np.random.default_rng(seed)
    return [synth.gen_sorted_unique(rng, int(rng.integers(0, 20_000)), 60_000)
            for _ in range(k)]


def _chunks_fold(nchunks, extra_long):
    """Lists B - C_j over a partition C_1..C_nchunks of B (equal lengths, so
    the fold takes them in order and loses one chunk per round after the
    first, which loses two), then extra_long longer lists holding all of B."""
    base = arr(np.arange(3000) * 7 + 11)
    chunks = np.array_split(base, nchunks)
    lists = [np.setdiff1d(base, c) for c in chunks]
    lists += [np.union1d(base, arr([5 + i, 2**63 + i])) for i in range(extra_long)]
    return lists


@functools.lru_cache(maxsize=None)
def fold_cases():
    """name -> list of lists."""
    rng = np.random.default_rng(SEED + 4)
    planted = np.unique(np.concatenate([arr([0, U64_MAX]),
                                        arr(rng.choice(2**40, size=298, replace=False))]))
    assert planted.size == 300
    out = {}
    for k in (9, 150):
        out[f"planted_k{k}"] = [np.union1d(x, planted) for x in _random_lists(SEED + k, k)]
    # one common value: 8 equal-length lists B - C_j plus {c}, then the longer B plus {c}
    c = arr([2**63])
    out["to_one_k9"] = [np.union1d(x, c) for x in _chunks_fold(8, 1)]
    # 10 lists, 9 rounds: six lists B - C_j empty the fold at round 5
    out["empties_at_round5_k10"] = _chunks_fold(6, 4)
    # equal lengths: the fold must keep the given order (stable sort)
    pool = np.setdiff1d(arr(np.arange(20_000)), planted)
    out["equal_len_k9"] = [np.union1d(planted[:200], arr(rng.choice(pool, 2800, replace=False)))
                           for _ in range(9)]
    return out
