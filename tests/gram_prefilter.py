"""Inputs, rule and CPU models of the Gram-tile prefilter tests (test_gram_prefilter_inputs.py on the CPU, test_gpu_gram_prefilter.py
on the device).

relative_neighbor_pruning<METRIC, MFMA = true> (csrc/dk_heuristic.h) settles `dist(s, c) < c.Dist` from a 32 x 32 tile
of v_mfma_f32_32x32x2_f32 dot products whenever the approximate margin exceeds E = (1.125 K + 32) 2^-24 (sq_euclid: Esq (n_i + n_j),
Esq = (2.25 K + 32) 2^-24 * 1.01); everything else goes back to the exact kernels.  I.i.d. uniform rows keep the two sums 25 to 50
times closer than E, so they cannot tell a right margin from a wrong one; the row families below are built to round in one
direction, to tie bit for bit, to fill several tiles of accepted ids, or to sit at the guards of the tile code.  `chain_dot` models
the tile's arithmetic, `prune_trace` restates the heuristic on the oracle's distances and reports every comparison the tiles can
be asked -- the CPU tier checks with them that each family does what the GPU tier relies on."""
import numpy as np

import oracle
import wide_beams as wb
from common import normalize_f32, uniform

U = 2.0 ** -24
HEADS = (0.3, 0.7)
COS_SCALES = (1e-14, 1.0, 3.0, 1e15)
LONG_LENGTHS = (1.0002, 1.5, 3.0)


def prefilter_applies(metric, dim, beam):
    """The rule of relative_neighbor_pruning's tile form: f32 row kinds, dim % 8 == 0, dim >= 256, and a beam kept in eight register
    sets (the form is instantiated for NS == 8 only)."""
    return metric in ("sq_euclid", "cosine", "ucosine") and dim % 8 == 0 and dim >= 256 and wb.sets_for(beam) == 8


def margin_E(dim):
    return np.float32((np.float32(1.125) * np.float32(dim) + np.float32(32.0)) * np.float32(5.9604645e-8))


def margin_Esq(dim):
    return np.float32((np.float32(2.25) * np.float32(dim) + np.float32(32.0)) * np.float32(5.9604645e-8) * np.float32(1.01))


# ---- row families (fixed seeds, float32) -----------------------------------------------------------------------------------------
def _unit_biased(n, dim, head, seed, amp):
    """Unit rows that are constant but for element 0 (= head after normalising) and 4 .. 16 positions moved by a factor 1 + amp * N(0, 1):
    the running sum of a dot product of two such rows sits in one binade for most of its K steps and every step adds nearly the
    same product, so a sequential chain rounds the same way again and again."""
    rng = np.random.default_rng(seed)
    c = np.sqrt((1.0 - head * head) / (dim - 1))
    x = np.full((n, dim), c, dtype=np.float64)
    x[:, 0] = head
    for i in range(n):
        pos = 1 + rng.choice(dim - 1, int(rng.integers(4, 17)), replace=False)
        x[i, pos] *= 1.0 + amp * rng.standard_normal(pos.size)
    return normalize_f32(x.astype(np.float32))


BIASED_AMP = 0.1


def biased(dim, head, metric="ucosine", n=2000, seed=401):
    """ucosine / sq_euclid: the unit rows.  cosine: the same rows times a per-row scale from COS_SCALES (norm products from 1e-28,
    just above the 1e-30 guard, to 1e30), and every 97th row all zero (norm product 0: the guard itself)."""
    x = _unit_biased(n, dim, head, seed, BIASED_AMP)
    if metric == "cosine":
        rng = np.random.default_rng(seed + 1)
        x = (x * np.asarray(COS_SCALES, dtype=np.float32)[rng.integers(0, len(COS_SCALES), n)][:, None]).astype(np.float32)
        x[5::97] = 0.0
    return x


def offset_cluster(dim, n=2000, seed=411):
    """sq_euclid far from the origin: 100 + 0.01 noise.  Squared norms about 2.6e6 at dim 256 and distances about 0.05, so
    Esq (n_i + n_j) -- about 190 -- swamps every distance and every comparison is uncertain."""
    return (np.float32(100.0) + np.float32(0.01) * np.random.default_rng(seed).standard_normal((n, dim), dtype=np.float32)).astype(np.float32)


OVERFLOW_ROWS = 6


def overflow(dim, n=2000, seed=421):
    """Uniform rows; six of them times 1e18 (squared norm about 8e37 at dim 256: finite, the top of the range) and six times 1e19
    (squared norm inf in float32: the tile's n_i + n_j - 2 dot is inf - inf = NaN, which must count as uncertain)."""
    x = uniform(n, dim, seed)
    pick = np.random.default_rng(seed + 1).choice(n, 2 * OVERFLOW_ROWS, replace=False)
    x[pick[:OVERFLOW_ROWS]] *= np.float32(1e18)
    x[pick[OVERFLOW_ROWS:]] *= np.float32(1e19)
    return x


def _shape(metric, x):
    return normalize_f32(x) if metric == "ucosine" else x


def near_duplicates(dim, metric="ucosine", n=2000, seed=431):
    """Uniform rows (unit length under ucosine); 10 % are bit-copies of other rows and a further 10 % copies with one element moved
    by one ulp up or down.  A copy of an accepted row makes dist(s, c) == c.Dist bit for bit."""
    x = _shape(metric, uniform(n, dim, seed))
    rng = np.random.default_rng(seed + 1)
    pick = rng.permutation(n)
    k = n // 10
    src, dup, near = pick[:k * 2], pick[2 * k:3 * k], pick[3 * k:4 * k]
    x[dup] = x[src[:k]]
    x[near] = x[src[k:]]
    col = rng.integers(0, dim, k)
    x[near, col] = np.nextafter(x[near, col], np.where(rng.integers(0, 2, k) == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    return x


def grid(dim, metric="sq_euclid", n=2000, seed=441):
    """Integer rows, values 0 .. 3: every sum is exact in either order, so equal distances are everywhere (raw rows for sq_euclid and
    cosine; ucosine measures the same raw rows, which are far longer than 1: its blocks take the long-row route)."""
    return np.random.default_rng(seed).integers(0, 4, (n, dim)).astype(np.float32)


def mixed_length(dim, n=2000, seed=451):
    """Unit rows of which 5 % have length 1.0002, 1.5 or 3 (ucosine): a block of 32 candidates that holds one of them goes to the
    exact kernels as a whole, its neighbours of unit rows take the tiles.  The rows are Gaussian, not uniform: in the positive
    orthant a row of length 3 is nearer to every row than any unit row is (1 - 3 cos), heads every list and turns every later
    candidate away; around the origin it is near to some rows and far from others, and lists run to MaxEdges."""
    rng = np.random.default_rng(seed)
    x = normalize_f32(rng.standard_normal((n, dim)).astype(np.float32))
    rng = np.random.default_rng(seed + 1)
    pick = rng.choice(n, n // 20, replace=False)
    x[pick] *= np.asarray(LONG_LENGTHS, dtype=np.float32)[rng.integers(0, len(LONG_LENGTHS), pick.size)][:, None]
    return x


def long_rows(x):
    """Which rows the tile code sends to the exact path: Gram diagonal above 1.0001."""
    return (x.astype(np.float64) ** 2).sum(axis=1) > 1.0001


N_BASIS = 768


def many_accepted(dim=768, n=1200, seed=461):
    """Accepted lists past one, two and three tiles.  I.i.d. near-orthogonal rows do not give them: every pair is about 1 apart, a
    candidate's own distance is below that only by its rank among the row's neighbours, and at efc 512 of 1 200 rows the lists end
    near 32 ids.  So: `dim` orthonormal rows (a random rotation of the basis; any two at distance 1 up to rounding) and n - dim HUB
    rows, the basis' centre plus 0.3 / sqrt(dim) noise per element.  A hub is 0.96 from every basis row, closer than they are to
    each other, so a hub's basis candidates are turned away only by the hubs accepted before them -- about half of them per hub.
    The first n - 200 rows are shuffled; the last 200 are hubs (the rows the CPU tier samples)."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((dim, dim)))
    hubs = q.sum(axis=0)[None] / np.sqrt(dim) + 0.3 * rng.standard_normal((n - dim, dim)) / np.sqrt(dim)
    x = normalize_f32(np.concatenate([q, hubs]).astype(np.float32))
    x[:n - 200] = x[rng.permutation(n - 200)]
    return x


def plain(dim, metric="ucosine", n=1000, seed=471):
    return _shape(wb.base_metric(metric), uniform(n, dim, seed))


NAN_ROWS = (150, 480, 811)


def nan_rows(dim, n=1000, seed=491):
    """Uniform unit rows of which three hold one NaN element: every distance to them is NaN, no comparison with a NaN holds, and the
    oracle's build takes them as they are (they are never turned away and never turn anything away).  On the device the Gram
    diagonal of such a row is NaN (not <= 1.0001: the long-row route) and every tile entry with it is NaN (uncertain)."""
    x = normalize_f32(uniform(n, dim, seed))
    x[list(NAN_ROWS), [3, 100, dim - 1]] = np.nan
    return x


def queries(x, nq=100, seed=499):
    """nq rows of the family itself, each element moved by a factor 1 + 0.01 N(0, 1) (zero rows stay zero, scales stay what they are)."""
    rng = np.random.default_rng(seed)
    pick = rng.choice(np.flatnonzero(~np.isnan(x).any(axis=1)), nq, replace=False)
    f = (1.0 + 0.01 * rng.standard_normal((nq, x.shape[1]))).astype(np.float32)
    with np.errstate(over="ignore"):
        return (x[pick] * f).astype(np.float32)


# ---- models ----------------------------------------------------------------------------------------------------------------------
def chain_dot(a, b):
    """The sequential fp32 FMA chain acc <- fl32(acc + a_k b_k), k = 0 .. K - 1, over the last axis, for every row of `a` against every
    row of `b`: [na, K] x [nb, K] -> [na, nb] float32.  Each step goes through float64 (the product of two float32 is exact there;
    the sum is rounded to 53 and then to 24 bits, which differs from one fused rounding only in rare double-rounding cases).  It
    models the MAGNITUDE of the MFMA's error against the lane-ordered sums, not its bits: the matrix core's internal order is its own."""
    a64, b64 = np.asarray(a, dtype=np.float32).astype(np.float64), np.asarray(b, dtype=np.float32).astype(np.float64)
    acc = np.zeros((a64.shape[0], b64.shape[0]), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(a64.shape[1]):
            acc = (acc + np.multiply.outer(a64[:, k], b64[:, k])).astype(np.float32)
    return acc


def chain_norm(x):
    """The Gram diagonal of chain_dot, per row."""
    x64 = np.asarray(x, dtype=np.float32).astype(np.float64)
    acc = np.zeros(x64.shape[0], dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(x64.shape[1]):
            acc = (acc + x64[:, k] * x64[:, k]).astype(np.float32)
    return acc


def lane_norm(x):
    """Squared norms in the order of the distance kernels (eight partial sums, multiply then add, the cosine tree): what row_sn holds
    the double square root of."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        p = np.zeros((x.shape[0], 8), dtype=np.float32)
        full = x.shape[1] & ~7
        for k in range(0, full, 8):
            p = p + x[:, k:k + 8] * x[:, k:k + 8]
        u = p[:, :4] + p[:, 4:]
        s = (u[:, 0] + u[:, 2]) + (u[:, 1] + u[:, 3])
        for k in range(full, x.shape[1]):
            s = s + x[:, k] * x[:, k]
    return s


def tile_distance(metric, rows, acc_ids, cand_ids):
    """What the tile code makes of chain_dot for (accepted x candidate): (d, scale) float32 [na, nc]; the margin of a pair is
    E * scale (ucosine, cosine: scale 1) or Esq * scale (sq_euclid: n_i + n_j off the chain's own diagonal)."""
    A, B = rows[acc_ids], rows[cand_ids]
    S = chain_dot(A, B)
    one = np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if metric == "ucosine":
            return one - S, np.ones_like(S)
        if metric == "sq_euclid":
            na, nb = chain_norm(A), chain_norm(B)
            nn = na[:, None] + nb[None, :]
            return nn - np.float32(2.0) * S, nn
        sa, sb = np.sqrt(lane_norm(A).astype(np.float64)), np.sqrt(lane_norm(B).astype(np.float64))
        denom = (sa[:, None] * sb[None, :]).astype(np.float32)
        d = np.where(denom < np.float32(1e-30), one, one - S / np.where(denom == 0, one, denom))
        return d.astype(np.float32), np.ones_like(S)


class Trace:
    """One heuristic call: `accepted` ids in order; per comparison (an accepted id against a later candidate, as the tiles see it: ALL
    ids accepted before the candidate, no early break) d_exact, thr, d_chain, scale; `n` candidates, `sorted_d` their distances."""
    __slots__ = ("accepted", "d_exact", "thr", "d_chain", "scale", "n", "sorted_ids", "sorted_d", "max_edges", "decided")


def prune_trace(ref, metric, rows, cands, max_edges, chain=True):
    """Heuristic.RelativeNeighborPruning (Heuristic.cs:11-46) restated on the oracle's own distances: `cands` = (ids, dists) in the heap
    order OracleIndex.search_layer returns.  Fewer than max_edges candidates: the ids as they come (:13-18).  Otherwise the BCL
    sort (oracle.dotnet_sort), then the greedy pass: a candidate is accepted unless some id accepted before it is closer to it
    than the inserted row is, dist(s, c) < c.Dist (oracle.dist_pairs)."""
    ids, dists = np.asarray(cands[0], dtype=np.int32), np.asarray(cands[1], dtype=np.float32)
    t = Trace()
    t.n, t.max_edges = ids.size, max_edges
    empty = np.zeros(0, dtype=np.float32)
    t.d_exact = t.thr = t.d_chain = t.scale = empty
    if ids.size < max_edges:
        t.accepted, t.sorted_ids, t.sorted_d, t.decided = ids.copy(), ids, dists, 0
        return t
    ids, dists = oracle.dotnet_sort(ids, dists)
    t.sorted_ids, t.sorted_d = ids, dists
    acc, when, de, th, pa, pc = [], [], [], [], [], []
    decided = 0
    for j in range(ids.size):
        if len(acc) >= max_edges:
            break
        decided += 1
        if acc:
            d = oracle.dist_pairs(metric, rows, np.asarray(acc, dtype=np.int32), np.full(len(acc), ids[j], dtype=np.int32))
            de.append(d); th.append(np.full(len(acc), dists[j], dtype=np.float32))
            pa.append(np.arange(len(acc))); pc.append(np.full(len(acc), j))
            if (d < dists[j]).any():
                continue
        acc.append(int(ids[j]))
    t.accepted, t.decided = np.asarray(acc, dtype=np.int32), decided
    if de:
        t.d_exact, t.thr = np.concatenate(de), np.concatenate(th)
        if chain:
            d, s = tile_distance(metric, rows, t.accepted, ids[:decided])
            pa, pc = np.concatenate(pa), np.concatenate(pc)
            t.d_chain, t.scale = d[pa, pc], s[pa, pc]
    return t


def margin(metric, dim):
    return margin_Esq(dim) if metric == "sq_euclid" else margin_E(dim)


def wrong_and_inside(metric, dim, t, divide=1.0):
    """(comparisons a prefilter with margin / divide (0: no margin) decides differently from the exact test, comparisons it leaves to
    the exact test) of a Trace: the tile code's own three-way test, in float32."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = (np.float32(0.0) if divide == 0 else np.float32(margin(metric, dim) / np.float32(divide))) * t.scale
        lo, hi = (t.thr - e).astype(np.float32), (t.thr + e).astype(np.float32)
        closer, farther = t.d_chain < lo, t.d_chain > hi
    exact = t.d_exact < t.thr
    return int((closer & ~exact).sum() + (farther & exact).sum()), int((~closer & ~farther).sum())


def insert_traces(ref, metric, rows, i, M, efc, chain=True):
    """The heuristic calls of HNSWIndex.Add(rows[i]) on the oracle index `ref` as it stands (rows 0 .. i - 1 linked): FindEntryPoint,
    then per layer SearchLayer -> RelativeNeighborPruning, the next entry being the first id selected (GraphConnector.cs:172-216).
    -> {layer: Trace}.  `level` comes from the index's own generator."""
    level = int(oracle.random_levels(31337, 1.0 / np.log(16), i + 1)[i])
    top = ref.max_layer(ref.entry_point)
    best = ref.find_entry_point(level, rows[i])
    out = {}
    for layer in range(min(level, top), -1, -1):
        cands = ref.search_layer(best, layer, efc, rows[i])
        out[layer] = prune_trace(ref, metric, rows, cands, 2 * M if layer == 0 else M, chain)
        best = int(out[layer].accepted[0])
    return out


# ---- the cases both tiers run ------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, metric, dim, M, efc, make, n=2000, schedules=("batch",), group="tight"):
        self.family, self.metric, self.dim, self.M, self.efc, self.make, self.n, self.schedules, self.group = family, metric, dim, M, efc, make, n, schedules, group
        self.id = f"{family}-{metric}-{dim}-M{M}-efc{efc}"
        self._rows = None

    def rows(self):
        if self._rows is None:
            self._rows = np.ascontiguousarray(self.make()[:self.n], dtype=np.float32)
            self._rows.setflags(write=False)
            assert self._rows.shape == (self.n, self.dim)
        return self._rows

    def eligible(self):
        return prefilter_applies(self.metric, self.dim, self.efc)


BATCH = 700           # Add's snapshot cap of the batched builds
TIE_SCHEDULES = ("batch", "calls")
CASES = [
    Case("biased0.7", "ucosine", 256, 24, 300, lambda: biased(256, 0.7)),
    Case("biased0.3", "ucosine", 256, 24, 300, lambda: biased(256, 0.3)),
    Case("biased0.7", "ucosine", 768, 24, 300, lambda: biased(768, 0.7, n=1200), n=1200),
    Case("biased0.3", "ucosine", 768, 24, 300, lambda: biased(768, 0.3, n=1200), n=1200),
    Case("biased0.7", "cosine", 264, 24, 300, lambda: biased(264, 0.7, "cosine")),
    Case("biased0.7", "sq_euclid", 256, 24, 300, lambda: biased(256, 0.7, "sq_euclid")),
    Case("offset_cluster", "sq_euclid", 256, 24, 300, lambda: offset_cluster(256)),
    Case("overflow", "sq_euclid", 256, 24, 300, lambda: overflow(256)),
] + [Case(f, m, 256, 24, 300, (lambda f=f, m=m: (near_duplicates if f == "near_duplicates" else grid)(256, m)), schedules=TIE_SCHEDULES, group="ties")
     for f in ("near_duplicates", "grid") for m in ("sq_euclid", "cosine", "ucosine")] + [
    Case("many_accepted", "ucosine", 768, 40, 512, many_accepted, n=1200, group="accepted"),
    Case("many_accepted", "ucosine", 768, 63, 512, many_accepted, n=1200, group="accepted"),
    Case("many_accepted", "ucosine", 768, 63, 257, many_accepted, n=1200, group="accepted"),
    Case("ragged", "ucosine", 256, 12, 300, lambda: biased(256, 0.7, n=400, seed=481), n=400, schedules=("seq",), group="ragged"),
    Case("mixed_length", "ucosine", 256, 8, 300, lambda: mixed_length(256), group="mixed"),
    Case("nan_rows", "ucosine", 256, 24, 300, lambda: nan_rows(256), n=1000, group="nan"),
]
EDGE_CASES = [          # the rule's edges: uniform rows, none of them eligible
    Case("uniform", "ucosine", 248, 24, 300, lambda: plain(248), n=1000, group="edge"),
    Case("uniform", "ucosine", 260, 24, 300, lambda: plain(260), n=1000, group="edge"),
    Case("uniform", "ucosine", 256, 24, 256, lambda: plain(256), n=1000, group="edge"),
    Case("uniform", "ucosine_f16", 256, 24, 300, lambda: plain(256, "ucosine_f16"), n=1000, group="edge"),
]
SAMPLE = 200          # inserted rows the CPU tier traces per case: the last ones, added one by one


def add_by_schedule(ix, rows, schedule, **kw):
    """How both tiers feed an OracleIndex: "batch" one call under a cap of BATCH, "calls" all but the last 400 rows in one call and
    those in calls of 40, "seq" row by row."""
    n = rows.shape[0]
    if schedule == "seq":
        ix.add(rows)
    elif schedule == "batch":
        ix.add_batched(rows, BATCH, **kw)
    else:
        ix.add_batched(rows[:n - 400], BATCH, **kw)
        for i in range(n - 400, n, 40):
            ix.add_batched(rows[i:i + 40], BATCH)


if __name__ == "__main__":
    # python tests/gram_prefilter.py <case id> <file>: 512 rows of the case as raw float32, for tools/mfma_probe.hip
    import sys
    case = next(c for c in CASES + EDGE_CASES if c.id == sys.argv[1])
    case.rows()[-512:].tofile(sys.argv[2])
    print(f"{case.id}: 512 rows of {case.dim} floats -> {sys.argv[2]}")
