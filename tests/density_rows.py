"""Inputs of the GPU tests of the density clusters (tests/test_gpu_density_clusters.py): 3 000 rows x dim 20 with structure planted on
top of uniform rows, the graph of the pairs that are to be within the radius, and the radius between those and every other pair.

Everything that has a shape is planted along an ARC: the points |b| (cos(t th) e1 + sin(t th) e2) for positions t in units of a
STEP, th = STEP / |b|, e1 the direction of a base row scaled to the norm R and e2 a random direction orthogonal to it.  Two points
at positions s and t are 2 R^2 (1 - cos((s - t) th)) apart by the squared-Euclidean kinds and 1 - cos((s - t) th) by the cosine
kinds: about (s - t)^2 times the distance of one step for both, so one layout serves all six row kinds.  Positions one step apart
(or less) are links, positions 1.8 steps apart (or more) are not: (1.8)^2 = 3.24 > 2, the margin the radius is asserted to have.

  CHAIN     ten rows at positions 0 .. 9: only consecutive rows are within.  Inner rows have two neighbours, the ends one.
  BIG       200 rows within NOISE of one row, spread over every chunk and round: the hot root and the hot counts.
  STRADDLE  twelve such rows under the ids around the chunk edge 700 and the tile edges 696 and 704.
  TRIPLE    one row under three ids.
  two copies of  B2 (6 rows at -2)  B1 (2 rows at -1)  X (at 0)  A1 (2 rows at 0.8)  A2 (6 rows at 1.8):  B = B1 + B2 and
            A = A1 + A2 are dense groups (every row has at least 7 neighbours); X is within the two rows of B1 (one step) and the
            two rows of A1 (0.8 steps, nearer) and nothing else: four neighbours.  B holds the smaller ids.  In the first copy X
            has an id below all of its neighbours (it is the query of its pairs), in the second an id above them (the candidate)."""
import numpy as np

from common import normalize_f32, uniform

N, DIM = 3000, 20
CHUNK, QTILE, ROUND = 700, 8, 512              # five chunks; tiles of 8 members; six rounds of 512 members
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
STEP, R = 0.1414, 2.5                          # one step of an arc as a chord; the norm of every arc
NOISE, TIGHT = 0.01, 0.002                     # half-width per element of BIG and STRADDLE; of the sub-blobs of A and B
MIN_SAMPLES = 6                                # where X (four neighbours) is a border and every row of A and B is core

TRIPLE = [100, 1500, 2900]
CHAIN = [1396, 1397, 1398, 1399, 1400, 1401, 1402, 2000, 2400, 2800]   # 1399 | 1400 is a chunk edge; the far end lies rounds away
STRADDLE = list(range(694, 706))


class AB:
    """One copy of B2 B1 X A1 A2, by ids."""
    def __init__(self, x, b1, b2, a1, a2):
        self.x, self.b1, self.b2, self.a1, self.a2 = x, b1, b2, a1, a2
        self.a, self.b = sorted(a1 + a2), sorted(b1 + b2)

    def ids(self):
        return [self.x] + self.a + self.b

    def parts(self):
        return ((self.b2, -2.0), (self.b1, -1.0), ([self.x], 0.0), (self.a1, 0.8), (self.a2, 1.8))


LOW = AB(300, [310, 1210], [320, 330, 900, 1250, 1260, 1270], [1700, 2210], [1710, 1720, 2220, 2230, 2600, 2610])      # X below its neighbours
HIGH = AB(2950, [1000, 1010], [1020, 1030, 1040, 1450, 1460, 2050], [2500, 2510], [2520, 2530, 2540, 2810, 2820, 2830])  # X' above them


def _big():
    taken = set(TRIPLE + CHAIN + STRADDLE + LOW.ids() + HIGH.ids())
    ids = [i for i in np.random.default_rng(9).permutation(N).tolist() if i not in taken][:200]
    return sorted(ids)


BIG = _big()


def _arc(rng, base, t):
    """The point at position t (in steps) of an arc of norm R that starts in the direction of `base`."""
    e1 = base.astype(np.float64) / np.linalg.norm(base.astype(np.float64))
    v = rng.standard_normal(DIM)
    v -= (v @ e1) * e1
    e2 = v / np.linalg.norm(v)
    th = STEP / R
    return lambda t: (R * (np.cos(t * th) * e1 + np.sin(t * th) * e2)).astype(np.float32)


def rows(metric):
    rng = np.random.default_rng(177)
    x = uniform(N, DIM, 1).copy()
    x[TRIPLE[1]] = x[TRIPLE[0]]
    x[TRIPLE[2]] = x[TRIPLE[0]]
    at = _arc(rng, x[CHAIN[0]], 0)
    for t, v in enumerate(CHAIN):
        x[v] = at(float(t))
    for ids in (STRADDLE, BIG):
        x[ids] = x[ids[0]] + rng.uniform(-NOISE, NOISE, (len(ids), DIM)).astype(np.float32)
    for ab in (LOW, HIGH):
        at = _arc(rng, x[ab.x], 0)
        for ids, t in ab.parts():
            x[ids] = at(t) + (rng.uniform(-TIGHT, TIGHT, (len(ids), DIM)).astype(np.float32) if len(ids) > 1 else 0)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def links():
    """The planted pairs (a < b) that are to be within the radius."""
    out = set()
    for ids in (TRIPLE, STRADDLE, BIG, LOW.a, LOW.b, HIGH.a, HIGH.b):
        out |= {(a, b) for i, a in enumerate(sorted(ids)) for b in sorted(ids)[i + 1:]}
    out |= {tuple(sorted(p)) for p in zip(CHAIN[:-1], CHAIN[1:])}
    for ab in (LOW, HIGH):
        out |= {tuple(sorted((ab.x, v))) for v in ab.a1 + ab.b1}
    return out


def numpy_dist(metric, x):
    """float64 distances of every pair of rows by the metric's formula (half-precision kinds: on the rounded rows)."""
    x = (x.astype(np.float16) if metric.endswith("_f16") else x).astype(np.float64)
    g = x @ x.T
    n2 = np.diag(g)
    if metric.startswith("sq_euclid"):
        return n2[:, None] + n2[None, :] - 2 * g
    return 1.0 - g if metric.startswith("ucosine") else 1.0 - g / np.sqrt(n2[:, None] * n2[None, :])


def radius_between(metric, x, pairs):
    """(radius, d): the geometric mean of the largest distance of `pairs` (a < b) and the smallest distance of any other pair, and the
    float64 distances.  The first is asserted to be less than half the second, so that no pair's distance is near the radius
    whichever row is the query and whatever the row kind rounds."""
    n = x.shape[0]
    d = numpy_dist(metric, x)
    link = np.zeros((n, n), bool)
    a, b = np.array(sorted(pairs)).T
    link[a, b] = True
    upper = np.triu(np.ones((n, n), bool), 1)
    largest_link, smallest_other = d[link].max(), d[upper & ~link].min()
    assert 0 < largest_link * 2 < smallest_other, (metric, largest_link, smallest_other)
    return float(np.float32(np.sqrt(largest_link * smallest_other))), d
