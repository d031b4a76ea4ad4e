"""Inputs of the GPU tests of the near-duplicate calls over the graph's edges (tests/test_gpu_graph_duplicate_groups.py): the planted
rows of tests/test_gpu_duplicate_groups.py (the recipe restated here, not imported from a test file), the radius between the planted
links and every other pair, an oracle graph in import_graph's layout, and hand-made layer-0 graphs."""
import numpy as np

from common import normalize_f32, uniform

N, DIM = 3000, 20
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
TRIPLE = [100, 1500, 2900]                     # one row under three ids
CHAIN = [1399, 1400, 2000]                     # a - b - c in steps of STEP: the ends are 2 STEP apart
STRADDLE = list(range(694, 706))
STEP, NOISE = np.float32(0.1414), 0.01         # the chain's step along a unit direction; the clusters' half-width per element


def _big():
    taken = set(TRIPLE + CHAIN + STRADDLE)
    ids = [i for i in np.random.default_rng(9).permutation(N).tolist() if i not in taken][:200]
    return sorted(ids)


BIG = _big()


def rows(metric):
    rng = np.random.default_rng(77)
    x = uniform(N, DIM, 1).copy()
    x[TRIPLE[1]] = x[TRIPLE[0]]
    x[TRIPLE[2]] = x[TRIPLE[0]]
    u = rng.standard_normal(DIM).astype(np.float32)
    u /= np.linalg.norm(u)
    x[CHAIN[1]] = x[CHAIN[0]] + STEP * u
    x[CHAIN[2]] = x[CHAIN[0]] + 2 * STEP * u
    for ids in (STRADDLE, BIG):
        x[ids] = x[ids[0]] + rng.uniform(-NOISE, NOISE, (len(ids), DIM)).astype(np.float32)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def links():
    """The planted pairs that are to be within the radius."""
    out = {(TRIPLE[0], TRIPLE[1]), (TRIPLE[0], TRIPLE[2]), (TRIPLE[1], TRIPLE[2]), (CHAIN[0], CHAIN[1]), (CHAIN[1], CHAIN[2])}
    for ids in (STRADDLE, BIG):
        out |= {(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]}
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
    """The geometric mean of the largest distance of `pairs` (a < b) and the smallest distance of any other pair; the first is
    asserted to be less than half the second, so that no pair's distance is near the radius whichever row is the query and
    whatever the row kind rounds."""
    n = x.shape[0]
    d = numpy_dist(metric, x)
    link = np.zeros((n, n), bool)
    a, b = np.array(sorted(pairs)).T
    link[a, b] = True
    upper = np.triu(np.ones((n, n), bool), 1)
    largest_link, smallest_other = d[link].max(), d[upper & ~link].min()
    assert 0 < largest_link * 2 < smallest_other, (metric, largest_link, smallest_other)
    return float(np.float32(np.sqrt(largest_link * smallest_other)))


def planted_labels():
    want = np.arange(N, dtype=np.int32)
    for ids in (TRIPLE, CHAIN, STRADDLE, BIG):
        want[ids] = min(ids)
    return want


def layers_of(edges_of, levels, stride):
    """A graph as (counts, edges) per layer, the layout of Index.export_edges / import_graph / DeviceBackend.set_graph."""
    levels = np.asarray(levels, np.int32)
    out = []
    for layer in range(int(levels.max()) + 1):
        counts = np.full(levels.size, -1, np.int32)
        edges = np.zeros((levels.size, stride), np.int32)
        for i in np.nonzero(levels >= layer)[0]:
            e = np.asarray(edges_of(int(i), layer), np.int32)
            counts[i] = e.size
            edges[i, :e.size] = e
        out.append((counts, edges))
    return out


def ring_lists(n, hops=(1, 2, 7)):
    """Layer-0 lists of a graph that hangs together and says nothing about distances: i lists i + h (mod n) for h in hops."""
    return {i: [(i + h) % n for h in hops] for i in range(n)}
