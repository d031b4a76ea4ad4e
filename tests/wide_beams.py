"""Inputs and counting rules of the wide-beam tests (test_wide_beam_inputs.py on the CPU, test_gpu_wide_beams.py on the device).

The device keeps a beam in registers: entry p in lane p & 63 of register set p >> 6 (csrc/dk_sorted_top.h, csrc/dk_pool_top.h), and
sorted_top_sets() in device_backend.hip picks the number of sets from the beam width -- `sets_for` restates that rule, so that every
test says which set count it is about.  The data is small (3 000 rows) and fixed: a PLAIN case of i.i.d. uniform rows, and a TIE
case, the same rows with six rows overwritten by six others, which gives every query six exactly equal pairs of distances, each at
a place of its list that depends on the query alone -- among 4 000 queries a few dozen have such a pair right across the edge of two
register sets (positions 64t - 1 and 64t), which is where the carry between the sets decides whether the tie is seen."""
import numpy as np

import oracle
from common import normalize_f32, uniform

ROW_KINDS = ("sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16")
F16 = {"sq_euclid_f16": "sq_euclid", "ucosine_f16": "ucosine"}
N, DIM, NQ = 3000, 40, 4000          # the query graphs; DIM_TAIL / DIM_F16_ODD: a scalar tail, 16-element f16 blocks left odd
DIM_TAIL, DIM_F16_ODD = 33, 120
# PAIR_SEED: of the seeds 1 .. 12, the one whose oracle lists hold the most straddling ties at the beam that has the fewest (4 000
# queries; test_wide_beam_inputs.py prints the counts: 20 or more per beam, 7 or more in the prefix, against thresholds of 10 and 5)
ROW_SEED, QUERY_SEED, PAIR_SEED, N_PAIRS = 77, 78, 9, 6
M, EFC = 12, 60
EDGE_BEAMS = (128, 129, 256, 257, 512, 513)
FORM_BEAMS = (200, 300)              # NS = 4 and NS = 8
TIE_BEAMS = (200, 300, 512)
PREFIX_BEAM, PREFIX_K = 300, 100     # k_out = 100 under beam 300: the ordered prefix ends inside register set 1
MIN_STRADDLING, MIN_STRADDLING_PREFIX = 10, 5
# Under sorted_top=1 a repeat is a hand-over to the exact two-heap traversal, which a query asks for only when it meets equal
# distances: the share of queries with ANY equal pair among their 600 nearest rows (test_wide_beam_inputs.py measures it by brute
# force: 0.06 for sq_euclid_i8 to 0.23 for ucosine_f16) bounds the repeats of the plain case from above, and a quarter lies above that.
REPEAT_CAP_SHARE = 0.25
TIE_WINDOW = 600


def sets_for(beam):
    """Register sets of the sorted list / the pool for that beam width (sorted_top_sets in device_backend.hip); 0: the exact
    two-heap traversal only."""
    return 2 if beam <= 128 else 4 if beam <= 256 else 8 if beam <= 512 else 0


def h(x):
    """What an f16 row kind stores: the rows rounded to binary16 (queries are never rounded)."""
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def base_metric(metric):
    return F16.get(metric, metric)


def oracle_rows(metric, x):
    """The rows the oracle is built on: an X_f16 index fed x is the X index fed h(x) (tests/test_gpu_f16.py)."""
    return h(x) if metric in F16 else x


def _shape(metric, x):
    return normalize_f32(x) if base_metric(metric) == "ucosine" else x


def plain_case(metric, n=N, dim=DIM, nq=NQ):
    """(rows, queries): i.i.d. uniform, unit length for the ucosine kinds."""
    return _shape(metric, uniform(n, dim, ROW_SEED)), _shape(metric, uniform(nq, dim, QUERY_SEED))


def duplicate_pairs(n=N, pairs=N_PAIRS, seed=PAIR_SEED):
    """(a, b) index arrays: row a[i] is overwritten by row b[i]; all 2 * pairs rows distinct."""
    picked = np.random.default_rng(seed).choice(n, 2 * pairs, replace=False)
    return picked[:pairs], picked[pairs:]


def tie_case(metric, n=N, dim=DIM, nq=NQ):
    """The plain case with six duplicate pairs: row a overwritten by row b (after normalising: the copies are bit-equal)."""
    x, q = plain_case(metric, n, dim, nq)
    a, b = duplicate_pairs(n)
    x = x.copy()
    x[a] = x[b]
    return x, q


def straddling_only(dists, upto=None):
    """Per result list (a row of `dists`, ascending): True when its first `upto` entries (all of them: None) hold exactly ONE pair of
    adjacent equal distances and that pair sits at positions (64t - 1, 64t) -- across the edge of two register sets, so that only
    the carry from lane 63 of set t - 1 into lane 0 of set t can see it."""
    d = np.asarray(dists)[:, :upto]
    eq = d[:, 1:].view(np.uint32) == d[:, :-1].view(np.uint32)      # eq[:, p - 1]: positions p - 1 and p
    at_edge = np.zeros(eq.shape[1], dtype=bool)
    at_edge[63::64] = True                                          # p = 64, 128, ...
    return (eq.sum(axis=1) == 1) & (eq & at_edge).any(axis=1)


def brute_force_lists(metric, rows, queries, k):
    """Per query the k smallest distances to `rows` by the oracle's own metric, ascending (ids do not matter here): [nq, k]."""
    ids = np.arange(rows.shape[0], dtype=np.int32)
    out = np.empty((queries.shape[0], k), dtype=np.float32)
    for i, qi in enumerate(queries):
        out[i] = np.sort(oracle.dist_query_rows(base_metric(metric), rows, qi, ids))[:k]
    return out


def any_tie_share(dists):
    """The share of result lists that hold any pair of equal distances."""
    d = np.asarray(dists)
    return float((d[:, 1:].view(np.uint32) == d[:, :-1].view(np.uint32)).any(axis=1).mean())


def query_oracle(metric, rows, min_nn=5, cap=16, n_threads=8):
    """The oracle index of the query graphs (M = 12, efc = 60) on `rows` under snapshot batches of `cap`."""
    ref = oracle.OracleIndex(rows.shape[1], base_metric(metric), max_edges=M, max_candidates=EFC, min_nn=min_nn, collection_size=rows.shape[0])
    ref.add_batched(oracle_rows(metric, rows), cap, threads=n_threads)
    return ref


def oracle_layers(ref, lv, m=M):
    """The oracle's graph as (counts, edges) per layer, the layout of Index.export_edges / import_graph."""
    out = []
    for layer in range(int(lv.max()) + 1):
        counts = np.full(lv.size, -1, np.int32)
        edges = np.zeros((lv.size, 2 * m + 2), np.int32)
        for i in np.nonzero(lv >= layer)[0]:
            e = ref.edges(int(i), layer)
            counts[i] = e.size
            edges[i, :e.size] = e
        out.append((counts, edges))
    return out


def oracle_with_min_nn(metric, rows, src, min_nn, lv=None, layers=None):
    """A second oracle holding src's graph with another MinNN (MinNN is fixed when an index is made): KnnQuery(k) searches with a
    beam of max(MinNN, k)."""
    lv = src.levels() if lv is None else lv
    layers = oracle_layers(src, lv) if layers is None else layers
    ref = oracle.OracleIndex(rows.shape[1], base_metric(metric), max_edges=M, max_candidates=EFC, min_nn=min_nn, collection_size=rows.shape[0],
                             allow_removals=False)
    ref.import_graph(oracle_rows(metric, rows), lv, src.entry_point, layers)
    assert ref.graph_hash() == src.graph_hash()
    return ref
