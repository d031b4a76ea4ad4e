"""GPU tier: the f32 passes of the 8-bit row-prefilter kernels take 16 rows, not 32 (form_measure_cap, csrc/dk_base.h).

Every measure_all inside kFormLeanPF8Fixed -- the re-read of the shadow pass's survivors, the descent, the exact two-heap traversal a
tied job falls into -- splits its rows into passes of 16.  A row's value is its own accumulator whatever pass it rides in, so the
answers stay the oracle's, ids equal and distances byte for byte, and the row counters stay the model's; what can go wrong is the
split itself: a row dropped or measured into another row's slot at a pass boundary.  row_prefilter=3 (the 8-bit form regardless),
lat=0 (these small calls take the lean family) throughout.

1. Pass boundaries.  A star: the entry node lists n ids, every other node lists the entry node.  The beam is wider than the graph, so
   the list never fills, nothing is turned away and the re-read takes all n rows (the counters say so).  n runs through both sides of
   every boundary of the 16-row split and of the 8-row groups inside a pass.  Each n runs three times: on uniform rows, with the row
   nearest to every query at list position 16, and at position 32 -- the first row of the second and of the third pass (the last
   position where the list is shorter).  Bitset and hashed kernels; one case on four register sets (k = 130).
2. The exact traversal inside the kernel, on rows of {0, 0.5, 1}^128 (equal distances everywhere) around a list of 24 ids.
3. The descent through upper layers whose lists hold 9 .. 16 ids.
4. rows_on_shadow / rows_reread are tests/row_prefilter8.py's model's; search_evals and search_repeats those of row_prefilter=0."""
import os

import numpy as np
import pytest

import oracle
import row_lengths as rl
import row_prefilter8 as r8
from common import set_diag, uniform

pytestmark = pytest.mark.gpu

DIM = r8.DIM
LISTS = (1, 8, 9, 16, 17, 24, 25, 31, 32, 33, 48, 49, 64)
NEAREST_AT = (None, 16, 32)          # list position of the row nearest to every query (None: uniform rows as they come)
NQ = 8
WIDE = 49                            # the n that also runs on four register sets


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _same(got, want):
    """ids equal, distances equal byte for byte; padding (-1 / NaN) in the same places."""
    (gi, gd), (wi, wd) = got, want
    pad = np.isnan(wd)
    return bool(gi.shape == wi.shape and (gi == wi).all() and (np.isnan(gd) == pad).all() and gd[~pad].tobytes() == wd[~pad].tobytes())


def _pair(Index, m, min_nn, rows, lv, entry, layers):
    """The same imported graph in an index and in the oracle."""
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(rows.shape[0]); ix.set_max_edges(m); ix.set_min_nn(min_nn); ix.set_allow_removals(False)
    ix.import_graph(rows, lv, entry, layers)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=m, min_nn=min_nn, collection_size=rows.shape[0], allow_removals=False)
    ref.import_graph(rows, lv, entry, layers)
    assert ix.graph_hash() == ref.graph_hash()
    return ix, ref


# ---- 1. pass boundaries ------------------------------------------------------------------------------------------------------------
def star_rows(n, nearest_at):
    """(rows, queries) of the star with n leaves: uniform; with nearest_at, the row at that list position (id position + 1: the
    entry node's list is 1 .. n in order) is the mean of the queries -- nearer to each of them than any uniform row by a wide margin
    (about 9 against 21).  The first seed without two equal distances by the oracle's metric."""
    for seed in range(8):
        x, q = uniform(n + 1, DIM, 9600 + 100 * seed + n).copy(), uniform(NQ, DIM, 9650 + 100 * seed + n)
        if nearest_at is not None:
            x[1 + min(nearest_at, n - 1)] = q.mean(axis=0, dtype=np.float64).astype(np.float32)
        if rl.distinct_distances("sq_euclid", x, q):
            return x, q
    raise AssertionError(f"no tie-free seed for {(n, nearest_at)}")


def _star_case(Index, n, nearest_at, min_nn, k):
    nodes, lv, layers = rl.hub_graph((n,))
    assert nodes == n + 1 and layers[0][0][0] == n and layers[0][1][0, :n].tolist() == list(range(1, n + 1))
    x, q = star_rows(n, nearest_at)
    ix, ref = _pair(Index, rl.GRAPH_M, min_nn, x, lv, 0, layers)
    want = ref.knn_query(q, k)
    assert (np.sort(want[0][:, :nodes], axis=1) == np.arange(nodes)).all()          # every node is an answer: every row counts
    if nearest_at is not None:
        assert (want[0][:, 0] == 1 + min(nearest_at, n - 1)).all()
    got = ix.knn_query(q, k)
    st, pf8 = ix.stats(), ix.row_prefilter8_stats()
    tag = (n, nearest_at, min_nn, k, pf8)
    assert _same(got, want), tag
    # the 8-bit form ran, in the sorted traversal alone; the entry node's n rows and each leaf's one, none of them turned away
    assert pf8["launches"] == 1 and pf8["fallbacks_to_f16"] == 0 and st["lean_launches"] == 1 and st["lat_launches"] == 0, tag
    assert st["search_overflows"] == 0 and st["search_repeats"] == 0, tag
    assert pf8["rows_on_shadow"] == pf8["rows_reread"] == NQ * 2 * n, tag
    return st


@pytest.mark.parametrize("vis_hash", [0, 1], ids=["bitset", "hashed"])
@pytest.mark.parametrize("n", LISTS)
def test_every_pass_boundary_of_the_survivor_re_read(Index, monkeypatch, n, vis_hash):
    set_diag(monkeypatch, lat=0, row_prefilter=3, vis_hash=vis_hash)
    for nearest_at in NEAREST_AT:
        st = _star_case(Index, n, nearest_at, 80, n + 1)                            # a beam of 80 > 65 nodes: two register sets
        assert (st["visited_hash_launches"] > 0) == bool(vis_hash)
        if n == WIDE:
            _star_case(Index, n, nearest_at, 200, 130)                              # four register sets; the answer is padded


# ---- 2. the exact traversal inside the kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vis_hash", [0, 1], ids=["bitset", "hashed"])
def test_the_exact_traversal_inside_the_kernel_over_a_list_of_24(Index, monkeypatch, vis_hash):
    """Rows and queries from {0, 0.5, 1}^128: squared distances are multiples of 0.25.  The oracle says first that some query has
    equal distances on both sides of the edge of its answer (entries k - 1 and k); such a job starts over in the exact traversal of
    the same kernel, whose first expansion measures the entry node's 24 rows in passes of 16 and 8."""
    set_diag(monkeypatch, lat=0, row_prefilter=3, vis_hash=vis_hash)
    n, ef, k = 24, 16, 10
    nodes, lv, layers = rl.hub_graph((n,))
    rng = np.random.default_rng(9700)
    x = rng.integers(0, 3, (nodes, DIM)).astype(np.float32) * np.float32(0.5)
    q = rng.integers(0, 3, (64, DIM)).astype(np.float32) * np.float32(0.5)
    ix, ref = _pair(Index, rl.GRAPH_M, ef, x, lv, 0, layers)
    beam = ref.knn_query(q, k + 1)[1]                                               # (the same beam: max(MinNN, k) = 16 for both)
    tied = int((beam[:, k - 1] == beam[:, k]).sum())
    print(f"{tied} of {q.shape[0]} queries have equal distances at the edge of their answer")
    assert tied > 0
    got, want = ix.knn_query(q, k), ref.knn_query(q, k)
    st, pf8 = ix.stats(), ix.row_prefilter8_stats()
    print(f"repeats {st['search_repeats']}, {pf8}")
    assert _same(got, want)
    assert st["search_repeats"] > 0 and st["search_overflows"] == 0
    assert pf8["launches"] == 1 and st["lean_launches"] == 1 and (st["visited_hash_launches"] > 0) == bool(vis_hash)


# ---- 3, 4. a built index: the descent, the counters -------------------------------------------------------------------------------------
M, N = 16, 2000


class Built:
    """A graph over uniform rows (M 16: upper-layer lists of up to 16 ids), built on the device with the prefilter off."""

    def __init__(self, Index):
        self.Index, self.x = Index, uniform(N, DIM, 9800)
        old = os.environ.get("HNSW_MI355X_DIAG")
        os.environ["HNSW_MI355X_DIAG"] = ((old + ",") if old else "") + "row_prefilter=0"
        try:
            ix = Index(DIM, "sq_euclid")
            ix.set_collection_size(N); ix.set_max_edges(M)
            ix.add(self.x)
        finally:
            if old is None:
                del os.environ["HNSW_MI355X_DIAG"]
            else:
                os.environ["HNSW_MI355X_DIAG"] = old
        self.lv, self.entry = ix.levels(), ix.entry_point
        self.layers = [ix.export_edges(L, 2 * M + 2 if L == 0 else M + 2) for L in range(int(self.lv.max()) + 1)]

    def pair(self, ef):
        return _pair(self.Index, M, ef, self.x, self.lv, self.entry, self.layers)

    def descent_lists(self, q):
        """The lengths of the lists the greedy descent of query q measures (GraphNavigator.cs:27-82), upper layers only."""
        adj = r8.adjacency(self.layers)
        dx = oracle.dist_query_rows("sq_euclid", self.x, q, np.arange(N, dtype=np.int32), use_avx=True)
        best, out = int(self.entry), []
        for layer in range(int(self.lv[best]), 0, -1):
            changed = True
            while changed:
                changed = False
                out.append(len(adj[layer][best]))
                for nb in adj[layer][best]:
                    if dx[nb] < dx[best]:
                        best, changed = nb, True
        return out


@pytest.fixture(scope="module")
def built(Index):
    return Built(Index)


def test_the_descent_crosses_lists_of_9_to_16_ids(built, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=3)
    q = uniform(64, DIM, 9801)
    assert int(built.lv.max()) >= 1
    crossed = [n for qi in q for n in built.descent_lists(qi)]
    print(f"lists measured by the descents: {sorted(set(crossed))}")
    assert sum(9 <= n <= 16 for n in crossed) >= q.shape[0] and any(n <= 8 for n in crossed)
    ix, ref = built.pair(64)
    assert _same(ix.knn_query(q, 10), ref.knn_query(q, 10, threads=8))
    assert ix.row_prefilter8_stats()["launches"] == 1 and ix.stats()["search_overflows"] == 0


def test_the_counters_do_not_move(built, monkeypatch):
    """shadow=0: whether an idle wave answers a tied job before its owner is a race that search_repeats would show."""
    ef, k = 64, 10
    q = uniform(24, DIM, 9802)
    set_diag(monkeypatch, lat=0, row_prefilter=3, shadow=0)
    ix, ref = built.pair(ef)
    want = ref.knn_query(q, k, threads=8)
    got = ix.knn_query(q, k)
    st, pf8 = ix.stats(), ix.row_prefilter8_stats()
    assert _same(got, want) and pf8["launches"] == 1
    peek = ix.row_prefilter8_peek(0, N)
    shadow = r8.decode(peek["codes"], peek["lo"], peek["step"])
    models = [r8.search_model8(built.x, shadow, built.layers, built.lv, built.entry, qi, ef, peek["e"]) for qi in q]
    assert all(m["ids"][:k] == row.tolist() for m, row in zip(models, got[0]))
    on, lo, hi = (sum(m[name] for m in models) for name in ("rows_on_shadow", "rows_reread_lo", "rows_reread_hi"))
    print(f"device {pf8}; model: on the shadow {on}, re-read {sum(m['rows_reread'] for m in models)} in [{lo}, {hi}]")
    assert pf8["rows_on_shadow"] == on and lo <= pf8["rows_reread"] <= hi
    assert 0 < pf8["rows_reread"] < pf8["rows_on_shadow"]
    set_diag(monkeypatch, row_prefilter=0)
    off, _ = built.pair(ef)
    assert _same(off.knn_query(q, k), want)
    st0 = off.stats()
    print(f"search_evals {st['search_evals']} (prefilter off: {st0['search_evals']}), search_repeats {st['search_repeats']} (off: {st0['search_repeats']})")
    assert off.row_prefilter8_stats()["launches"] == 0
    assert st["search_evals"] == st0["search_evals"] > 0 and st["search_repeats"] == st0["search_repeats"]
