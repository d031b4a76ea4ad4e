"""GPU tier: KnnQuery's half-precision row prefilter (kFormLeanPF).  The lean search form measures the listed
neighbours on the index's half-precision shadow rows and reads the f32 row only of those the shadow value cannot turn away -- so the
answers must be the oracle's, ids equal and distances byte-equal, with the prefilter forced on (diag row_prefilter=2) exactly as with
it off (0), on every register-set count and beam edge, on rows where it pays (uniform) and where it cannot (a tight cluster, which
must cost one launch and then fall back), and after every kind of write to the stored rows: a stale shadow row would answer
wrongly without any other sign.  lat=0 throughout, so that these small calls take the lean family (tests/row_prefilter.py holds
the bound itself, tests/test_row_prefilter_model.py checks it on the CPU)."""
import numpy as np
import pytest

import oracle
from common import default_cap, set_diag, uniform

pytestmark = pytest.mark.gpu

N, NQ, M = 6000, 300, 16
BEAMS = [(16, 10), (64, 10), (65, 65), (128, 10), (200, 100)]      # (efSearch = MinNN, k): one and two register sets of two, the edge, four sets
ZERO = {"launches": 0, "rows_on_shadow": 0, "rows_reread": 0, "rows_packed": 0}


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


def _tight(n, dim, seed):
    """c + 1e-4 noise: neighbouring halves near c are 2.4e-4 .. 4.9e-4 apart, so almost every row lies inside the bound of every other."""
    rng = np.random.default_rng(seed)
    c = rng.random(dim, dtype=np.float32)
    return (c + np.float32(1e-4) * rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)


class Graph:
    """One graph (M = 16, default schedule) built on the device with the prefilter off, its hash the oracle's; at(ef) is that graph in
    an index and an oracle whose MinNN is ef (MinNN is fixed when an index is made), want(ef, k) the oracle's answer, computed once."""

    def __init__(self, Index, kind, dim):
        self.Index, self.dim = Index, dim
        self.x = uniform(N, dim, 40 + dim) if kind == "uniform" else _tight(N, dim, 41)
        self.q = uniform(NQ, dim, 50 + dim) if kind == "uniform" else _tight(NQ, dim, 51)
        ix = self._index(5)
        ix.add(self.x)
        ref = oracle.OracleIndex(dim, "sq_euclid", max_edges=M, collection_size=N)
        ref.add_batched(self.x, default_cap(), threads=8)
        assert ix.graph_hash() == ref.graph_hash()
        self.hash, self.lv, self.entry = ix.graph_hash(), ix.levels(), ix.entry_point
        self.layers = [ix.export_edges(L, 2 * M + 2 if L == 0 else M + 2) for L in range(int(self.lv.max()) + 1)]
        self._want = {}

    def _index(self, min_nn):
        ix = self.Index(self.dim, "sq_euclid")
        ix.set_collection_size(N); ix.set_max_edges(M); ix.set_min_nn(min_nn)
        return ix

    def at(self, ef):
        ix = self._index(ef)
        ix.import_graph(self.x, self.lv, self.entry, self.layers)
        assert ix.graph_hash() == self.hash
        return ix

    def want(self, ef, k):
        if (ef, k) not in self._want:
            ref = oracle.OracleIndex(self.dim, "sq_euclid", max_edges=M, min_nn=ef, collection_size=N, allow_removals=False)
            ref.import_graph(self.x, self.lv, self.entry, self.layers)
            assert ref.graph_hash() == self.hash
            self._want[(ef, k)] = ref.knn_query(self.q, k, threads=8)
        return self._want[(ef, k)]


@pytest.fixture(scope="module")
def graphs(Index):
    cache = {}

    def get(kind, dim):
        if (kind, dim) not in cache:
            import os
            old = os.environ.get("HNSW_MI355X_DIAG")
            os.environ["HNSW_MI355X_DIAG"] = ((old + ",") if old else "") + "row_prefilter=0"   # (built once, whatever test comes first)
            try:
                cache[(kind, dim)] = Graph(Index, kind, dim)
            finally:
                if old is None:
                    del os.environ["HNSW_MI355X_DIAG"]
                else:
                    os.environ["HNSW_MI355X_DIAG"] = old
        return cache[(kind, dim)]
    return get


@pytest.mark.parametrize("ef,k", BEAMS)
@pytest.mark.parametrize("kind,dim", [("uniform", 8), ("uniform", 100), ("uniform", 128), ("tight", 100)])
def test_answers_are_the_oracles_with_the_prefilter_on_and_off(graphs, monkeypatch, kind, dim, ef, k):
    g = graphs(kind, dim)
    want = g.want(ef, k)
    got = {}
    for mode in (0, 2):
        set_diag(monkeypatch, lat=0, row_prefilter=mode)
        ix = g.at(ef)
        got[mode] = ix.knn_query(g.q, k)
        st, pf = ix.stats(), ix.row_prefilter_stats()
        assert _same(got[mode], want), (kind, dim, ef, k, mode)
        assert st["lean_launches"] > 0 and st["lat_launches"] == 0 and st["search_overflows"] == 0
        print(f"row prefilter {mode} {kind} dim {dim} ef {ef} k {k}: {pf}, search_evals {st['search_evals']}, repeats {st['search_repeats']}")
        if mode == 0:
            assert pf == ZERO                                            # off: nothing ran, nothing was packed (or allocated)
        else:
            assert pf["launches"] > 0 and pf["rows_packed"] == N
            assert 0 < pf["rows_reread"] <= pf["rows_on_shadow"]
            if kind == "uniform":
                assert pf["rows_reread"] < pf["rows_on_shadow"]          # rows were turned away on the shadow value
    assert _same(got[0], got[2])


def test_a_tight_cluster_costs_one_launch_and_falls_back(graphs, monkeypatch):
    g = graphs("tight", 100)
    set_diag(monkeypatch, lat=0)                                         # row_prefilter at its default, 1
    ix = g.at(64)
    first = ix.knn_query(g.q, 10)
    pf1 = ix.row_prefilter_stats()
    assert pf1["launches"] == 1 and 2 * pf1["rows_reread"] > pf1["rows_on_shadow"]
    second = ix.knn_query(g.q, 10)
    pf2 = ix.row_prefilter_stats()
    assert pf2["launches"] == 1 and pf2["rows_on_shadow"] == pf1["rows_on_shadow"]   # the lean form answered the second call
    assert _same(first, g.want(64, 10)) and _same(second, g.want(64, 10))
    assert ix.stats()["lean_launches"] == 2


def test_uniform_rows_keep_the_prefilter_by_default(graphs, monkeypatch):
    g = graphs("uniform", 128)
    set_diag(monkeypatch, lat=0)
    ix = g.at(128)
    for _ in range(2):
        assert _same(ix.knn_query(g.q, 10), g.want(128, 10))
    pf = ix.row_prefilter_stats()
    assert pf["launches"] == 2 and pf["rows_packed"] == N and 2 * pf["rows_reread"] < pf["rows_on_shadow"]


def test_every_write_to_the_stored_rows_reaches_the_shadow(Index, monkeypatch, tmp_path):
    """query; Add within the capacity; Add past it (the row matrix moves); Serialize / Deserialize; Remove + Add into the freed slots --
    each step against the oracle, the prefilter forced on.  Every Add here makes rows that are nearer to the queries than anything
    before (they are copies of the queries, slightly moved): a query answered from a stale shadow would turn them away."""
    set_diag(monkeypatch, lat=0, row_prefilter=2)
    dim, n0 = 100, 3000
    x, q = uniform(n0, dim, 71), uniform(NQ, dim, 72)
    near = lambda seed: (q[:200] + np.float32(1e-2) * uniform(200, dim, seed)).astype(np.float32)
    ix = Index(dim, "sq_euclid")
    ix.set_collection_size(n0 + 300); ix.set_max_edges(M)
    ref = oracle.OracleIndex(dim, "sq_euclid", max_edges=M, collection_size=n0 + 300)

    def step(what, packed):
        got, want = ix.knn_query(q, 10), ref.knn_query(q, 10, threads=8)
        assert ix.graph_hash() == ref.graph_hash(), what
        assert _same(got, want), what
        pf = ix.row_prefilter_stats()
        assert pf["rows_packed"] == packed, (what, pf)
        return pf

    assert (ix.add(x) == ref.add_batched(x, default_cap(), threads=8)).all()
    step("built", n0)
    step("again: nothing to pack", n0)
    a = near(73)
    assert (ix.add(a) == ref.add_batched(a, default_cap(), threads=8)).all()
    step("added within the capacity", n0 + 200)                          # only the new rows
    b = np.concatenate([near(74), uniform(300, dim, 75)])
    assert (ix.add(b) == ref.add_batched(b, default_cap(), threads=8)).all()
    grown = step("grown past the collection size", n0 + 200 + (n0 + 700))["launches"]   # the matrix moved: all of it again
    path = tmp_path / "index.bin"
    ix.serialize(path)
    ix2 = Index.deserialize(path)
    got, want = ix2.knn_query(q, 10), ref.knn_query(q, 10, threads=8)
    assert _same(got, want) and ix2.row_prefilter_stats()["launches"] > 0 and ix2.row_prefilter_stats()["rows_packed"] == n0 + 700
    gone = np.arange(n0, n0 + 200, dtype=np.int32)                       # the first batch of near rows leaves ...
    ix.remove(gone); ref.remove(gone)
    c = near(76)                                                         # ... and other near rows take their slots
    ids_c, want_c = ix.add(c), ref.add_batched(c, default_cap(), threads=8)
    assert (ids_c == want_c).all() and set(ids_c.tolist()) == set(gone.tolist())
    after = step("slots re-used", ix.row_prefilter_stats()["rows_packed"] + (n0 + 700 - int(ids_c.min())))
    assert after["launches"] > grown


def test_one_element_beyond_the_half_range_turns_nothing_away(Index, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=2)
    dim, n = 24, 2000
    x, q = uniform(n, dim, 81), uniform(NQ, dim, 82)
    x[1234, 5] = 7e4                                                     # rounds to +inf in binary16: E = +inf
    ix = Index(dim, "sq_euclid")
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_min_nn(64)
    ref = oracle.OracleIndex(dim, "sq_euclid", max_edges=M, min_nn=64, collection_size=n)
    assert (ix.add(x) == ref.add_batched(x, default_cap(), threads=8)).all()
    assert _same(ix.knn_query(q, 10), ref.knn_query(q, 10, threads=8))
    pf = ix.row_prefilter_stats()
    assert pf["launches"] == 1 and pf["rows_on_shadow"] > 0 and pf["rows_reread"] == pf["rows_on_shadow"]
