"""GPU tier: the fixed-length form of KnnQuery's row prefilter (kFormLeanPFFixed).  An index whose rows are 128 words
long runs the prefilter in a kernel with that length compiled in, at four waves per SIMD; diag pf_fixed_dim=0 keeps the form that
reads the length at run time.  Both run the same instructions on the same data, so here they must agree in everything that can be
seen: ids and distance bytes (the oracle's), the rows measured on the shadow and re-read, the jobs the exact traversal answered --
and row_prefilter_form_stats() must say which of the two ran.  Other row lengths must keep the run-time form.

lat=0 (these small calls take the lean family) and row_prefilter=2 (on regardless) throughout.  Where counters are compared,
shadow=0 as well: an idle wave that starts the exact traversal of a job beside its owner may answer it first, and whether it does
is a race that search_repeats would show."""
import os

import numpy as np
import pytest

import oracle
from common import set_diag, uniform

pytestmark = pytest.mark.gpu

M = 16
BEAMS = [(64, 10), (128, 10), (200, 130)]                               # (efSearch = MinNN, k); the last one: four register sets


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


class Graph:
    """One graph over rows x (M = 16), built on the device with the prefilter off; at(ef) is that graph in a fresh index whose MinNN
    is ef, want(q, ef, k) the oracle's answer on the same graph."""

    def __init__(self, Index, x):
        self.Index, self.x, self.dim = Index, x, x.shape[1]
        old = os.environ.get("HNSW_MI355X_DIAG")
        os.environ["HNSW_MI355X_DIAG"] = ((old + ",") if old else "") + "row_prefilter=0"
        try:
            ix = self._index(5)
            ix.add(x)
        finally:
            if old is None:
                del os.environ["HNSW_MI355X_DIAG"]
            else:
                os.environ["HNSW_MI355X_DIAG"] = old
        self.hash, self.lv, self.entry = ix.graph_hash(), ix.levels(), ix.entry_point
        self.layers = [ix.export_edges(L, 2 * M + 2 if L == 0 else M + 2) for L in range(int(self.lv.max()) + 1)]
        self._refs = {}

    def _index(self, min_nn):
        ix = self.Index(self.dim, "sq_euclid")
        ix.set_collection_size(self.x.shape[0]); ix.set_max_edges(M); ix.set_min_nn(min_nn)
        return ix

    def at(self, ef):
        ix = self._index(ef)
        ix.import_graph(self.x, self.lv, self.entry, self.layers)
        assert ix.graph_hash() == self.hash
        return ix

    def ref(self, ef):
        if ef not in self._refs:
            r = oracle.OracleIndex(self.dim, "sq_euclid", max_edges=M, min_nn=ef, collection_size=self.x.shape[0], allow_removals=False)
            r.import_graph(self.x, self.lv, self.entry, self.layers)
            assert r.graph_hash() == self.hash
            self._refs[ef] = r
        return self._refs[ef]

    def want(self, q, ef, k):
        return self.ref(ef).knn_query(q, k, threads=8)


@pytest.fixture(scope="module")
def g128(Index):
    return Graph(Index, uniform(3000, 128, 9100))


@pytest.fixture(scope="module")
def q128():
    return uniform(256, 128, 9101)


def _run(g, q, ef, k):
    """A fresh index of the graph, one call: (answer, prefilter counters, form counters, device counters)."""
    ix = g.at(ef)
    got = ix.knn_query(q, k)
    return got, ix.row_prefilter_stats(), ix.row_prefilter_form_stats(), ix.stats()


@pytest.mark.parametrize("ef,k", BEAMS)
def test_both_forms_give_the_oracles_answers_and_equal_counters(g128, q128, monkeypatch, ef, k):
    want = g128.want(q128, ef, k)
    set_diag(monkeypatch, lat=0, row_prefilter=2, shadow=0, pf_fixed_dim=1)
    fixed, pf1, form1, st1 = _run(g128, q128, ef, k)
    set_diag(monkeypatch, pf_fixed_dim=0)
    runtime, pf0, form0, st0 = _run(g128, q128, ef, k)
    set_diag(monkeypatch, row_prefilter=0, pf_fixed_dim=1)
    off, pfoff, formoff, stoff = _run(g128, q128, ef, k)
    print(f"ef {ef} k {k}: fixed {pf1} {form1} repeats {st1['search_repeats']}; run-time {pf0} {form0} repeats {st0['search_repeats']}; "
          f"off repeats {stoff['search_repeats']}")
    assert _same(fixed, want) and _same(runtime, want) and _same(off, want)
    assert _same(fixed, runtime) and _same(fixed, off)
    # the right form
    assert form1 == {"runtime_dim": 0, "fixed_dim": pf1["launches"]} and pf1["launches"] > 0
    assert form0 == {"runtime_dim": pf0["launches"], "fixed_dim": 0} and pf0["launches"] == pf1["launches"]
    assert formoff == {"runtime_dim": 0, "fixed_dim": 0} and pfoff["launches"] == 0
    for st in (st1, st0, stoff):
        assert st["lean_launches"] > 0 and st["lat_launches"] == 0 and st["search_overflows"] == 0
    # the same decisions
    assert pf1["rows_on_shadow"] == pf0["rows_on_shadow"] > 0 and pf1["rows_reread"] == pf0["rows_reread"] > 0
    assert pf1["rows_reread"] < pf1["rows_on_shadow"]
    assert st1["search_repeats"] == st0["search_repeats"]


def test_the_default_is_the_fixed_form_with_shadow_traversals_on(g128, q128, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=2)                        # pf_fixed_dim and shadow at their defaults
    got, pf, form, st = _run(g128, q128, 128, 10)
    assert _same(got, g128.want(q128, 128, 10))
    assert pf["launches"] > 0 and form == {"runtime_dim": 0, "fixed_dim": pf["launches"]}


@pytest.mark.parametrize("dim", [127, 129, 120, 256])
def test_other_row_lengths_keep_the_run_time_form(Index, monkeypatch, dim):
    set_diag(monkeypatch, lat=0, row_prefilter=2)
    g, q = Graph(Index, uniform(1500, dim, 9200 + dim)), uniform(64, dim, 9300 + dim)
    got, pf, form, st = _run(g, q, 64, 10)
    print(f"dim {dim}: {pf} {form}")
    assert _same(got, g.want(q, 64, 10))
    assert pf["launches"] > 0 and form == {"runtime_dim": pf["launches"], "fixed_dim": 0}
    assert st["lean_launches"] > 0 and st["lat_launches"] == 0


def test_the_hashed_form(g128, q128, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=2, vis_hash=1)
    got, pf, form, st = _run(g128, q128, 64, 10)
    set_diag(monkeypatch, pf_fixed_dim=0)
    got0, pf0, form0, st0 = _run(g128, q128, 64, 10)
    assert _same(got, g128.want(q128, 64, 10)) and _same(got, got0)
    assert st["visited_hash_launches"] > 0 and st0["visited_hash_launches"] > 0
    assert pf["launches"] > 0 and form == {"runtime_dim": 0, "fixed_dim": pf["launches"]}
    assert form0 == {"runtime_dim": pf0["launches"], "fixed_dim": 0}


def test_the_exact_traversal_inside_the_fixed_form(Index, monkeypatch):
    """Rows and queries from {0, 0.5, 1}^128: squared distances are multiples of 0.25, so equal ones are everywhere.  The oracle says
    so first, on the CPU: some query's result list has equal distances on both sides of its edge (entries k - 1 and k of the beam,
    which OrderBy + Take(k) decides between).  Such a job leaves the sorted traversal for the exact two-heap one in the same kernel."""
    ef, k = 64, 10
    rng = np.random.default_rng(9400)
    x = (rng.integers(0, 3, (1500, 128)).astype(np.float32) * np.float32(0.5))
    q = (rng.integers(0, 3, (64, 128)).astype(np.float32) * np.float32(0.5))
    g = Graph(Index, x)
    beam = g.want(q, ef, k + 1)[1]                                       # (the same beam: efSearch is max(MinNN, k) = 64 for both)
    tied = int((beam[:, k - 1] == beam[:, k]).sum())
    print(f"{tied} of {q.shape[0]} queries have equal distances at the edge of their list")
    assert tied > 0
    want = g.want(q, ef, k)
    set_diag(monkeypatch, lat=0, row_prefilter=2)
    got, pf, form, st = _run(g, q, ef, k)
    print(f"fixed form: {pf} {form} repeats {st['search_repeats']} overflows {st['search_overflows']}")
    assert _same(got, want)
    assert st["search_repeats"] > 0
    assert pf["launches"] > 0 and form == {"runtime_dim": 0, "fixed_dim": pf["launches"]}


def test_more_jobs_than_resident_waves(g128, monkeypatch):
    """8192 queries are more jobs than the four-wave grid holds: one call (a wave takes job after job) and 32 calls of 256 (a wave
    takes at most one) must answer alike and measure and re-read the same rows."""
    set_diag(monkeypatch, lat=0, row_prefilter=2, shadow=0)
    ef, k = 64, 10
    q = uniform(8192, 128, 9500)
    want = g128.want(q, ef, k)
    one, many = g128.at(ef), g128.at(ef)
    assert _same(one.knn_query(q, k), want)
    parts = [many.knn_query(q[i:i + 256], k) for i in range(0, q.shape[0], 256)]
    assert _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want)
    a, b = one.row_prefilter_stats(), many.row_prefilter_stats()
    fa, fb = one.row_prefilter_form_stats(), many.row_prefilter_form_stats()
    print(f"one call {a} {fa}, 32 calls {b} {fb}")
    assert a["launches"] == 1 and b["launches"] == 32
    assert fa == {"runtime_dim": 0, "fixed_dim": 1} and fb == {"runtime_dim": 0, "fixed_dim": 32}
    assert a["rows_on_shadow"] == b["rows_on_shadow"] > 0 and a["rows_reread"] == b["rows_reread"] > 0
    assert a["rows_reread"] < a["rows_on_shadow"] and a["rows_packed"] == b["rows_packed"] == g128.x.shape[0]
    assert one.stats()["search_repeats"] == many.stats()["search_repeats"]
