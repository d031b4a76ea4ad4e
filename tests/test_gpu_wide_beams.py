"""GPU tier: the 4- and 8-register-set forms of the traversal kernels (beams of 129 .. 256 and 257 .. 512 entries).

Every query and every Add keeps its beam in registers, as SortedTop<NS> or PoolTop<NS>: entry p in lane p & 63 of register set
p >> 6.  What differs between the set counts -- the carry from lane 63 of one set into lane 0 of the next (insert, adjacent_equal),
the per-set shifts of merge, the lookups past the first 64 entries, the pool's per-set masks and its final sort -- is what these
tests reach: every row kind, every form (latency / lean / plain; bitset, hash table or no visited set), beams exactly at the
edges between the set counts, lists that never fill, and equal distances right across the edge of two sets.  The reference is
the oracle everywhere: graph hashes equal, ids equal, distances byte-equal.  tests/test_wide_beam_inputs.py checks on the CPU that
the inputs hold the ties and the tie-free lists this file relies on; `sets_for` says which set count a case is about."""
import numpy as np
import pytest

import oracle
import wide_beams as wb
from common import default_cap, novis_active, set_diag

pytestmark = pytest.mark.gpu

NQ_SMALL = 300                     # the calls of the edge and form cases (the tie cases and one default call take all 4 000)


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


def _form(st):
    return "latency" if st["lat_launches"] else "lean" if st["lean_launches"] else "plain"


class Graph:
    """One query graph (M = 12, efc = 60, default schedule) built on the device, its hash checked against the oracle's, kept as
    rows + exported lists; `at(beam)` is that graph in an index (and an oracle) whose MinNN is the beam -- MinNN is fixed when an
    index is made -- so that knn_query(q, k) runs a beam of max(beam, k) and reads k entries of it."""

    def __init__(self, Index, case, metric, n=wb.N, dim=wb.DIM):
        self.Index, self.metric, self.n, self.dim = Index, metric, n, dim
        self.x, self.q = (wb.tie_case if case == "tie" else wb.plain_case)(metric, n=n, dim=dim)
        ix = self._index(5)
        ix.add(self.x)
        self.ref = wb.query_oracle(metric, self.x, cap=default_cap())
        assert ix.graph_hash() == self.ref.graph_hash(), (case, metric, n, dim)
        self.lv, self.entry = ix.levels(), ix.entry_point
        assert self.lv.tolist() == self.ref.levels().tolist()
        self.layers = [ix.export_edges(L, 2 * wb.M + 2 if L == 0 else wb.M + 2) for L in range(int(self.lv.max()) + 1)]
        self.hash = ix.graph_hash()
        self._at = (None, None, None)
        self._want = {}

    def _index(self, min_nn):
        ix = self.Index(self.dim, self.metric)
        ix.set_collection_size(self.n); ix.set_max_edges(wb.M); ix.set_max_candidates(wb.EFC); ix.set_min_nn(min_nn)
        return ix

    def at(self, beam):
        if self._at[0] != beam:                                     # one imported pair at a time: the cases of a beam run together
            self._at = (None, None, None)
            ix = self._index(beam)
            ix.import_graph(self.x, self.lv, self.entry, self.layers)
            assert ix.graph_hash() == self.hash
            self._at = (beam, ix, wb.oracle_with_min_nn(self.metric, self.x, self.ref, beam, self.lv, self.layers))
        return self._at[1], self._at[2]

    def want(self, beam, k, nq):
        """The oracle's answer to knn_query(q[:nq], k) under MinNN = beam, computed once."""
        if (beam, k, nq) not in self._want:
            self._want[(beam, k, nq)] = self.at(beam)[1].knn_query(self.q[:nq], k, threads=8)
        return self._want[(beam, k, nq)]


@pytest.fixture(scope="module")
def graphs(Index):
    cache = {}

    def get(case, metric, n=wb.N, dim=wb.DIM):
        key = (case, metric, n, dim)
        if key not in cache:
            cache[key] = Graph(Index, case, metric, n, dim)
        return cache[key]
    return get


def _ask(g, beam, k, nq):
    """knn_query(q[:nq], k) under a beam of max(beam, k) against the oracle; on the plain case the wide form must be what answered:
    nothing handed back, and at most a quarter of the jobs repeated by the exact traversal (a repeat needs a tie:
    wide_beams.REPEAT_CAP_SHARE).  Returns the call's counters."""
    ix, _ = g.at(beam)
    want = g.want(beam, k, nq)
    ix.reset_stats()
    got = ix.knn_query(g.q[:nq], k)
    st = ix.stats()
    assert _same(got, want), (g.metric, beam, k, nq, wb.sets_for(max(beam, k)))
    assert st["search_overflows"] == 0
    if wb.sets_for(max(beam, k)):
        print(f"search_repeats {g.metric} n {g.n} dim {g.dim} beam {max(beam, k)} k_out {k}: {st['search_repeats']} of {nq} ({_form(st)} form)")
        assert st["search_repeats"] <= wb.REPEAT_CAP_SHARE * nq, (g.metric, beam, k, st["search_repeats"], nq)
    return st


# ---- 2. queries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lat", [0, 2], ids=["sorted", "pool"])
@pytest.mark.parametrize("beam", wb.EDGE_BEAMS)
@pytest.mark.parametrize("metric", wb.ROW_KINDS)
def test_beams_at_the_edges_of_the_set_counts(graphs, monkeypatch, metric, beam, lat):
    """128 | 129, 256 | 257, 512 | 513: the last beam of one set count and the first of the next (513: the exact two-heap traversal
    from the start), with the whole list read (k_out = beam) and with ten entries of it (k_out = 10 under MinNN = beam), on the
    sorted list (lat=0) and on the pool (lat=2)."""
    set_diag(monkeypatch, lat=lat)
    g = graphs("plain", metric)
    st = _ask(g, beam, beam, NQ_SMALL)
    assert (st["lat_launches"] > 0) == (lat == 2 and wb.sets_for(beam) != 0)     # (no latency form of the exact-only launch)
    _ask(g, beam, 10, NQ_SMALL)


@pytest.mark.parametrize("lat", [0, 2], ids=["sorted", "pool"])
@pytest.mark.parametrize("metric,dim", [("sq_euclid", wb.DIM_TAIL), ("cosine", wb.DIM_TAIL), ("ucosine", wb.DIM_TAIL), ("sq_euclid_i8", wb.DIM_TAIL),
                                        ("sq_euclid_f16", wb.DIM_TAIL), ("sq_euclid_f16", wb.DIM_F16_ODD), ("ucosine_f16", wb.DIM_F16_ODD)])
def test_rows_with_a_scalar_tail_and_odd_f16_blocks_under_wide_beams(graphs, monkeypatch, metric, dim, lat):
    set_diag(monkeypatch, lat=lat)
    g = graphs("plain", metric, dim=dim)
    for beam in wb.FORM_BEAMS:
        _ask(g, beam, beam, NQ_SMALL)
        _ask(g, beam, 10, NQ_SMALL)


@pytest.mark.parametrize("lat", [0, 2], ids=["sorted", "pool"])
@pytest.mark.parametrize("beam", [300, 512])
@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_a_beam_wider_than_the_graph_never_fills(graphs, monkeypatch, metric, beam, lat):
    """90 nodes under beams of 300 and 512: the list stays short of k, so every count-bounded loop over the sets ends early and the
    answers are padded."""
    assert wb.sets_for(beam) == 8
    set_diag(monkeypatch, lat=lat)
    g = graphs("plain", metric, n=90)
    _ask(g, beam, beam, NQ_SMALL)
    _ask(g, beam, 10, NQ_SMALL)
    ids, d = g.at(beam)[0].knn_query(g.q[:4], beam)
    assert (ids[:, :90] >= 0).all() and (ids[:, 90:] == -1).all() and np.isnan(d[:, 90:]).all()


FORMS = [dict(lat=2), dict(lat=0), dict(lat=0, lean=0), dict(lat=0, novis=0), dict(lat=0, vis_hash=1)]


@pytest.mark.parametrize("hooks", FORMS, ids=lambda hk: ",".join(f"{k}={v}" for k, v in hk.items()))
@pytest.mark.parametrize("beam", wb.FORM_BEAMS)
@pytest.mark.parametrize("metric", wb.ROW_KINDS)
def test_every_form_of_the_four_and_eight_set_kernels(graphs, monkeypatch, metric, beam, hooks):
    """Beam 200 (NS = 4) and 300 (NS = 8) under each switch that picks a form: the latency form (pool), the lean form (NS = 4 only),
    the plain form reading flags 9, the plain form with its bitsets, the hashed form (NS = 4) and its bitset fallback (NS = 8)."""
    ns = wb.sets_for(beam)
    assert ns == {200: 4, 300: 8}[beam]
    set_diag(monkeypatch, **hooks)
    g = graphs("plain", metric)
    st = _ask(g, beam, beam, NQ_SMALL)
    _ask(g, beam, 10, NQ_SMALL)
    if hooks.get("lat") == 2:
        assert st["lat_launches"] > 0
    else:
        assert st["lat_launches"] == 0
    if hooks == dict(lat=0):
        if ns == 8:
            assert st["lean_launches"] == 0                          # the eight-set kernels have no lean form
        elif novis_active(st):
            assert st["lean_launches"] > 0
    if hooks.get("lean") == 0:
        assert st["lean_launches"] == 0
    if hooks.get("vis_hash") == 1:
        assert (st["visited_hash_launches"] > 0) == (ns == 4)        # NS = 8: the bitset fallback


@pytest.mark.parametrize("nq", [9, wb.NQ])
@pytest.mark.parametrize("beam", wb.FORM_BEAMS)
@pytest.mark.parametrize("metric", wb.ROW_KINDS)
def test_default_configuration_calls_of_9_and_4000_queries(graphs, metric, beam, nq):
    """Whatever form the defaults pick for a call that does not fill the chip and for one that does (printed, not asserted: it
    follows the device's resident waves)."""
    g = graphs("plain", metric)
    st = _ask(g, beam, beam, nq)
    print(f"default form {metric} NS={wb.sets_for(beam)} beam {beam} nq {nq}: {_form(st)}")


@pytest.mark.parametrize("lat", [0, 2], ids=["sorted", "pool"])
@pytest.mark.parametrize("beam,k_out", [(b, b) for b in wb.TIE_BEAMS] + [(wb.PREFIX_BEAM, wb.PREFIX_K)])
@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_ties_across_the_edges_of_register_sets_are_noticed(graphs, monkeypatch, metric, beam, k_out, lat):
    """The tie case: six duplicate pairs of rows, 4 000 queries.  A query whose list holds ONE pair of equal distances, at positions
    (64t - 1, 64t) of what the caller reads in order, is seen only through the carry between two register sets (sorted list) or
    through the pool's final sort; each of them must be handed to the exact traversal -- so search_repeats is at least their
    number -- and every answer must be the oracle's."""
    set_diag(monkeypatch, lat=lat)
    g = graphs("tie", metric)
    want = g.want(beam, k_out, wb.NQ)
    straddling = int(wb.straddling_only(want[1], k_out).sum())
    assert straddling >= (wb.MIN_STRADDLING if k_out == beam else wb.MIN_STRADDLING_PREFIX), straddling
    ix, _ = g.at(beam)
    ix.reset_stats()
    got = ix.knn_query(g.q, k_out)
    st = ix.stats()
    bad = np.flatnonzero((got[0] != want[0]).any(axis=1) | (got[1].view(np.uint32) != want[1].view(np.uint32)).any(axis=1))
    assert bad.size == 0, (metric, beam, k_out, bad[:8].tolist(), wb.straddling_only(want[1], k_out)[bad[:8]].tolist())
    assert (st["lat_launches"] > 0) == (lat == 2) and st["search_overflows"] == 0
    print(f"tie case {metric} beam {beam} k_out {k_out} lat={lat}: straddling-only {straddling}, search_repeats {st['search_repeats']}")
    assert st["search_repeats"] >= straddling
    # ... and those queries alone (most of the repeats above are ties INSIDE a set): every one of them must be repeated
    only = np.flatnonzero(wb.straddling_only(want[1], k_out))
    ix.reset_stats()
    got = ix.knn_query(g.q[only], k_out)
    assert _same(got, (want[0][only], want[1][only]))
    assert ix.stats()["search_repeats"] == only.size, (metric, beam, k_out, (only.size, ix.stats()["search_repeats"]))


# ---- 3. builds -----------------------------------------------------------------------------------------------------------
NB, MB = 2000, 12


def _build_rows(case, metric, dim=wb.DIM):
    return (wb.tie_case if case == "tie" else wb.plain_case)(metric, n=NB, dim=dim, nq=NQ_SMALL)   # (tie: the six pairs among the 2 000 rows)


_REFS = {}


def _build_oracle(case, metric, efc, schedule, dim=wb.DIM, M=MB, n=NB):
    """The oracle's graph of a build case, once per module: `schedule` "batch" = one call under a cap of 4 096, "calls" = 1 600 rows in
    one call and 400 in calls of 40, "seq" = strictly sequential."""
    key = (case, metric, efc, schedule, dim, M, n)
    if key not in _REFS:
        x, q = _build_rows(case, metric, dim)
        rows = wb.oracle_rows(metric, x)[:n]
        ref = oracle.OracleIndex(dim, wb.base_metric(metric), max_edges=M, max_candidates=efc, collection_size=n)
        if schedule == "seq":
            ref.add(rows)
        elif schedule == "batch":
            ref.add_batched(rows, 4096, threads=8)
        else:
            ref.add_batched(rows[:1600], 4096, threads=8)
            for i in range(1600, n, 40):
                ref.add_batched(rows[i:i + 40], 4096)
        _REFS[key] = (ref, ref.knn_query(q, 10, threads=8))
    return _REFS[key]


def _build(Index, monkeypatch, case, metric, efc, schedule, dim=wb.DIM, M=MB, n=NB, hooks=None):
    """Builds on the device what _build_oracle builds; graph hash, levels and a 300-query call must be the oracle's.  The small
    calls of "calls" run under lat=2.  Returns the index's counters after the build."""
    ref, want = _build_oracle(case, metric, efc, schedule, dim, M, n)
    x, q = _build_rows(case, metric, dim)
    set_diag(monkeypatch, **(hooks or {}))
    ix = Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_max_candidates(efc)
    ix.set_insert_batch(1 if schedule == "seq" else 4096)
    if schedule == "calls":
        ix.add(x[:1600])
        ix.reset_stats()
        set_diag(monkeypatch, lat=2)
        for i in range(1600, n, 40):
            ix.add(x[i:i + 40])
    else:
        ix.add(x[:n])
    st = ix.stats()
    assert ix.graph_hash() == ref.graph_hash(), (case, metric, efc, schedule, wb.sets_for(efc))
    assert ix.levels().tolist() == ref.levels().tolist() and ix.entry_point == ref.entry_point
    assert _same(ix.knn_query(q, 10), want)
    if schedule == "calls":
        assert st["lat_launches"] > 0
    return st


@pytest.mark.parametrize("schedule", ["batch", "calls"])
@pytest.mark.parametrize("efc", [200, 300])
@pytest.mark.parametrize("metric", wb.ROW_KINDS)
def test_builds_under_four_and_eight_sets(Index, monkeypatch, metric, efc, schedule):
    """efc 200 (NS = 4) and 300 (NS = 8), every row kind: the plain insert form (one call) and the latency insert form (calls of 40
    under lat=2)."""
    assert wb.sets_for(efc) == {200: 4, 300: 8}[efc]
    _build(Index, monkeypatch, "plain", metric, efc, schedule)


@pytest.mark.parametrize("efc", [129, 256, 257, 512, 513])
@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_builds_at_the_edges_of_the_set_counts(Index, monkeypatch, metric, efc):
    _build(Index, monkeypatch, "plain", metric, efc, "batch")


@pytest.mark.parametrize("efc", [200, 300])
@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_builds_with_the_visited_sets_kept(Index, monkeypatch, metric, efc):
    _build(Index, monkeypatch, "plain", metric, efc, "batch", hooks=dict(novis_insert=0))


@pytest.mark.parametrize("efc", [200, 300])
@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_builds_on_hashed_visited_sets_and_their_bitset_fallback(Index, monkeypatch, metric, efc):
    st = _build(Index, monkeypatch, "plain", metric, efc, "batch", hooks=dict(vis_hash=1))
    assert (st["visited_hash_launches"] > 0) == (wb.sets_for(efc) == 4)      # NS = 8: bitsets whatever is asked


@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_sequential_build_under_a_beam_wider_than_the_graph(Index, monkeypatch, metric):
    # 300 rows one at a time at efc 300: every search's list ends short of k
    _build(Index, monkeypatch, "plain", metric, 300, "seq", n=300)


@pytest.mark.parametrize("mfma", [0, 1])
def test_gram_tile_under_the_latency_insert_form(Index, monkeypatch, mfma):
    """The MFMA Gram-block prefilter of the neighbour heuristic (beams above 256 candidates, unit rows of 256 floats) behind the
    eight-set latency insert form: the last 400 rows in calls of 40 under lat=2."""
    assert wb.sets_for(300) == 8
    _build(Index, monkeypatch, "plain", "ucosine", 300, "calls", dim=256, M=24, hooks=dict(mfma=mfma))


@pytest.mark.parametrize("schedule", ["batch", "calls"])
@pytest.mark.parametrize("efc", [200, 300])
@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_builds_on_the_tie_case_rerun_what_meets_a_tie(Index, monkeypatch, metric, efc, schedule):
    """Duplicate rows under a build: the heuristic reads all k entries, so every doubt stays a doubt and an equal pair anywhere in the
    list sends the search to the exact traversal."""
    st = _build(Index, monkeypatch, "tie", metric, efc, schedule)
    assert st["insert_tie_reruns"] > 0
