"""GPU tier: the measure passes alone, at the row lengths of tests/row_lengths.py, on hand-made graphs.

The inner boundary (DeviceBackend.upload_rows, set_graph, knn_search, range_search) on a chain of hubs whose layer-0 lists have
exactly the lengths 1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 57 and 64: measure_all's selections of one to four rows per lane group, its
second round of 32 rows and the widest list the latency form takes.  A beam as wide as the graph returns every node, so every list
is measured whole, and the answer is the oracle's traversal of the same graph: ids equal, distances equal byte for byte, and again
equal to oracle.dist_query_rows of the returned ids.  No query has two equal distances (tests/test_row_length_inputs.py).

Each case runs under every switch that picks a form, and stats() must say that the form ran -- a hand-back to the host would
otherwise count as a pass.  The full graph (327 nodes) is searched on eight register sets, which have the plain and the latency
forms; the lean forms and the row prefilter exist for up to four sets, so two smaller graphs (206 and 221 nodes) carry the same
list lengths for those.  The prefilter's counters belong to an index, so that one run goes through Index.import_graph."""
import numpy as np
import pytest

import oracle
import row_lengths as rl
import wide_beams as wb
from common import set_diag
from filtered_model import filtered_knn_batch

pytestmark = pytest.mark.gpu

# the switches, and which graphs they run on ("full", "lean0", "lean1")
SWITCHES = (
    ({}, ("full", "lean0", "lean1")),
    ({"lat": 0}, ("full", "lean0", "lean1")),
    ({"lat": 2}, ("full", "lean0", "lean1")),
    ({"lean": 0, "lat": 0}, ("full", "lean0")),
    ({"sorted_top": 0}, ("full",)),
    ({"novis": 0}, ("full", "lean1")),
    ({"novis": 0, "lat": 0}, ("full", "lean1")),
)
GRAPHS = {"full": rl.HUB_LISTS, "lean0": rl.LEAN_LISTS[0], "lean1": rl.LEAN_LISTS[1]}


@pytest.fixture(scope="module")
def net():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.net_amd


def _same(got, want):
    """ids equal, distances equal byte for byte; padding (-1 / NaN) in the same places."""
    (gi, gd), (wi, wd) = got, want
    pad = np.isnan(wd)
    return bool((gi == wi).all() and (np.isnan(gd) == pad).all() and gd[~pad].tobytes() == wd[~pad].tobytes())


def _same_lists(got, want):
    return all(a.tolist() == c.tolist() and b.tobytes() == d.tobytes() for a, b, c, d in zip(got[0], got[1], want[0], want[1])) and len(got[0]) == len(want[0])


class Case:
    """One (kind, length, graph): the backend with the rows and the graph, and the oracle holding the same graph."""

    def __init__(self, net, kind, dim, shifted, lists):
        self.kind, self.dim, self.base = kind, dim, wb.base_metric(kind)
        self.n, self.lv, self.layers = rl.hub_graph(lists)
        x, self.q = rl.pass_rows(kind, dim, shifted)
        self.x = x[:self.n]
        self.rows = wb.oracle_rows(kind, self.x)                  # what the oracle holds: the f16 kinds' rows rounded
        self.ref = oracle.OracleIndex(dim, self.base, max_edges=rl.GRAPH_M, min_nn=5, collection_size=self.n, allow_removals=False)
        self.ref.import_graph(self.rows, self.lv, 0, self.layers)
        self.want = self.ref.knn_query(self.q, self.n)
        self.ids = np.arange(self.n, dtype=np.int32)
        # the reference side: every node, strictly ascending, the distances those of the metric alone
        for i, qi in enumerate(self.q):
            assert sorted(self.want[0][i].tolist()) == self.ids.tolist() and (np.diff(self.want[1][i]) > 0).all()
            assert self.want[1][i].tobytes() == oracle.dist_query_rows(self.base, self.rows, qi, self.want[0][i]).tobytes()
        self.dev = net.DeviceBackend(dim, kind, capacity=self.n)
        self.dev.upload_rows(0, self.x)
        self.dev.set_graph(self.lv, self.layers, rl.GRAPH_M)

    def knn(self, tag):
        ids, d, flags = self.dev.knn_search(self.q, 0, self.n, self.n)
        assert (flags == 0).all(), tag
        assert (ids == self.want[0]).all(), tag
        assert d.tobytes() == self.want[1].tobytes(), tag


def _run_switches(monkeypatch, c, graph, tag):
    for diag, graphs in SWITCHES:
        if graph not in graphs:
            continue
        with monkeypatch.context() as m:
            set_diag(m, **diag)
            c.dev.reset_stats()
            c.knn(tag + (diag,))
            st = c.dev.stats()
        plan = rl.search_plan(c.kind, c.dim, c.n, rl.GRAPH_M, diag)
        t = tag + (diag, plan["form"], {k: st[k] for k in ("search_launches", "lat_launches", "lean_launches", "search_overflows", "search_repeats", "launches")})
        assert st["search_launches"] >= 1 and st["search_overflows"] == 0 and st["launches"] == 0, t
        assert (st["lat_launches"] > 0) == (plan["form"] == "lat"), t
        assert (st["lean_launches"] > 0) == (plan["form"] == "lean"), t
        if diag.get("lat") == 2:
            assert plan["lat_ok"] and st["lat_launches"] > 0, t
        if plan["novis"] and diag == {"lat": 0} and graph != "full":
            assert st["lean_launches"] > 0, t


@pytest.mark.parametrize("kind,dim,shifted", rl.pass_cases(), ids=lambda v: str(v))
def test_every_list_length_under_every_form(net, monkeypatch, kind, dim, shifted):
    for graph, lists in GRAPHS.items():
        c = Case(net, kind, dim, shifted, lists)
        tag = (kind, dim, shifted, graph)
        _run_switches(monkeypatch, c, graph, tag)
        if graph != "full":
            continue
        # RangeQuery on the same graph (graph_range_kernel measures eight lists at once): everything, and the median fourth distance
        for radius in (1e30, float(np.median(c.want[1][:, 3]))):
            got_ids, got_d, flags = c.dev.range_search(c.q, 0, radius)
            assert (flags == 0).all(), tag
            assert _same_lists((got_ids, got_d), c.ref.range_query(c.q, radius)), tag + (radius,)
        st = c.dev.stats()
        assert st["range_launches"] == 2 and st["range_handbacks"] == 0, tag
        # the two-heap predicate traversal over every third id
        mask = c.ids % 3 == 0
        got_ids, got_d, flags = c.dev.knn_search(c.q, 0, c.n, c.n, allowed=mask)
        assert (flags == 0).all(), tag
        want = filtered_knn_batch(c.ref, c.rows, c.base, c.q, c.n, c.n, mask)
        assert _same((got_ids, got_d), want), tag
        assert (np.sort(want[0][:, :int(mask.sum())], axis=1) == np.flatnonzero(mask)).all() and (want[0][:, int(mask.sum()):] == -1).all(), tag


PF_LENGTHS = tuple(d for d in rl.F32_LENGTHS if d <= 256)


@pytest.mark.parametrize("dim", PF_LENGTHS)
def test_row_prefilter_at_every_list_length(monkeypatch, dim):
    """The lean form's row prefilter (sq_euclid, rows of up to 256 elements) forced on: the same graphs imported into an index,
    whose KnnQuery(k = n) searches with a beam of n from the same entry point.  Its launches must be counted."""
    import hnswindex
    set_diag(monkeypatch, row_prefilter=2, lat=0)
    for graph in ("lean0", "lean1"):
        n, lv, layers = rl.hub_graph(GRAPHS[graph])
        x, q = rl.pass_rows("sq_euclid", dim)
        ref = oracle.OracleIndex(dim, "sq_euclid", max_edges=rl.GRAPH_M, min_nn=5, collection_size=n, allow_removals=False)
        ref.import_graph(x[:n], lv, 0, layers)
        ix = hnswindex.Index(dim, "sq_euclid")
        ix.set_collection_size(n); ix.set_max_edges(rl.GRAPH_M)
        ix.import_graph(x[:n], lv, 0, layers)
        assert ix.graph_hash() == ref.graph_hash() and rl.search_plan("sq_euclid", dim, n, rl.GRAPH_M, {"lat": 0})["form"] == "lean"
        ix.reset_stats()
        got, want = ix.knn_query(q, n), ref.knn_query(q, n)
        assert (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes(), (dim, graph)
        st, pf = ix.stats(), ix.row_prefilter_stats()
        assert st["search_launches"] == 1 and st["lean_launches"] == 1 and st["search_overflows"] == 0 and st["launches"] == 0, (dim, graph, st)
        assert pf["launches"] == 1 and pf["rows_on_shadow"] > 0 and pf["rows_packed"] >= n, (dim, graph, pf)
