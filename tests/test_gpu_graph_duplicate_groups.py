"""GPU tier: graph_duplicate_groups and near_edges -- near-duplicates over the layer-0 edges of the graph: every
member's list measured once by graph_edge_kernel, the edges within the radius joined in a union-find on the device or returned as
they are.  The contract is tests/graph_dup_model.py; the rows are the planted rows of the duplicate_groups tests (graph_dup_rows.py):
an exact triple, a chain whose ends are apart, a cluster of 12 and one of 200, a radius far from every pair distance.  Labels, info
and edges must equal the model over the index's own lists and the distances exact_range_query_by_id reports; the groups must refine
duplicate_groups', equal them on the oracle's graphs, and follow the graph where the two differ."""
import ctypes as ct

import numpy as np
import pytest

import graph_dup_rows as gr
from common import set_diag, uniform
from graph_dup_model import dist_from_range_lists, graph_duplicate_groups, near_edges

pytestmark = pytest.mark.gpu

N, DIM, ROUND = gr.N, gr.DIM, 512              # six rounds of 512 owners
_I, _F = ct.POINTER(ct.c_int), ct.POINTER(ct.c_float)


def _index(dim, metric, n, max_edges=8):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(max_edges); ix.set_insert_batch(0)
    return ix


def _model(ix, members, r, length=None, lists=None):
    """(labels, info, (src, dst, dist)) of the contract over the index's own layer-0 lists and the distances of its range lists."""
    members = np.asarray(members, np.int32)
    ids, d = ix.exact_range_query_by_id(members, r) if lists is None else lists
    dist = dist_from_range_lists(members, ids, d)
    edges_of = lambda i: ix.edges(i, 0)
    length = ix.length if length is None else length
    labels, info = graph_duplicate_groups(edges_of, length, members, dist, r)
    src, dst, dd, _ = near_edges(edges_of, members, dist, r)
    return labels, info, (src, dst, dd)


def _same_edges(got, want):
    return got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2].tobytes() == want[2].tobytes() and \
        (got[0].dtype, got[1].dtype, got[2].dtype) == (np.int32, np.int32, np.float32)


def _info(info, launches):
    return {k: v for k, v in info.items() if k != "launches"}, info["launches"] == launches


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x = gr.rows(metric)
        self.r = gr.radius_between(metric, self.x, gr.links())
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        self.lists = self.ix.exact_range_query_by_id(np.arange(N), self.r)
        self.want = _model(self.ix, np.arange(N), self.r, lists=self.lists)     # computed once
        self.want[0].setflags(write=False)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


# ---------------------------------------------------------------- 1. six row kinds, the index's own graph
@pytest.mark.parametrize("metric", gr.METRICS)
def test_groups_and_edges_are_the_model_over_the_index_lists(cases, monkeypatch, metric):
    c = cases(metric)
    want_labels, want_info, want_edges = c.want
    assert want_info["members"] == N and want_info["edges_within"] > 0 and want_info["edges_measured"] > want_info["edges_within"]
    first = None
    for knobs, launches in (({}, 1), (dict(edge_round=ROUND), 6)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for _ in range(3):                                               # the unions arrive in another order every time
            c.ix.reset_stats()
            labels, info = c.ix.graph_duplicate_groups(c.r)
            assert labels.dtype == np.int32 and labels.tobytes() == want_labels.tobytes(), (metric, knobs)
            assert _info(info, launches) == (want_info, True), (metric, knobs, info)
            assert c.ix.stats()["exact_launches"] == 0                   # no scan ran: the distances are the edges'
            first = first or labels.tobytes()
            assert labels.tobytes() == first
        assert _same_edges(c.ix.near_edges(c.r), want_edges), (metric, knobs)
    # a refinement of the exact groups: every graph group lies inside one exact group
    exact, _ = c.ix.duplicate_groups(c.r)
    assert (exact[labels] == exact).all() and (labels >= exact).all(), metric
    assert exact.tolist() == gr.planted_labels().tolist()


# ---------------------------------------------------------------- 2. the oracle's graph, float32 kinds
@pytest.mark.parametrize("max_edges", [8, 40])
@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine"])
def test_on_the_oracles_graph_the_groups_are_the_exact_groups(metric, max_edges):
    import oracle
    x = gr.rows(metric)
    r = gr.radius_between(metric, x, gr.links())
    ref = oracle.OracleIndex(DIM, metric, max_edges=max_edges, collection_size=N)
    ref.add(x)
    lv = ref.levels()
    layers = gr.layers_of(ref.edges, lv, 2 * max_edges + 2)
    longest = int(layers[0][0].max())
    assert longest > 64 if max_edges == 40 else longest <= 16            # past one wave's 64 entries at MaxEdges 40
    ix = _index(DIM, metric, N, max_edges)
    ix.import_graph(x, lv, ref.entry_point, layers)
    labels, info = ix.graph_duplicate_groups(r)
    exact, exact_info = ix.duplicate_groups(r)
    assert labels.tobytes() == exact.tobytes() and info["groups"] == exact_info["groups"] == N - 2 - 2 - 11 - 199, (metric, max_edges, info)
    dist = lambda own, cand: oracle.dist_query_rows(metric, x, x[own], np.asarray(cand, np.int32)) if len(cand) else np.zeros(0, np.float32)
    edges_of = lambda i: ref.edges(i, 0)
    want_labels, want_info = graph_duplicate_groups(edges_of, N, np.arange(N), dist, r)
    assert labels.tobytes() == want_labels.tobytes() and _info(info, 1) == (want_info, True), (metric, max_edges, info, want_info)
    want = near_edges(edges_of, np.arange(N), dist, r)
    assert _same_edges(ix.near_edges(r), want[:3]), (metric, max_edges)
    assert info["edges_measured"] == int(layers[0][0].sum())


# ---------------------------------------------------------------- 3. a planted graph: the call reads the graph
def _planted_graph():
    n, dim, m = 400, 8, 40
    x = uniform(n, dim, 91).copy()
    near = np.float32(0.005)
    x[300] = x[10]                                   # identical rows, no path of within-edges between them
    x[200] = x[100] + near                           # 200 lists 100, 100 does not list 200
    x[[51, 52, 53, 54, 55]] = x[50] + near * np.arange(1, 6, dtype=np.float32)[:, None] / 5    # the tail of 50's long list
    lists = gr.ring_lists(n, hops=(60, 121, 187))    # (no hop joins two planted rows)
    lists[200] = [100] + lists[200]
    far = [i for i in range(56, 400) if i not in (100, 200, 300)][:65]
    lists[50] = far + [51, 52, 53, 54, 55]           # 70 members; only entries 65 .. 69 are within the radius
    pairs = {(10, 300), (100, 200)} | {(a, b) for a in range(50, 56) for b in range(a + 1, 56)}
    r = gr.radius_between("sq_euclid", x, pairs)
    return n, dim, m, x, lists, r


def test_a_planted_graph_is_followed_edge_by_edge():
    n, dim, m, x, lists, r = _planted_graph()
    ix = _index(dim, "sq_euclid", n, m)
    ix.import_graph(x, np.zeros(n, np.int32), 0, gr.layers_of(lambda i, layer: lists[i], np.zeros(n, np.int32), 2 * m + 2))
    assert len(lists[50]) == 70 and ix.edges(50, 0).tolist() == lists[50] and ix.edges(50, 0)[65:].tolist() == [51, 52, 53, 54, 55]
    labels, info = ix.graph_duplicate_groups(r)
    want_labels, want_info, want_edges = _model(ix, np.arange(n), r)
    assert labels.tobytes() == want_labels.tobytes() and _info(info, 1) == (want_info, True)
    exact, _ = ix.duplicate_groups(r)
    assert exact[300] == 10 and labels[300] == 300 and labels[10] == 10                  # duplicates the graph does not connect stay apart
    assert labels[200] == 100 and labels[100] == 100                                     # one direction, towards the smaller id, is enough
    assert labels[50:56].tolist() == [50] * 6 and info["edges_within"] == 6              # entries 65 .. 69 of a list of 70, and 200 -> 100
    assert info["groups"] == n - 1 - 5 and info["edges_measured"] == 3 * n + 1 + 67
    got = ix.near_edges(r)
    assert _same_edges(got, want_edges) and got[0].tolist() == [50] * 5 + [200] and got[1].tolist() == [51, 52, 53, 54, 55, 100]


# ---------------------------------------------------------------- 4. row lengths
@pytest.mark.parametrize("metric,dim", [("sq_euclid", 3), ("sq_euclid", 33), ("sq_euclid", 128), ("sq_euclid_i8", 33), ("ucosine_f16", 33)])
def test_row_lengths(metric, dim):
    n = 600
    x = uniform(n, dim, 17 + dim).copy()
    rng = np.random.default_rng(dim)
    pairs = [(i, i + 300) for i in range(0, 40, 2)]
    for a, b in pairs:
        x[b] = x[a] + rng.uniform(-1, 1, dim).astype(np.float32) * np.float32(0.01 if dim > 3 else 0.0005)
    if metric.startswith("ucosine"):
        from common import normalize_f32
        x = normalize_f32(x)
    r = gr.radius_between(metric, x, pairs)
    ix = _index(dim, metric, n)
    ix.add(x)
    want_labels, want_info, want_edges = _model(ix, np.arange(n), r)
    assert want_info["edges_within"] > 0
    labels, info = ix.graph_duplicate_groups(r)
    assert labels.tobytes() == want_labels.tobytes() and _info(info, 1) == (want_info, True), (metric, dim, info, want_info)
    assert _same_edges(ix.near_edges(r), want_edges)
    exact, _ = ix.duplicate_groups(r)
    assert (exact[labels] == exact).all()


# ---------------------------------------------------------------- 5. allow-sets, radii, removed ids
@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_allowed_sets_nan_and_infinity(cases, monkeypatch, metric):
    c = cases(metric)
    set_diag(monkeypatch, edge_round=ROUND)
    allowed = np.ones(N, bool)
    out = [gr.CHAIN[1], gr.TRIPLE[0]] + gr.STRADDLE[:4] + gr.BIG[::2] + list(range(2100, 2400))
    allowed[out] = False
    members = np.flatnonzero(allowed)
    want_labels, want_info, want_edges = _model(c.ix, members, c.r)
    labels, info = c.ix.graph_duplicate_groups(c.r, allowed=allowed)
    assert labels.tobytes() == want_labels.tobytes() and _info(info, -(-members.size // ROUND)) == (want_info, True), (info, want_info)
    assert (labels[out] == -1).all() and (labels[members] >= 0).all()
    assert labels[gr.CHAIN[0]] == gr.CHAIN[0] and labels[gr.CHAIN[2]] == gr.CHAIN[2]     # the chain fell apart: its middle is no member
    assert _same_edges(c.ix.near_edges(c.r, allowed=allowed), want_edges)
    as_ids = c.ix.graph_duplicate_groups(c.r, allowed=members)                           # the set as an id list
    assert as_ids[0].tobytes() == labels.tobytes() and as_ids[1] == info
    assert _same_edges(c.ix.near_edges(c.r, allowed=members), want_edges)
    # NaN: every member its own group; +inf: every edge between members; -1: ordinary, nothing within it here
    measured = c.want[1]["edges_measured"]
    labels, info = c.ix.graph_duplicate_groups(float("nan"))
    assert labels.tolist() == list(range(N)) and _info(info, 6)[0] == {"members": N, "groups": N, "edges_within": 0, "edges_measured": measured}
    assert c.ix.near_edges(float("nan"))[0].size == 0
    # (at +inf the model needs no distance beyond "a number": every edge between members is within)
    edges_of, any_number = (lambda i: c.ix.edges(i, 0)), (lambda own, cand: np.zeros(len(cand), np.float32))
    want_labels, want_info = graph_duplicate_groups(edges_of, N, members, any_number, float("inf"))
    labels, info = c.ix.graph_duplicate_groups(float("inf"), allowed=allowed)
    assert labels.tobytes() == want_labels.tobytes() and _info(info, -(-members.size // ROUND)) == (want_info, True)
    assert info["edges_within"] == info["edges_measured"] > 0
    src, dst, d = c.ix.near_edges(float("inf"), allowed=allowed)
    w_src, w_dst, _, _ = near_edges(edges_of, members, any_number, float("inf"))
    assert src.tolist() == w_src.tolist() and sorted(zip(src.tolist(), dst.tolist())) == sorted(zip(w_src.tolist(), w_dst.tolist()))
    same_owner = src[1:] == src[:-1]
    assert (d[1:][same_owner] >= d[:-1][same_owner]).all() and not np.isnan(d).any()     # ascending inside one owner
    labels, info = c.ix.graph_duplicate_groups(-1.0)
    assert labels.tolist() == list(range(N)) and info["edges_within"] == 0 and c.ix.near_edges(-1.0)[2].size == 0


def test_removed_ids_are_no_members():
    n = 300
    x = uniform(n, DIM, 23).copy()
    x[[10, 150, 290]] = x[10]                                             # a triple whose smallest id is removed below
    x[201] = x[200] + np.float32(0.05)
    x[202] = x[200] + np.float32(0.10)                                    # a chain 200 - 201 - 202 whose middle is removed below
    ix = _index(DIM, "sq_euclid", n)
    ix.add(x)
    r = 0.06                                                              # 20 * 0.05^2 = 0.05 < r < 20 * 0.1^2 = 0.2; the background is far above
    labels, info = ix.graph_duplicate_groups(r)
    want = _model(ix, np.arange(n), r)
    assert labels.tobytes() == want[0].tobytes() and _info(info, 1) == (want[1], True) and info["edges_within"] > 0
    ix.remove([10, 201])
    live = np.delete(np.arange(n), [10, 201])
    labels, info = ix.graph_duplicate_groups(r)
    want = _model(ix, live, r)
    assert labels.tobytes() == want[0].tobytes() and _info(info, 1) == (want[1], True)
    assert labels[[10, 201]].tolist() == [-1, -1] and labels[200] == 200 and labels[202] == 202 and info["members"] == n - 2
    assert _same_edges(ix.near_edges(r), want[2])
    assert not np.isin(ix.near_edges(float("inf"))[1], [10, 201]).any()   # a removed id is no end of any edge


# ---------------------------------------------------------------- 6. components
def test_infinite_radius_gives_the_components_of_layer_0(cases):
    c = cases("sq_euclid")
    labels, info = c.ix.graph_duplicate_groups(float("inf"))
    assert info["groups"] == int(c.ix.connected_component_counts()[0]) and info["edges_within"] == info["edges_measured"]
    assert np.unique(labels).size == info["groups"]


# ---------------------------------------------------------------- 7. small inputs, caps, the context-level calls
def test_small_inputs_and_caps():
    import hnswindex
    import importlib
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)
    none = {"members": 0, "groups": 0, "edges_within": 0, "edges_measured": 0, "launches": 0}
    empty = hnswindex.Index(DIM, "sq_euclid")
    labels, info = empty.graph_duplicate_groups(1.0)
    assert labels.size == 0 and info == none and all(a.size == 0 for a in empty.near_edges(1.0))
    one = _index(DIM, "sq_euclid", 16)
    one.add(uniform(1, DIM, 3))
    labels, info = one.graph_duplicate_groups(float("inf"))
    assert labels.tolist() == [0] and info == dict(none, members=1, groups=1) and one.near_edges(float("inf"))[0].size == 0
    two = _index(DIM, "sq_euclid", 16)
    two.add(uniform(2, DIM, 3))
    labels, info = two.graph_duplicate_groups(float("inf"), allowed=[1])  # one member of two items: nothing to measure
    assert labels.tolist() == [-1, 1] and info == dict(none, members=1, groups=1)
    labels, info = two.graph_duplicate_groups(float("inf"), allowed=np.zeros(2, bool))
    assert labels.tolist() == [-1, -1] and info == none
    labels, info = two.graph_duplicate_groups(float("inf"))
    assert labels.tolist() == [0, 0] and info == {"members": 2, "groups": 1, "edges_within": 2, "edges_measured": 2, "launches": 1}
    src, dst, d = two.near_edges(float("inf"))
    assert src.tolist() == [0, 1] and dst.tolist() == [1, 0] and d[0].tobytes() == d[1].tobytes()
    # cap below the length, cap below the result count: -1 and a message, nothing written
    out, inf = np.full(2, 7, np.int32), (ct.c_uint64 * 5)()
    assert net.lib.hnsw_mi355x_graph_duplicate_groups(two._h, 1.0, None, 0, out.ctypes.data_as(_I), 1, inf) == -1
    assert "cap = 1 is below the index's length of 2" in net.last_error() and (out == 7).all()
    a, b, dd = np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.float32)
    assert net.lib.hnsw_mi355x_near_edges_results(two._h, a.ctypes.data_as(_I), b.ctypes.data_as(_I), dd.ctypes.data_as(_F), 1) == -1
    assert "cap = 1 is below the 2 edges kept" in net.last_error() and (a == 7).all() and (b == 7).all()
    assert net.lib.hnsw_mi355x_near_edges_results(two._h, a.ctypes.data_as(_I), b.ctypes.data_as(_I), dd.ctypes.data_as(_F), 2) == 0
    assert a.tolist() == [0, 1] and b.tolist() == [1, 0]


def test_device_backend_forms_leave_the_resident_set_and_pending_results():
    import hnswindex
    n, dim, m = 900, 33, 8
    x = uniform(n, dim, 41).copy()
    x[[5, 450, 899]] = x[5]
    lists = gr.ring_lists(n)
    lists[450] = lists[450] + [5]
    lists[899] = lists[899] + [450]
    dev = hnswindex.DeviceBackend(dim, "sq_euclid", capacity=n)
    dev.upload_rows(0, x)
    with pytest.raises(RuntimeError, match="no graph committed"):
        dev.graph_edge_groups(1e-6, n)
    dev.set_graph(np.zeros(n, np.int32), gr.layers_of(lambda i, layer: lists[i], np.zeros(n, np.int32), 2 * m + 2), m)
    q = uniform(6, dim, 43)
    dev.set_queries(q)
    before = dev.exact_range_grouped(None, 3.5, np.zeros(n, np.int32), np.zeros(6, np.int32), 1)   # answered from the resident set
    pending = dev.exact_range(q[:3], 3.2)                                                          # ... and these results stay pending
    total = sum(l.size for l in pending[0])
    assert total > 0
    labels, info = dev.graph_edge_groups(1e-6, n)
    assert labels.tolist() == [5 if v in (450, 899) else v for v in range(n)]
    assert info == {"members": n, "groups": n - 2, "edges_within": 2, "edges_measured": 3 * n + 2, "launches": 1}
    src, dst, d = dev.graph_near_edges(1e-6, n)
    assert src.tolist() == [450, 899] and dst.tolist() == [5, 450] and d.tolist() == [0.0, 0.0]
    ids, dd = np.empty(total, np.int32), np.empty(total, np.float32)
    assert hnswindex.net_amd.lib.hnswdev_exact_range_results(dev._ctx, ids.ctypes.data_as(_I), dd.ctypes.data_as(_F)) == 0
    assert ids.tolist() == np.concatenate(pending[0]).tolist() and dd.tobytes() == np.concatenate(pending[1]).tobytes()
    after = dev.exact_range_grouped(None, 3.5, np.zeros(n, np.int32), np.zeros(6, np.int32), 1)
    assert all(a.tolist() == b.tolist() and u.tobytes() == v.tobytes() for a, b, u, v in zip(before[0], after[0], before[1], after[1]))
    assert sum(l.size for l in after[0]) > 0
    # rows [0, 500): 899 is no member, and the ring's edges that leave [0, 500) are no edges; an allow-set on top
    labels, info = dev.graph_edge_groups(1e-6, 500)
    inside = sum(1 for i in range(500) for j in lists[i] if j < 500)
    assert labels.shape == (500,) and labels[450] == 5 and info == {"members": 500, "groups": 499, "edges_within": 1, "edges_measured": inside, "launches": 1}
    labels, info = dev.graph_edge_groups(1e-6, 500, allowed=np.arange(1, 500))
    assert labels[0] == -1 and labels[450] == 5 and info["members"] == 499 and info["groups"] == 498
    labels, info = dev.graph_edge_groups(1e-6, 500, allowed=np.delete(np.arange(500), 5))
    assert labels[5] == -1 and labels[450] == 450 and info["groups"] == 499 and info["edges_within"] == 0
    assert dev.graph_near_edges(1e-6, 500, allowed=np.delete(np.arange(500), 5))[0].size == 0
    # the results call with a cap below what is kept
    src, dst, d = dev.graph_near_edges(1e-6, n)
    one = np.empty(1, np.int32), np.empty(1, np.int32), np.empty(1, np.float32)
    assert hnswindex.net_amd.lib.hnswdev_graph_near_edges_results(dev._ctx, one[0].ctypes.data_as(_I), one[1].ctypes.data_as(_I), one[2].ctypes.data_as(_F), 1) == -1
