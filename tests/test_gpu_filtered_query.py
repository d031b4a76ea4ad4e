"""GPU tier: filtered KnnQuery (hnsw_mi355x_knn_query_filtered / Index.knn_query(..., allowed=...)) against the plain-Python
restatement of the filtered SearchLayerQuery (tests/filtered_model.py) on graphs whose hash equals the CPU oracle's: ids and
distance bits, at the four metrics, several selectivities and a correlated mask, k below and above MinNN, the entry point
disallowed, equal distances, fewer allowed ids than the beam, nothing allowed -- and the same answers through every other
path (hand-backs, hashed visited sets, host traversal, two contexts, concurrent callers)."""
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from filtered_model import filtered_knn_batch

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 1200, 16, 8, 20


def _data(metric, n, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, DIM)).astype(np.float32) if grid else uniform(n, DIM, seed)
    return normalize_f32(x) if metric == "ucosine" else x


def _build(metric, x, m=M, **knobs):
    import hnswindex
    import oracle
    ix = hnswindex.Index(DIM, metric)
    ix.set_collection_size(N); ix.set_max_edges(m); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    ref = oracle.OracleIndex(DIM, metric, max_edges=m, min_nn=MIN_NN, collection_size=N)
    ref.add(x)
    assert ix.graph_hash() == ref.graph_hash(), metric
    return ix, ref


def _layers(ref, lv, m):
    """The oracle's graph as (counts, edges) per layer, the layout of Index.export_edges / import_graph and DeviceBackend.set_graph."""
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


def _masks(x, seed):
    rng = np.random.default_rng(seed)
    out = {f"sel{s}": rng.random(x.shape[0]) < s for s in (1.0, 0.5, 0.1, 0.02)}
    out["correlated"] = x[:, 0] < np.quantile(x[:, 0], 0.15)   # a threshold on one coordinate: allowed ids cluster in space
    return out


def _same(a, b):
    return (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            x = _data(metric, N, 1 if not grid else 2, grid)
            cache[(metric, grid)] = (x, *_build(metric, x))
        return cache[(metric, grid)]
    return get


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8"])
def test_filtered_query_is_the_reference_on_the_device(built, metric):
    x, ix, ref = built(metric)
    q = _data(metric, 12, 9)
    for name, mask in _masks(x, 3).items():
        for k in (5, 40):   # below and above MinNN
            ix.reset_stats()
            got = ix.knn_query(q, k, allowed=mask)
            st = ix.stats()
            assert st["search_launches"] >= 1 and st["launches"] == 0, (metric, name, k, st)   # the device traversal answered
            want = filtered_knn_batch(ref, x, metric, q, k, MIN_NN, mask)
            assert _same(got, want), (metric, name, k)
            assert np.isin(got[0][got[0] >= 0], np.flatnonzero(mask)).all()


def test_entry_point_disallowed_and_ties(built):
    for grid in (False, True):
        x, ix, ref = built("sq_euclid", grid)
        q = _data("sq_euclid", 16, 5, grid)
        mask = np.random.default_rng(4).random(N) < 0.5
        mask[[ref.find_entry_point(0, qi) for qi in q]] = False   # every query's layer-0 entry (the descent's answer) disallowed
        for k in (10, 30):
            assert _same(ix.knn_query(q, k, allowed=mask), filtered_knn_batch(ref, x, "sq_euclid", q, k, MIN_NN, mask)), (grid, k)


def test_lists_beyond_64_ids():
    """MaxEdges = 60 at dim 64: layer-0 lists of up to 120 ids, past the overlapped form -- the allow words are read after the
    distances there."""
    import hnswindex
    import oracle
    dim, m = 64, 60
    x, q = uniform(N, dim, 31), uniform(10, dim, 32)
    ix = hnswindex.Index(dim, "cosine")
    ix.set_collection_size(N); ix.set_max_edges(m); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    ix.add(x)
    ref = oracle.OracleIndex(dim, "cosine", max_edges=m, min_nn=MIN_NN, collection_size=N)
    ref.add(x)
    assert ix.graph_hash() == ref.graph_hash()
    assert sum(ref.edges(i, 0).size > 64 for i in range(N)) > N // 4
    for name, mask in _masks(x, 12).items():
        for k in (5, 40):
            ix.reset_stats()
            got = ix.knn_query(q, k, allowed=mask)
            st = ix.stats()
            assert st["search_launches"] >= 1 and st["launches"] == 0, (name, k, st)
            assert _same(got, filtered_knn_batch(ref, x, "cosine", q, k, MIN_NN, mask)), (name, k)


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_device_backend_knn_search_filtered(built, metric):
    """The inner boundary: a host-supplied graph, hnswdev_knn_search_filtered (DeviceBackend.knn_search(..., allowed=...))."""
    import hnswindex
    x, _, ref = built(metric)
    lv = ref.levels()
    dev = hnswindex.DeviceBackend(DIM, metric, capacity=N)
    dev.upload_rows(0, x)
    dev.set_graph(lv, _layers(ref, lv, M), M)
    q = _data(metric, 12, 14)
    for name, mask in _masks(x, 15).items():
        ids, d, flags = dev.knn_search(q, ref.entry_point, 32, 10, allowed=mask)
        assert (flags == 0).all(), name
        assert _same((ids, d), filtered_knn_batch(ref, x, metric, q, 10, 32, mask)), name
    assert dev.stats()["search_launches"] >= 5
    ids, d, flags = dev.knn_search(q, ref.entry_point, 32, 10, allowed=np.zeros(N, dtype=bool))
    assert (ids == -1).all() and np.isnan(d).all() and (flags == 0).all()
    with pytest.raises(RuntimeError, match="bad argument"):
        dev.knn_search(q, N + 5, 32, 10, allowed=mask)


def test_host_path_with_queries_sharded_over_two_contexts(built):
    """Shapes the device kernels do not fit, with set_devices(2): the queries were sharded over the contexts, the host traversal
    answers on the primary.  MaxEdges = 64 (lists of up to 128 ids), and a beam past the LDS budget on a graph that does fit."""
    import hnswindex
    import oracle
    x = _data("sq_euclid", N, 41)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=64, min_nn=MIN_NN, collection_size=N)
    ref.add(x)
    lv = ref.levels()
    ix = hnswindex.Index(DIM)
    ix.set_collection_size(N); ix.set_max_edges(64); ix.set_min_nn(MIN_NN); ix.set_devices(2)
    ix.import_graph(x, lv, ref.entry_point, _layers(ref, lv, 64))
    assert ix.graph_hash() == ref.graph_hash()
    q = _data("sq_euclid", 10, 42)
    for name, mask in _masks(x, 16).items():
        assert _same(ix.knn_query(q, 10, allowed=mask), filtered_knn_batch(ref, x, "sq_euclid", q, 10, MIN_NN, mask)), name
    x8, _, ref8 = built("sq_euclid")
    lv8 = ref8.levels()
    iy = hnswindex.Index(DIM)
    iy.set_collection_size(N); iy.set_max_edges(M); iy.set_min_nn(MIN_NN); iy.set_devices(2)
    iy.import_graph(x8, lv8, ref8.entry_point, _layers(ref8, lv8, M))
    assert iy.graph_hash() == ref8.graph_hash()
    mask = _masks(x8, 17)["sel0.5"]
    assert _same(iy.knn_query(q, 8200, allowed=mask), filtered_knn_batch(ref8, x8, "sq_euclid", q, 8200, MIN_NN, mask))


def test_fewer_allowed_than_the_beam_and_none(built):
    import oracle
    x, ix, ref = built("sq_euclid")
    q = _data("sq_euclid", 10, 6)
    allowed = np.random.default_rng(8).choice(N, 7, replace=False)
    ids, d = ix.knn_query(q, 5, allowed=allowed)          # an id list; top never fills: all of layer 0 is searched
    mask = np.zeros(N, dtype=bool)
    mask[allowed] = True
    assert _same((ids, d), filtered_knn_batch(ref, x, "sq_euclid", q, 5, MIN_NN, mask))
    srt = np.sort(allowed)
    for i in range(q.shape[0]):                          # layer 0 is connected here: brute force over the allowed rows
        bd = oracle.dist_query_rows("sq_euclid", x, q[i], srt)
        order = np.argsort(bd, kind="stable")[:5]
        assert set(ids[i].tolist()) == set(srt[order].tolist())
        assert np.sort(d[i]).tobytes() == np.sort(bd[order]).tobytes()
    for nothing in (np.zeros(N, dtype=bool), np.zeros(0, dtype=np.int32), np.array([N + 5])):
        ids, d = ix.knn_query(q, 5, allowed=nothing)
        assert (ids == -1).all() and np.isnan(d).all()


def test_all_allowed_equals_knn_query_at_100k():
    import hnswindex
    x = uniform(100_000, 128, 21)
    q = uniform(2000, 128, 22)
    ix = hnswindex.Index(128)
    ix.set_collection_size(x.shape[0])
    ix.add(x)
    for k in (10, 100):
        a = ix.knn_query(q, k)
        b = ix.knn_query(q, k, allowed=np.ones(x.shape[0], dtype=bool))
        assert _same(a, b), k


def _other_path(metric, x, ref, q, masks, monkeypatch=None, **knobs):
    import hnswindex
    ix = hnswindex.Index(DIM, metric)
    ix.set_collection_size(N); ix.set_max_edges(M); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    assert ix.graph_hash() == ref.graph_hash()
    ix.reset_stats()
    for name, mask in masks.items():
        for k in (5, 40):
            assert _same(ix.knn_query(q, k, allowed=mask), filtered_knn_batch(ref, x, metric, q, k, MIN_NN, mask)), (knobs, name, k)
    return ix.stats()


def test_forced_handbacks_give_the_same_answers(built, monkeypatch):
    x, ix, ref = built("cosine")
    q = _data("cosine", 8, 7)
    masks = {k: v for k, v in _masks(x, 5).items() if k in ("sel0.5", "sel0.02")}
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    ix.reset_stats()
    for name, mask in masks.items():
        for k in (5, 40):
            assert _same(ix.knn_query(q, k, allowed=mask), filtered_knn_batch(ref, x, "cosine", q, k, MIN_NN, mask)), (name, k)
    assert ix.stats()["search_overflows"] > 0


def _overflows(ix, contexts):
    return ix.stats()["search_overflows"] + sum(ix.stats_at(g)["search_overflows"] for g in range(1, contexts))


def test_two_contexts_with_forced_handbacks(built, monkeypatch):
    """Sharded over two contexts AND jobs handed back: the shards are gathered to the primary, where the host traversal redoes them."""
    import hnswindex
    x, ix, ref = built("cosine")
    q = _data("cosine", 24, 7)
    masks = {k: v for k, v in _masks(x, 5).items() if k in ("sel0.5", "sel0.02")}
    want = {(name, k): ix.knn_query(q, k, allowed=mask) for name, mask in masks.items() for k in (5, 40)}   # one context, nothing forced
    assert _same(want["sel0.5", 40], filtered_knn_batch(ref, x, "cosine", q, 40, MIN_NN, masks["sel0.5"]))
    two = hnswindex.Index(DIM, "cosine")
    two.set_collection_size(N); two.set_max_edges(M); two.set_min_nn(MIN_NN); two.set_insert_batch(1); two.set_devices(2)
    two.add(x)
    assert two.graph_hash() == ref.graph_hash()
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    two.reset_stats()
    for (name, k), w in want.items():
        assert _same(two.knn_query(q, k, allowed=masks[name]), w), (name, k)
    assert _overflows(two, 2) > 0 and two.stats_at(1)["search_launches"] >= 4


def test_hashed_visited_sets_host_traversal_and_two_contexts(built, monkeypatch):
    x, ix, ref = built("ucosine")
    q = _data("ucosine", 8, 11)
    masks = {k: v for k, v in _masks(x, 6).items() if k in ("sel1.0", "sel0.1", "correlated")}
    set_diag(monkeypatch, vis_hash="1")
    st = _other_path("ucosine", x, ref, q, masks)
    assert st["visited_hash_launches"] > 0
    monkeypatch.undo()
    st = _other_path("ucosine", x, ref, q, masks, set_device_traversal=False)
    assert st["search_launches"] == 0
    _other_path("ucosine", x, ref, q, masks, set_devices=2)


def test_threads_mixing_filtered_and_unfiltered_calls(built):
    x, ix, ref = built("sq_euclid")
    q = _data("sq_euclid", 24, 13)
    masks = list(_masks(x, 9).values())
    want_f = [filtered_knn_batch(ref, x, "sq_euclid", q, 10, MIN_NN, m) for m in masks]
    want_u = ref.knn_query(q, 10)
    errors = []

    def work(t):
        try:
            for r in range(6):
                i = (t + r) % len(masks)
                if (t + r) % 2:
                    assert _same(ix.knn_query(q, 10, allowed=masks[i]), want_f[i])
                else:
                    assert _same(ix.knn_query(q, 10), want_u)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
