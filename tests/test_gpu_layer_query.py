"""GPU tier: the `layer` argument of KnnQuery / RangeQuery and MultiLayerKnnQuery against the plain-Python restatement
(tests/layer_query_model.py): ids, distance bits, order and padding equal, at the four metrics (int8 against its own CPU
statement), on every layer of graphs with many layers and top layers smaller than k, with and without an allow-set, on tie-heavy
data, on graphs built here and imported from the oracle -- and the same answers through every other path (host traversal, forced
hand-backs, hashed visited sets, two contexts, the inner boundary, concurrent callers)."""
import math
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from filtered_range_model import HeapEmpty
from layer_query_model import knn_at_layer_batch, multilayer_chain, multilayer_knn_batch, range_at_layer_batch, top_layer

pytestmark = pytest.mark.gpu

MIN_NN = 5
GRAPHS = {   # many layers; the top ones hold fewer nodes than k
    "sq_euclid": dict(n=6000, dim=16, M=4, rate=1 / math.log(3)),
    "cosine": dict(n=6000, dim=24, M=8, rate=1 / math.log(4)),
    "ucosine": dict(n=3000, dim=16, M=4, rate=1 / math.log(3)),
    "sq_euclid_i8": dict(n=3000, dim=16, M=4, rate=1 / math.log(3)),
}


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric == "ucosine" else x


def _oracle(metric, x):
    import oracle
    g = GRAPHS[metric]
    ref = oracle.OracleIndex(g["dim"], metric, max_edges=g["M"], distribution_rate=g["rate"], min_nn=MIN_NN, collection_size=x.shape[0])
    ref.add(x)
    return ref


def _index(metric, n, **knobs):
    import hnswindex
    g = GRAPHS[metric]
    ix = hnswindex.Index(g["dim"], metric)
    ix.set_collection_size(n); ix.set_max_edges(g["M"]); ix.set_min_nn(MIN_NN); ix.set_distribution_rate(g["rate"]); ix.set_insert_batch(1)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    return ix


def _layers(ref, lv, m):
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


def _imported(metric, x, ref, **knobs):
    ix = _index(metric, x.shape[0], **knobs)
    lv = ref.levels()
    ix.import_graph(x, lv, ref.entry_point, _layers(ref, lv, GRAPHS[metric]["M"]))
    assert ix.graph_hash() == ref.graph_hash()
    return ix


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _same_lists(a, b):
    return all(p.tobytes() == r.tobytes() for p, r in zip(a[0] + a[1], b[0] + b[1])) and len(a[0]) == len(b[0])


@pytest.fixture(scope="module")
def built():
    """(x, product index BUILT here, oracle) per (metric, grid); the graphs are equal by hash."""
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            g = GRAPHS[metric]
            x = _data(metric, g["n"], g["dim"], 1 if not grid else 2, grid)
            ref = _oracle(metric, x)
            ix = _index(metric, g["n"])
            ix.add(x)
            assert ix.graph_hash() == ref.graph_hash(), metric
            assert ix.top_layer() == top_layer(ref) >= 4
            cache[(metric, grid)] = (x, ix, ref)
        return cache[(metric, grid)]
    return get


def _queries(metric, n, seed, grid=False):
    return _data(metric, n, GRAPHS[metric]["dim"], seed, grid)


def _masks(x, ref, q, layer, seed):
    rng = np.random.default_rng(seed)
    out = {"sel0.5": rng.random(x.shape[0]) < 0.5, "sel0.1": rng.random(x.shape[0]) < 0.1}
    no_entry = rng.random(x.shape[0]) < 0.6
    no_entry[[ref.find_entry_point(layer, qi) for qi in q]] = False   # the descent's result is not allowed
    out["entry_excluded"] = no_entry
    return out


def _k_beyond_top(ref):
    lv = ref.levels()
    return int((lv >= top_layer(ref)).sum()) + 7


@pytest.mark.parametrize("metric", list(GRAPHS))
def test_knn_query_on_every_layer(built, metric):
    x, ix, ref = built(metric)
    q = _queries(metric, 8, 9)
    top = ix.top_layer()
    for layer in range(top + 1):
        for k in (1, 2, 10, _k_beyond_top(ref)):
            got = ix.knn_query(q, k, layer=layer)
            assert _same(got, knn_at_layer_batch(ref, x, metric, q, k, MIN_NN, layer)), (metric, layer, k)
        for name, mask in _masks(x, ref, q, layer, 3 + layer).items():
            for k in (2, 10):
                ix.reset_stats()
                got = ix.knn_query(q, k, allowed=mask, layer=layer)
                st = ix.stats()
                assert st["search_launches"] >= 1 and st["launches"] == 0, (metric, layer, name, st)   # the device traversal answered
                assert _same(got, knn_at_layer_batch(ref, x, metric, q, k, MIN_NN, layer, mask)), (metric, layer, name, k)


@pytest.mark.parametrize("metric", list(GRAPHS))
def test_range_query_on_every_layer(built, metric):
    x, ix, ref = built(metric)
    q = _queries(metric, 8, 10)
    top = ix.top_layer()
    for layer in range(top + 1):
        d = knn_at_layer_batch(ref, x, metric, q, 10, MIN_NN, layer)[1]
        fin = d[np.isfinite(d)]
        for radius in (float(np.median(fin)), float(fin.max())):
            ix.reset_stats()
            got = ix.range_query(q, radius, layer=layer)
            st = ix.stats()
            assert st["range_launches"] >= 1 and st["launches"] == 0, (metric, layer, st)
            assert _same_lists(got, range_at_layer_batch(ref, x, metric, q, radius, layer)), (metric, layer, radius)
            for name, mask in _masks(x, ref, q, layer, 5 + layer).items():
                got = ix.range_query(q, radius, allowed=mask, layer=layer)
                assert _same_lists(got, range_at_layer_batch(ref, x, metric, q, radius, layer, mask)), (metric, layer, radius, name)


def _windows(top):
    return [(None, 0), (top, 0), (top - 1, 1), (top - 2, top - 2), (top + 5, 0), (None, top + 1), (0, 0), (-1, 0)]


@pytest.mark.parametrize("metric", list(GRAPHS))
def test_multilayer_is_the_reference_on_the_device(built, metric):
    x, ix, ref = built(metric)
    q = _queries(metric, 10, 11)
    top = ix.top_layer()
    for k in (1, 2, 10, _k_beyond_top(ref)):
        for hi, lo in _windows(top):
            ix.reset_stats()
            got = ix.multilayer_knn_query(q, k, hi, lo)
            want = multilayer_knn_batch(ref, q, k, hi, lo)
            assert _same(got, want), (metric, k, hi, lo)
            st = ix.stats()
            runs = k > 1 and hi != -1 and lo <= min(top, top if hi is None else hi)
            if runs and metric != "sq_euclid_i8":   # uniform float data: no NaN / -0, and a beam this small cannot outgrow the spill area
                assert st["multilayer_jobs"] == q.shape[0] and st["multilayer_handbacks"] == 0 and st["launches"] == 0, (metric, k, hi, lo, st)
            if runs and metric == "sq_euclid_i8":
                assert st["multilayer_jobs"] == q.shape[0], st
    assert got[0].shape == (q.shape[0], 0, _k_beyond_top(ref) - 1)   # (the last window: max_layer == -1)


def test_multilayer_evaluations_are_the_oracles(built, monkeypatch):
    """The launch keeps visited sets: the kernel measures exactly the rows the reference's chain does."""
    x, ix, ref = built("sq_euclid")
    q = _queries("sq_euclid", 16, 12)
    ref.reset_n_eval()
    for qi in q:
        multilayer_chain(ref, qi, 10)
    want = ref.n_eval
    ix.reset_stats()
    ix.multilayer_knn_query(q, 10)
    st = ix.stats()
    assert st["multilayer_launches"] == 1 and st["search_evals"] == want, (st["search_evals"], want)


def test_argument_errors_and_an_empty_index(built):
    import hnswindex
    x, ix, ref = built("sq_euclid")
    q = _queries("sq_euclid", 3, 13)
    top = ix.top_layer()
    for bad in (-1, top + 1):
        with pytest.raises(RuntimeError, match="layer"):
            ix.knn_query(q, 3, layer=bad)
        with pytest.raises(RuntimeError, match="layer"):
            ix.knn_query(q, 3, allowed=np.ones(x.shape[0], bool), layer=bad)
        with pytest.raises(RuntimeError, match="layer"):
            ix.range_query(q, 1.0, layer=bad)
    for bad in ((-2, 0), (top, -1)):
        with pytest.raises(RuntimeError, match="max_layer"):
            ix.multilayer_knn_query(q, 3, *bad)
    ids, d = ix.knn_query(q, 0 + 1, layer=top)
    assert ids.shape == (3, 1)
    # layers_cap too small: an error that names the needed value
    import ctypes as ct
    net = hnswindex.net_amd
    out_i = np.zeros((3, top, 2), np.int32)
    out_d = np.zeros((3, top, 2), np.float32)
    rc = net.lib.hnsw_mi355x_multilayer_knn_query(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), 3, q.shape[1], 3, 2 ** 31 - 1, 0, top,
                                                  out_i.ctypes.data_as(ct.POINTER(ct.c_int)), out_d.ctypes.data_as(ct.POINTER(ct.c_float)))
    assert rc == -1 and str(top + 1) in net.last_error()
    # a roomier layers_cap: rows at or above the returned count are not written
    out_i = np.full((3, top + 3, 2), 77, np.int32)
    out_d = np.full((3, top + 3, 2), 77, np.float32)
    rc = net.lib.hnsw_mi355x_multilayer_knn_query(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), 3, q.shape[1], 3, 2 ** 31 - 1, 0, top + 3,
                                                  out_i.ctypes.data_as(ct.POINTER(ct.c_int)), out_d.ctypes.data_as(ct.POINTER(ct.c_float)))
    assert rc == top + 1 and (out_i[:, top + 1:] == 77).all() and (out_d[:, top + 1:] == 77).all()
    assert _same((np.ascontiguousarray(out_i[:, :top + 1]), np.ascontiguousarray(out_d[:, :top + 1])), multilayer_knn_batch(ref, q, 3))
    # k == 1: nothing is written, the count comes back
    rc = net.lib.hnsw_mi355x_multilayer_knn_query(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), 3, q.shape[1], 1, 2 ** 31 - 1, 0, top + 3, None, None)
    assert rc == top + 1
    q4 = np.zeros((2, 4), np.float32)
    for with_handle in (False, True):   # nothing added yet: no native handle; and a native index that holds nothing
        empty = hnswindex.Index(4)
        if with_handle:
            empty._initialize()
        ids, d = empty.knn_query(q4, 3, layer=9)
        assert (ids == -1).all() and np.isnan(d).all()
        assert all(a.size == 0 for a in empty.range_query(q4, 1.0, layer=9)[0])
        assert empty.multilayer_knn_query(q4, 3)[0].shape == (2, 0, 2)
        assert empty.top_layer() == -1


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_tie_heavy_grid_data(built, metric):
    """Integer grid rows: many equal distances, so heap layout decides ids and the chain's next entry."""
    x, ix, ref = built(metric, True)
    q = _queries(metric, 8, 14, True)
    top = ix.top_layer()
    for layer in range(top + 1):
        mask = np.random.default_rng(layer).random(x.shape[0]) < 0.5
        for k in (2, 10):
            assert _same(ix.knn_query(q, k, layer=layer), knn_at_layer_batch(ref, x, metric, q, k, MIN_NN, layer)), (layer, k)
            assert _same(ix.knn_query(q, k, allowed=mask, layer=layer), knn_at_layer_batch(ref, x, metric, q, k, MIN_NN, layer, mask)), (layer, k)
        d = knn_at_layer_batch(ref, x, metric, q, 10, MIN_NN, layer)[1]
        radius = float(np.median(d[np.isfinite(d)]))
        assert _same_lists(ix.range_query(q, radius, layer=layer), range_at_layer_batch(ref, x, metric, q, radius, layer)), layer
        assert _same_lists(ix.range_query(q, radius, allowed=mask, layer=layer), range_at_layer_batch(ref, x, metric, q, radius, layer, mask)), layer
    for k in (2, 10, 40):
        for hi, lo in ((None, 0), (top - 1, 1)):
            assert _same(ix.multilayer_knn_query(q, k, hi, lo), multilayer_knn_batch(ref, q, k, hi, lo)), (k, hi, lo)


def _every_call(ix, ref, x, metric, q, what=""):
    top = top_layer(ref)
    for layer in (0, 1, top // 2, top):
        mask = np.random.default_rng(40 + layer).random(x.shape[0]) < 0.3
        for k in (2, 10):
            assert _same(ix.knn_query(q, k, layer=layer), knn_at_layer_batch(ref, x, metric, q, k, MIN_NN, layer)), (what, layer, k)
            assert _same(ix.knn_query(q, k, allowed=mask, layer=layer), knn_at_layer_batch(ref, x, metric, q, k, MIN_NN, layer, mask)), (what, layer, k)
        d = knn_at_layer_batch(ref, x, metric, q, 10, MIN_NN, layer)[1]
        radius = float(np.median(d[np.isfinite(d)]))
        assert _same_lists(ix.range_query(q, radius, layer=layer), range_at_layer_batch(ref, x, metric, q, radius, layer)), (what, layer)
        assert _same_lists(ix.range_query(q, radius, allowed=mask, layer=layer), range_at_layer_batch(ref, x, metric, q, radius, layer, mask)), (what, layer)
    for k in (1, 2, 10, 40):
        for hi, lo in ((None, 0), (top - 1, 1), (top + 3, top + 1)):
            assert _same(ix.multilayer_knn_query(q, k, hi, lo), multilayer_knn_batch(ref, q, k, hi, lo)), (what, k, hi, lo)


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_imported_graphs(built, metric):
    x, _, ref = built(metric)
    ix = _imported(metric, x, ref)
    _every_call(ix, ref, x, metric, _queries(metric, 6, 15), "imported")


def test_host_traversal(built):
    x, _, ref = built("cosine")
    ix = _imported("cosine", x, ref, set_device_traversal=False)
    ix.reset_stats()
    _every_call(ix, ref, x, "cosine", _queries("cosine", 6, 16), "host")
    st = ix.stats()
    assert st["search_launches"] == 0 and st["multilayer_jobs"] == 0 and st["launches"] > 0


def test_forced_handbacks_give_the_same_answers(built, monkeypatch):
    x, ix, ref = built("cosine")
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    ix.reset_stats()
    _every_call(ix, ref, x, "cosine", _queries("cosine", 6, 17), "handbacks")
    st = ix.stats()
    assert st["multilayer_handbacks"] > 0 and st["search_overflows"] > 0, st


def test_two_contexts_with_forced_handbacks(built, monkeypatch):
    """No filter at layer >= 1, sharded over two contexts AND jobs handed back: the shards are gathered to the primary, where the host
    traversal redoes them."""
    x, ix, ref = built("cosine", True)    # the grid data: without a filter a beam of 40 outgrows the forced caps on tie-heavy data only
    q = _queries("cosine", 24, 19, True)
    layers = (1, top_layer(ref) // 2)
    want = {(layer, k): ix.knn_query(q, k, layer=layer) for layer in layers for k in (5, 40)}   # one context, nothing forced
    assert _same(want[1, 40], knn_at_layer_batch(ref, x, "cosine", q, 40, MIN_NN, 1))
    two = _imported("cosine", x, ref, set_devices=2)
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    two.reset_stats()
    for (layer, k), w in want.items():
        assert _same(two.knn_query(q, k, layer=layer), w), (layer, k)
    assert two.stats()["search_overflows"] + two.stats_at(1)["search_overflows"] > 0
    assert two.stats_at(1)["search_launches"] >= 4


def test_hashed_visited_sets_and_two_contexts(built, monkeypatch):
    x, _, ref = built("sq_euclid")
    q = _queries("sq_euclid", 6, 18)
    set_diag(monkeypatch, vis_hash="1")
    ix = _imported("sq_euclid", x, ref)
    ix.reset_stats()
    _every_call(ix, ref, x, "sq_euclid", q, "vis_hash")
    st = ix.stats()
    assert st["visited_hash_launches"] > 0 and st["multilayer_jobs"] > 0 and st["multilayer_handbacks"] == 0, st
    monkeypatch.undo()
    _every_call(_imported("sq_euclid", x, ref, set_devices=2), ref, x, "sq_euclid", q, "two contexts")


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_device_backend_directly(built, metric):
    """The inner boundary: a host-supplied graph, hnswdev_*_at_layer and hnswdev_multilayer_search."""
    import hnswindex
    x, _, ref = built(metric)
    g = GRAPHS[metric]
    lv = ref.levels()
    dev = hnswindex.DeviceBackend(g["dim"], metric, capacity=x.shape[0])
    dev.upload_rows(0, x)
    dev.set_graph(lv, _layers(ref, lv, g["M"]), g["M"])
    q = _queries(metric, 8, 19)
    top, ep = top_layer(ref), ref.entry_point
    for layer in (1, top // 2, top):
        mask = np.random.default_rng(60 + layer).random(x.shape[0]) < 0.4
        for m in (None, mask):
            ids, d, flags = dev.knn_search(q, ep, 16, 10, allowed=m, layer=layer)
            assert (flags == 0).all()
            assert _same((ids, d), knn_at_layer_batch(ref, x, metric, q, 10, 16, layer, m)), (layer, m is None)
            dd = knn_at_layer_batch(ref, x, metric, q, 10, MIN_NN, layer)[1]
            radius = float(np.median(dd[np.isfinite(dd)]))
            rids, rd, rflags = dev.range_search(q, ep, radius, allowed=m, layer=layer)
            assert (rflags == 0).all()
            assert _same_lists((list(rids), list(rd)), range_at_layer_batch(ref, x, metric, q, radius, layer, m)), (layer, m is None)
    for k in (2, 10):
        for hi, lo in ((None, 0), (top - 1, 1), (top + 2, 0)):
            ids, d, flags = dev.multilayer_search(q, ep, k, hi, lo)
            assert (flags == 0).all()
            assert _same((ids, d), multilayer_knn_batch(ref, q, k, hi, lo)), (k, hi, lo)
    st = dev.stats()
    assert st["multilayer_jobs"] == 6 * q.shape[0] and st["multilayer_handbacks"] == 0
    with pytest.raises(RuntimeError, match="layer"):
        dev.knn_search(q, ep, 16, 10, layer=top + 1)
    with pytest.raises(RuntimeError, match="layer"):
        dev.range_search(q, ep, 1.0, layer=top + 1)
    with pytest.raises(RuntimeError, match="layers_cap"):
        dev.multilayer_search(q, ep, 3, None, 0, layers_cap=top)


def test_filtered_range_below_zero_fails_like_the_reference(built):
    """range < 0 on cosine distances at an upper layer: the empty-heap rule holds there too."""
    x, ix, ref = built("cosine")
    q = _queries("cosine", 8, 20)
    layer = 1
    mask = np.zeros(x.shape[0], bool)
    try:
        want = range_at_layer_batch(ref, x, "cosine", q, -0.5, layer, mask)
    except HeapEmpty:
        want = None
    if want is None:
        with pytest.raises(RuntimeError, match="Heap is empty"):
            ix.range_query(q, -0.5, allowed=mask, layer=layer)
    else:
        assert _same_lists(ix.range_query(q, -0.5, allowed=mask, layer=layer), want)


def test_threads_mixing_layer_multilayer_and_plain_calls(built):
    x, ix, ref = built("sq_euclid")
    q = _queries("sq_euclid", 16, 21)
    top = ix.top_layer()
    mask = np.random.default_rng(9).random(x.shape[0]) < 0.4
    want_plain = ref.knn_query(q, 10)
    want_layer = knn_at_layer_batch(ref, x, "sq_euclid", q, 10, MIN_NN, 2)
    want_filtered = knn_at_layer_batch(ref, x, "sq_euclid", q, 10, MIN_NN, 1, mask)
    want_multi = multilayer_knn_batch(ref, q, 10)
    want_range = range_at_layer_batch(ref, x, "sq_euclid", q, 0.8, 1)
    errors = []

    def work(t):
        try:
            for r in range(5):
                c = (t + r) % 5
                if c == 0:
                    assert _same(ix.knn_query(q, 10), want_plain)
                elif c == 1:
                    assert _same(ix.knn_query(q, 10, layer=2), want_layer)
                elif c == 2:
                    assert _same(ix.knn_query(q, 10, allowed=mask, layer=1), want_filtered)
                elif c == 3:
                    assert _same(ix.multilayer_knn_query(q, 10), want_multi)
                else:
                    assert _same_lists(ix.range_query(q, 0.8, layer=1), want_range)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert top >= 4


def test_layer_zero_through_the_new_entry_points_at_100k():
    """layer = 0 through hnsw_mi355x_*_at_layer equals hnsw_knn_query / hnsw_range_query bit for bit."""
    import ctypes as ct
    import hnswindex
    net = hnswindex.net_amd
    x = uniform(100_000, 128, 21)
    q = uniform(2000, 128, 22)
    ix = hnswindex.Index(128)
    ix.set_collection_size(x.shape[0])
    ix.add(x)
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    for k in (10, 100):
        a = ix.knn_query(q, k)
        ids = np.empty((q.shape[0], k), np.int32)
        d = np.empty((q.shape[0], k), np.float32)
        assert net.lib.hnsw_mi355x_knn_query_at_layer(ix._h, q.ctypes.data_as(F), q.shape[0], 128, k, 0, None, 0, ids.ctypes.data_as(I), d.ctypes.data_as(F)) == 0
        assert _same(a, (ids, d)), k
    n = 256
    radius = float(np.median(ix.knn_query(q[:n], 20)[1][:, -1]))
    a = ix.range_query(q[:n], radius)
    pi, pd, cnt = (ct.c_void_p * n)(), (ct.c_void_p * n)(), (ct.c_int * n)()
    assert net.lib.hnsw_mi355x_range_query_at_layer(ix._h, q.ctypes.data_as(F), n, 128, radius, 0, None, 0, pi, pd, cnt) == 0
    try:
        for i in range(n):
            m = cnt[i]
            assert m == a[0][i].size
            if m:
                assert np.ctypeslib.as_array(ct.cast(pi[i], I), (m,)).tobytes() == a[0][i].tobytes()
                assert np.ctypeslib.as_array(ct.cast(pd[i], F), (m,)).tobytes() == a[1][i].tobytes()
    finally:
        net.lib.hnsw_free_results(pi, pd, n)
    assert ix.top_layer() >= 1
    b = ix.knn_query(q[:64], 10, layer=1)
    lv = ix.levels()
    assert (lv[b[0][b[0] >= 0]] >= 1).all()
