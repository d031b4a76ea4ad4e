"""CPU tier: the `layer` argument of KnnQuery / RangeQuery and MultiLayerKnnQuery.  The plain-Python restatement
(tests/layer_query_model.py) pinned to the oracle -- at layer 0 to OracleIndex.knn_query / range_query and to the layer-0 models,
above it to the direct composition of OracleIndex.find_entry_point and OracleIndex.search_layer -- and the new symbols of the
header and the library."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from common import normalize_f32, uniform
from filtered_model import filtered_knn_batch
from filtered_range_model import filtered_range_batch
from layer_query_model import (LayerOutOfRange, knn_at_layer, knn_at_layer_batch, multilayer_chain, multilayer_knn, multilayer_knn_batch,
                               range_at_layer, range_at_layer_batch, stable_by_dist, top_layer)

ROOT = Path(__file__).resolve().parent.parent

NEW_INDEX_SYMBOLS = ("hnsw_mi355x_knn_query_at_layer", "hnsw_mi355x_range_query_at_layer", "hnsw_mi355x_multilayer_knn_query")
NEW_CONTEXT_SYMBOLS = ("hnswdev_knn_search_at_layer", "hnswdev_range_search_at_layer", "hnswdev_multilayer_search")


@pytest.fixture(scope="module")
def net():
    import hnswindex
    return hnswindex.net_amd


def test_new_symbols_are_declared_and_exported(net):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)
    for s in NEW_INDEX_SYMBOLS + NEW_CONTEXT_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert hasattr(net.lib, s), s
    for f in ("multilayer_launches", "multilayer_jobs", "multilayer_handbacks"):
        assert re.search(r"\b" + f + r"\b", text), f
    names = [f[0] for f in net.bindings.Stats._fields_]
    assert names[-3:] == ["multilayer_launches", "multilayer_jobs", "multilayer_handbacks"]   # appended at the end only


def test_null_handles_follow_the_existing_rule(net):
    """Null handle: 0 for the index calls (the hnsw_knn_query rule), -1 for the context calls (the hnswdev_* rule)."""
    import ctypes as ct
    lib = net.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), dtype=np.float32)
    ids = np.zeros((2, 6), dtype=np.int32)
    d = np.zeros((2, 6), dtype=np.float32)
    w = np.ones(1, dtype=np.uint32)
    pp = (ct.c_void_p * 2)()
    cnt = (ct.c_int * 2)()
    vp, ip, dp, wp = v.ctypes.data_as(F), ids.ctypes.data_as(I), d.ctypes.data_as(F), w.ctypes.data_as(U)
    assert lib.hnsw_mi355x_knn_query_at_layer(None, vp, 2, 4, 3, 1, wp, 32, ip, dp) == 0
    assert lib.hnsw_mi355x_knn_query_at_layer(None, vp, 2, 4, 3, 1, None, 0, ip, dp) == 0
    assert lib.hnsw_mi355x_range_query_at_layer(None, vp, 2, 4, 1.0, 1, None, 0, pp, pp, cnt) == 0
    assert lib.hnsw_mi355x_multilayer_knn_query(None, vp, 2, 4, 3, 5, 0, 3, ip, dp) == 0
    assert lib.hnswdev_knn_search_at_layer(None, vp, 2, 0, 3, 3, 1, None, 0, ip, dp, ip) == -1
    assert lib.hnswdev_range_search_at_layer(None, vp, 2, 0, 1.0, 1, None, 0, ip, ip) == -1
    assert lib.hnswdev_multilayer_search(None, vp, 2, 0, 3, 5, 0, 3, ip, dp, ip) == -1


def test_python_surface_takes_the_layer(net):
    import inspect
    assert inspect.signature(net.Index.knn_query).parameters["layer"].default == 0
    assert inspect.signature(net.Index.range_query).parameters["layer"].default == 0
    sig = inspect.signature(net.Index.multilayer_knn_query)
    assert sig.parameters["max_layer"].default is None and sig.parameters["min_layer"].default == 0
    assert hasattr(net.Index, "top_layer")
    assert inspect.signature(net.DeviceBackend.knn_search).parameters["layer"].default == 0
    assert inspect.signature(net.DeviceBackend.range_search).parameters["layer"].default == 0
    assert hasattr(net.DeviceBackend, "multilayer_search")


# graphs with many layers, the top ones holding fewer nodes than k
GRAPHS = {
    "sq_m4": dict(metric="sq_euclid", n=1500, dim=16, M=4, rate=1 / math.log(3)),
    "cos_m8": dict(metric="cosine", n=1500, dim=24, M=8, rate=1 / math.log(4)),
    "ucos_m4": dict(metric="ucosine", n=1000, dim=12, M=4, rate=1 / math.log(3)),
    "i8_m4": dict(metric="sq_euclid_i8", n=1000, dim=16, M=4, rate=1 / math.log(3)),
}
MIN_NN = 5


def _data(metric, kind, n, dim, seed):
    if kind == "grid":   # integer grid: many equal distances (heap layout decides ids)
        x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32)
    else:
        x = uniform(n, dim, seed)
    return normalize_f32(x) if metric == "ucosine" else x


@pytest.fixture(scope="module", params=[(g, kind) for g in GRAPHS for kind in ("random", "grid")], ids=lambda p: f"{p[0]}-{p[1]}")
def built(request):
    import oracle
    name, kind = request.param
    g = GRAPHS[name]
    x = _data(g["metric"], kind, g["n"], g["dim"], 21)
    q = _data(g["metric"], kind, 12, g["dim"], 22)
    ix = oracle.OracleIndex(g["dim"], g["metric"], max_edges=g["M"], distribution_rate=g["rate"], min_nn=MIN_NN, max_candidates=30,
                            collection_size=g["n"])
    ix.add(x)
    assert top_layer(ix) >= 3, "the case needs several layers"
    return g["metric"], ix, x, q


def test_layer_zero_is_the_oracle_and_the_layer_zero_models(built):
    metric, ix, x, q = built
    mask = np.random.default_rng(5).random(x.shape[0]) < 0.4
    for k in (1, 3, 10):
        want = ix.knn_query(q, k)
        got = knn_at_layer_batch(ix, x, metric, q, k, MIN_NN, 0, None)
        assert (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()
        want = filtered_knn_batch(ix, x, metric, q, k, MIN_NN, mask)
        got = knn_at_layer_batch(ix, x, metric, q, k, MIN_NN, 0, mask)
        assert (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()
    d0 = ix.knn_query(q, 10)[1]
    radius = float(np.median(d0[:, 5]))
    want = ix.range_query(q, radius)
    got = range_at_layer_batch(ix, x, metric, q, radius, 0, None)
    for a, b in zip(want[0] + want[1], got[0] + got[1]):
        assert a.tobytes() == b.tobytes()
    want = filtered_range_batch(ix, x, metric, q, radius, mask)
    got = range_at_layer_batch(ix, x, metric, q, radius, 0, mask)
    for a, b in zip(want[0] + want[1], got[0] + got[1]):
        assert a.tobytes() == b.tobytes()


def test_upper_layers_are_the_oracle_composition(built):
    """Unfiltered, KnnQuery(layer) = stable OrderBy of SearchLayer(FindEntryPoint(layer), layer, max(MinNN, k)), first k."""
    metric, ix, x, q = built
    top = top_layer(ix)
    for layer in range(1, top + 1):
        for k in (1, 2, 10, 40):
            for qi in range(q.shape[0]):
                ep = ix.find_entry_point(layer, q[qi])
                ids, ds = ix.search_layer(ep, layer, max(MIN_NN, k), q[qi])
                ordered = stable_by_dist(list(zip(ids.tolist(), ds.tolist())))[:k]
                got_ids, got_d = knn_at_layer(ix, x, metric, q[qi], k, MIN_NN, layer)
                assert got_ids[:len(ordered)].tolist() == [i for i, _ in ordered], (layer, k, qi)
                assert got_d[:len(ordered)].tobytes() == np.array([d for _, d in ordered], dtype=np.float32).tobytes()
                assert (got_ids[len(ordered):] == -1).all() and np.isnan(got_d[len(ordered):]).all()


def test_results_live_on_the_layer(built):
    metric, ix, x, q = built
    top = top_layer(ix)
    mask = np.random.default_rng(6).random(x.shape[0]) < 0.5
    levels = ix.levels()
    for layer in range(0, top + 1):
        for m in (None, mask):
            ids, _ = knn_at_layer_batch(ix, x, metric, q, 10, MIN_NN, layer, m)
            live = ids[ids >= 0]
            assert (levels[live] >= layer).all()
            if m is not None:
                assert m[live].all()
            rid, _ = range_at_layer_batch(ix, x, metric, q, 1e30, layer, m)   # everything the layer's component holds
            for r in rid:
                assert (levels[r] >= layer).all()
                if m is not None:
                    assert m[r].all()
    on_top = int((levels >= top).sum())
    ids, d = knn_at_layer_batch(ix, x, metric, q, on_top + 3, MIN_NN, top, None)
    assert ((ids >= 0).sum(axis=1) <= on_top).all() and (ids[:, on_top:] == -1).all() and np.isnan(d[:, on_top:]).all()


def test_multilayer_is_the_chain_of_search_layers(built):
    """[chain entry] + result[layer] is the stably ordered search_layer output of each step, entered at the step before's nearest."""
    metric, ix, x, q = built
    top = top_layer(ix)
    for k in (1, 2, 10, 40):
        for qi in range(q.shape[0]):
            ids, d = multilayer_knn(ix, q[qi], k)
            assert ids.shape == (top + 1, k - 1)
            ep = ix.entry_point
            for layer in range(top, -1, -1):
                sid, sd = ix.search_layer(ep, layer, k, q[qi])
                ordered = stable_by_dist(list(zip(sid.tolist(), sd.tolist())))
                rest = ordered[1:]
                assert ids[layer, :len(rest)].tolist() == [i for i, _ in rest], (k, qi, layer)
                assert d[layer, :len(rest)].tobytes() == np.array([dd for _, dd in rest], dtype=np.float32).tobytes()
                assert (ids[layer, len(rest):] == -1).all() and np.isnan(d[layer, len(rest):]).all()
                ep = ordered[0][0]


def test_multilayer_windows_and_edge_cases(built):
    metric, ix, x, q = built
    top = top_layer(ix)
    full_ids, full_d = multilayer_knn_batch(ix, q, 6)
    # max_layer above the top layer: the top layer
    ids, d = multilayer_knn_batch(ix, q, 6, top + 7, 0)
    assert ids.tobytes() == full_ids.tobytes() and d.tobytes() == full_d.tobytes()
    # a middle window: the first step enters where FindEntryPointQuery(max_layer) arrives; slots below min_layer stay empty
    hi, lo = top - 1, 1
    ids, d = multilayer_knn_batch(ix, q, 6, hi, lo)
    assert ids.shape == (q.shape[0], hi + 1, 5)
    assert (ids[:, :lo] == -1).all() and np.isnan(d[:, :lo]).all()
    for qi in range(q.shape[0]):
        nslots, steps = multilayer_chain(ix, q[qi], 6, hi, lo)
        assert nslots == hi + 1 and [s[0] for s in steps] == list(range(hi, lo - 1, -1))
        assert steps[0][1] == ix.find_entry_point(hi, q[qi])
        for (_, _, ordered), (_, nxt, _) in zip(steps, steps[1:]):
            assert nxt == ordered[0][0]
    # min_layer above the last slot: nothing runs, every slot empty
    ids, d = multilayer_knn_batch(ix, q, 6, None, top + 1)
    assert ids.shape == (q.shape[0], top + 1, 5) and (ids == -1).all() and np.isnan(d).all()
    # max_layer == -1: an empty array; k == 1: empty lists, the chain still runs; k < 1: empty
    assert multilayer_knn(ix, q[0], 6, -1, 0)[0].shape == (0, 5)
    assert multilayer_knn(ix, q[0], 1)[0].shape == (top + 1, 0)
    assert len(multilayer_chain(ix, q[0], 1)[1]) == top + 1
    assert multilayer_knn(ix, q[0], 0)[0].shape[0] == 0
    for bad in ((-2, 0), (top, -1)):
        with pytest.raises(LayerOutOfRange):
            multilayer_knn(ix, q[0], 6, *bad)
    for bad in (-1, top + 1):
        with pytest.raises(LayerOutOfRange):
            knn_at_layer(ix, x, metric, q[0], 3, MIN_NN, bad)
        with pytest.raises(LayerOutOfRange):
            range_at_layer(ix, x, metric, q[0], 1.0, bad)
    # k < 1 returns before `layer` is looked at
    assert knn_at_layer(ix, x, metric, q[0], 0, MIN_NN, top + 5)[0].shape == (0,)


def test_an_empty_index_answers_whatever_the_layer():
    import oracle
    ix = oracle.OracleIndex(4)
    q = np.zeros(4, dtype=np.float32)
    x = np.zeros((0, 4), dtype=np.float32)
    ids, d = knn_at_layer(ix, x, "sq_euclid", q, 3, MIN_NN, 9)
    assert (ids == -1).all() and np.isnan(d).all()
    assert range_at_layer(ix, x, "sq_euclid", q, 1.0, 9)[0].size == 0
    assert multilayer_knn(ix, q, 3)[0].shape == (0, 2)
