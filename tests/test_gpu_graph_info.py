"""GPU tier: HNSWIndex.GetInfo / GetConnectedComponentCounts computed on the device from the graph mirror (hnsw_mi355x_get_info,
hnsw_mi355x_connected_component_counts, hnswdev_graph_info, hnswdev_graph_components).  Every expectation comes from
the numpy restatement tests/graph_info_model.py, which the CPU tier pins to the oracle; nothing here is compared with itself."""
import ctypes as ct

import numpy as np
import pytest

import graph_info_model as gm
import refinputs
from common import uniform

pytestmark = pytest.mark.gpu

INT_FIELDS = gm.FIELDS[:8]


def _same(got, want, where=""):
    """One layer: the integer fields equal, the two averages bit for bit."""
    for f in INT_FIELDS:
        assert got[f] == want[f], (where, f, got, want)
    for f in ("avg_out_edges", "avg_in_edges"):
        assert np.float64(got[f]).tobytes() == np.float64(want[f]).tobytes(), (where, f, got, want)


# ---------------------------------------------------------------- hand-made graphs through DeviceBackend.set_graph
def _backend(n, max_edges, levels, layer_edges):
    import hnswindex
    dev = hnswindex.DeviceBackend(4, "sq_euclid", capacity=max(n, 1))
    dev.upload_rows(0, np.zeros((n, 4), np.float32))     # graph_commit needs n rows
    dev.set_graph(levels, layer_edges, max_edges)
    return dev


def _random_graph(n, max_edges, seed):
    """Levels with a top of 3 (n >= 2) and, per layer, lists among the layer's members: empty ones, full ones of MaxEdges + 1
    entries (2M + 1 on layer 0, M + 1 above), a self-loop, duplicates."""
    rng = np.random.default_rng(seed)
    levels = np.minimum(rng.geometric(0.6, n) - 1, 3).astype(np.int32)
    levels[rng.integers(n)] = 3 if n >= 2 else 2
    stride = 2 * max_edges + 2
    layer_edges = []
    for layer in range(int(levels.max()) + 1):
        mem = np.nonzero(levels >= layer)[0]
        full = (2 * max_edges if layer == 0 else max_edges) + 1
        counts = np.full(n, -1, np.int32)
        edges = np.zeros((n, stride), np.int32)
        for j, v in enumerate(mem):
            kind = rng.random()
            c = 0 if kind < 0.25 else full if kind < 0.5 else int(rng.integers(0, full + 1))
            if j == 0:
                c = max(c, 1)
            counts[v] = c
            edges[v, :c] = rng.choice(mem, c)
            if j == 0:
                edges[v, 0] = v   # a self-loop
        layer_edges.append((counts, edges))
    return levels, layer_edges


def _check_backend(dev, levels, layer_edges, live, with_in_edges=True):
    """Every layer of a committed graph against the model; returns the model's entry count for the two passes."""
    read = 0
    mask = live
    if live is not None and np.asarray(live).dtype != np.bool_:     # an id list: the model takes the mask
        mask = np.zeros(levels.size, bool)
        mask[np.asarray(live, np.int64)] = True
    for layer, (counts, edges) in enumerate(layer_edges):
        _same(dev.graph_info(layer, live=live, with_in_edges=with_in_edges), gm.layer_info(levels, mask, layer, counts, edges, with_in_edges), layer)
        assert dev.graph_components(layer, live=live) == gm.components(levels, mask, layer, counts, edges), layer
        read += 2 * gm.entries(levels, mask, layer, counts, edges)
    return read


@pytest.mark.parametrize("max_edges", [4, 15, 16])      # layer-0 strides 10, 32 and 34: a wave's flat scan starts mid-list, is exactly two lists, ends mid-list
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_hand_made_graphs_match_the_model(n, max_edges):
    levels, layer_edges = _random_graph(n, max_edges, 1000 * n + max_edges)
    assert len(layer_edges) >= 3
    dev = _backend(n, max_edges, levels, layer_edges)
    dev.reset_stats()
    read = _check_backend(dev, levels, layer_edges, None)
    c = dev.graph_info_counters()
    assert c["entries"] == read and c["info_layers"] == c["component_layers"] == len(layer_edges) and c["launches"] >= 4 * len(layer_edges)
    # a live set: edges that it invalidates stay in the out-degrees and vanish from in-degrees and connectivity; members of every
    # layer change, nodes of level 0 (upper[v] == -1) never reach an upper layer's pool
    live = np.random.default_rng(n + max_edges).random(n) < 0.6
    read += _check_backend(dev, levels, layer_edges, live)
    read += _check_backend(dev, levels, layer_edges, np.nonzero(live)[0][: n // 2], with_in_edges=False)   # an id list, shorter than n
    assert dev.graph_info_counters()["entries"] == read
    none = dev.graph_info(0, live=np.zeros(n, bool))
    assert none["nodes_count"] == 0 and none["max_out_edges"] == 0 and none["avg_in_edges"] == 0.0 and dev.graph_components(0, live=np.zeros(0, bool)) == 0
    dev.reset_stats()
    assert dev.graph_info_counters() == dict(info_layers=0, component_layers=0, entries=0, launches=0)
    for bad in (-1, len(layer_edges)):
        with pytest.raises(RuntimeError, match="layer"):
            dev.graph_info(bad)
        with pytest.raises(RuntimeError, match="layer"):
            dev.graph_components(bad)


def test_no_committed_graph_is_an_error():
    import hnswindex
    dev = hnswindex.DeviceBackend(4, "sq_euclid", capacity=8)
    with pytest.raises(RuntimeError, match="no graph committed"):
        dev.graph_info(0)
    with pytest.raises(RuntimeError, match="no graph committed"):
        dev.graph_components(0)


def _flat(n, max_edges, src, dst):
    """A level-0 graph of n nodes with the single edges src[i] -> dst[i] (at most one per source)."""
    counts = np.zeros(n, np.int32)
    edges = np.zeros((n, 2 * max_edges + 2), np.int32)
    counts[src] = 1
    edges[src, 0] = dst
    return np.zeros(n, np.int32), [(counts, edges)]


def test_directed_path_under_a_permutation_is_one_component():
    """20 000 nodes, forward edges only, ids permuted: weak connectivity, deep find chains, and one launch of the edge pass."""
    n = 20000
    perm = np.random.default_rng(7).permutation(n)
    levels, layer_edges = _flat(n, 4, perm[:-1], perm[1:])
    dev = _backend(n, 4, levels, layer_edges)
    dev.reset_stats()
    assert dev.graph_components(0) == 1
    assert dev.graph_info_counters() == dict(info_layers=0, component_layers=1, entries=n - 1, launches=3)
    _same(dev.graph_info(0), gm.layer_info(levels, None, 0, *layer_edges[0]))
    # ... and without an articulation node it is two
    live = np.ones(n, bool)
    live[perm[n // 3]] = False
    assert dev.graph_components(0, live=live) == 2 == gm.components(levels, live, 0, *layer_edges[0])


def test_disjoint_cycles_and_isolated_nodes():
    """37 directed cycles of lengths 2 .. 38 and 11 isolated nodes, ids permuted: 48 components."""
    lengths = np.arange(2, 39)
    n = int(lengths.sum()) + 11
    perm = np.random.default_rng(11).permutation(n)
    src, dst, at = [], [], 0
    for k in lengths:
        ring = perm[at:at + k]
        src += ring.tolist()
        dst += np.roll(ring, -1).tolist()
        at += k
    levels, layer_edges = _flat(n, 15, np.array(src), np.array(dst))
    dev = _backend(n, 15, levels, layer_edges)
    assert dev.graph_components(0) == 48 == gm.components(levels, None, 0, *layer_edges[0])
    info = dev.graph_info(0)
    _same(info, gm.layer_info(levels, None, 0, *layer_edges[0]))
    assert (info["min_out_edges"], info["max_out_edges"], info["min_in_edges"], info["max_in_edges"]) == (0, 1, 0, 1)


def test_live_set_without_an_articulation_node():
    """0 -> 1 -> 2 -> 3 -> 4 and 2 not live: two components; 1 keeps its out-degree; 3 has no in-edge; 2 counts nowhere."""
    levels, layer_edges = _flat(5, 4, np.arange(4), np.arange(1, 5))
    dev = _backend(5, 4, levels, layer_edges)
    assert dev.graph_components(0) == 1
    live = np.array([True, True, False, True, True])
    assert dev.graph_components(0, live=live) == 2
    info = dev.graph_info(0, live=live)
    _same(info, gm.layer_info(levels, live, 0, *layer_edges[0]))
    assert info["nodes_count"] == 4 and info["avg_out_edges"] == 3 / 4 and info["avg_in_edges"] == 2 / 4
    assert (info["max_in_edges"], info["min_in_edges"], info["in_edges_median"], info["out_edges_median"]) == (1, 0, 0, 1)
    assert dev.graph_info(0, live=[0, 1])["nodes_count"] == 2    # ids >= nbits are not live


# ---------------------------------------------------------------- through Index.import_graph, with validated lists
def _model_of(ix, with_in_edges=True):
    """(get_info, component counts) of the model on the exported graph -- call it AFTER the calls under test: the export refreshes
    the host copy of the lists."""
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.ids()] = True
    top = ix.top_layer()
    layer_edges = [ix.export_edges(layer, 2 * 16 + 2) for layer in range(top + 1)]
    return gm.get_info(levels, live, layer_edges, top, with_in_edges), gm.component_counts(levels, live, layer_edges, top)


def _check_index(ix, with_in_edges=True, where=""):
    got, comp = ix.get_info(), ix.connected_component_counts()
    want, want_comp = _model_of(ix, with_in_edges)
    assert len(got) == len(want) == ix.top_layer() + 1 and comp.dtype == np.int32
    for g, w in zip(got, want):
        _same(g, w, where)
    assert comp.tolist() == want_comp, where
    return got, comp


def _hub_index(n, extra=()):
    """n level-0 nodes, i -> 0 for every i > 0, node 0 with no edge and the entry point; extra: (source, target) pairs that replace a source's edge."""
    import hnswindex
    src, dst = np.arange(1, n), np.zeros(n - 1, np.int64)
    for s, t in extra:
        dst[s - 1] = t
    levels, layer_edges = _flat(n, 16, src, dst)
    ix = hnswindex.Index(4)
    ix.set_collection_size(n)
    ix.import_graph(uniform(n, 4, 5), levels, 0, layer_edges)
    return ix


def test_hub_in_degree_beyond_16_bits():
    ix = _hub_index(70001)
    info, comp = _check_index(ix)
    assert len(info) == 1 and comp.tolist() == [1]
    i = info[0]
    assert (i["nodes_count"], i["max_in_edges"], i["min_in_edges"], i["in_edges_median"]) == (70001, 70000, 0, 0)
    assert i["avg_in_edges"] == i["avg_out_edges"] == 70000 / 70001
    assert (i["max_out_edges"], i["min_out_edges"], i["out_edges_median"]) == (1, 0, 1)
    # 200 removals, the entry point (the hub) among them: the live set is a real bitset now
    gone = np.concatenate([[0], np.random.default_rng(3).choice(np.arange(1, 70001), 199, replace=False)]).astype(np.int32)
    ix.remove(gone)
    info, comp = _check_index(ix, where="after remove")
    assert info[0]["nodes_count"] == 70001 - 200


def test_two_hubs_and_an_even_count():
    """70 002 nodes, the last one pointing at node 1: an even member count, the two middle ranks both 0."""
    ix = _hub_index(70002, extra=[(70001, 1)])
    info, comp = _check_index(ix)
    i = info[0]
    assert (i["nodes_count"], i["max_in_edges"], i["min_in_edges"], i["in_edges_median"], i["out_edges_median"]) == (70002, 70000, 0, 0, 1)
    assert i["avg_in_edges"] == i["avg_out_edges"] == 70001 / 70002 and comp.tolist() == [1]


# ---------------------------------------------------------------- through a built index
def _balanced(info):
    for i in info:
        assert np.float64(i["avg_out_edges"]).tobytes() == np.float64(i["avg_in_edges"]).tobytes(), i


@pytest.mark.parametrize("metric,n,more,gone", [("sq_euclid", 3000, 500, 700), ("sq_euclid_i8", 1000, 200, 250)])
def test_built_index_matches_the_model(metric, n, more, gone):
    """n x 16, default Add (device-linked): after the build, after a second add (the mirror is appended to), after removals and with
    the host traversal switched on -- the calls run on the device either way.  int8 rows: the mirror is the same, a smaller index."""
    import hnswindex
    x = uniform(n + more, 16, 99)
    ix = hnswindex.Index(16, metric)
    ids = ix.add(x[:n])
    ix.reset_stats()
    info, comp = _check_index(ix, where="built")
    _balanced(info)
    assert info[0]["nodes_count"] == n and len(info) >= 2
    c = ix.graph_info_counters()
    assert c["info_layers"] == c["component_layers"] == len(info) and c["entries"] == 2 * sum(round(i["avg_out_edges"] * i["nodes_count"]) for i in info)
    ix.add(x[n:])
    info, _ = _check_index(ix, where="second add")
    _balanced(info)
    assert info[0]["nodes_count"] == n + more
    ix.remove(ids[np.random.default_rng(1).choice(n, gone, replace=False)])
    info, _ = _check_index(ix, where="removed")
    _balanced(info)
    assert info[0]["nodes_count"] == n + more - gone
    ix.set_device_traversal(False)
    info, _ = _check_index(ix, where="host traversal")
    _balanced(info)


def test_without_removals_the_in_edge_fields_are_zero():
    import hnswindex
    ix = hnswindex.Index(16)
    ix.set_allow_removals(False)
    ix.add(uniform(1000, 16, 5))
    info, _ = _check_index(ix, with_in_edges=False)
    for i in info:
        assert (i["max_in_edges"], i["min_in_edges"], i["in_edges_median"]) == (0, 0, 0) and i["avg_in_edges"] == 0.0
    assert info[0]["nodes_count"] == 1000 and info[0]["avg_out_edges"] > 0      # (the top layer may be one node without an edge)


def test_reference_connected_component_counts_per_layer():
    """GraphTests.ConnectedComponentCountsPerLayerTest (:253-273) on the reference's own inputs: 256 unit vectors, one Add per item."""
    v = refinputs.normalize(refinputs.random_vectors(128, 2000)[:256])
    a = refinputs.ProductAdapter(128, "ucosine", random_seed=12345)
    a.add_each(v)
    counts = a.ix.connected_component_counts()
    assert counts.size >= 1 and (counts == 1).all()
    assert counts.tolist() == _model_of(a.ix)[1]


def test_empty_index_and_null_handle():
    import hnswindex
    ix = hnswindex.Index(8)
    counts = ix.connected_component_counts()
    assert counts.size == 0 and counts.dtype == np.int32
    with pytest.raises(RuntimeError, match="IndexOutOfRangeException"):
        ix.get_info()
    assert ix.graph_info_counters() == dict(info_layers=0, component_layers=0, entries=0, launches=0)
    lib = hnswindex.net_amd.lib
    out = (hnswindex.net_amd.LayerInfo * 2)()
    cnt = (ct.c_int * 2)()
    assert lib.hnsw_mi355x_get_info(None, out, 2) == 0 and lib.hnsw_mi355x_connected_component_counts(None, cnt, 2) == 0
    # cap below the count is no error: the count comes back, cap entries are written
    ix.add(uniform(400, 8, 2))
    top = ix.top_layer()
    assert top >= 1
    full = ix.connected_component_counts()
    cnt[1] = -7
    assert lib.hnsw_mi355x_connected_component_counts(ix._h, cnt, 1) == top + 1 == full.size and cnt[0] == full[0] and cnt[1] == -7
    assert lib.hnsw_mi355x_get_info(ix._h, out, 1) == top + 1 and out[0].nodes_count == 400
