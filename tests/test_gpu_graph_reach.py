"""GPU tier: reachability from the entry point over out-edges, computed on the device from the graph mirror (hnsw_mi355x_reachability,
hnsw_mi355x_unreachable_ids, hnsw_mi355x_hop_counts, hnswdev_graph_reach_layer, hnswdev_graph_reach).  Every expectation
comes from the numpy / deque restatement tests/graph_reach_model.py, which the CPU tier pins to a graph the oracle builds and to the
oracle's own searches; nothing here is compared with itself."""
import ctypes as ct

import numpy as np
import pytest

import graph_info_model as gm
import graph_reach_model as rm
from common import set_diag, uniform

pytestmark = pytest.mark.gpu

COUNTERS0 = dict(layers=0, rounds=0, entries=0, launches=0)


# ---------------------------------------------------------------- hand-made graphs through DeviceBackend.set_graph
def _backend(n, max_edges, levels, layer_edges):
    import hnswindex
    dev = hnswindex.DeviceBackend(4, "sq_euclid", capacity=max(n, 1))
    dev.upload_rows(0, np.zeros((n, 4), np.float32))     # graph_commit needs n rows
    dev.set_graph(levels, layer_edges, max_edges)
    return dev


def _caps(max_edges):
    """Entries a list of the mirror holds on layer 0 and above it: MaxEdges(layer) + 1."""
    return dict(cap0=2 * max_edges + 1, capU=max_edges + 1)


def _random_graph(n, max_edges, seed):
    """Levels with a top of 3 (n >= 2: four layers) and, per layer, lists among the layer's members: empty ones, full ones of
    MaxEdges + 1 entries (2M + 1 on layer 0, M + 1 above), a self-loop, duplicates (targets are drawn with replacement)."""
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
            c = 0 if kind < 0.35 else full if kind < 0.5 else int(rng.integers(0, 3))    # sparse: several BFS levels, parts left unreached
            if j == 0:
                c = max(c, 1)
            counts[v] = c
            edges[v, :c] = rng.choice(mem, c)
            if j == 0:
                edges[v, 0] = v   # a self-loop
        layer_edges.append((counts, edges))
    return levels, layer_edges


def _as_mask(n, live):
    return None if live is None else rm.as_mask(n, live)


def _check_layers(dev, levels, layer_edges, live, seeds, max_edges):
    """Every layer of a committed graph from `seeds` against the model; returns the model's (layers, rounds, entries)."""
    n = levels.size
    walked = spun = read = 0
    for layer, (counts, edges) in enumerate(layer_edges):
        cap = 2 * max_edges + 1 if layer == 0 else max_edges + 1
        want = rm.reach_layer(levels, _as_mask(n, live), layer, counts, edges, seeds, cap)
        mask, hops, summary = dev.graph_reach_layer(layer, seeds, live=live)
        assert hops.tolist() == want.tolist(), (layer, "hops")
        assert mask.tolist() == (want >= 0).tolist(), (layer, "mask")
        assert summary == rm.summary(want), layer
        walked += 1
        spun += rm.rounds(want)
        read += rm.expanded_entries(levels, _as_mask(n, live), layer, counts, edges, want, cap)
    return walked, spun, read


def _check_chain(dev, levels, layer_edges, live, entry, max_edges, min_layer=0):
    n = levels.size
    want_layers, want_hops, by_layer = rm.reach_chain(levels, _as_mask(n, live), layer_edges, entry, min_layer, **_caps(max_edges))
    got_layers, mask, hops = dev.graph_reach(entry, live=live, min_layer=min_layer)
    assert got_layers == want_layers
    assert hops.tolist() == want_hops.tolist() and mask.tolist() == (want_hops >= 0).tolist()
    read = sum(rm.expanded_entries(levels, _as_mask(n, live), L, *layer_edges[L], h, 2 * max_edges + 1 if L == 0 else max_edges + 1) for L, h in by_layer.items())
    return len(by_layer), sum(rm.rounds(h) for h in by_layer.values()), read


@pytest.mark.parametrize("max_edges", [4, 15, 16])      # expansion items per node 9, 31 and 33: a wave's items start mid-list, are two lists, end mid-list
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 257])     # the word edges of the packed bitset and of a 64-lane ballot
def test_hand_made_graphs_match_the_model(n, max_edges):
    levels, layer_edges = _random_graph(n, max_edges, 1000 * n + max_edges)
    assert len(layer_edges) == (4 if n >= 2 else 3)
    dev = _backend(n, max_edges, levels, layer_edges)
    dev.reset_stats()
    rng = np.random.default_rng(n + max_edges)
    total = np.zeros(3, np.int64)
    seed_mask = rng.random(n) < 0.15
    seed_mask[np.argmax(levels)] = True                       # a member of every layer
    seed_ids = np.nonzero(seed_mask)[0]
    live = rng.random(n) < 0.6
    live[np.argmax(levels)] = True
    total += _check_layers(dev, levels, layer_edges, None, seed_mask, max_edges)              # seeds as a mask ...
    total += _check_layers(dev, levels, layer_edges, live, seed_ids, max_edges)               # ... and as an id list, under a live mask
    total += _check_layers(dev, levels, layer_edges, np.nonzero(live)[0][: n // 2], seed_mask, max_edges)   # a live id list, shorter than n
    total += _check_layers(dev, levels, layer_edges, None, np.ones(n, bool), max_edges)       # everything a seed: one round per layer
    total += _check_layers(dev, levels, layer_edges, None, np.zeros(0, bool), max_edges)      # no seed: nothing reached, no round
    c = dev.graph_reach_counters()
    assert (c["layers"], c["rounds"], c["entries"]) == tuple(total.tolist())     # entries == expanded_entries: every node expanded once
    assert c["launches"] == c["rounds"] + 2 * c["layers"]
    # the chain from the top node, from a level-0 node and with a live set, down to layer 0 and down to layer 1
    top_node = int(np.argmax(levels))
    total += _check_chain(dev, levels, layer_edges, None, top_node, max_edges)
    total += _check_chain(dev, levels, layer_edges, live, top_node, max_edges)
    total += _check_chain(dev, levels, layer_edges, None, int(np.argmin(levels)), max_edges)
    if levels[top_node] >= 1:
        total += _check_chain(dev, levels, layer_edges, live, top_node, max_edges, min_layer=1)
    # an entry point that is no member of its own level, and one out of range (top: the graph's), reach nothing on any layer
    dead = live.copy()
    dead[top_node] = False
    for entry, lv in ((top_node, dead), (n, None), (-1, live)):
        before = total.copy()
        total += _check_chain(dev, levels, layer_edges, lv, entry, max_edges)
        assert (total - before).tolist() == [len(layer_edges), 0, 0]
        assert all(layer["reached"] == 0 for layer in dev.graph_reach(entry, live=lv)[0])
        total[0] += len(layer_edges)
    c = dev.graph_reach_counters()
    assert (c["layers"], c["rounds"], c["entries"]) == tuple(total.tolist())
    dev.reset_stats()
    assert dev.graph_reach_counters() == COUNTERS0
    for bad in (-1, len(layer_edges)):
        with pytest.raises(RuntimeError, match="layer"):
            dev.graph_reach_layer(bad, seed_mask)
    with pytest.raises(RuntimeError, match="min_layer"):
        dev.graph_reach(top_node, min_layer=int(levels[top_node]) + 1)


def test_no_committed_graph_and_null_seeds_are_errors():
    import hnswindex
    lib = hnswindex.net_amd.lib
    dev = hnswindex.DeviceBackend(4, "sq_euclid", capacity=8)
    with pytest.raises(RuntimeError, match="no graph committed"):
        dev.graph_reach_layer(0, [0])
    with pytest.raises(RuntimeError, match="no graph committed"):
        dev.graph_reach(0)
    levels, layer_edges = _flat(3, 4, np.array([0]), np.array([1]))
    dev = _backend(3, 4, levels, layer_edges)
    summary = (ct.c_uint64 * 4)()
    assert lib.hnswdev_graph_reach_layer(dev._ctx, 0, None, 0, None, 0, None, None, summary) != 0 and "seed_bits" in dev.last_error()
    # the outputs are optional
    words = np.array([1], np.uint32)
    assert lib.hnswdev_graph_reach_layer(dev._ctx, 0, None, 0, words.ctypes.data_as(ct.POINTER(ct.c_uint32)), 1, None, None, summary) == 0
    assert list(summary) == [3, 1, 2, 1]


def _flat(n, max_edges, src, dst):
    """A level-0 graph of n nodes with the edges src[i] -> dst[i], in that order in each source's list."""
    counts = np.zeros(n, np.int32)
    edges = np.zeros((n, 2 * max_edges + 2), np.int32)
    for s, t in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        edges[s, counts[s]] = t
        counts[s] += 1
    return np.zeros(n, np.int32), [(counts, edges)]


def test_a_directed_path_is_walked_one_way_only():
    """300 nodes, forward edges only, ids permuted: one weak component; from its head every node at its position, in 300 rounds;
    from its tail nothing but the tail."""
    n = 300
    perm = np.random.default_rng(7).permutation(n)
    levels, layer_edges = _flat(n, 4, perm[:-1], perm[1:])
    dev = _backend(n, 4, levels, layer_edges)
    assert dev.graph_components(0) == 1 == gm.components(levels, None, 0, *layer_edges[0])
    dev.reset_stats()
    mask, hops, summary = dev.graph_reach_layer(0, [int(perm[0])])
    assert hops[perm].tolist() == list(range(n)) and mask.all()
    assert hops.tolist() == rm.reach_layer(levels, None, 0, *layer_edges[0], [int(perm[0])]).tolist()
    assert summary == dict(nodes_count=n, seeds=1, reached=n, max_hops=n - 1)
    assert dev.graph_reach_counters() == dict(layers=1, rounds=n, entries=n - 1, launches=n + 2)
    mask, hops, summary = dev.graph_reach_layer(0, [int(perm[-1])])
    assert summary == dict(nodes_count=n, seeds=1, reached=1, max_hops=0) and mask.sum() == 1 and hops[perm[-1]] == 0 and (np.delete(hops, perm[-1]) == -1).all()
    layers, mask, hops = dev.graph_reach(int(perm[-1]))
    assert layers == [dict(layer_id=0, nodes_count=n, seeds=1, reached=1, max_hops=0)] and dev.graph_components(0) == 1


def test_a_wide_frontier():
    """A complete 32-ary out-tree of depth 3 under a permutation: frontiers of 1 / 32 / 1 024 / 32 768 nodes, the last appended by
    well over a hundred blocks (1 024 nodes x 33 slots = 33 792 items, 132 blocks of 256)."""
    n = 1 + 32 + 32 ** 2 + 32 ** 3
    assert n == 33825
    perm = np.random.default_rng(3).permutation(n)
    inner = np.arange(1 + 32 + 32 ** 2)
    src = np.repeat(inner, 32)
    dst = 32 * src + 1 + np.tile(np.arange(32), inner.size)
    counts = np.zeros(n, np.int32)
    counts[perm[inner]] = 32
    edges = np.zeros((n, 34), np.int32)
    edges[perm[inner], :32] = perm[dst].reshape(-1, 32)
    levels = np.zeros(n, np.int32)
    dev = _backend(n, 16, levels, [(counts, edges)])
    dev.reset_stats()
    root = int(perm[0])
    mask, hops, summary = dev.graph_reach_layer(0, [root])
    want = rm.reach_layer(levels, None, 0, counts, edges, [root], 33)
    assert np.bincount(want).tolist() == [1, 32, 1024, 32768]
    assert (hops == want).all() and mask.all() and summary == dict(nodes_count=n, seeds=1, reached=n, max_hops=3)
    assert dev.graph_reach_counters() == dict(layers=1, rounds=4, entries=n - 1, launches=6)
    # ... and from the 32 768 leaves at once: a seed queue appended by every block of the init pass
    leaves = perm[1 + 32 + 32 ** 2:]
    mask, hops, summary = dev.graph_reach_layer(0, leaves)
    assert summary == dict(nodes_count=n, seeds=32768, reached=32768, max_hops=0) and mask.sum() == 32768 and (hops[leaves] == 0).all()


def test_many_parents_reach_one_child_in_the_same_round():
    """64 parents of one child, all seeds: one of them wins the child, which has hop 1 and is expanded once -- its one entry is read once."""
    n = 66
    levels, layer_edges = _flat(n, 4, list(range(64)) + [64], [64] * 64 + [65])
    dev = _backend(n, 4, levels, layer_edges)
    dev.reset_stats()
    mask, hops, summary = dev.graph_reach_layer(0, np.arange(64))
    assert hops.tolist() == [0] * 64 + [1, 2] and summary == dict(nodes_count=n, seeds=64, reached=n, max_hops=2)
    assert hops.tolist() == rm.reach_layer(levels, None, 0, *layer_edges[0], np.arange(64)).tolist()
    assert dev.graph_reach_counters() == dict(layers=1, rounds=3, entries=65, launches=5)


def test_what_is_no_member_is_never_dereferenced_and_never_reached(monkeypatch):
    """Lists that no build writes (staged unchecked: diag graph_unchecked): entries of -1, n, 2^31 - 1, of an id that is not live and,
    on layer 1, of a level-0 id; count words of -5 and of stride + 7; a seed bitset longer than the graph."""
    n, max_edges = 40, 4
    stride0, strideU = 2 * max_edges + 2, max_edges + 2
    levels = np.zeros(n, np.int32)
    levels[[0, 1, 2, 3]] = 1
    c0 = np.zeros(n, np.int32)
    e0 = np.zeros((n, stride0), np.int32)
    c0[0], e0[0, :6] = 6, [-1, n, 2 ** 31 - 1, 5, 1, -2 ** 31]       # 5 is not live below
    c0[1], e0[1, :2] = -5, [7, 8]                                    # a negative count word: an empty list
    c0[2], e0[2] = stride0 + 7, np.arange(10, 10 + stride0)          # beyond the capacity: the 9 entries the list holds
    c0[10], e0[10, :2] = 2, [2, 30]
    c0[5], e0[5, :1] = 1, [31]                                       # the list of a node that is not live is never read
    c1 = np.full(n, -1, np.int32)
    e1 = np.zeros((n, stride0), np.int32)
    c1[0], e1[0, :4] = 4, [9, 1, n + 3, -1]                          # 9 has level 0: no member of layer 1
    c1[1], e1[1, :1] = strideU + 7, [2]
    c1[2], c1[3] = -5, 0
    layer_edges = [(c0, e0), (c1, e1)]
    set_diag(monkeypatch, graph_unchecked=1)
    dev = _backend(n, max_edges, levels, layer_edges)
    set_diag(monkeypatch, graph_unchecked=0)
    live = np.ones(n, bool)
    live[5] = False
    dev.reset_stats()
    total = np.zeros(3, np.int64)
    long_seeds = np.zeros(n + 100, bool)
    long_seeds[[0, n + 50]] = True
    for seeds in (long_seeds, [0, 10], [1], np.ones(n + 7, bool)):
        total += _check_layers(dev, levels, layer_edges, live, seeds, max_edges)
    total += _check_chain(dev, levels, layer_edges, live, 0, max_edges)
    c = dev.graph_reach_counters()
    assert (c["layers"], c["rounds"], c["entries"]) == tuple(total.tolist())
    # what the model says about this graph, spelled out: from 0 on layer 0 only 1 is new; 31 (behind the dead 5) stays outside
    _, hops, _ = dev.graph_reach_layer(0, [0], live=live)
    assert hops[[0, 1, 5, 31]].tolist() == [0, 1, -2, -1] and (hops >= 0).sum() == 2
    _, hops, _ = dev.graph_reach_layer(0, [10], live=live)
    assert sorted(np.nonzero(hops >= 0)[0].tolist()) == [2, 10, 11, 12, 13, 14, 15, 16, 17, 18, 30]
    _, hops, summary = dev.graph_reach_layer(1, [0], live=live)
    assert hops[:4].tolist() == [0, 1, 2, -1] and (hops[4:] == -2).all() and summary == dict(nodes_count=4, seeds=1, reached=3, max_hops=2)


# ---------------------------------------------------------------- through Index.import_graph
def test_the_chain_arrives_from_the_layer_above():
    """E (the entry point, level 1) -> A on layer 1, A -> B on layer 0, E's layer-0 list empty: B is reachable only through the
    layer-1 arrival.  C is live, has an out-edge and no in-edge: the one id no query can return."""
    import hnswindex
    E, A, B, C = 0, 1, 2, 3
    n, stride = 4, 2 * 16 + 2
    levels = np.array([1, 1, 0, 0], np.int32)
    c0, e0 = np.array([0, 1, 0, 1], np.int32), np.zeros((n, stride), np.int32)
    e0[A, 0] = B
    e0[C, 0] = B
    c1, e1 = np.array([1, 0, -1, -1], np.int32), np.zeros((n, stride), np.int32)
    e1[E, 0] = A
    layer_edges = [(c0, e0), (c1, e1)]
    x = uniform(n, 4, 5)
    ix = hnswindex.Index(4)
    ix.set_collection_size(n)
    ix.import_graph(x, levels, E, layer_edges)
    want_layers, want_hops, _ = rm.reach_chain(levels, None, layer_edges, E)
    assert ix.reachability() == want_layers == [dict(layer_id=0, nodes_count=4, seeds=2, reached=3, max_hops=1),
                                                dict(layer_id=1, nodes_count=2, seeds=1, reached=2, max_hops=1)]
    assert ix.unreachable_ids().tolist() == [C] and ix.unreachable_ids(1).size == 0
    assert ix.hop_counts().tolist() == want_hops.tolist() == [0, 0, 1, -1]
    assert ix.hop_counts(1).tolist() == [0, 1, -2, -2]
    ids, _ = ix.knn_query(x[C], ix.count)
    assert C not in ids.ravel().tolist() and B in ids.ravel().tolist()
    ids, d = ix.exact_knn_query(x[C], ix.count)
    assert ids[0, 0] == C and d[0, 0] == 0.0


# ---------------------------------------------------------------- through a built index
def _model_of(ix, stride):
    """(per-layer dicts, per-layer hop arrays) of the model on the exported graph."""
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.ids()] = True
    layer_edges = [ix.export_edges(layer, stride) for layer in range(ix.top_layer() + 1)]
    per_layer, _, by_layer = rm.reach_chain(levels, live, layer_edges, ix.entry_point)
    return per_layer, by_layer


def _check_index(ix, stride, where):
    got = ix.reachability()
    lost = [ix.unreachable_ids(layer) for layer in range(len(got))]
    hops0 = ix.hop_counts(0)
    want, by_layer = _model_of(ix, stride)
    assert got == want and len(got) == ix.top_layer() + 1, where
    for layer, ids in enumerate(lost):
        assert ids.dtype == np.int32 and ids.tolist() == rm.unreachable_ids(by_layer[layer]).tolist(), (where, layer)
    assert hops0.tolist() == by_layer[0].tolist(), where
    assert lost[0].size > 0, where        # the CPU restatements of the build's schedules leave 86 - 89 ids outside, 142 - 147 after the removals
    return lost[0]


def _never_returned(ix, x, lost, where):
    for q in (uniform(1000, x.shape[1], 77), x[lost]):
        found, _ = ix.knn_query(q, 50)
        assert not np.isin(found, lost).any(), where


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_built_index_matches_the_model(metric):
    """2000 x 64, M = 4, the default Add: after the build, after a second add (the mirror is appended to) and after every other id
    has been removed (the live set is a real bitset).  No query returns an id the chain leaves outside."""
    import hnswindex
    x = uniform(2300, 64, 13)
    ix = hnswindex.Index(64, metric)
    ix.set_max_edges(4)
    ix.set_collection_size(4096)
    ids = ix.add(x[:2000])
    ix.reset_stats()
    lost = _check_index(ix, 10, "built")
    c = ix.graph_reach_counters()
    layers = ix.top_layer() + 1
    assert c["layers"] == layers + sum(layers - L for L in range(layers)) + layers     # reachability, unreachable_ids(L) for each L, hop_counts(0)
    _never_returned(ix, x, lost, "built")
    ix.add(x[2000:])
    lost = _check_index(ix, 10, "second add")
    _never_returned(ix, x, lost, "second add")
    ix.remove(ids[1::2])
    lost = _check_index(ix, 10, "removed")
    assert not np.isin(lost, ids[1::2]).any()
    _never_returned(ix, x, lost, "removed")


def test_built_index_with_the_host_traversal():
    """The calls run on the device whatever device_traversal says: the mirror is brought up to date from the host's lists first."""
    import hnswindex
    x = uniform(1000, 64, 13)
    ix = hnswindex.Index(64)
    ix.set_max_edges(4)
    ix.set_collection_size(2048)
    ix.set_device_traversal(False)
    ids = ix.add(x)
    ix.remove(ids[1::2])
    ix.reset_stats()
    lost = _check_index(ix, 10, "host traversal")
    assert ix.graph_reach_counters()["rounds"] > 0
    _never_returned(ix, x, lost, "host traversal")


def test_conventions():
    import hnswindex
    lib = hnswindex.net_amd.lib
    ix = hnswindex.Index(8)
    assert ix.reachability() == [] and ix.unreachable_ids().size == 0 and ix.hop_counts().size == 0
    assert ix.unreachable_ids().dtype == np.int32 and ix.graph_reach_counters() == COUNTERS0
    n = 2000
    ix2 = hnswindex.Index(64)      # the built fixture of the test above: its schedules leave 86 - 89 ids outside
    ix2.set_max_edges(4)
    ix2.set_collection_size(4096)
    ix2.add(uniform(n, 64, 13))
    top = ix2.top_layer()
    assert top >= 1
    full = ix2.reachability()
    lost = ix2.unreachable_ids()
    hops = ix2.hop_counts()
    assert len(full) == top + 1 and lost.size >= 2 and hops.size == n and (hops[lost] == -1).all() and (hops == -1).sum() == lost.size
    # cap below the count is no error: the count comes back, cap entries are written
    I = ct.POINTER(ct.c_int)
    out = (hnswindex.net_amd.LayerReach * 2)()
    out[1].reached = -7
    assert lib.hnsw_mi355x_reachability(ix2._h, out, 1) == top + 1 and out[0].as_dict() == full[0] and out[1].reached == -7
    buf = np.full(4, -7, np.int32)
    assert lib.hnsw_mi355x_unreachable_ids(ix2._h, 0, buf.ctypes.data_as(I), 1) == lost.size and buf.tolist() == [int(lost[0]), -7, -7, -7]
    assert lib.hnsw_mi355x_hop_counts(ix2._h, 0, buf.ctypes.data_as(I), 3) == n and buf.tolist() == hops[:3].tolist() + [-7]
    assert lib.hnsw_mi355x_unreachable_ids(ix2._h, 0, None, 0) == lost.size and lib.hnsw_mi355x_hop_counts(ix2._h, 0, None, 0) == n
    for bad in (-1, top + 1):
        with pytest.raises(RuntimeError, match="layer"):
            ix2.unreachable_ids(bad)
        with pytest.raises(RuntimeError, match="layer"):
            ix2.hop_counts(bad)
    assert ix2.graph_reach_counters()["layers"] > 0
    ix2.reset_stats()
    assert ix2.graph_reach_counters() == COUNTERS0
