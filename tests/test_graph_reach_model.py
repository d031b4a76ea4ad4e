"""CPU tier: tests/graph_reach_model.py -- the restatement of reachability from the entry point over out-edges that the
GPU tier (tests/test_gpu_graph_reach.py) holds the device to -- pinned on a graph the oracle builds, and held against the oracle's own
searches: an id outside the chain's reached set is never a result of a query."""
import numpy as np
import pytest

import graph_reach_model as rm
import oracle
from common import uniform


def _graph_of(ix, stride):
    """(levels, live, layer_edges in export_edges' layout, entry point) of an oracle index."""
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.active_ids()] = True
    layer_edges = []
    for layer in range(int(levels[ix.entry_point]) + 1):
        counts = np.full(levels.size, -1, np.int32)
        edges = np.zeros((levels.size, stride), np.int32)
        for i in np.nonzero(live & (levels >= layer))[0]:
            e = ix.edges(int(i), layer)
            counts[i] = e.size
            edges[i, :e.size] = e
        layer_edges.append((counts, edges))
    return levels, live, layer_edges, ix.entry_point


@pytest.fixture(scope="module")
def built():
    """2000 x 64, M = 4, one Add per item in order: (oracle index, rows, ids)."""
    x = uniform(2000, 64, 13)
    ix = oracle.OracleIndex(64, "sq_euclid", max_edges=4, collection_size=4096)
    ids = ix.add(x)
    return ix, x, ids


def test_the_chain_on_a_built_graph_and_its_soundness(built):
    ix, x, ids = built
    levels, live, layer_edges, entry = _graph_of(ix, 10)
    per_layer, hops, _ = rm.reach_chain(levels, live, layer_edges, entry)
    got = [(p["layer_id"], p["nodes_count"], p["reached"], p["max_hops"]) for p in per_layer]
    assert got == [(0, 2000, 1914, 5), (1, 124, 107, 5), (2, 7, 7, 2), (3, 1, 1, 0)]
    assert [p["seeds"] for p in per_layer] == [107, 7, 1, 1]
    lost = rm.unreachable_ids(hops)
    assert lost.size == 86 and lost[:5].tolist() == [26, 33, 103, 136, 154]
    # in-degree 0 is not the answer: 85 such nodes, 86 unreachable ids
    indeg = np.bincount(np.concatenate([layer_edges[0][1][i, :layer_edges[0][0][i]] for i in range(2000)]), minlength=2000)
    assert int((indeg == 0).sum()) == 85
    # soundness against the oracle's own searches: no query returns an unreachable id
    found, _ = ix.knn_query(x[lost], 50)
    assert not np.isin(found, lost).any()
    found, _ = ix.knn_query(uniform(1000, 64, 77), 50)
    assert not np.isin(found, lost).any()
    in_range, _ = ix.range_query(x[lost][:20], 8.0)
    assert sum(r.size for r in in_range) > 0 and not any(np.isin(r, lost).any() for r in in_range)
    # the per-layer figures follow from the hop arrays
    assert rm.rounds(hops) == 6 and rm.expanded_entries(levels, live, 0, *layer_edges[0], hops) == int(layer_edges[0][0][hops >= 0].sum())
    # after removals (the last test of the module's fixture: it edits the index)
    ix.remove(ids[1::2])
    levels, live, layer_edges, entry = _graph_of(ix, 10)
    per_layer, hops, _ = rm.reach_chain(levels, live, layer_edges, entry)
    assert per_layer[0]["nodes_count"] == 1000 and rm.unreachable_ids(hops).size == 145 and per_layer[0]["reached"] == 855


def _flat(n, pairs, stride=4):
    counts = np.zeros(n, np.int32)
    edges = np.zeros((n, stride), np.int32)
    for u, v in pairs:
        edges[u, counts[u]] = v
        counts[u] += 1
    return np.zeros(n, np.int32), counts, edges


def test_a_target_that_is_no_member_ends_the_walk():
    """0 -> 1 -> 2 with 1 not live: 2 is a member that nothing reaches, 1 is no member."""
    levels, counts, edges = _flat(3, [(0, 1), (1, 2)])
    assert rm.reach_layer(levels, None, 0, counts, edges, [0]).tolist() == [0, 1, 2]
    live = np.array([True, False, True])
    hops = rm.reach_layer(levels, live, 0, counts, edges, [0])
    assert hops.tolist() == [0, -2, -1]
    assert rm.summary(hops) == dict(nodes_count=2, seeds=1, reached=1, max_hops=0)
    assert rm.expanded_entries(levels, live, 0, counts, edges, hops) == 1 and rm.rounds(hops) == 1
    assert rm.unreachable_ids(hops).tolist() == [2]


def test_seeds_that_are_no_members_and_the_empty_seed_set():
    levels, counts, edges = _flat(4, [(0, 1), (1, 2), (3, 0)])
    levels[2] = 1
    live = np.array([True, True, True, False])
    # 3 is not live, 9 is out of range, a mask longer than the graph: only 1 starts
    assert rm.reach_layer(levels, live, 0, counts, edges, [1, 3, 9]).tolist() == [-1, 0, 1, -2]
    assert rm.reach_layer(levels, live, 0, counts, edges, np.array([False, True, False, True, True, True])).tolist() == [-1, 0, 1, -2]
    # on layer 1 only node 2 is a member; a seed below the layer is ignored
    assert rm.reach_layer(levels, live, 1, np.zeros(4, np.int32), edges, [0, 1]).tolist() == [-2, -2, -1, -2]
    none = rm.reach_layer(levels, live, 0, counts, edges, [])
    assert none.tolist() == [-1, -1, -1, -2] and rm.rounds(none) == 0 and rm.expanded_entries(levels, live, 0, counts, edges, none) == 0
    assert rm.summary(none) == dict(nodes_count=3, seeds=0, reached=0, max_hops=0)


def test_direction_matters():
    """A path 0 -> 1 -> 2 -> 3: everything from its head, only itself from its tail; a node of in-degree 0 is reached by nobody else."""
    levels, counts, edges = _flat(5, [(0, 1), (1, 2), (2, 3), (4, 0)])
    assert rm.reach_layer(levels, None, 0, counts, edges, [0]).tolist() == [0, 1, 2, 3, -1]     # 4 has out-edges and no in-edge
    assert rm.reach_layer(levels, None, 0, counts, edges, [3]).tolist() == [-1, -1, -1, 0, -1]
    assert rm.reach_layer(levels, None, 0, counts, edges, [4]).tolist() == [1, 2, 3, 4, 0]
    hops = rm.reach_layer(levels, None, 0, counts, edges, [0])
    assert rm.rounds(hops) == 4 and rm.expanded_entries(levels, None, 0, counts, edges, hops) == 3


def test_self_loops_duplicates_and_clamped_counts():
    levels, counts, edges = _flat(3, [(0, 0), (0, 1), (0, 1), (1, 0)])
    hops = rm.reach_layer(levels, None, 0, counts, edges, [0])
    assert hops.tolist() == [0, 1, -1] and rm.expanded_entries(levels, None, 0, counts, edges, hops) == 4
    counts[0], counts[1] = 11, -5       # clamped to the list's capacity and to 0
    edges[0, 3] = 2
    hops = rm.reach_layer(levels, None, 0, counts, edges, [0])
    assert hops.tolist() == [0, 1, 1] and rm.expanded_entries(levels, None, 0, counts, edges, hops) == 4
    assert rm.reach_layer(levels, None, 0, counts, edges, [0], cap=3).tolist() == [0, 1, -1]


def test_the_chain_arrives_from_the_layer_above():
    """E (level 1) -> A on layer 1, A -> B on layer 0, E's layer-0 list empty: B is reached only through the layer-1 arrival at A."""
    E, A, B, C = 0, 1, 2, 3
    levels = np.array([1, 1, 0, 0], np.int32)
    l0 = (np.array([0, 1, 0, 1], np.int32), np.array([[0, 0], [B, 0], [0, 0], [B, 0]], np.int32))
    l1 = (np.array([1, 0, -1, -1], np.int32), np.array([[A, 0], [0, 0], [0, 0], [0, 0]], np.int32))
    per_layer, hops, by_layer = rm.reach_chain(levels, None, [l0, l1], E)
    assert by_layer[1].tolist() == [0, 1, -2, -2] and hops.tolist() == [0, 0, 1, -1]
    assert per_layer == [dict(layer_id=0, nodes_count=4, seeds=2, reached=3, max_hops=1), dict(layer_id=1, nodes_count=2, seeds=1, reached=2, max_hops=1)]
    assert rm.unreachable_ids(hops).tolist() == [C]
    # min_layer = 1 stops above; an entry point that is not live, or out of range, reaches nothing
    assert [p["layer_id"] for p in rm.reach_chain(levels, None, [l0, l1], E, min_layer=1)[0]] == [1]
    dead = rm.reach_chain(levels, np.array([False, True, True, True]), [l0, l1], E)[0]
    assert [(p["nodes_count"], p["reached"]) for p in dead] == [(3, 0), (1, 0)]
    assert [(p["nodes_count"], p["reached"]) for p in rm.reach_chain(levels, None, [l0, l1], 7)[0]] == [(4, 0), (2, 0)]
