"""CPU tier: tests/graph_info_model.py -- the numpy restatement of HNSWIndex.GetInfo / GetConnectedComponentCounts that the GPU tier
(tests/test_gpu_graph_info.py) holds the device to -- pinned against the oracle's real in-edge lists and the test side's union-find."""
import numpy as np
import pytest

import graph_info_model as gm
import oracle
import refinputs
from common import uniform


@pytest.fixture(scope="module")
def half_removed():
    """About 600 x 8, M = 6, every other item removed: (oracle index, levels, live, layer_edges in export_edges' layout)."""
    x = uniform(600, 8, 20261)
    ix = oracle.OracleIndex(8, "sq_euclid", max_edges=6, collection_size=1024)
    ids = ix.add(x)
    ix.remove(ids[1::2])
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.active_ids()] = True
    layer_edges = []
    for layer in range(int(levels[live].max()) + 1):
        counts = np.full(levels.size, -1, np.int32)
        edges = np.zeros((levels.size, 14), np.int32)
        for i in np.nonzero(live & (levels >= layer))[0]:
            e = ix.edges(int(i), layer)
            counts[i] = e.size
            edges[i, :e.size] = e
        layer_edges.append((counts, edges))
    return ix, levels, live, layer_edges


def test_in_degrees_are_the_oracles_in_edge_lists(half_removed):
    """InEdges[L] is the transpose of the out-lists: the model's in-degree of every live node equals the length of the list the
    oracle really keeps, on every layer."""
    ix, levels, live, layer_edges = half_removed
    assert live.sum() == 300 and len(layer_edges) >= 2
    for layer, (counts, edges) in enumerate(layer_edges):
        deg = gm.in_degrees(levels, live, layer, counts, edges)
        for i in np.nonzero(live & (levels >= layer))[0]:
            assert deg[i] == len(ix.edges(int(i), layer, incoming=True)), (layer, i)
        assert deg[~(live & (levels >= layer))].sum() == 0


def test_component_counts_are_the_union_finds(half_removed):
    _, levels, live, layer_edges = half_removed
    want = refinputs.components_per_layer(np.where(live, levels, -1), layer_edges)
    assert gm.component_counts(levels, live, layer_edges, len(layer_edges) - 1) == want


def test_average_is_exact_and_balanced(half_removed):
    """LINQ's Average: int64 sum / count in double -- so AvgOutEdges == AvgInEdges bit for bit wherever the in-lists are the transpose."""
    _, levels, live, layer_edges = half_removed
    for info in gm.get_info(levels, live, layer_edges, len(layer_edges) - 1):
        assert info["nodes_count"] > 0
        assert np.float64(info["avg_out_edges"]).tobytes() == np.float64(info["avg_in_edges"]).tobytes()
        assert info["max_out_edges"] <= (12 if info["layer_id"] == 0 else 6) and info["min_in_edges"] <= info["in_edges_median"] <= info["max_in_edges"]
    assert gm.average([1, 2]) == 1.5 and gm.average([2**31 - 1] * 3) == float(2**31 - 1)
    without = gm.get_info(levels, live, layer_edges, 0, with_in_edges=False)[0]
    assert (without["max_in_edges"], without["min_in_edges"], without["in_edges_median"], without["avg_in_edges"]) == (0, 0, 0, 0.0)


def test_median_is_the_references():
    """HNSWInfo.cs:45-51: sorted[n / 2] for an odd count; the integer mean of the two middle values for an even one."""
    assert gm.median([5]) == 5
    assert gm.median([3, 1, 2]) == 2
    assert gm.median([9, 1, 1, 9, 4]) == 4
    assert gm.median([1, 2]) == 1               # (1 + 2) / 2 in integer arithmetic
    assert gm.median([4, 1, 3, 2]) == 2         # (2 + 3) / 2
    assert gm.median([0, 0, 7, 7]) == 3
    assert gm.median([0] * 5 + [70000]) == 0


def test_entries_that_name_no_member_count_only_as_out_degree():
    """0 -> 1 -> 2 with 1 not live: both lists keep their out-degree, nobody has an in-edge from or to 1, and 0 and 2 fall apart."""
    levels = np.zeros(3, np.int32)
    counts = np.array([1, 1, 0], np.int32)
    edges = np.array([[1, 0], [2, 0], [0, 0]], np.int32)
    assert gm.components(levels, None, 0, counts, edges) == 1
    live = np.array([True, False, True])
    info = gm.layer_info(levels, live, 0, counts, edges)
    assert (info["nodes_count"], info["max_out_edges"], info["min_out_edges"], info["max_in_edges"]) == (2, 1, 0, 0)
    assert info["avg_out_edges"] == 0.5 and info["avg_in_edges"] == 0.0
    assert gm.components(levels, live, 0, counts, edges) == 2 and gm.entries(levels, live, 0, counts, edges) == 1
    empty = gm.layer_info(levels, np.zeros(3, bool), 0, counts, edges)
    assert empty["nodes_count"] == 0 and gm.components(levels, np.zeros(3, bool), 0, counts, edges) == 0
