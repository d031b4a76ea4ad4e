"""CPU tier: tests/graph_repair_model.py -- the restatement of repair_reachability that the GPU tier
(tests/test_gpu_graph_repair.py) holds the device to -- pinned on a graph the oracle builds, its invariant asserted after every round,
and the proposal and apply rules on hand-made lists."""
import numpy as np
import pytest

import graph_reach_model as rm
import graph_repair_model as rp
import oracle
from common import uniform
from test_graph_reach_model import _graph_of

M = 4


@pytest.fixture(scope="module")
def built():
    """2000 x 64, M = 4, one Add per item in order: the graph, the rows, and the two plugged-in functions on the oracle's metric."""
    x = uniform(2000, 64, 13)
    ix = oracle.OracleIndex(64, "sq_euclid", max_edges=M, collection_size=4096)
    ix.add(x)
    levels, live, layer_edges, entry = _graph_of(ix, 2 * M + 2)
    cand_fn = rp.nearest_by_rows(x, lambda q, ids: oracle.dist_query_rows("sq_euclid", x, q, ids))
    dist_fn = lambda a, b: oracle.dist_pairs("sq_euclid", x, a, b)   # noqa: E731
    return ix, x, levels, live, layer_edges, entry, cand_fn, dist_fn


def _monotone(before, after):
    """Reached before a round => reached after it, in no more hops."""
    old = before >= 0
    assert (after[old] >= 0).all() and (after[old] <= before[old]).all()


def _well_formed(levels, live, layer_edges, before):
    for layer, (counts, edges) in enumerate(layer_edges):
        cap = 2 * M if layer == 0 else M
        for i in np.nonzero(live & (levels >= layer))[0]:
            own = edges[i, :counts[i]].tolist()
            old = before[layer][1][i, :before[layer][0][i]].tolist()
            assert counts[i] <= cap                                        # MaxEdges(layer): the build leaves no longer list, the repair makes none
            assert len(set(own)) == len(own) or len(set(old)) != len(old)  # no duplicate introduced
            assert (i in own) <= (i in old)                                # no self entry introduced
            assert all(live[v] and levels[v] >= layer for v in own)


def test_the_built_graph_is_repaired_in_one_round_per_layer(built):
    ix, x, levels, live, layer_edges, entry, cand_fn, dist_fn = built
    new, rep = rp.repair(levels, live, layer_edges, entry, cand_fn, dist_fn, M, 8, 8, _monotone)
    assert [tuple(r[f] for f in rp.FIELDS) for r in rep] == [(0, 82, 82, 81, 1, 0), (1, 17, 17, 17, 1, 0), (2, 0, 0, 0, 0, 0), (3, 0, 0, 0, 0, 0)]
    _well_formed(levels, live, new, layer_edges)
    per_layer, hops, _ = rm.reach_chain(levels, live, new, entry)
    assert all(p["reached"] == p["nodes_count"] for p in per_layer) and rm.unreachable_ids(hops).size == 0
    # a second pass finds nothing to do
    again, rep2 = rp.repair(levels, live, new, entry, cand_fn, dist_fn, M, 8, 8, _monotone)
    assert all(tuple(r[f] for f in rp.FIELDS[1:]) == (0, 0, 0, 0, 0) for r in rep2)
    assert all((a[0] == b[0]).all() and (a[1] == b[1]).all() for a, b in zip(again, new))
    # the oracle's own search on the repaired lists returns some of the formerly lost ids for their own rows; it returned none before
    lost = rm.unreachable_ids(rm.reach_chain(levels, live, layer_edges, entry)[1])
    assert lost.size == 86
    assert not (ix.knn_query(x[lost], 1)[0][:, 0] == lost).any()
    ref = oracle.OracleIndex(64, "sq_euclid", max_edges=M, collection_size=4096)
    ref.import_graph(x, levels, entry, new)
    assert int((ref.knn_query(x[lost], 1)[0][:, 0] == lost).sum()) == 25


def test_one_candidate_leaves_a_remainder_that_is_reported(built):
    _, _, levels, live, layer_edges, entry, cand_fn, dist_fn = built
    new, rep = rp.repair(levels, live, layer_edges, entry, cand_fn, dist_fn, M, 1, 1, _monotone)
    assert [tuple(r[f] for f in rp.FIELDS) for r in rep][:2] == [(0, 82, 75, 74, 1, 7), (1, 17, 13, 13, 1, 3)]
    _well_formed(levels, live, new, layer_edges)
    hops = rm.reach_chain(levels, live, new, entry)[1]
    assert rm.unreachable_ids(hops).size == 7
    # more rounds help, and a round that applies nothing ends the layer before max_rounds
    new, rep = rp.repair(levels, live, layer_edges, entry, cand_fn, dist_fn, M, 1, 8, _monotone)
    assert [tuple(r[f] for f in rp.FIELDS) for r in rep][:2] == [(0, 82, 79, 78, 4, 3), (1, 17, 15, 15, 3, 1)]
    _well_formed(levels, live, new, layer_edges)


# ---- the rules on hand-made lists: one layer, ids 0 .. n - 1 at level 0 ------------------------------------------------------
def _lists(n, lists, stride):
    counts = np.zeros(n, np.int32)
    edges = np.zeros((n, stride), np.int32)
    for u, l in lists.items():
        counts[u] = len(l)
        edges[u, :len(l)] = l
    return np.zeros(n, np.int32), counts, edges


def _by_table(table):
    """dist_fn from a dict {(a, b): d}; pairs not in it are 1.0."""
    return lambda a, b: np.array([table.get((int(i), int(j)), 1.0) for i, j in zip(a, b)], np.float32)


def test_append_below_max_edges_and_no_proposal_for_padding():
    levels, counts, edges = _lists(4, {0: [1], 1: [0]}, 3)
    hops = rm.reach_layer(levels, None, 0, counts, edges, [0])
    assert hops.tolist() == [0, 1, -1, -1]
    codes, measured = rp.propose(levels, None, 0, counts, edges, hops, [[1, 0, -1], [0, -1, -1]], _by_table({}), 2)
    assert codes.tolist() == [[1, 1, -1], [1, -1, -1]] and measured == 0


def test_a_full_list_of_tree_edges_has_no_evictable_entry():
    """0 -> 1, 2 and 1 -> 3: with MaxEdges 2 the list of 0 is full and both entries lead one hop further; the list of 1 is not full."""
    levels, counts, edges = _lists(5, {0: [1, 2], 1: [3]}, 3)
    hops = rm.reach_layer(levels, None, 0, counts, edges, [0])
    assert hops.tolist() == [0, 1, 1, 2, -1]
    codes, measured = rp.propose(levels, None, 0, counts, edges, hops, [[0, 1]], _by_table({}), 2)
    assert codes.tolist() == [[-1, 1]] and measured == 0


def test_self_loop_dead_target_equal_distances_and_nan():
    # list of 0: itself (hop 0 <= 0: evictable), 1 (hop 1: a tree edge), 5 (not live: never evictable), 0 again
    live = np.array([True, True, True, True, True, False, True])
    levels, counts, edges = _lists(7, {0: [0, 1, 5, 0], 1: [0, 2, 3, 2]}, 5)
    hops = rm.reach_layer(levels, live, 0, counts, edges, [0])
    assert hops.tolist() == [0, 1, 2, 2, -1, -2, -1]
    seen = []
    def dist(a, b):
        seen.extend(zip(a.tolist(), b.tolist()))
        return _by_table({(1, 0): 2.0})(a, b)
    codes, measured = rp.propose(levels, live, 0, counts, edges, hops, [[0, 1]], dist, 4)
    # 0: the two self entries tie at 1.0, the larger slot wins; 1: only 1 -> 0 is evictable (2 and 3 are further from the seeds)
    assert codes.tolist() == [[3, 0]] and measured == 3
    assert (0, 5) not in seen and all(b != 5 for _, b in seen)             # the dead target is not measured
    # a NaN distance is not evictable: the other self entry is taken, and with both NaN nothing is
    nan = np.float32("nan")
    codes, _ = rp.propose(levels, live, 0, counts, edges, hops, [[0]], lambda a, b: np.array([1.0, nan], np.float32), 4)
    assert codes.tolist() == [[0]]
    codes, _ = rp.propose(levels, live, 0, counts, edges, hops, [[0]], lambda a, b: np.array([nan, nan], np.float32), 4)
    assert codes.tolist() == [[-1]]
    # the largest distance wins over the slot
    codes, _ = rp.propose(levels, live, 0, counts, edges, hops, [[0]], lambda a, b: np.array([3.0, 1.0], np.float32), 4)
    assert codes.tolist() == [[0]]


def test_two_u_want_the_same_v_and_max_rounds():
    """0 <-> 1 reached, 2, 3 and 4 lost; MaxEdges 2.  Everybody's first candidate is 0."""
    levels, counts, edges = _lists(5, {0: [1], 1: [0]}, 3)
    cand_fn = lambda layer, U, reached, C: np.array([[0, 1][:C] + [-1] * (C - 2) for _ in U], np.int32)   # noqa: E731
    U = np.array([2, 3, 4])
    hops = rm.reach_layer(levels, None, 0, counts, edges, [0])
    cd = cand_fn(0, U, None, 2)
    codes, _ = rp.propose(levels, None, 0, counts, edges, hops, cd, _by_table({}), 2)
    assert codes.tolist() == [[1, 1]] * 3
    c2, e2, linked, evicted, claimed = rp.apply_round(counts, edges, U, cd, codes)
    # 2 takes 0, 3 takes its next candidate 1, 4 waits
    assert (linked, evicted, claimed) == (2, 0, [0, 1]) and e2[0, :2].tolist() == [1, 2] and e2[1, :2].tolist() == [0, 3] and c2.tolist() == [2, 2, 0, 0, 0]
    # the whole layer, the candidates the reached ids in ascending order: in round 2 the list of 0 is full of tree edges (1 and 2 are a
    # hop further), the list of 1 is full too but its entry 1 -> 0 leads back towards the seed: 4 takes its place
    def cand2(layer, U, reached, C):
        ids = np.nonzero(reached)[0][:C]
        return np.array([ids.tolist() + [-1] * (C - ids.size) for _ in U], np.int32)
    c3, e3, rep, hops3 = rp.repair_layer(levels, None, 0, counts, edges, [0], cand2, _by_table({}), 2, cands=4, max_rounds=8, check=_monotone)
    assert rep == dict(unreachable_before=3, linked=3, evicted=1, rounds=2, unreachable_after=0)
    assert e3[1, :2].tolist() == [4, 3] and c3.tolist() == [2, 2, 0, 0, 0] and hops3.tolist() == [0, 1, 1, 2, 2]
    # max_rounds = 1 stops after the first and reports the one that waits
    _, _, rep, hops1 = rp.repair_layer(levels, None, 0, counts, edges, [0], cand2, _by_table({}), 2, cands=4, max_rounds=1)
    assert rep == dict(unreachable_before=3, linked=2, evicted=0, rounds=1, unreachable_after=1) and hops1.tolist() == [0, 1, 1, 2, -1]
    # one candidate only: 3 and 4 wait in round 1, and a round that applies nothing ends the layer
    _, _, rep, _ = rp.repair_layer(levels, None, 0, counts, edges, [0], cand_fn, _by_table({}), 2, cands=1, max_rounds=8)
    assert rep == dict(unreachable_before=3, linked=1, evicted=0, rounds=2, unreachable_after=2)


def test_an_entry_point_that_is_not_live_changes_nothing():
    levels, counts, edges = _lists(4, {0: [1], 1: [0, 2], 2: [3]}, 3)
    live = np.array([False, True, True, True])
    cand_fn = rp.nearest_by_rows(np.zeros((4, 2), np.float32), lambda q, ids: np.zeros(ids.size, np.float32))
    new, rep = rp.repair(levels, live, [(counts, edges)], 0, cand_fn, _by_table({}), 1)
    assert rep == [dict(layer_id=0, unreachable_before=3, linked=0, evicted=0, rounds=1, unreachable_after=3)]
    assert (new[0][0] == counts).all() and (new[0][1] == edges).all()
