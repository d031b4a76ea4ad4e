"""CPU tier: the plain-Python statement of the near-duplicate calls over the graph's edges (tests/graph_dup_model.py) on graphs small
enough to check by hand -- what an edge is (directed, member to member), what the groups are (components of the within-edges read
both ways), the order of near_edges, and where the call differs from duplicate_groups: it joins only what the graph connects."""
import numpy as np

import oracle
from graph_dup_model import dist_from_range_lists, graph_duplicate_groups, near_edges
from near_dup_model import duplicate_groups, exact_range_by_id

# points on a line: 1 - 2 - 3 is a chain with steps of 1 and ends 2 apart; 0, 5 and 7 are one point; 4 is far from everything
X = np.array([[0.0], [10.0], [11.0], [12.0], [50.0], [0.0], [10.5], [0.0]], np.float32)
# 5 lists 0 and 0 does not list 5 (one direction, towards the smaller id); 7 is a duplicate of 0 and 5 that no list names and that
# names nobody within the radius; 2 lists both ends of its chain, the ends list only far items; 6 lists 2 and 1
EDGES = {0: [4], 1: [4], 2: [3, 1, 4], 3: [4], 4: [0, 1], 5: [0, 4], 6: [2, 1], 7: [4]}


def dist_to(own, cand):
    d = X[np.asarray(cand, np.int64), 0] - X[own, 0]
    return (d * d).astype(np.float32)


def edges_of(i):
    return EDGES[i]


def test_hand_made_graph():
    labels, info = graph_duplicate_groups(edges_of, 8, np.arange(8), dist_to, 1.0)
    # 5 -> 0 joins the two although 0 does not list 5; 1 - 2 - 3 is one group through 2's list alone, although d(1, 3) = 4 > 1;
    # 7 equals 0 and 5 and stays alone: no within-edge reaches it
    assert labels.tolist() == [0, 1, 1, 1, 4, 0, 1, 7] and labels.dtype == np.int32
    assert info == {"members": 8, "groups": 4, "edges_within": 5, "edges_measured": 13}
    assert duplicate_groups(dist_to, 8, np.arange(8), 1.0)[0].tolist() == [0, 1, 1, 1, 4, 0, 1, 0]   # the exact call joins 7
    src, dst, d, measured = near_edges(edges_of, np.arange(8), dist_to, 1.0)
    assert src.tolist() == [2, 2, 5, 6, 6] and dst.tolist() == [1, 3, 0, 1, 2] and d.tolist() == [1.0, 1.0, 0.0, 0.25, 0.25] and measured == 13
    assert (src.dtype, dst.dtype, d.dtype) == (np.int32, np.int32, np.float32)


def test_order_inside_one_owner_is_distance_then_id():
    e = {0: [3, 2, 1, 4], 1: [], 2: [], 3: [], 4: []}
    d = {1: 2.0, 2: -0.0, 3: 0.0, 4: np.nan}
    src, dst, dist, measured = near_edges(lambda i: e[i], np.arange(5), lambda own, cand: np.asarray([d[int(c)] for c in cand], np.float32), np.inf)
    assert src.tolist() == [0, 0, 0] and dst.tolist() == [2, 3, 1] and measured == 4      # -0 == +0: the id decides; NaN is never within
    assert np.signbit(dist[0]) and not np.signbit(dist[1])


def test_radius_nan_infinity_and_negative():
    labels, info = graph_duplicate_groups(edges_of, 8, np.arange(8), dist_to, np.nan)
    assert labels.tolist() == list(range(8)) and info == {"members": 8, "groups": 8, "edges_within": 0, "edges_measured": 13}
    labels, info = graph_duplicate_groups(edges_of, 8, np.arange(8), dist_to, np.inf)
    assert labels.tolist() == [0] * 8 and info["edges_within"] == 13 and info["groups"] == 1   # the graph hangs together through 4
    labels, info = graph_duplicate_groups(edges_of, 8, np.arange(8), dist_to, -1.0)
    assert labels.tolist() == list(range(8)) and info["edges_within"] == 0
    assert near_edges(edges_of, np.arange(8), dist_to, np.nan)[0].size == 0


def test_allow_set_that_removes_the_chains_middle():
    members = [0, 1, 3, 4, 5, 6, 7]
    labels, info = graph_duplicate_groups(edges_of, 8, members, dist_to, 1.0)
    # 2 is no member: -1, its list is not read, and 6 -> 2 is no edge; 6 -> 1 still is
    assert labels.tolist() == [0, 1, -1, 3, 4, 0, 1, 7]
    assert info == {"members": 7, "groups": 5, "edges_within": 2, "edges_measured": 9}
    labels, info = graph_duplicate_groups(edges_of, 8, [], dist_to, 1.0)
    assert labels.tolist() == [-1] * 8 and info == {"members": 0, "groups": 0, "edges_within": 0, "edges_measured": 0}


def test_complete_graph_gives_the_exact_groups_on_the_oracles_distances():
    n, dim = 60, 5
    x = np.random.default_rng(5).random((n, dim)).astype(np.float32)
    x[[7, 30, 55]] = x[7]
    x[41] = x[40] + np.float32(0.02)
    x[42] = x[40] + np.float32(0.04)
    for metric in ("sq_euclid", "cosine", "ucosine"):
        rows = x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32) if metric == "ucosine" else x
        dist = lambda own, cand: oracle.dist_query_rows(metric, rows, rows[own], np.asarray(cand, np.int32)) if len(cand) else np.zeros(0, np.float32)
        d_all = np.concatenate([dist(i, np.arange(n)) for i in range(n)])
        u = np.unique(d_all[d_all > 1e-6])
        k = 10 + int(np.argmax(u[11:21] / u[10:20]))                                  # a few pairs besides the plant, the radius in the
        r = float(np.sqrt(u[k] * u[k + 1]))                                           # widest gap there: no pair distance is near it
        complete = lambda i: [j for j in range(n) if j != i]
        for members in (np.arange(n), np.delete(np.arange(n), [7, 41])):
            got = graph_duplicate_groups(complete, n, members, dist, r)
            want = duplicate_groups(dist, n, members, r)
            assert got[0].tobytes() == want[0].tobytes() and got[1]["groups"] == want[1]["groups"] < members.size, metric
            assert got[1]["edges_measured"] == members.size * (members.size - 1)


def test_distances_from_range_lists():
    members = np.arange(8)
    ids, d = exact_range_by_id(dist_to, members, members, 1.0)
    table = dist_from_range_lists(members, ids, d)
    assert table(2, [1, 3, 4]).tolist() == [1.0, 1.0, np.inf] and table(2, [1]).dtype == np.float32
    got = graph_duplicate_groups(edges_of, 8, members, table, 1.0)
    want = graph_duplicate_groups(edges_of, 8, members, dist_to, 1.0)
    assert got[0].tolist() == want[0].tolist() and got[1] == want[1]
