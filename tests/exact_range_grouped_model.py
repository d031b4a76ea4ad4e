"""The reference of hnsw_mi355x_exact_range_query_grouped / hnswdev_exact_range_grouped: exact_range_model.exact_range
one group at a time.  Query i is answered from the candidates of its group -- the live ids j < len(row_group) with
row_group[j] == query_group[i]; a row_group value outside [0, n_groups) is in no group -- and the lists go back to the caller's order."""
import numpy as np

from exact_grouped_model import group_mask
from exact_knn_model import candidates
from exact_range_model import exact_range, within


def from_matrix(dist, radius, row_group, query_group, n_groups, live=None):
    """exact_range_grouped from a matrix the caller computed once (dist[i, j]: query i to id j, exact_knn_model.distances over
    ids 0 .. n-1): the same candidates, compare and order, for tests that ask many radii of one data set."""
    dist = np.atleast_2d(np.asarray(dist, dtype=np.float32))
    ids, d = [], []
    for i, g in enumerate(np.asarray(query_group, dtype=np.int64).reshape(-1)):
        c = candidates(dist.shape[1], group_mask(row_group, int(g), n_groups), live)
        a, b = within(dist[i, c], c, radius)
        ids.append(a)
        d.append(b)
    return ids, d


def exact_range_grouped(metric, x, q, radius, row_group, query_group, n_groups, live=None):
    """(list of int32 id arrays, list of float32 distance arrays), one pair per query in the caller's order: the model's answer."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    qg = np.asarray(query_group, dtype=np.int64).reshape(-1)
    assert qg.size == q.shape[0] and ((qg >= 0) & (qg < n_groups)).all()
    ids, d = [None] * qg.size, [None] * qg.size
    for g in np.unique(qg):
        sel = np.flatnonzero(qg == g)
        g_ids, g_d = exact_range(metric, x, q[sel], radius, mask=group_mask(row_group, int(g), n_groups), live=live)
        for j, i in enumerate(sel):
            ids[i], d[i] = g_ids[j], g_d[j]
    return ids, d
