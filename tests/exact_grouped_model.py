"""The reference of hnsw_mi355x_exact_knn_query_grouped / hnswdev_exact_knn_grouped: exact_knn_model.exact_knn one
group at a time.  Query i is answered from the candidates of its group -- the live ids j < len(row_group) with
row_group[j] == query_group[i]; a row_group value outside [0, n_groups) is in no group -- and the rows go back to the caller's order."""
import numpy as np

from exact_knn_model import PAD_ID, exact_knn


def group_mask(row_group, g, n_groups):
    """The bool mask (indexed by id) of group g's members; ids past the array's end are in none."""
    rg = np.asarray(row_group, dtype=np.int64).reshape(-1)
    return (rg == g) if 0 <= g < n_groups else np.zeros(rg.size, bool)


def members(n, row_group, n_groups, live=None):
    """Per group the number of candidate ids among n rows (live: None = 0 .. n-1)."""
    rg = np.asarray(row_group, dtype=np.int64).reshape(-1)[:n]
    ok = (rg >= 0) & (rg < n_groups)
    if live is not None:
        alive = np.zeros(n, bool)
        alive[np.asarray(live, dtype=np.int64)] = True
        ok &= alive[:rg.size]
    return np.bincount(rg[ok], minlength=n_groups).astype(np.int64)


def exact_knn_grouped(metric, x, q, k, row_group, query_group, n_groups, live=None):
    """(ids [nq, k] int32, dists [nq, k] float32): the model's answer."""
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    qg = np.asarray(query_group, dtype=np.int64).reshape(-1)
    assert qg.size == q.shape[0] and ((qg >= 0) & (qg < n_groups)).all()
    ids = np.full((q.shape[0], k), PAD_ID, dtype=np.int32)
    d = np.full((q.shape[0], k), np.nan, dtype=np.float32)
    for g in np.unique(qg):
        sel = np.flatnonzero(qg == g)
        ids[sel], d[sel] = exact_knn(metric, x, q[sel], k, mask=group_mask(row_group, int(g), n_groups), live=live)
    return ids, d


def evals(n, row_group, query_group, n_groups, live=None):
    """(query, row) pairs the call measures: the sum over the queries of the candidates of their groups."""
    return int(members(n, row_group, n_groups, live)[np.asarray(query_group, dtype=np.int64)].sum())


def info(n, row_group, query_group, n_groups, live=None):
    """(groups scanned, ids listed) of one call: groups with a query and a candidate; ids that are in a group."""
    m = members(n, row_group, n_groups, live)
    named = np.bincount(np.asarray(query_group, dtype=np.int64), minlength=n_groups) > 0
    return int((named & (m > 0)).sum()), int(m.sum())
