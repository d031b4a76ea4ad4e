"""The contract of knn_query_grouped (include/hnsw_mi355x.h hnsw_mi355x_knn_query_grouped) in plain Python, on the CPU oracle's graph:
for every group g the queries with query_group == g are answered by the filtered KnnQuery of tests/filtered_model.py with the
allow-set {id : row_group[id] == g}, and their rows are scattered back to the queries' places.  row_group[id] is an id's group; a
value outside 0 .. n_groups - 1, or an id past the array's end, has no group."""
import numpy as np

from filtered_model import filtered_knn_batch


def group_mask(row_group, g, n_groups, n):
    """The allow-set of group g as a bool mask over ids 0 .. n - 1."""
    rg = np.asarray(row_group, dtype=np.int64).ravel()[:n]
    mask = np.zeros(n, dtype=bool)
    if 0 <= g < n_groups:
        mask[:rg.size] = rg == g
    return mask


def check_group_args(row_group, query_group, n_groups, nq):
    qg = np.asarray(query_group, dtype=np.int64).ravel()
    if qg.size != nq:
        raise ValueError(f"query_group has {qg.size} entries for {nq} queries")
    if not 1 <= n_groups <= 65536:
        raise ValueError(f"n_groups = {n_groups} is outside 1 .. 65536")
    if qg.size and (qg.min() < 0 or qg.max() >= n_groups):
        raise ValueError("query_group outside 0 .. n_groups - 1")
    return qg


def grouped_knn_batch(ix, rows, metric, queries, k, min_nn, row_group, query_group, n_groups):
    """(ids[nq, k], dists[nq, k]).  ix: an oracle.OracleIndex holding `rows` (metric and rows as tests/filtered_model.py takes
    them); a query whose group holds no id gets a row of padding."""
    queries = np.asarray(queries, dtype=np.float32)
    qg = check_group_args(row_group, query_group, n_groups, queries.shape[0])
    ids = np.full((queries.shape[0], max(k, 0)), -1, dtype=np.int32)
    dists = np.full((queries.shape[0], max(k, 0)), np.nan, dtype=np.float32)
    if k < 1:
        return ids, dists
    for g in np.unique(qg):
        mask = group_mask(row_group, int(g), n_groups, rows.shape[0])
        sel = qg == g
        if mask.any():
            ids[sel], dists[sel] = filtered_knn_batch(ix, rows, metric, queries[sel], k, min_nn, mask)
    return ids, dists
