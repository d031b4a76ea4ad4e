"""The reference of hnsw_mi355x_exact_knn_query / hnswdev_exact_knn: every candidate measured with the oracle's
metric (oracle.dist_query_rows -- the reference's arithmetic, bit for bit) and the k smallest taken in (distance, id) order,
np.lexsort((ids, dist)): distances as IEEE numbers (-0 == +0), NaN after +inf, equal distances and NaNs by id."""
import numpy as np

PAD_ID = -1


def select(dist, ids, k):
    """(ids [k], dists [k]) of the k candidates of smallest (distance, id), padded with -1 / NaN."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.int32)
    order = np.lexsort((ids, dist))[:k]
    out_ids = np.full(k, PAD_ID, dtype=np.int32)
    out_d = np.full(k, np.nan, dtype=np.float32)
    out_ids[:order.size] = ids[order]
    out_d[:order.size] = dist[order]
    return out_ids, out_d


def stored(metric, x):
    """(base metric, rows as the index stores them): X_f16 is X on the rows rounded to binary16."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if metric.endswith("_f16"):
        with np.errstate(over="ignore"):
            return metric[:-4], x.astype(np.float16).astype(np.float32)
    return metric, x


def candidates(n, mask=None, live=None):
    """Candidate ids: live (None: 0 .. n-1) and allowed by the bool mask indexed by id (ids past its end are not allowed)."""
    ids = np.arange(n, dtype=np.int32) if live is None else np.sort(np.asarray(live, dtype=np.int32))
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        ids = ids[ids < mask.size]
        ids = ids[mask[ids]]
    return ids


def distances(metric, x, q, ids):
    """[nq, len(ids)] distances of the candidates, from the oracle."""
    import oracle
    base, rows = stored(metric, x)
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    out = np.empty((q.shape[0], ids.size), dtype=np.float32)
    for i in range(q.shape[0]):
        if ids.size:
            out[i] = oracle.dist_query_rows(base, rows, q[i], ids)
    return out


def exact_knn(metric, x, q, k, mask=None, live=None):
    """(ids [nq, k] int32, dists [nq, k] float32): the model's answer."""
    ids = candidates(np.shape(x)[0], mask, live)
    d = distances(metric, x, q, ids)
    out = [select(d[i], ids, k) for i in range(d.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def boundary_tie(metric, x, q, k, mask=None, live=None):
    """True when, for some query, the candidates of rank k-1 and k (0-based) have equal distances: the tie the id order decides."""
    ids = candidates(np.shape(x)[0], mask, live)
    if ids.size <= k:
        return False
    d = distances(metric, x, q, ids)
    for row in d:
        s = row[np.lexsort((ids, row))]
        if s[k - 1] == s[k]:
            return True
    return False
