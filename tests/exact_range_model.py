"""The reference of hnsw_mi355x_exact_range_query / hnswdev_exact_range: the candidates and the oracle's
distances of tests/exact_knn_model.py; per query every candidate with d <= radius (the IEEE float compare: a NaN distance or a
NaN radius admits nothing, -0.0 admits distance 0, +inf admits +inf), ascending by (distance, id) -- np.lexsort((ids, dist))."""
import numpy as np

from exact_knn_model import candidates, distances


def within(dist, ids, radius):
    """(ids, dists) of one query: the entries of dist (one per id) within the radius, in (distance, id) order; -0 as +0."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        keep = dist <= np.float32(radius)
    d, i = dist[keep] + np.float32(0.0), ids[keep]     # x + 0.0 turns -0 into +0 and leaves every other number as it is
    order = np.lexsort((i, d))
    return i[order], d[order]


def exact_range(metric, x, q, radius, mask=None, live=None):
    """(list of int32 id arrays, list of float32 distance arrays), one pair per query: the model's answer."""
    ids = candidates(np.shape(x)[0], mask, live)
    d = distances(metric, x, q, ids)
    out = [within(d[i], ids, radius) for i in range(d.shape[0])]
    return [o[0] for o in out], [o[1] for o in out]
