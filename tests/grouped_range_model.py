"""RangeQuery with a group filter per query (range_query_grouped), restated: filtered_range_model's
filtered_range_batch run once per group -- the queries that name group g against the allow-set {id : row_group[id] == g} -- and
the lists put back in the caller's query order.  A row_group value outside [0, n_groups) puts the id in no group; ids past the
array's end are in no group.  HeapEmpty propagates: the loop of filtered calls fails at the first group whose call throws."""
import numpy as np

from filtered_range_model import HeapEmpty, filtered_range_batch, heap_empty_closed_form  # noqa: F401  (re-exported for the tests)


def group_mask(row_group, g, n):
    """The allow-set of group g over ids 0 .. n - 1 as a bool mask."""
    rg = np.asarray(row_group).reshape(-1)
    mask = np.zeros(n, dtype=bool)
    m = min(n, rg.shape[0])
    mask[:m] = rg[:m] == g
    return mask


def grouped_range(ix, rows, metric, queries, radius, row_group, query_group, n_groups=None):
    """(ids, dists): per query the filtered RangeQuery of its group, in the caller's order."""
    q = np.asarray(queries, dtype=np.float32)
    qg = np.asarray(query_group).reshape(-1)
    assert qg.shape[0] == q.shape[0]
    if n_groups is None:
        n_groups = max(int(np.asarray(row_group).max(initial=-1)), int(qg.max(initial=-1))) + 1
    assert ((qg >= 0) & (qg < n_groups)).all()
    ids, dists = [None] * q.shape[0], [None] * q.shape[0]
    for g in range(n_groups):
        which = np.flatnonzero(qg == g)
        if which.size == 0:
            continue
        a, d = filtered_range_batch(ix, rows, metric, q[which], radius, group_mask(row_group, g, rows.shape[0]))
        for w, ai, di in zip(which, a, d):
            ids[w], dists[w] = ai, di
    return ids, dists
