"""A plain-Python restatement of RangeQuery with a filter at layer 0 (HNSWIndex.RangeQuery(query, range, filterFnc),
HNSWIndex.cs:144-156, and GraphNavigator.SearchLayerRange, GraphNavigator.cs:262-325), on the CPU oracle's graph: the unfiltered
descent by OracleIndex.find_entry_point, adjacency by OracleIndex.edges, distances by oracle.dist_query_rows, and the two
BinaryHeaps of tests/filtered_model.py.  The filter is an allow-set over ids (a bool mask indexed by id; ids past its end are not
allowed; None: no filter).

Where the reference pops its empty top heap -- a disallowed in-range neighbour met before any push, with range < 0, so that
Peek() reads buffer[0] = default(NodeDistance) (distance 0) -- the model raises HeapEmpty, as BinaryHeap.Pop throws
InvalidOperationException("Heap is empty") (BinaryHeap.cs:56)."""
import numpy as np

from filtered_model import FLOAT_MAX, BinaryHeap, closer_first, farther_first, is_allowed


class HeapEmpty(Exception):
    """InvalidOperationException("Heap is empty")."""


def filtered_range(ix, rows, metric, q, radius, mask):
    """One query: (ids, dists) of the filtered RangeQuery in the reference's order; raises HeapEmpty where it throws."""
    import oracle
    q = np.ascontiguousarray(q, dtype=np.float32)
    r = float(np.float32(radius))
    ep = ix.find_entry_point(0, q)                        # FindEntryPointQuery: NOT filtered (HNSWIndex.cs:152)
    d_ep = float(oracle.dist_query_rows(metric, rows, q, [ep])[0])
    top, cand = BinaryHeap(farther_first), BinaryHeap(closer_first)
    farthest = FLOAT_MAX                                  # :269
    if is_allowed(mask, ep) and d_ep <= r:                # :271-275
        top.push((ep, d_ep))
        farthest = d_ep
    cand.push((ep, d_ep))                                 # :277
    visited = {ep}
    while len(cand):
        c = cand.peek()                                   # :285
        if c[1] > farthest and c[1] > r:                  # :286-289
            break
        cand.pop()
        for n in ix.edges(c[0], 0):                       # :294
            n = int(n)
            if n in visited:
                continue
            d = float(oracle.dist_query_rows(metric, rows, q, [n])[0])
            if d <= r:                                    # :302
                cand.push((n, d))                         # :305
                if is_allowed(mask, n):                   # :307-308
                    top.push((n, d))
                peek = top.peek()[1] if len(top) else 0.0  # :310 -- buffer[0] is default(NodeDistance) before the first push
                if peek > r:
                    if not len(top):
                        raise HeapEmpty("Heap is empty")
                    top.pop()
                if len(top):                              # :313-314
                    farthest = top.peek()[1]
            visited.add(n)                                # :318
    arr = sorted(top.buf, key=lambda e: e[1])             # OrderBy(Dist): stable over the heap array (HNSWIndex.cs:155)
    return np.array([i for i, _ in arr], dtype=np.int32), np.array([d for _, d in arr], dtype=np.float32)


def filtered_range_batch(ix, rows, metric, queries, radius, mask):
    """BatchRangeQuery: per query (ids, dists); raises HeapEmpty if any query does (Parallel.For rethrows)."""
    out = [filtered_range(ix, rows, metric, q, radius, mask) for q in np.asarray(queries, dtype=np.float32)]
    return [o[0] for o in out], [o[1] for o in out]


def heap_empty_closed_form(ix, rows, metric, q, radius, mask):
    """Rule 5 without the traversal: the reference throws iff range < 0, the entry point is not both allowed and in range, its
    distance is not +inf, and the first id of its layer-0 list within range is disallowed."""
    import oracle
    r = float(np.float32(radius))
    if not r < 0:
        return False
    q = np.ascontiguousarray(q, dtype=np.float32)
    ep = ix.find_entry_point(0, q)
    d_ep = float(oracle.dist_query_rows(metric, rows, q, [ep])[0])
    if (is_allowed(mask, ep) and d_ep <= r) or d_ep == float("inf"):
        return False
    for n in ix.edges(ep, 0):
        n = int(n)
        if n == ep:
            continue
        if float(oracle.dist_query_rows(metric, rows, q, [n])[0]) <= r:
            return not is_allowed(mask, n)
    return False
