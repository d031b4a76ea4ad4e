"""A plain-Python restatement of KnnQuery with a filter at layer 0 (HNSWIndex.KnnQuery(query, k, filterFnc),
HNSWIndex.cs:107-124, and GraphNavigator.SearchLayerQuery, GraphNavigator.cs:194-256), on the CPU oracle's graph:
descent by OracleIndex.find_entry_point, adjacency by OracleIndex.edges, distances by oracle.dist_query_rows, and the two
BinaryHeaps (BinaryHeap.cs:30-107) with float.CompareTo order.  The filter is an allow-set over ids (a bool mask indexed by id;
ids past its end are not allowed)."""
import math

import numpy as np

FLOAT_MAX = float(np.finfo(np.float32).max)


def float_compare_to(x, y):
    """float.CompareTo: NaN sorts below everything, NaN == NaN, -0 == +0."""
    if x < y:
        return -1
    if x > y:
        return 1
    if x == y:
        return 0
    if math.isnan(x):
        return 0 if math.isnan(y) else -1
    return 1


def farther_first(a, b):
    """DistanceComparer (DistanceComparer.cs:9-14): the root is the farthest."""
    return float_compare_to(a[1], b[1])


def closer_first(a, b):
    """ReverseDistanceComparer (DistanceComparer.cs:20-25): the root is the closest."""
    return float_compare_to(b[1], a[1])


class BinaryHeap:
    """BinaryHeap.cs:30-107: SiftUp stops on cmp <= 0; SiftDown takes the right child only if left < right strictly and stops on
    cmp <= 0.  Entries are (id, distance)."""

    def __init__(self, cmp):
        self.cmp = cmp
        self.buf = []

    def __len__(self):
        return len(self.buf)

    def peek(self):
        return self.buf[0]

    def push(self, item):
        b = self.buf
        b.append(item)
        i = len(b) - 1
        while i > 0:
            p = (i - 1) >> 1
            if self.cmp(item, b[p]) <= 0:
                break
            b[i] = b[p]
            i = p
        b[i] = item

    def pop(self):
        b = self.buf
        result = b[0]
        item = b.pop()
        n = len(b)
        if n:
            i, half = 0, n >> 1
            while i < half:
                left = 2 * i + 1
                right = left + 1
                mc = right if right < n and self.cmp(b[left], b[right]) < 0 else left
                if self.cmp(b[mc], item) <= 0:
                    break
                b[i] = b[mc]
                i = mc
            b[i] = item
        return result


def is_allowed(mask, i):
    return mask is None or (0 <= i < len(mask) and bool(mask[i]))


def filtered_knn(ix, rows, metric, q, k, min_nn, mask):
    """One query: (ids[k], dists[k]) of the filtered KnnQuery, padded with -1 / NaN (HNSWIndexExports.cs:144).
    ix: an oracle.OracleIndex holding `rows`; mask: bool mask indexed by id, or None (no filter)."""
    import oracle
    q = np.ascontiguousarray(q, dtype=np.float32)
    ep = ix.find_entry_point(0, q)                        # FindEntryPointQuery(layer, query): NOT filtered (HNSWIndex.cs:116)
    d_ep = float(oracle.dist_query_rows(metric, rows, q, [ep])[0])
    kb = max(min_nn, k)                                   # :115
    top, cand = BinaryHeap(farther_first), BinaryHeap(closer_first)
    visited = {ep}
    farthest = FLOAT_MAX
    if is_allowed(mask, ep):                              # GraphNavigator.cs:203-211
        top.push((ep, d_ep))
        farthest = d_ep
    cand.push((ep, d_ep))
    while len(cand):
        c = cand.pop()
        if c[1] > farthest and len(top) >= kb:            # :218
            break
        fresh = [int(n) for n in ix.edges(c[0], 0) if int(n) not in visited]
        visited.update(fresh)
        if not fresh:
            continue
        ds = oracle.dist_query_rows(metric, rows, q, fresh)
        for n, d in zip(fresh, ds):
            d = float(d)
            if len(top) < kb or d < farthest:             # :233
                cand.push((n, d))                         # :236
                if is_allowed(mask, n):                   # :238-239
                    top.push((n, d))
                if len(top) > kb:
                    top.pop()
                if len(top) > 0:                          # :244-245
                    farthest = top.peek()[1]
    arr = sorted(top.buf, key=lambda e: e[1])             # OrderBy(Dist): stable over the heap array (:119-123)
    ids = np.full(k, -1, dtype=np.int32)
    dists = np.full(k, np.nan, dtype=np.float32)
    for j, (i, d) in enumerate(arr[:k]):
        ids[j] = i
        dists[j] = np.float32(d)
    return ids, dists


def filtered_knn_batch(ix, rows, metric, queries, k, min_nn, mask):
    out = [filtered_knn(ix, rows, metric, q, k, min_nn, mask) for q in np.asarray(queries, dtype=np.float32)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
