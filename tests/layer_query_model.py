"""A plain-Python restatement of the reference's queries on ANY layer, on the CPU oracle's graph:

  knn_at_layer     HNSWIndex.KnnQuery(query, k, filterFnc, layer)         HNSWIndex.cs:107-124
  range_at_layer   HNSWIndex.RangeQuery(query, range, filterFnc, layer)   HNSWIndex.cs:144-156
  multilayer_knn   HNSWIndex.MultiLayerKnnQuery(query, k, maxLayer, minLayer)   HNSWIndex.cs:173-187

FindEntryPointQuery(layer, query) descends, unfiltered, from the entry point's top layer down to but not including `layer`
(GraphNavigator.cs:39-45: OracleIndex.find_entry_point); SearchLayerQuery / SearchLayerRange then run on `layer`'s lists
(OracleIndex.edges(id, layer)) with the two BinaryHeaps of tests/filtered_model.py -- the layer-0 models of
tests/filtered_model.py and tests/filtered_range_model.py with the layer made an argument.  A layer below 0 or above the entry
point's MaxLayer indexes OutEdges out of range in the reference: LayerOutOfRange here.

MultiLayerKnnQuery is written on the oracle's own pieces: find_entry_point and search_layer (SearchLayer = SearchLayerQuery plus
locks, GraphNavigator.cs:123-256), a stable sort by float.CompareTo, candidates[0] leading on."""
import functools

import numpy as np

from filtered_model import FLOAT_MAX, BinaryHeap, closer_first, farther_first, float_compare_to, is_allowed
from filtered_range_model import HeapEmpty

INT_MAX = 2 ** 31 - 1


class LayerOutOfRange(Exception):
    """IndexOutOfRangeException / ArgumentOutOfRangeException / OverflowException of the reference."""


def top_layer(ix):
    return ix.max_layer(ix.entry_point)


def stable_by_dist(pairs):
    """OrderBy(c => c.Dist): a stable sort with float.CompareTo (NaN first, -0 == +0)."""
    return sorted(pairs, key=functools.cmp_to_key(lambda a, b: float_compare_to(a[1], b[1])))


def _check_layer(ix, layer):
    if layer < 0 or layer > top_layer(ix):
        raise LayerOutOfRange(layer)


def knn_at_layer(ix, rows, metric, q, k, min_nn, layer=0, mask=None):
    """One query: (ids[k], dists[k]), padded with -1 / NaN.  mask: bool mask indexed by id, or None (no filter)."""
    import oracle
    ids = np.full(max(k, 0), -1, dtype=np.int32)
    dists = np.full(max(k, 0), np.nan, dtype=np.float32)
    if ix.count <= 0 or k < 1:                            # :109, before `layer` is looked at
        return ids, dists
    _check_layer(ix, layer)
    q = np.ascontiguousarray(q, dtype=np.float32)
    ep = ix.find_entry_point(layer, q)                    # :116, not filtered
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
        fresh = [int(n) for n in ix.edges(c[0], layer) if int(n) not in visited]
        visited.update(fresh)
        if not fresh:
            continue
        ds = oracle.dist_query_rows(metric, rows, q, fresh)
        for n, d in zip(fresh, ds):
            d = float(d)
            if len(top) < kb or d < farthest:             # :233
                cand.push((n, d))
                if is_allowed(mask, n):                   # :238-239
                    top.push((n, d))
                if len(top) > kb:
                    top.pop()
                if len(top) > 0:
                    farthest = top.peek()[1]
    for j, (i, d) in enumerate(stable_by_dist(top.buf)[:k]):
        ids[j] = i
        dists[j] = np.float32(d)
    return ids, dists


def knn_at_layer_batch(ix, rows, metric, queries, k, min_nn, layer=0, mask=None):
    out = [knn_at_layer(ix, rows, metric, q, k, min_nn, layer, mask) for q in np.asarray(queries, dtype=np.float32)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def range_at_layer(ix, rows, metric, q, radius, layer=0, mask=None):
    """One query: (ids, dists) in the reference's order; raises HeapEmpty where the reference pops its empty heap."""
    import oracle
    if ix.count <= 0:                                     # :146
        return np.empty(0, dtype=np.int32), np.empty(0, dtype=np.float32)
    _check_layer(ix, layer)
    q = np.ascontiguousarray(q, dtype=np.float32)
    r = float(np.float32(radius))
    ep = ix.find_entry_point(layer, q)                    # :152, not filtered
    d_ep = float(oracle.dist_query_rows(metric, rows, q, [ep])[0])
    top, cand = BinaryHeap(farther_first), BinaryHeap(closer_first)
    farthest = FLOAT_MAX
    if is_allowed(mask, ep) and d_ep <= r:                # GraphNavigator.cs:271-275
        top.push((ep, d_ep))
        farthest = d_ep
    cand.push((ep, d_ep))
    visited = {ep}
    while len(cand):
        c = cand.peek()
        if c[1] > farthest and c[1] > r:                  # :286-289
            break
        cand.pop()
        for n in ix.edges(c[0], layer):                   # :294
            n = int(n)
            if n in visited:
                continue
            d = float(oracle.dist_query_rows(metric, rows, q, [n])[0])
            if d <= r:                                    # :302
                cand.push((n, d))
                if is_allowed(mask, n):                   # :307-308
                    top.push((n, d))
                peek = top.peek()[1] if len(top) else 0.0  # :310 reads default(NodeDistance) before the first push
                if peek > r:
                    if not len(top):
                        raise HeapEmpty("Heap is empty")
                    top.pop()
                if len(top):
                    farthest = top.peek()[1]
            visited.add(n)
    arr = stable_by_dist(top.buf)                         # HNSWIndex.cs:155
    return np.array([i for i, _ in arr], dtype=np.int32), np.array([d for _, d in arr], dtype=np.float32)


def range_at_layer_batch(ix, rows, metric, queries, radius, layer=0, mask=None):
    out = [range_at_layer(ix, rows, metric, q, radius, layer, mask) for q in np.asarray(queries, dtype=np.float32)]
    return [o[0] for o in out], [o[1] for o in out]


def multilayer_chain(ix, q, k, max_layer=None, min_layer=0):
    """The chain itself: (nslots, steps), steps = [(layer, entry id, ordered [(id, dist), ...]), ...] from the top down --
    `ordered` is the stably sorted SearchLayerQuery output of that step, whose first entry is the next step's entry."""
    max_layer = INT_MAX if max_layer is None else int(max_layer)
    if ix.count <= 0 or k < 1:                            # :176
        return 0, []
    if max_layer < -1 or min_layer < 0:                   # new List[negative]; OutEdges[-1]
        raise LayerOutOfRange((max_layer, min_layer))
    if max_layer == -1:                                   # an empty array, the loop never runs
        return 0, []
    q = np.ascontiguousarray(q, dtype=np.float32)
    top = top_layer(ix)
    ep = ix.find_entry_point(max_layer, q) if top >= max_layer else ix.entry_point   # :178
    first = min(top, max_layer)                           # == min(ep.MaxLayer, maxLayer): ep lives on layer maxLayer when top >= maxLayer
    steps = []
    for layer in range(first, min_layer - 1, -1):         # :180
        ids, ds = ix.search_layer(ep, layer, k, q)        # beam k, no filter, a fresh visited list
        ordered = stable_by_dist(list(zip(ids.tolist(), ds.tolist())))
        steps.append((layer, ep, ordered))
        ep = ordered[0][0]                                # :182
    return first + 1, steps


def multilayer_knn(ix, q, k, max_layer=None, min_layer=0):
    """One query: (ids, dists) of shape [nslots, k - 1]; slot L = layer L's candidates[1..], -1 / NaN where there are fewer and in
    the slots the loop never reached (null in the reference)."""
    nslots, steps = multilayer_chain(ix, q, k, max_layer, min_layer)
    per = max(k - 1, 0)
    ids = np.full((nslots, per), -1, dtype=np.int32)
    dists = np.full((nslots, per), np.nan, dtype=np.float32)
    for layer, _, ordered in steps:
        for j, (i, d) in enumerate(ordered[1:]):          # :183
            ids[layer, j] = i
            dists[layer, j] = np.float32(d)
    return ids, dists


def multilayer_knn_batch(ix, queries, k, max_layer=None, min_layer=0):
    queries = np.asarray(queries, dtype=np.float32)
    out = [multilayer_knn(ix, q, k, max_layer, min_layer) for q in queries]
    if not out:
        nslots, _ = (0, None) if ix.count <= 0 or k < 1 else (min(top_layer(ix), INT_MAX if max_layer is None else max_layer) + 1, None)
        return np.empty((0, max(nslots, 0), max(k - 1, 0)), dtype=np.int32), np.empty((0, max(nslots, 0), max(k - 1, 0)), dtype=np.float32)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
