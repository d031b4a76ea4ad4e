"""Reachability from the entry point over OUT-edges restated with numpy and a deque: what hnsw_mi355x_reachability,
hnsw_mi355x_unreachable_ids, hnsw_mi355x_hop_counts and the per-layer hnswdev_graph_reach_layer / hnswdev_graph_reach must return.

A graph is (levels[n], live[n] bool or None, layer_edges) as in graph_info_model.py: per layer a (counts[n], edges[n, stride]) pair in
the layout of Index.export_edges.  A layer's MEMBERS are the live ids with levels >= layer.  An entry u -> v counts only if both u and
v are members; a target that is no member (out of range, not live, below the layer) is ignored.  The count is clamped to
0 .. capacity, the capacity being the list's stride - 1 on the device (`cap`; None: the width of `edges`).

hops[n]: 0 for the member seeds, the BFS distance for what they reach, -1 for the other members, -2 for everything else."""
from collections import deque

import numpy as np

import graph_info_model as gm

FIELDS = ("layer_id", "nodes_count", "seeds", "reached", "max_hops")


def as_mask(n, ids_or_mask):
    """A bool mask of length n from a bool mask of any length (ids past its end are not in it) or a list of ids (ids >= n dropped)."""
    a = np.asarray(ids_or_mask)
    out = np.zeros(n, bool)
    if a.dtype == np.bool_:
        k = min(n, a.size)
        out[:k] = a.ravel()[:k]
    else:
        ids = a.astype(np.int64).ravel()
        out[ids[(ids >= 0) & (ids < n)]] = True
    return out


def out_degrees(levels, live, layer, counts, edges, cap=None):
    """The clamped count of every member's list, 0 elsewhere."""
    m = gm.members(levels, live, layer)
    cap = np.asarray(edges).shape[1] if cap is None else min(cap, np.asarray(edges).shape[1])
    return np.where(m, np.clip(np.asarray(counts, np.int64), 0, cap), 0)


def reach_layer(levels, live, layer, counts, edges, seeds, cap=None):
    """hops[n] of one layer from `seeds` (a bool mask or an id list; seeds that are no members are ignored)."""
    m = gm.members(levels, live, layer)
    n = m.size
    deg = out_degrees(levels, live, layer, counts, edges, cap)
    edges = np.asarray(edges)
    hops = np.where(m, -1, -2).astype(np.int32)
    start = np.nonzero(as_mask(n, seeds) & m)[0]
    hops[start] = 0
    todo = deque(start.tolist())
    while todo:
        u = todo.popleft()
        for v in edges[u, :deg[u]].tolist():
            if 0 <= v < n and m[v] and hops[v] == -1:
                hops[v] = hops[u] + 1
                todo.append(v)
    return hops


def summary(hops):
    """members, reached and the largest hop of a hop array (the seeds are its zeros)."""
    reached = hops >= 0
    return dict(nodes_count=int((hops >= -1).sum()), seeds=int((hops == 0).sum()), reached=int(reached.sum()),
                max_hops=int(hops[reached].max()) if reached.any() else 0)


def expanded_entries(levels, live, layer, counts, edges, hops, cap=None):
    """List entries the expansions read: the sum of the clamped out-degrees over the REACHED members -- each is expanded exactly once."""
    return int(out_degrees(levels, live, layer, counts, edges, cap)[hops >= 0].sum())


def rounds(hops):
    """Expansion launches of one layer: one per BFS level, the last of which finds nothing new; none when nothing was reached."""
    return int(hops.max()) + 1 if (hops >= 0).any() else 0


def reach_chain(levels, live, layer_edges, entry_point, min_layer=0, cap0=None, capU=None):
    """The chain F_top = reach_top({entry_point}), F_L = reach_L(F_{L+1}) down to min_layer: (per-layer dicts for min_layer .. top in
    ascending layer order, hops[n] of min_layer, per-layer hop arrays by layer).  top is the entry point's level; of an entry point
    out of range -- it reaches nothing -- the largest level."""
    levels = np.asarray(levels)
    n = levels.size
    in_range = 0 <= entry_point < n
    top = int(levels[entry_point]) if in_range else int(levels.max())
    seeds = np.zeros(n, bool)
    if in_range:
        seeds[entry_point] = True
    per_layer, all_hops = {}, {}
    hops = None
    for layer in range(top, min_layer - 1, -1):
        counts, edges = layer_edges[layer]
        hops = reach_layer(levels, live, layer, counts, edges, seeds, cap0 if layer == 0 else capU)
        per_layer[layer] = dict(layer_id=layer, **summary(hops))
        all_hops[layer] = hops
        seeds = hops >= 0
    return [per_layer[L] for L in range(min_layer, top + 1)], hops, all_hops


def unreachable_ids(hops):
    """The members outside the reached set, ascending."""
    return np.nonzero(hops == -1)[0].astype(np.int32)
