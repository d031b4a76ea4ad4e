"""repair_reachability restated with numpy on top of graph_reach_model.py: what hnsw_mi355x_repair_reachability and
the per-round hnswdev_graph_repair_propose must return.

A graph is (levels[n], live[n] bool or None, layer_edges) as in graph_reach_model.py; layer_edges[L] = (counts[n], edges[n, stride]).
Two functions are plugged in, so that the rule is tested apart from the arithmetic:
    cand_fn(layer, U, reached_mask, C) -> int array [len(U), C]: per u the C nearest reached members by (distance, id), padded with -1
    dist_fn(a_ids, b_ids) -> float32 array: the metric's value for stored rows a_ids[i], b_ids[i]
A slot code is a 0-based position in the candidate's list: the count for an append, the evicted entry's position, -1 for "nowhere"."""
import numpy as np

import graph_info_model as gm
import graph_reach_model as rm

FIELDS = ("layer_id", "unreachable_before", "linked", "evicted", "rounds", "unreachable_after")


def propose(levels, live, layer, counts, edges, hops, cand_ids, pair_dist, max_edges, cap=None):
    """codes[len(U), C] for the candidates cand_ids[len(U), C] (-1: padding, code -1) from the lists as they stand.  pair_dist is
    dist_fn; cap the capacity that clamps a count (None: the width of `edges`).  Also returns how many distances were measured."""
    m = gm.members(levels, live, layer)
    n = m.size
    deg = rm.out_degrees(levels, live, layer, counts, edges, cap)
    edges = np.asarray(edges)
    cand_ids = np.asarray(cand_ids, np.int64)
    codes = np.full(cand_ids.shape, -1, np.int32)
    measured = 0
    memo = {}
    for idx in np.ndindex(*cand_ids.shape):
        v = int(cand_ids[idx])
        if v < 0 or v >= n or not m[v]:
            continue
        if v not in memo:
            c = int(deg[v])
            if c < max_edges:
                memo[v] = (c, 0)
            else:
                slots = [s for s in range(c) if 0 <= edges[v, s] < n and m[edges[v, s]] and 0 <= hops[edges[v, s]] <= hops[v]]
                best, best_d = -1, None
                if slots:
                    d = np.asarray(pair_dist(np.full(len(slots), v, np.int32), edges[v, slots].astype(np.int32)), np.float32)
                    for s, ds in zip(slots, d):          # ascending slots: >= lets the larger slot win among equal distances
                        if not np.isnan(ds) and (best < 0 or ds >= best_d):
                            best, best_d = s, ds
                memo[v] = (best, len(slots))
        codes[idx] = memo[v][0]
        measured += memo[v][1]
    return codes, measured


def apply_round(counts, edges, U, cand_ids, codes, max_edges=None):
    """The apply step on copies of (counts, edges): U ascending, u takes its first candidate with a code whose list nobody has taken
    in this round.  A list that is longer than max_edges (a foreign snapshot may hold MaxEdges + 1 entries) is left alone.
    (counts, edges, linked, evicted, changed list owners in the order they were changed)."""
    counts, edges = np.array(counts, np.int32), np.array(edges, np.int32)
    claimed, linked, evicted = [], 0, 0
    taken = set()
    for i, u in enumerate(np.asarray(U).tolist()):
        for v, code in zip(np.asarray(cand_ids)[i].tolist(), np.asarray(codes)[i].tolist()):
            if v < 0 or code < 0 or v in taken or (max_edges is not None and counts[v] > max_edges):
                continue
            if code == counts[v]:
                counts[v] += 1
            else:
                evicted += 1
            edges[v, code] = u
            linked += 1
            taken.add(v)
            claimed.append(v)
            break
    return counts, edges, linked, evicted, claimed


def repair_layer(levels, live, layer, counts, edges, seeds, cand_fn, dist_fn, max_edges, cands=8, max_rounds=8, cap=None, check=None):
    """One layer: (counts, edges, report dict without layer_id, final hops).  check(hops_before, hops_after), if given, is called
    after every round that changed a list."""
    counts, edges = np.array(counts, np.int32), np.array(edges, np.int32)
    rep = dict(unreachable_before=0, linked=0, evicted=0, rounds=0, unreachable_after=0)
    hops = None
    for r in range(max_rounds):
        hops = rm.reach_layer(levels, live, layer, counts, edges, seeds, cap)
        U = rm.unreachable_ids(hops)
        if r == 0:
            rep["unreachable_before"] = int(U.size)
        rep["unreachable_after"] = int(U.size)
        if U.size == 0:
            break
        rep["rounds"] += 1
        cd = np.asarray(cand_fn(layer, U, hops >= 0, cands), np.int32).reshape(U.size, cands)
        codes, _ = propose(levels, live, layer, counts, edges, hops, cd, dist_fn, max_edges, cap)
        counts, edges, linked, evicted, claimed = apply_round(counts, edges, U, cd, codes, max_edges)
        rep["linked"] += linked
        rep["evicted"] += evicted
        if not claimed:
            break
        after = rm.reach_layer(levels, live, layer, counts, edges, seeds, cap)
        if check:
            check(hops, after)
        hops = after
        rep["unreachable_after"] = int((hops == -1).sum())
    return counts, edges, rep, hops


def repair(levels, live, layer_edges, entry_point, cand_fn, dist_fn, max_edges, cands=8, max_rounds=8, check=None):
    """The whole call: (new layer_edges, per-layer reports in ascending layer order).  max_edges: M (2 M on layer 0)."""
    levels = np.asarray(levels)
    n = levels.size
    top = int(levels[entry_point])
    seeds = np.zeros(n, bool)
    seeds[entry_point] = True
    out = [(np.array(c, np.int32), np.array(e, np.int32)) for c, e in layer_edges]
    reports = {}
    for layer in range(top, -1, -1):
        counts, edges = out[layer]
        me = max_edges * 2 if layer == 0 else max_edges
        counts, edges, rep, hops = repair_layer(levels, live, layer, counts, edges, seeds, cand_fn, dist_fn, me, cands, max_rounds, None, check)
        out[layer] = (counts, edges)
        reports[layer] = dict(layer_id=layer, **rep)
        seeds = hops >= 0
    return out, [reports[L] for L in range(top + 1)]


def nearest_by_rows(rows, query_dist):
    """A cand_fn from query_dist(q_row, ids) -> float32 distances: np.lexsort((ids, dist)) over the reached members."""
    def cand_fn(layer, U, reached, C):
        ids = np.nonzero(reached)[0].astype(np.int32)
        out = np.full((len(U), C), -1, np.int32)
        for i, u in enumerate(np.asarray(U).tolist()):
            if ids.size:
                d = np.asarray(query_dist(rows[u], ids), np.float32)
                order = np.lexsort((ids, d))[:C]
                out[i, :order.size] = ids[order]
        return out
    return cand_fn
