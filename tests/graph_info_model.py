"""HNSWIndex.GetInfo / GetConnectedComponentCounts restated in numpy (src/HNSWIndex/HNSWInfo.cs:5-53, GraphNavigator.cs:331-419):
what hnsw_mi355x_get_info / hnsw_mi355x_connected_component_counts and their per-layer hnswdev_* forms must return.

A graph is (levels[n], live[n] bool, layer_edges): per layer a (counts[n], edges[n, stride]) pair in the layout of Index.export_edges
(counts are ignored where the node is no member).  A layer's MEMBERS are the live ids with levels >= layer.  out_deg(v) is the count
word of v's list, whatever the entries point to; in_deg(v) counts the entries u -> v over members u, for a member v; an entry whose
target is no member (out of range, not live, below the layer) is ignored for in-degrees and for connectivity."""
import numpy as np

FIELDS = ("layer_id", "nodes_count", "max_out_edges", "min_out_edges", "max_in_edges", "min_in_edges", "out_edges_median",
          "in_edges_median", "avg_out_edges", "avg_in_edges")


def median(values):
    """HNSWInfo.LayerInfo.Median (HNSWInfo.cs:45-51): ascending; an odd count takes sorted[n / 2], an even count the integer mean
    (sorted[n / 2 - 1] + sorted[n / 2]) / 2."""
    s = sorted(int(v) for v in values)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) // 2


def average(values):
    """LINQ's Average over ints: the sum as int64, converted to double, divided by the count."""
    v = np.asarray(values, dtype=np.int64)
    return float(np.float64(v.sum(dtype=np.int64)) / np.float64(v.size))


def members(levels, live, layer):
    levels = np.asarray(levels)
    live = np.ones(levels.size, bool) if live is None else np.asarray(live, bool)
    return live & (levels >= layer)


def member_edges(levels, live, layer, counts, edges):
    """(member mask, out_deg[n], (u, v) of every entry between two members, duplicates kept)."""
    m = members(levels, live, layer)
    n = m.size
    counts, edges = np.asarray(counts), np.asarray(edges)
    out_deg = np.where(m, counts, 0).astype(np.int64)
    slot = np.arange(edges.shape[1])[None, :] < out_deg[:, None]
    u = np.broadcast_to(np.arange(n)[:, None], edges.shape)[slot]
    v = edges[slot].astype(np.int64)
    ok = (v >= 0) & (v < n)
    ok[ok] = m[v[ok]]
    return m, out_deg, u[ok], v[ok]


def in_degrees(levels, live, layer, counts, edges):
    m, _, _, v = member_edges(levels, live, layer, counts, edges)
    return np.bincount(v, minlength=m.size).astype(np.int64)


def layer_info(levels, live, layer, counts, edges, with_in_edges=True):
    """HNSWInfo.LayerInfo of one layer as a dict of hnsw_mi355x_layer_info's fields.  No member: every statistic 0."""
    m, out_deg, _, v = member_edges(levels, live, layer, counts, edges)
    info = dict.fromkeys(FIELDS, 0)
    info["avg_out_edges"] = info["avg_in_edges"] = 0.0
    info["layer_id"] = layer
    if not m.any():
        return info
    o = out_deg[m]
    info.update(nodes_count=int(m.sum()), max_out_edges=int(o.max()), min_out_edges=int(o.min()), avg_out_edges=average(o),
                out_edges_median=median(o))
    if with_in_edges:
        i = np.bincount(v, minlength=m.size)[m]
        info.update(max_in_edges=int(i.max()), min_in_edges=int(i.min()), avg_in_edges=average(i), in_edges_median=median(i))
    return info


def entries(levels, live, layer, counts, edges):
    """List entries the layer's pass reads: the sum of the members' out-degrees."""
    return int(member_edges(levels, live, layer, counts, edges)[1].sum())


def components(levels, live, layer, counts, edges):
    """Weakly connected components among the layer's members (CountWeaklyConnectedComponentsAtLayer, GraphNavigator.cs:350-419)."""
    m, _, u, v = member_edges(levels, live, layer, counts, edges)
    parent = list(range(m.size))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(u.tolist(), v.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return sum(1 for i in np.nonzero(m)[0].tolist() if parent[i] == i)


def get_info(levels, live, layer_edges, top, with_in_edges=True):
    """HNSWIndex.GetInfo(): layers 0 .. top (top = the entry point's level)."""
    return [layer_info(levels, live, L, *layer_edges[L], with_in_edges=with_in_edges) for L in range(top + 1)]


def component_counts(levels, live, layer_edges, top):
    """HNSWIndex.GetConnectedComponentCounts(): layers 0 .. top."""
    return [components(levels, live, L, *layer_edges[L]) for L in range(top + 1)]
