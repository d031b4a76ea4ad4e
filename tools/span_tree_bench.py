#!/usr/bin/env python3
"""single_linkage_tree at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128) with the rows and the plant
of tools/near_dup_bench.py (1 % of the rows are near-duplicates of other rows), over the first 131 072 ids, all in one session:
    single_linkage_tree                 Boruvka's rounds on the device; info says rounds, pairs measured and skipped, launches
    duplicate_groups at one radius      one scan of the same triangle: the tree's cost is compared with this x rounds
    single_linkage_cut                  the host pass that reads one radius off the tree; its labels must be duplicate_groups'
    the composition the call replaces   exact_knn_graph's loop (exact_knn_query_by_id in pieces, k = 16, the members as the candidates)
                                        plus Kruskal in numpy over its edges, at --small members (a k-NN graph need not be connected,
                                        so it gives a spanning forest of that graph, not necessarily the tree)
Per line: the median wall time of --steps calls after one warm-up call.  The call reports totals over its rounds; a split per round
is not reported (out_info has no per-round slots).  The file is rewritten after every line.
    python tools/span_tree_bench.py [--out profiles/span_tree_c2.json] [--steps 5]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def median_ms(f, steps):
    out = f()   # warm-up (a first call allocates its scratch)
    walls = []
    for _ in range(steps):
        t = time.perf_counter()
        out = f()
        walls.append(time.perf_counter() - t)
    return out, round(1e3 * float(np.median(walls)), 3), [round(1e3 * w, 3) for w in walls]


def knn_graph_forest(ix, members, k):
    """exact_knn_graph's edges, each once as (a < b) with the distance from a's list where it has one, and Kruskal over them."""
    ids = np.full((members.size, k), -1, np.int32)
    d = np.full((members.size, k), np.nan, np.float32)
    for at in range(0, members.size, 65536):                     # exact_knn_graph's pieces, with the members as the candidates
        ids[at:at + 65536], d[at:at + 65536] = ix.exact_knn_query_by_id(members[at:at + 65536], k, allowed=members)
    a = np.repeat(members, k)
    b, d = ids.ravel(), d.ravel()
    keep = b >= 0
    a, b, d = a[keep], b[keep], d[keep]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    order = np.lexsort((hi, lo, d))
    parent = np.arange(int(members.max()) + 1)
    n_edges = 0
    for e in order:
        ra, rb = lo[e], hi[e]
        while parent[ra] != ra:
            parent[ra] = parent[parent[ra]]
            ra = parent[ra]
        while parent[rb] != rb:
            parent[rb] = parent[parent[rb]]
            rb = parent[rb]
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            n_edges += 1
    return n_edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "span_tree_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--subset", type=int, default=131072)
    ap.add_argument("--small", type=int, default=16384, help="members of the composition's leg")
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, m_edges = 128, 16
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    rng = np.random.default_rng(14)
    dup = rng.choice(a.n, a.n // 100, replace=False)
    src = rng.integers(0, a.n, dup.size)
    src = np.where(np.isin(src, dup), (src + 1) % a.n, src)
    x[dup] = x[src]
    x[dup[::2]] += rng.uniform(-1e-3, 1e-3, (dup[::2].size, dim)).astype(np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(m_edges); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    radius = 0.05
    members = np.arange(min(a.subset, a.n), dtype=np.int32)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": m_edges, "ef_construction": 200, "min_nn": 128, "planted_duplicates": int(dup.size),
                      "members": int(members.size), "radius": radius, "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(time.perf_counter() - t0, 2)}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    def scan_kernel_ms(f):
        ix.set_profiling(True)
        ix.reset_stats()
        f()
        st = ix.stats()
        ix.set_profiling(False)
        return round(st["exact_kernel_ms"], 3), int(st["exact_launches"])

    call = lambda: ix.single_linkage_tree(allowed=members)
    tree, wall, walls = median_ms(call, a.steps)
    k_ms, launches = scan_kernel_ms(call)
    all_pairs = members.size * (members.size - 1) // 2
    res["single_linkage_tree"] = c = {**tree[3], "ms": wall, "ms_repeats": walls, "scan_kernel_ms": k_ms, "scan_launches": launches,
                                      "share_of_pairs_measured": round(tree[3]["pairs_measured"] / (tree[3]["rounds"] * all_pairs), 4)}
    print("single_linkage_tree", c, flush=True)
    save()
    call = lambda: ix.duplicate_groups(radius, allowed=members)
    (groups, g_info), g_wall, walls = median_ms(call, a.steps)
    k_ms, launches = scan_kernel_ms(call)
    res["duplicate_groups"] = c = {**g_info, "ms": g_wall, "ms_repeats": walls, "scan_kernel_ms": k_ms, "scan_launches": launches}
    print("duplicate_groups", c, flush=True)
    save()
    cut, cut_ms, walls = median_ms(lambda: ix.single_linkage_cut(tree, radius, allowed=members), 1)
    res["single_linkage_cut"] = c = {"ms": cut_ms, "labels_equal_duplicate_groups": bool(cut.tobytes() == groups.tobytes())}
    print("single_linkage_cut", c, flush=True)
    save()
    small = members[:a.small]
    small_tree, small_ms, walls = median_ms(lambda: ix.single_linkage_tree(allowed=small), a.steps)
    n_forest, host_ms, host_walls = median_ms(lambda: knn_graph_forest(ix, small, 16), 1)
    res["composition_at_small"] = c = {"members": int(small.size), "k": 16, "single_linkage_tree_ms": small_ms, "tree_edges": small_tree[3]["edges"],
                                       "exact_knn_graph_and_kruskal_ms": host_ms, "forest_edges_of_the_knn_graph": int(n_forest)}
    res["ratios"] = {"tree_over_duplicate_groups": round(wall / g_wall, 3), "tree_over_duplicate_groups_times_rounds": round(wall / (g_wall * tree[3]["rounds"]), 4),
                     "composition_over_tree_at_small": round(host_ms / small_ms, 2)}
    print("composition", c, res["ratios"], flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
