#!/usr/bin/env python3
"""Reachability from the entry point on the device (hnsw_mi355x_reachability, hnsw_mi355x_unreachable_ids) at C2
(1M x 128, sq_euclid, default Add), one session, one build:
 1. reachability(), unreachable_ids(0) and, for scale, connected_component_counts(): wall time around the call, one warm-up (it
    allocates the scratch), then the median of five; every repeat is kept.  Beside them the counters of one call each.
 2. export_edges of layer 0 alone on the same index: the copy any host-side BFS starts with.  The first export after the build pays
    the mirror fetch (the host copy is stale after a device-linked Add), the later ones only the copy; both are reported.  It runs
    AFTER part 1, so that part 1 is timed with the lists in HBM only.
 3. what the calls found: per layer members / seeds / reached / max_hops, and how many of the items no query can return.
 4. a check at this size: the same chain on the host, a numpy frontier BFS over the exported lists of every layer (timed, for the
    record: it is what the device call replaces once the lists have been copied).
The ABI has no counter for these kernels' HIP-event time (hnswdev_stats is fixed), so "kernel_ms" is null: wall time is what is measured.
    python tools/graph_reach_bench.py [--out profiles/graph_reach_c2.json] [--n 1000000] [--quick]
--quick: 20 000 rows (a check that the tool runs)."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def walls_of(call, steps):
    call()   # warm-up
    walls = []
    for _ in range(steps):
        t = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t)
    return walls


def host_reach(member, counts, edges, seeds):
    """reached[n] over out-edges among `member` from the member seeds: a frontier at a time, numpy."""
    reached = seeds & member
    frontier = np.nonzero(reached)[0]
    cols = np.arange(edges.shape[1])[None, :]
    while frontier.size:
        c = np.clip(counts[frontier], 0, edges.shape[1])
        v = edges[frontier][cols < c[:, None]]
        v = np.unique(v[(v >= 0) & (v < member.size)])
        v = v[member[v] & ~reached[v]]
        reached[v] = True
        frontier = v
    return reached


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_reach_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.n = 20_000
    import hnswindex
    net = hnswindex.net_amd
    dim = 128
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    ix = hnswindex.Index(dim, "sq_euclid")
    ix.set_collection_size(a.n)
    t = time.perf_counter()
    ix.add(x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "add": "default", "timed_calls": a.steps},
           "add_s": time.perf_counter() - t, "kernel_ms": None}

    def line(name, call, counters):
        walls = walls_of(call, a.steps)
        ix.reset_stats()
        call()
        res[name] = {"median_ms": 1e3 * statistics.median(walls), "walls_ms": [1e3 * w for w in walls], "counters": counters()}
        print(name, res[name], flush=True)

    line("reachability", ix.reachability, ix.graph_reach_counters)
    line("unreachable_ids_layer0", lambda: ix.unreachable_ids(0), ix.graph_reach_counters)
    line("connected_component_counts", ix.connected_component_counts, ix.graph_info_counters)
    res["layers"] = ix.reachability()
    lost = ix.unreachable_ids(0)
    res["unreachable_layer0"] = {"count": int(lost.size), "of": int(ix.count), "first_ids": lost[:16].tolist()}
    res["components"] = ix.connected_component_counts().tolist()
    print("layers", res["layers"], "unreachable", res["unreachable_layer0"], flush=True)
    stride = 2 * 16 + 2
    t = time.perf_counter()
    counts, _ = ix.export_edges(0, stride)
    first = time.perf_counter() - t
    walls = walls_of(lambda: ix.export_edges(0, stride), a.steps)
    res["export_edges_layer0"] = {"first_ms": 1e3 * first, "median_ms": 1e3 * statistics.median(walls), "walls_ms": [1e3 * w for w in walls],
                                  "entries": int(counts[counts > 0].sum())}
    print("export_edges_layer0", res["export_edges_layer0"], flush=True)
    # the same chain on the host, from the exported lists
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.ids()] = True
    t = time.perf_counter()
    seeds = np.zeros(levels.size, bool)
    seeds[ix.entry_point] = True
    host_layers = []
    for layer in range(ix.top_layer(), -1, -1):
        c, e = ix.export_edges(layer, stride)
        member = live & (levels >= layer)
        seeds = host_reach(member, c, e, seeds)
        host_layers.append({"layer_id": layer, "nodes_count": int(member.sum()), "reached": int(seeds.sum())})
    host_lost = np.nonzero(live & ~seeds)[0]
    res["host_check"] = {"wall_ms": 1e3 * (time.perf_counter() - t), "layers": host_layers[::-1],
                         "same_unreachable_ids": bool(host_lost.size == lost.size and (host_lost == lost).all())}
    print("host_check", res["host_check"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if not res["host_check"]["same_unreachable_ids"]:
        raise SystemExit("the device's unreachable ids differ from the host's")


if __name__ == "__main__":
    main()
