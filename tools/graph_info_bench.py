#!/usr/bin/env python3
"""GetInfo / GetConnectedComponentCounts on the device (hnsw_mi355x_get_info, hnsw_mi355x_connected_component_counts)
at C2 (1M x 128, sq_euclid, default Add), one session, one build:
 1. get_info() and connected_component_counts(): wall time around the call, one warm-up (it allocates the scratch), then the median
    of five; every repeat is kept.  Beside them the counters of one call each (layers, list entries read, kernel launches).
 2. export_edges of layer 0 alone on the same index: the mirror fetch plus the copy -- the lower bound of ANY computation of the same
    answers on the host.  The first export after the build pays the fetch (the host copy is stale after a device-linked Add); the
    later ones only the copy; both are reported.  It runs AFTER part 1, so that part 1 is timed with the lists in HBM only.
 3. the answers themselves (they are small), so that a reader sees what was computed.
The ABI has no counter for these kernels' HIP-event time (hnswdev_stats is fixed), so "kernel_ms" is null: wall time is what is measured.
    python tools/graph_info_bench.py [--out profiles/graph_info_c2.json] [--n 1000000] [--quick]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_info_c2.json"))
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

    def line(name, call):
        walls = walls_of(call, a.steps)
        ix.reset_stats()
        call()
        res[name] = {"median_ms": 1e3 * statistics.median(walls), "walls_ms": [1e3 * w for w in walls], "counters": ix.graph_info_counters()}
        print(name, res[name], flush=True)

    line("get_info", ix.get_info)
    line("connected_component_counts", ix.connected_component_counts)
    res["info"] = ix.get_info()
    res["components"] = ix.connected_component_counts().tolist()
    stride = 2 * 16 + 2
    t = time.perf_counter()
    counts, _ = ix.export_edges(0, stride)
    first = time.perf_counter() - t
    walls = walls_of(lambda: ix.export_edges(0, stride), a.steps)
    res["export_edges_layer0"] = {"first_ms": 1e3 * first, "median_ms": 1e3 * statistics.median(walls), "walls_ms": [1e3 * w for w in walls],
                                  "entries": int(counts[counts > 0].sum())}
    print("export_edges_layer0", res["export_edges_layer0"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
