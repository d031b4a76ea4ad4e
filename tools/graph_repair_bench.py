#!/usr/bin/env python3
"""repair_reachability (hnsw_mi355x_repair_reachability) at C2 (1M x 128, sq_euclid, default Add), one session, one
build, measured against the same index before the call:
 1. unreachable_ids(0) before; recall@10 of knn_query against exact_knn_query on a fresh query set before.
 2. the call: its wall time (one call: it edits the graph, so there is no repeat and no warm-up -- the first round allocates the
    scratch), its per-layer report and its counters.
 3. unreachable_ids(0) after; recall@10 on the same queries after; the share of the formerly lost ids that a self-query (the id's own
    stored row, k = 1) returns now, and how many it returned before (none can be: they were unreachable).
 4. a second call: the wall time of finding nothing to do.
No threshold is asserted on any figure.  Wall time is what is measured: profiling is off, so the flat scans' share (they count in the
exact family of hnswdev_stats) is not recorded, and the other kernels have no event time.
    python tools/graph_repair_bench.py [--out profiles/graph_repair_c2.json] [--n 1000000] [--queries 10000] [--quick]
--quick: 20 000 rows with M = 4 (a check that the tool runs on a graph that has something to repair)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def recall_at(ix, q, k):
    got, _ = ix.knn_query(q, k)
    want, _ = ix.exact_knn_query(q, k)
    return float(np.mean([np.intersect1d(g, w).size / k for g, w in zip(got, want)]))


def self_found(ix, x, ids):
    if ids.size == 0:
        return 0
    return int((ix.knn_query(x[ids], 1)[0][:, 0] == ids).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_repair_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--cands", type=int, default=8)
    ap.add_argument("--max-rounds", type=int, default=8)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim = 128
    ix = hnswindex.Index(dim, "sq_euclid")
    if a.quick:
        a.n, a.queries = 20_000, 1_000
        ix.set_max_edges(4)
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(271828).random((a.queries, dim), dtype=np.float32)
    ix.set_collection_size(a.n)
    t = time.perf_counter()
    ix.add(x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "add": "default", "queries": a.queries, "k": 10, "cands": a.cands,
                      "max_rounds": a.max_rounds, "quick": a.quick},
           "add_s": time.perf_counter() - t, "kernel_ms": None}
    lost = ix.unreachable_ids(0)
    res["before"] = {"unreachable_layer0": int(lost.size), "layers": ix.reachability(), "recall_at_10": recall_at(ix, q, 10),
                     "self_query_finds_lost": self_found(ix, x, lost)}
    print("before", res["before"], flush=True)
    ix.reset_stats()
    t = time.perf_counter()
    report = ix.repair_reachability(a.cands, a.max_rounds)
    wall = time.perf_counter() - t
    res["repair"] = {"wall_ms": 1e3 * wall, "report": report, "counters": ix.graph_repair_counters(), "reach_counters": ix.graph_reach_counters()}
    print("repair", res["repair"], flush=True)
    found = self_found(ix, x, lost)
    res["after"] = {"unreachable_layer0": int(ix.unreachable_ids(0).size), "layers": ix.reachability(), "recall_at_10": recall_at(ix, q, 10),
                    "self_query_finds_lost": found, "self_query_share_of_lost": found / lost.size if lost.size else None}
    print("after", res["after"], flush=True)
    t = time.perf_counter()
    again = ix.repair_reachability(a.cands, a.max_rounds)
    res["second_call"] = {"wall_ms": 1e3 * (time.perf_counter() - t), "linked": sum(r["linked"] for r in again)}
    print("second_call", res["second_call"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
