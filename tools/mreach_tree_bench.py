#!/usr/bin/env python3
"""mutual_reachability_tree against single_linkage_tree on the rows of tools/span_tree_bench.py: C2's 1M x 128 sq_euclid
rows with 1 % planted near-duplicates, of which the first --subset (131 072) are the members.  Only those rows are added -- the scans
read stored rows, never the graph -- so the session spends its time on the calls.  One session:
    A/B   single_linkage_tree (span_scan_kernel) and mutual_reachability_tree(1) (mreach_scan_kernel; the same tree, byte for byte)
          alternate, --steps calls each after one warm-up call each; per call the wall time and the HIP-event time of its scan launches
          (profiling on for every timed call of both legs), and from info the pairs measured: ns per measured pair is the comparison
    min_samples 5 and 16: the whole call, the core stage's launches and event time, the tree's rounds
The file is rewritten after every line.
    python tools/mreach_tree_bench.py [--out profiles/mreach_tree_c2.json] [--steps 3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mreach_tree_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--subset", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=3)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim = 128
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    rng = np.random.default_rng(14)
    dup = rng.choice(a.n, a.n // 100, replace=False)
    src = rng.integers(0, a.n, dup.size)
    src = np.where(np.isin(src, dup), (src + 1) % a.n, src)
    x[dup] = x[src]
    x[dup[::2]] += rng.uniform(-1e-3, 1e-3, (dup[::2].size, dim)).astype(np.float32)
    m = min(a.subset, a.n)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(m); ix.set_max_edges(8); ix.set_insert_batch(0)
    ix.add(x[:m])
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"rows_generated": a.n, "dim": dim, "metric": "sq_euclid", "planted_duplicates": int(dup.size), "members": m, "rows_added": m,
                      "timed_calls_per_leg": a.steps, "protocol": "one warm-up call per leg, then the legs alternate; profiling on in every timed call"}}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    def timed(f):
        ix.reset_stats()
        t = time.perf_counter()
        out = f()
        wall = 1e3 * (time.perf_counter() - t)
        st = ix.stats()
        return out, round(wall, 3), round(st["exact_kernel_ms"], 3), int(st["exact_launches"])

    ix.set_profiling(True)
    legs = {"single_linkage_tree": lambda: ix.single_linkage_tree(), "mutual_reachability_tree_1": lambda: ix.mutual_reachability_tree(1)}
    runs = {name: [] for name in legs}
    outs = {name: f() for name, f in legs.items()}                       # warm-up (a first call allocates its scratch)
    for _ in range(a.steps):
        for name, f in legs.items():
            out, wall, k_ms, launches = timed(f)
            info = out[-1]
            runs[name].append({"ms": wall, "scan_kernel_ms": k_ms, "scan_launches": launches, "rounds": info["rounds"], "pairs_measured": info["pairs_measured"],
                               "pairs_skipped": info["pairs_skipped"], "ns_per_measured_pair": round(1e6 * k_ms / info["pairs_measured"], 6)})
    for name in legs:
        per = [r["ns_per_measured_pair"] for r in runs[name]]
        res[name] = {"runs": runs[name], "median_ms": float(np.median([r["ms"] for r in runs[name]])), "median_ns_per_measured_pair": float(np.median(per)),
                     "spread_ns_per_measured_pair": [min(per), max(per)]}
        print(name, res[name], flush=True)
    res["same_bytes_at_min_samples_1"] = all(g.tobytes() == w.tobytes() for g, w in zip(outs["mutual_reachability_tree_1"][:3], outs["single_linkage_tree"][:3]))
    res["new_over_old_ns_per_measured_pair"] = round(res["mutual_reachability_tree_1"]["median_ns_per_measured_pair"] / res["single_linkage_tree"]["median_ns_per_measured_pair"], 4)
    save()
    for s in (5, 16):
        ix.mutual_reachability_tree(s)
        rows = []
        for _ in range(a.steps):
            out, wall, k_ms, launches = timed(lambda: ix.mutual_reachability_tree(s))
            info = out[-1]
            rows.append({"ms": wall, "all_scan_kernel_ms": k_ms, "all_scan_launches": launches, **info})
        ix.reset_stats()                                                 # the core stage alone: the by-id top-(s - 1) scan it runs, one launch per 65 536 members
        t = time.perf_counter()
        for at in range(0, m, 65536):
            ix.exact_knn_query_by_id(np.arange(at, min(at + 65536, m), dtype=np.int32), s - 1)
        st = ix.stats()
        res[f"min_samples_{s}"] = c = {"runs": rows, "median_ms": float(np.median([r["ms"] for r in rows])),
                                       "core_stage_as_exact_knn_query_by_id": {"ms_with_results_copied_out": round(1e3 * (time.perf_counter() - t), 3),
                                                                               "scan_kernel_ms": round(st["exact_kernel_ms"], 3), "launches": int(st["exact_launches"])}}
        print(f"min_samples_{s}", c, flush=True)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
