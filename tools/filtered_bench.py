#!/usr/bin/env python3
"""Filtered KnnQuery at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128, k = 10; 65 536 queries per call):
per allow-set -- random at selectivity 1.0 / 0.5 / 0.1 / 0.01 and one correlated with the data (a threshold on coordinate 0) --
queries/s, kernel ms (profiling on), device evaluations per query, bytes/s = evaluations x 512 B / kernel time against the 8 TB/s
peak, and hand-backs; the unfiltered call on the same index; the lock-step filtered path (device traversal off, the same graph
imported) on a 1 024-query subset; recall@10 against brute force over the allowed rows (reported, not gated).
    python tools/filtered_bench.py [--out profiles/filtered_knn_c2.json] [--steps 3] [--quick]
--quick (the rocprofv3 run): one timed call per mask, no lock-step path, no recall."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_GBPS = 8000.0
ROW_BYTES = 128 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filtered_knn_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, k = 128, 10
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((a.nq, dim), dtype=np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    build_s = time.perf_counter() - t0
    rng = np.random.default_rng(7)
    masks = {f"random_{s}": rng.random(a.n) < s for s in (1.0, 0.5, 0.1, 0.01)}
    masks["correlated_x0_lt_0.5"] = x[:, 0] < 0.5
    ix.set_profiling(True)

    def measure(allowed):
        out = ix.knn_query(q, k, allowed=allowed)   # warm-up (first filtered call allocates its scratch)
        ix.reset_stats()
        walls = []
        for _ in range(1 if a.quick else a.steps):
            t = time.perf_counter()
            out = ix.knn_query(q, k, allowed=allowed)
            walls.append(time.perf_counter() - t)
        st = ix.stats()
        calls = len(walls)
        kms = st["search_kernel_ms"] / calls
        evals = st["search_timed_evals"] / calls
        return out, {"queries_per_sec": round(a.nq / float(np.median(walls)), 1), "ms_per_call": round(1e3 * float(np.median(walls)), 3),
                     "kernel_ms": round(kms, 3), "evals_per_query": round(evals / a.nq, 1),
                     "GBps": round(evals * ROW_BYTES / (kms * 1e-3) / 1e9, 1) if kms > 0 else None,
                     "frac_of_peak": round(evals * ROW_BYTES / (kms * 1e-3) / 1e9 / PEAK_GBPS, 4) if kms > 0 else None,
                     "handbacks": int(st["search_overflows"]) // calls, "search_launches_per_call": st["search_launches"] / calls,
                     "distance_launches": int(st["launches"])}
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(), "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": 16,
           "ef_construction": 200, "min_nn": 128, "k": k, "queries_per_call": a.nq, "timed_calls": 1 if a.quick else a.steps},
           "build_seconds": round(build_s, 2), "peak_GBps": PEAK_GBPS, "bytes_per_eval": ROW_BYTES}
    unf, m = measure(None)
    res["unfiltered"] = m
    res["masks"] = {}
    outs = {}
    for name, mask in masks.items():
        outs[name], m = measure(mask)
        m["selectivity"] = round(float(mask.mean()), 4)
        res["masks"][name] = m
        print(name, m, flush=True)
    res["selectivity_1_equals_unfiltered"] = bool((outs["random_1.0"][0] == unf[0]).all() and outs["random_1.0"][1].tobytes() == unf[1].tobytes())
    if not a.quick:
        import torch
        sub = 1024
        # the lock-step path on the same graph: imported into an index with the device traversal off
        levels = ix.levels()
        layers = [ix.export_edges(l, 33) for l in range(int(levels.max()) + 1)]
        iy = hnswindex.Index(dim)
        iy.set_collection_size(a.n); iy.set_max_edges(16); iy.set_max_candidates(200); iy.set_min_nn(128); iy.set_device_traversal(False)
        iy.import_graph(x, levels, ix.entry_point, layers)
        assert iy.graph_hash() == ix.graph_hash()
        res["lockstep_subset"] = {"queries": sub}
        for name in ("random_1.0", "random_0.1", "random_0.01"):
            t = time.perf_counter()
            ids, d = iy.knn_query(q[:sub], k, allowed=masks[name])
            wall = time.perf_counter() - t
            same = bool((ids == outs[name][0][:sub]).all() and d.tobytes() == outs[name][1][:sub].tobytes())
            dev_qps = res["masks"][name]["queries_per_sec"]
            res["lockstep_subset"][name] = {"queries_per_sec": round(sub / wall, 1), "same_as_device": same,
                                            "device_speedup": round(dev_qps / (sub / wall), 1)}
            print("lockstep", name, res["lockstep_subset"][name], flush=True)
        # recall@10 against brute force over the allowed rows (float32 on the GPU; reported, not gated)
        rsub = 512
        xt = torch.from_numpy(x).cuda()
        qt = torch.from_numpy(q[:rsub]).cuda()
        dd = (qt * qt).sum(1, keepdim=True) - 2 * qt @ xt.T + (xt * xt).sum(1)[None, :]
        for name, mask in masks.items():
            mt = torch.from_numpy(mask).cuda()
            gt = torch.where(mt[None, :], dd, torch.full_like(dd, float("inf"))).topk(k, largest=False).indices.cpu().numpy()
            got = outs[name][0][:rsub]
            res["masks"][name]["recall_at_10"] = round(float(np.mean([len(set(g.tolist()) & set(h.tolist())) / k for g, h in zip(gt, got)])), 4)
        del xt, qt, dd
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
