#!/usr/bin/env python3
"""Half-precision row storage next to f32 rows, same box, same session, same build.  C2: 1M x 128, M = 16,
efConstruction = 200, MinNN (ef) = 128, k = 10; sq_euclid_f16 beside sq_euclid.  Per metric: default Add adds/s; per call size
(65 536 and 12 500 queries) queries/s through hnsw_knn_query with profiling off (two warm-up calls, then the median of --steps timed
calls), then in a pass of its own search-kernel ms per launch and evaluations per launch from hnswdev_stats with profiling on, achieved bytes/s over the algorithmic evals x
row_bytes against the 8 TB/s peak; recall@10 of both against brute force on the f32 rows.  --c3: the same at 1M x 768,
ucosine_f16 beside ucosine.
    python tools/f16_bench.py [--out profiles/f16_c2.json] [--steps 5] [--n 1000000] [--c3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_GBPS = 8000.0


def recall_at_k(x, q, got, unit):
    """recall@k of `got` against exact brute force over the f32 rows (float32 matmul on the GPU, a subset of the queries)."""
    import torch
    xt, qt = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
    dd = -(qt @ xt.T) if unit else (xt * xt).sum(1)[None, :] - 2 * qt @ xt.T
    gt = dd.topk(got.shape[1], largest=False).indices.cpu().numpy()
    del xt, qt, dd
    return round(float(np.mean([len(set(g.tolist()) & set(h.tolist())) / got.shape[1] for g, h in zip(gt, got)])), 4)


def run_metric(hnswindex, metric, x, qs, k, steps, unit):
    dim = x.shape[1]
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(x.shape[0]); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    build_s = time.perf_counter() - t0
    out = {"adds_per_sec": round(x.shape[0] / build_s, 1), "build_seconds": round(build_s, 2), "graph_hash": f"{ix.graph_hash():016x}", "calls": {}}
    for nq, q in qs.items():
        ix.set_profiling(False)                              # wall clock: no event bracketing inside the timed calls
        ix.knn_query(q, k)                                   # warm-up
        ix.knn_query(q, k)
        walls = []
        for _ in range(steps):
            t = time.perf_counter()
            ids, _ = ix.knn_query(q, k)
            walls.append(time.perf_counter() - t)
        ix.set_profiling(True)                               # kernel time: a pass of its own, HIP events around every launch
        ix.knn_query(q, k)
        ix.reset_stats()
        for _ in range(steps):
            ix.knn_query(q, k)
        st = ix.stats()
        launches = max(1, st["search_timed_launches"])
        kms, evals = st["search_kernel_ms"] / launches, st["search_timed_evals"] / launches
        gbps = evals * st["row_bytes"] / (kms * 1e-3) / 1e9 if kms > 0 else None
        out["calls"][str(nq)] = {"queries_per_sec": round(nq / float(np.median(walls)), 1), "ms_per_call": round(1e3 * float(np.median(walls)), 3),
                                 "search_kernel_ms_per_launch": round(kms, 4), "launches_per_call": st["search_launches"] / steps,
                                 "evals_per_launch": round(evals, 1), "row_bytes": int(st["row_bytes"]),
                                 "GBps": round(gbps, 1) if gbps else None, "frac_of_peak": round(gbps / PEAK_GBPS, 4) if gbps else None,
                                 "handbacks": int(st["search_overflows"])}
        print(metric, nq, out["calls"][str(nq)], flush=True)
        rsub = min(512, nq)
        out["calls"][str(nq)]["recall_at_10"] = recall_at_k(x, q[:rsub], ids[:rsub], unit)
    del ix
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "f16_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--c3", action="store_true", help="1M x 768 ucosine_f16 beside ucosine instead of C2")
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, k = (768, 10) if a.c3 else (128, 10)
    pair = ("ucosine_f16", "ucosine") if a.c3 else ("sq_euclid_f16", "sq_euclid")
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    qs = {nq: np.random.default_rng(65540 + nq).random((nq, dim), dtype=np.float32) for nq in (65536, 12500)}
    if a.c3:
        norm = lambda v: (v / np.sqrt((v * v).sum(axis=1, dtype=np.float32, keepdims=True))).astype(np.float32)
        x, qs = norm(x), {nq: norm(q) for nq, q in qs.items()}
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "M": 16, "ef_construction": 200, "min_nn": 128, "k": k, "timed_calls": a.steps, "warmup_calls": 2},
           "peak_GBps": PEAK_GBPS, "metrics": {}}
    for metric in pair:
        res["metrics"][metric] = run_metric(hnswindex, metric, x, qs, k, a.steps, a.c3)
    f16, f32 = res["metrics"][pair[0]], res["metrics"][pair[1]]
    res["f16_over_f32"] = {nq: {"queries_per_sec": round(f16["calls"][nq]["queries_per_sec"] / f32["calls"][nq]["queries_per_sec"], 3),
                                "search_kernel_ms_per_launch": round(f16["calls"][nq]["search_kernel_ms_per_launch"] / f32["calls"][nq]["search_kernel_ms_per_launch"], 3)}
                           for nq in f16["calls"]}
    res["f16_over_f32"]["adds_per_sec"] = round(f16["adds_per_sec"] / f32["adds_per_sec"], 3)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["f16_over_f32"]))


if __name__ == "__main__":
    main()
