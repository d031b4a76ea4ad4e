#!/usr/bin/env python3
"""The exact k-NN call (hnsw_mi355x_exact_knn_query) at C2 (1M x 128, k = 10):
 1. no filter, 4 096 queries per call, for sq_euclid, sq_euclid_f16 and sq_euclid_i8: queries/s through the export (warm-up call,
    median of five), kernel ms of scan + merge from a separate profiling-on pass, exact_evals, the fraction of the 157.3 TFLOP/s
    f32 vector peak at 3 * dim flop per evaluation -- and the same workload through bench.py's brute_force_topk
    (a torch GEMM, not bit-exact) as the dense reference;
 2. sq_euclid with the random masks of tools/filtered_bench.py at selectivity 0.1 / 0.01 / 0.001, 65 536 queries per call: the
    exact call beside knn_query(allowed=...) on the same index in the same session -- queries/s, evaluations per query, recall@10
    of both against the oracle's exact answer on 512 queries (exact must be 1.0);
 3. exact_evals == queries x allowed rows, in every line.
    python tools/exact_knn_bench.py [--out profiles/exact_knn_c2.json] [--n 1000000] [--quick]
--quick: one metric, no torch reference, 64 model queries (a check that the tool runs)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PEAK_TFLOPS = 157.3


def median_wall(call, steps):
    call()   # warm-up (the first call allocates its workspace)
    walls = []
    for _ in range(steps):
        t = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t)
    return float(np.median(walls))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_knn_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nq-filtered", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import hnswindex
    import oracle
    net = hnswindex.net_amd
    dim, k = 128, 10
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    qf = np.random.default_rng(65540).random((a.nq_filtered, dim), dtype=np.float32)
    q = qf[:a.nq]
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "k": k, "queries_per_call": a.nq, "queries_per_filtered_call": a.nq_filtered, "timed_calls": a.steps,
                      "peak_f32_vector_TFLOPs": PEAK_TFLOPS, "flop_per_eval": 3 * dim},
           "unfiltered": {}, "masks": {}, "evals_check": True}

    def exact_line(ix, queries, allowed, n_allowed):
        nq = queries.shape[0]
        ix.set_profiling(False)
        wall = median_wall(lambda: ix.exact_knn_query(queries, k, allowed=allowed), a.steps)
        ix.set_profiling(True)    # kernel time: a pass of its own
        ix.reset_stats()
        out = ix.exact_knn_query(queries, k, allowed=allowed)
        st = ix.stats()
        ix.set_profiling(False)
        ok = st["exact_evals"] == nq * n_allowed
        res["evals_check"] = bool(res["evals_check"] and ok)
        kms = st["exact_kernel_ms"]
        return out, {"queries_per_sec": round(nq / wall, 1), "ms_per_call": round(1e3 * wall, 3), "kernel_ms_scan_plus_merge": round(kms, 3),
                     "exact_launches": int(st["exact_launches"]), "exact_evals": int(st["exact_evals"]), "evals_equal_nq_x_allowed": bool(ok),
                     "evals_per_query": n_allowed, "TFLOPs": round(st["exact_evals"] * 3 * dim / (kms * 1e-3) / 1e12, 2) if kms > 0 else None,
                     "frac_of_f32_vector_peak": round(st["exact_evals"] * 3 * dim / (kms * 1e-3) / 1e12 / PEAK_TFLOPS, 4) if kms > 0 else None}

    def build(metric, c2):
        ix = hnswindex.Index(dim, metric)
        ix.set_collection_size(a.n)
        if c2:
            ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
        else:   # the scan reads no graph: a cheap one
            ix.set_max_edges(4); ix.set_max_candidates(8)
        t0 = time.perf_counter()
        ix.add(x)
        return ix, round(time.perf_counter() - t0, 2)

    # ---- 1. no filter ----
    ix, res["build_seconds"] = build("sq_euclid", True)
    exact_unf, line = exact_line(ix, q, None, a.n)
    if not a.quick:
        import torch
        import bench
        xt = torch.from_numpy(x).cuda()
        torch.cuda.synchronize()

        def gemm():
            r = bench.brute_force_topk(xt, q, k, "sq_euclid")
            torch.cuda.synchronize()
            return r
        wall = median_wall(gemm, a.steps)
        gt = gemm()
        del xt
        torch.cuda.empty_cache()
        line["torch_gemm_queries_per_sec"] = round(a.nq / wall, 1)
        line["ratio_to_torch_gemm"] = round(line["queries_per_sec"] / (a.nq / wall), 3)
        line["torch_gemm_agrees_at_10"] = round(float(np.mean([len(set(g.tolist()) & set(h.tolist())) / k for g, h in zip(gt, exact_unf[0])])), 5)
    res["unfiltered"]["sq_euclid"] = line
    print("sq_euclid", line, flush=True)

    # ---- 2. masks, beside the filtered traversal ----
    rng = np.random.default_rng(7)
    masks = {f"random_{s}": rng.random(a.n) < s for s in (1.0, 0.5, 0.1, 0.01)}   # (drawn as tools/filtered_bench.py draws them)
    masks = {name: masks[name] for name in ("random_0.1", "random_0.01")}
    masks["random_0.001"] = np.random.default_rng(8).random(a.n) < 0.001
    msub = 64 if a.quick else 512
    for name, mask in masks.items():
        allowed_ids = np.flatnonzero(mask).astype(np.int32)
        e_out, e_line = exact_line(ix, qf, mask, int(allowed_ids.size))
        # the traversal explores about k / selectivity rows per query: below 0.5 % a call of 4 096 queries is long enough to time
        qt = qf if mask.mean() >= 0.005 else qf[:min(4096, a.nq_filtered)]
        t = time.perf_counter()
        f_out = ix.knn_query(qt, k, allowed=mask)        # warm-up, and how long a call takes
        first = time.perf_counter() - t
        steps = a.steps if first < 1.0 else 1            # a traversal of seconds per call is timed once
        ix.reset_stats()
        walls = []
        for _ in range(steps):
            t = time.perf_counter()
            f_out = ix.knn_query(qt, k, allowed=mask)
            walls.append(time.perf_counter() - t)
        st = ix.stats()
        f_wall = float(np.median(walls))
        f_line = {"queries_per_call": int(qt.shape[0]), "queries_per_sec": round(qt.shape[0] / f_wall, 1), "ms_per_call": round(1e3 * f_wall, 3),
                  "timed_calls": steps, "evals_per_query": round(st["search_evals"] / steps / qt.shape[0], 1),
                  "handbacks": int(st["search_overflows"]) // steps}
        # the model on a subset: the oracle's distances to every allowed row, np.lexsort((ids, dist))
        rec_e, rec_f, same = [], [], True
        for i in range(msub):
            d = oracle.dist_query_rows("sq_euclid", x, qf[i], allowed_ids)
            order = np.lexsort((allowed_ids, d))[:k]
            truth = allowed_ids[order]
            same = same and (e_out[0][i][:truth.size] == truth).all() and e_out[1][i][:truth.size].tobytes() == d[order].tobytes()
            rec_e.append(len(set(truth.tolist()) & set(e_out[0][i].tolist())) / k)
            rec_f.append(len(set(truth.tolist()) & set(f_out[0][i].tolist())) / k)
        e_line["recall_at_10"] = round(float(np.mean(rec_e)), 4)
        e_line["equals_model_bytes"] = bool(same)
        f_line["recall_at_10"] = round(float(np.mean(rec_f)), 4)
        res["masks"][name] = {"selectivity": round(float(mask.mean()), 5), "allowed": int(allowed_ids.size), "model_queries": msub,
                              "exact": e_line, "filtered_traversal": f_line,
                              "exact_over_filtered": round(e_line["queries_per_sec"] / f_line["queries_per_sec"], 2)}
        print(name, res["masks"][name], flush=True)
    res["exact_faster_at_random_0.01"] = bool(res["masks"]["random_0.01"]["exact_over_filtered"] > 1.0)
    del ix

    # ---- 1b. the other row kinds, no filter ----
    for metric in (() if a.quick else ("sq_euclid_f16", "sq_euclid_i8")):
        iy, _ = build(metric, False)
        _, line = exact_line(iy, q, None, a.n)
        res["unfiltered"][metric] = line
        print(metric, line, flush=True)
        del iy
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
