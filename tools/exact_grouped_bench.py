#!/usr/bin/env python3
"""The grouped exact k-NN call (hnswdev_exact_knn_grouped) at C2 rows (1M x 128, k = 10) beside the loop it replaces,
in one session and one build.  The rows are uploaded to a context (the scan reads no graph, so none is built).
 1. Partitions of the rows into 10, 100 and 1 000 random groups, 65 536 queries assigned uniformly to the groups.  Per partition:
    the grouped call's wall time (warm-up, median of five); the HIP-event times of its list-building kernels
    (hnswdev_exact_grouped_list_ms) and of its scan + merge (hnswdev_stats.exact_kernel_ms), from a profiling-on pass of its own;
    the wall time of a grouped call of ONE query in a one-row group of the same row_group array, which is the list building with
    its upload and copy back plus the fixed cost of a call; and the same work as a loop of
    exact_knn(q[query_group == g], k, allowed = (row_group == g)) over the groups: the baseline.  Both answers are compared, bytes.
 2. The guard against a costly descriptor path: n_groups = 1 and 4 096 queries, the grouped call beside the plain unfiltered call.
    python tools/exact_grouped_bench.py [--out profiles/exact_grouped_c2.json] [--n 1000000] [--quick]
--quick: 100 000 rows, 4 096 queries, partitions of 10 and 100 (a check that the tool runs)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def walls(call, steps):
    call()   # warm-up (the first call allocates its workspace)
    out = []
    for _ in range(steps):
        t = time.perf_counter()
        call()
        out.append(time.perf_counter() - t)
    return float(np.median(out)), [round(1e3 * w, 3) for w in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_grouped_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.n, a.nq = min(a.n, 100_000), min(a.nq, 4096)
    import hnswindex
    net = hnswindex.net_amd
    dim, k = 128, 10
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((a.nq, dim), dtype=np.float32)
    db = hnswindex.DeviceBackend(dim, "sq_euclid", capacity=a.n)
    db.upload_rows(0, x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "k": k, "queries_per_call": a.nq, "timed_calls": a.steps, "metric": "sq_euclid",
                      "baseline": "a loop of exact_knn(q[query_group == g], k, allowed = (row_group == g)) over the groups, same session"},
           "partitions": {}, "evals_check": True, "answers_equal": True}

    def profiled(call):
        db.set_profiling(True)
        db.reset_stats()
        call()
        st = db.stats()
        st["list_ms"] = db.exact_grouped_list_ms()
        db.set_profiling(False)
        return st

    for ng in ((10, 100) if a.quick else (10, 100, 1000)):
        rng = np.random.default_rng(100 + ng)
        rg = rng.integers(0, ng, a.n).astype(np.int32)
        qg = rng.integers(0, ng, a.nq).astype(np.int32)
        members = np.bincount(rg, minlength=ng)
        pairs = int(members[qg].sum())
        masks = [rg == g for g in range(ng)]
        sels = [np.flatnonzero(qg == g) for g in range(ng)]
        parts = [np.ascontiguousarray(q[s]) for s in sels]

        def grouped():
            return db.exact_knn_grouped(q, k, rg, qg, ng)

        def loop():
            ids = np.full((a.nq, k), -1, np.int32)
            d = np.full((a.nq, k), np.nan, np.float32)
            for g in range(ng):
                if sels[g].size:
                    ids[sels[g]], d[sels[g]] = db.exact_knn(parts[g], k, allowed=masks[g])
            return ids, d

        g_wall, g_all = walls(grouped, a.steps)
        l_wall, l_all = walls(loop, a.steps if ng <= 100 else max(1, a.steps // 2))
        g_out, l_out = grouped(), loop()
        same = bool((g_out[0] == l_out[0]).all() and g_out[1].tobytes() == l_out[1].tobytes())
        g_st = profiled(grouped)
        gi = db.exact_grouped_info()   # (read before the next reset_stats)
        l_st = profiled(loop)
        ok = g_st["exact_evals"] == pairs and l_st["exact_evals"] == pairs
        res["evals_check"] = bool(res["evals_check"] and ok)
        res["answers_equal"] = bool(res["answers_equal"] and same)
        # the fixed cost of a call with this row_group: one query in a one-row group of the same array
        one = rg.copy()
        one[0] = ng
        lists_wall, _ = walls(lambda: db.exact_knn_grouped(q[:1], k, one, np.array([ng], np.int32), ng + 1), a.steps)
        line = {"groups": ng, "rows_per_group_mean": round(float(members.mean()), 1), "pairs": pairs,
                "grouped": {"ms_per_call": round(1e3 * g_wall, 3), "calls_ms": g_all, "queries_per_sec": round(a.nq / g_wall, 1),
                            "kernel_ms_scan_plus_merge": round(g_st["exact_kernel_ms"], 3), "kernel_ms_list_building": round(g_st["list_ms"], 3),
                            "exact_launches": int(g_st["exact_launches"]), "scan_blocks": gi["scan_blocks"], "groups_scanned": gi["groups_scanned"],
                            "ms_one_query_call": round(1e3 * lists_wall, 3)},
                "loop_of_exact_knn": {"ms_per_batch": round(1e3 * l_wall, 3), "batches_ms": l_all, "queries_per_sec": round(a.nq / l_wall, 1),
                                      "kernel_ms_scan_plus_merge": round(l_st["exact_kernel_ms"], 3), "exact_launches": int(l_st["exact_launches"])},
                "grouped_over_loop": round(l_wall / g_wall, 2), "answers_equal_bytes": same, "evals_equal_pairs": bool(ok)}
        res["partitions"][str(ng)] = line
        print(ng, line, flush=True)

    # ---- the guard: one group, beside the plain call ----
    nq1 = min(4096, a.nq)
    zeros_r, zeros_q = np.zeros(a.n, np.int32), np.zeros(nq1, np.int32)
    p_wall, p_all = walls(lambda: db.exact_knn(q[:nq1], k), a.steps)
    s_wall, s_all = walls(lambda: db.exact_knn_grouped(q[:nq1], k, zeros_r, zeros_q, 1), a.steps)
    p_st = profiled(lambda: db.exact_knn(q[:nq1], k))
    s_st = profiled(lambda: db.exact_knn_grouped(q[:nq1], k, zeros_r, zeros_q, 1))
    res["single_group_guard"] = {"queries": nq1, "plain_ms": round(1e3 * p_wall, 3), "plain_calls_ms": p_all, "grouped_ms": round(1e3 * s_wall, 3),
                                 "grouped_calls_ms": s_all, "grouped_over_plain_time": round(s_wall / p_wall, 4),
                                 "plain_kernel_ms": round(p_st["exact_kernel_ms"], 3), "grouped_kernel_ms": round(s_st["exact_kernel_ms"], 3),
                                 "within_10_percent": bool(s_wall <= 1.10 * p_wall)}
    print("guard", res["single_group_guard"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
