#!/usr/bin/env python3
"""The grouped exact range call (hnswdev_exact_range_grouped) at C2 rows (1M x 128, sq_euclid) beside the loop it
replaces, in one session and one build.  The rows are uploaded to a context (the scan reads no graph, so none is built).
 1. Partitions of the rows into 10, 100 and 1 000 random groups, 65 536 queries assigned uniformly to the groups, at radii that
    give about 10 and about 340 results per query within its group (order statistics of the oracle's distances of 64 of the
    queries to the rows of their groups).  Per (partition, radius): the grouped call's wall time (warm-up, median of five); the
    HIP-event times of its list-building kernels (hnswdev_exact_grouped_list_ms) and of its scan (hnswdev_stats.exact_kernel_ms)
    from a profiling-on pass of its own; hnswdev_exact_range_grouped_info; and the same work as a loop of
    exact_range(q[query_group == g], radius, allowed = (row_group == g)) over the groups: the baseline.  Both answers are
    compared: counts, ids and distance bytes.
 2. The guard against a costly descriptor path: n_groups = 1 and 4 096 queries, the grouped call beside the plain unfiltered
    exact_range; the margin is the spread of the plain call's own timings.
    python tools/exact_range_grouped_bench.py [--out profiles/exact_range_grouped_c2.json] [--n 1000000] [--quick]
The file is rewritten after every line, so a run that is cut short leaves what it measured.
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
    return float(np.median(out)), out


def ms(ws):
    return [round(1e3 * w, 3) for w in ws]


def same_lists(a, b):
    return bool(len(a[0]) == len(b[0]) and all(u.size == v.size and (u == v).all() and s.tobytes() == t.tobytes()
                                               for u, v, s, t in zip(a[0], b[0], a[1], b[1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_range_grouped_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.n, a.nq = min(a.n, 100_000), min(a.nq, 4096)
    import hnswindex
    import oracle
    net = hnswindex.net_amd
    dim = 128
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((a.nq, dim), dtype=np.float32)
    db = hnswindex.DeviceBackend(dim, "sq_euclid", capacity=a.n)
    db.upload_rows(0, x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "queries_per_call": a.nq, "timed_calls": a.steps, "metric": "sq_euclid",
                      "baseline": "a loop of exact_range(q[query_group == g], radius, allowed = (row_group == g)) over the groups, same session"},
           "lines": {}, "evals_check": True, "answers_equal": True}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    def profiled(call):
        db.set_profiling(True)
        db.reset_stats()
        call()
        st = db.stats()
        st["list_ms"] = db.exact_grouped_list_ms()
        st["info"] = db.exact_range_grouped_info()
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
        # radii: order statistics of 64 queries' distances to the rows of their groups
        sub = 64
        pooled = np.sort(np.concatenate([oracle.dist_query_rows("sq_euclid", x, q[i], np.flatnonzero(masks[qg[i]]).astype(np.int32)) for i in range(sub)]))
        for target in (10, 340):
            if sub * target > pooled.size:
                continue
            radius = float(pooled[sub * target - 1])

            def grouped():
                return db.exact_range_grouped(q, radius, rg, qg, ng)

            def loop():
                ids, d = [None] * a.nq, [None] * a.nq
                for g in range(ng):
                    if sels[g].size:
                        g_ids, g_d = db.exact_range(parts[g], radius, allowed=masks[g])
                        for j, i in enumerate(sels[g]):
                            ids[i], d[i] = g_ids[j], g_d[j]
                return ids, d

            g_wall, g_all = walls(grouped, a.steps)
            l_wall, l_all = walls(loop, a.steps if ng <= 100 else max(1, a.steps // 2))
            g_out, l_out = grouped(), loop()
            same = same_lists(g_out, l_out)
            g_st, l_st = profiled(grouped), profiled(loop)
            repeated = g_st["info"]["repeated_pieces"]
            ok = (g_st["exact_evals"] == pairs if repeated == 0 else pairs < g_st["exact_evals"] <= 2 * pairs) and l_st["exact_evals"] >= pairs
            res["evals_check"] = bool(res["evals_check"] and ok)
            res["answers_equal"] = bool(res["answers_equal"] and same)
            total = int(sum(v.size for v in g_out[0]))
            line = {"groups": ng, "radius": radius, "rows_per_group_mean": round(float(members.mean()), 1), "pairs": pairs,
                    "results_per_query": round(total / a.nq, 2), "longest_list": int(max(v.size for v in g_out[0])),
                    "grouped": {"ms_per_call": round(1e3 * g_wall, 3), "calls_ms": ms(g_all), "queries_per_sec": round(a.nq / g_wall, 1),
                                "kernel_ms_scan": round(g_st["exact_kernel_ms"], 3), "kernel_ms_list_building": round(g_st["list_ms"], 3),
                                "exact_launches": int(g_st["exact_launches"]), "exact_evals": int(g_st["exact_evals"]), **g_st["info"]},
                    "loop_of_exact_range": {"ms_per_batch": round(1e3 * l_wall, 3), "batches_ms": ms(l_all), "queries_per_sec": round(a.nq / l_wall, 1),
                                            "kernel_ms_scan": round(l_st["exact_kernel_ms"], 3), "exact_launches": int(l_st["exact_launches"])},
                    "grouped_over_loop": round(l_wall / g_wall, 2), "answers_equal_bytes": same, "evals_check": bool(ok)}
            res["lines"][f"{ng}_groups_about_{target}"] = line
            print(f"{ng}_groups_about_{target}", line, flush=True)
            save()

    # ---- the guard: one group, beside the plain call ----
    nq1 = min(4096, a.nq)
    zeros_r, zeros_q = np.zeros(a.n, np.int32), np.zeros(nq1, np.int32)
    every = np.arange(a.n, dtype=np.int32)
    pooled = np.sort(np.concatenate([oracle.dist_query_rows("sq_euclid", x, q[i], every) for i in range(16)]))
    radius = float(pooled[16 * 340 - 1])
    p_wall, p_all = walls(lambda: db.exact_range(q[:nq1], radius), a.steps)
    s_wall, s_all = walls(lambda: db.exact_range_grouped(q[:nq1], radius, zeros_r, zeros_q, 1), a.steps)
    p_st = profiled(lambda: db.exact_range(q[:nq1], radius))
    s_st = profiled(lambda: db.exact_range_grouped(q[:nq1], radius, zeros_r, zeros_q, 1))
    spread = max(p_all) - min(p_all)
    res["single_group_guard"] = {"queries": nq1, "radius": radius, "plain_ms": round(1e3 * p_wall, 3), "plain_calls_ms": ms(p_all),
                                 "grouped_ms": round(1e3 * s_wall, 3), "grouped_calls_ms": ms(s_all), "plain_spread_ms": round(1e3 * spread, 3),
                                 "grouped_minus_plain_ms": round(1e3 * (s_wall - p_wall), 3), "grouped_over_plain_time": round(s_wall / p_wall, 4),
                                 "plain_kernel_ms": round(p_st["exact_kernel_ms"], 3), "grouped_kernel_ms": round(s_st["exact_kernel_ms"], 3),
                                 "grouped_list_building_ms": round(s_st["list_ms"], 3),
                                 "answers_equal_bytes": same_lists(db.exact_range(q[:nq1], radius), db.exact_range_grouped(q[:nq1], radius, zeros_r, zeros_q, 1)),
                                 "slower_by_more_than_the_plain_spread": bool(s_wall - p_wall > spread)}
    print("guard", res["single_group_guard"], flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
