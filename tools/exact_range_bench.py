#!/usr/bin/env python3
"""The exact range call (hnsw_mi355x_exact_range_query) at C2 (1M x 128, sq_euclid), one session, one build:
 1. 4 096 queries per call at radii that give about 10, 340 and 5 000 results per query (order statistics of the oracle's
    distances of 64 of the queries to every row), unfiltered and under random allow-sets of 10 % and 1 %: queries/s through the
    export (warm-up call, median of five), results per query, scan launches, kernel ms from a profiling-on pass of its own, and
    hnsw_mi355x_exact_range_info (lists ordered on the device / on the host, rounds repeated with exact capacities);
 2. beside each line the traversal -- range_query / range_query(allowed=...) on the same index -- and its recall against the
    exact lists: results found / results that exist, over all queries of the call;
 3. exact_evals == queries x allowed rows in every line that repeated no round (above it, and at most twice it, otherwise);
 4. one comparison: at a radius that admits nothing the scan does exact_knn(k = 10)'s arithmetic without its merges -- both are
    timed five times on the same 4 096 x 1M shape (every repeat is kept, not the median alone).
    python tools/exact_range_bench.py [--out profiles/exact_range_c2.json] [--n 1000000] [--quick]
The file is rewritten after every line, so a run that is cut short leaves what it measured.
--quick: the smallest radius and the 1 % mask only (a check that the tool runs)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def walls_of(call, steps):
    call()   # warm-up (the first call allocates its workspace)
    walls = []
    for _ in range(steps):
        t = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t)
    return walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_range_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import hnswindex
    import oracle
    net = hnswindex.net_amd
    dim = 128
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((a.nq, dim), dtype=np.float32)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "queries_per_call": a.nq, "timed_calls": a.steps},
           "lines": {}, "evals_check": True}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    ix = hnswindex.Index(dim, "sq_euclid")
    ix.set_collection_size(a.n)
    ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    res["build_seconds"] = round(time.perf_counter() - t0, 2)

    # radii: order statistics of 64 queries' distances to every row
    sub = 64
    every = np.arange(a.n, dtype=np.int32)
    pooled = np.sort(np.concatenate([oracle.dist_query_rows("sq_euclid", x, q[i], every) for i in range(sub)]))
    targets = (10,) if a.quick else (10, 340, 5000)
    radii = {t: float(pooled[sub * t - 1]) for t in targets}
    rng = np.random.default_rng(7)
    masks = {"unfiltered": None, "random_0.1": rng.random(a.n) < 0.1, "random_0.01": rng.random(a.n) < 0.01}
    if a.quick:
        masks = {"random_0.01": masks["random_0.01"]}

    for target, radius in radii.items():
        for name, mask in masks.items():
            n_allowed = a.n if mask is None else int(mask.sum())
            ix.set_profiling(False)
            walls = walls_of(lambda: ix.exact_range_query(q, radius, allowed=mask), a.steps)
            ix.set_profiling(True)    # kernel time and counters: a pass of its own
            ix.reset_stats()
            e_ids, _ = ix.exact_range_query(q, radius, allowed=mask)
            st, info = ix.stats(), ix.exact_range_info()
            ix.set_profiling(False)
            pairs = a.nq * n_allowed   # one pass; the queries of a repeated round are measured twice
            ok = st["exact_evals"] == pairs if info["repeated_rounds"] == 0 else pairs < st["exact_evals"] <= 2 * pairs
            res["evals_check"] = bool(res["evals_check"] and ok)
            wall = float(np.median(walls))
            total = int(sum(v.size for v in e_ids))
            line = {"radius": radius, "allowed": n_allowed, "results_per_query": round(total / a.nq, 2),
                    "longest_list": int(max(v.size for v in e_ids)),
                    "exact": {"queries_per_sec": round(a.nq / wall, 1), "ms_per_call": round(1e3 * wall, 3), "ms_per_call_repeats": [round(1e3 * w, 3) for w in walls],
                              "scan_kernel_ms": round(st["exact_kernel_ms"], 3), "exact_launches": int(st["exact_launches"]),
                              "exact_evals": int(st["exact_evals"]), **{k: int(v) for k, v in info.items()}}}
            # the traversal beside it
            call = (lambda: ix.range_query(q, radius)) if mask is None else (lambda: ix.range_query(q, radius, allowed=mask))
            t = time.perf_counter()
            t_ids, _ = call()
            first = time.perf_counter() - t
            steps = a.steps if first < 1.0 else 1
            tw = []
            for _ in range(steps):
                t = time.perf_counter()
                t_ids, _ = call()
                tw.append(time.perf_counter() - t)
            t_wall = float(np.median(tw))
            found = int(sum(np.isin(t_ids[i], e_ids[i]).sum() for i in range(a.nq)))
            line["traversal"] = {"queries_per_sec": round(a.nq / t_wall, 1), "ms_per_call": round(1e3 * t_wall, 3), "timed_calls": steps,
                                 "results_per_query": round(sum(v.size for v in t_ids) / a.nq, 2),
                                 "results_not_in_the_exact_lists": int(sum(v.size for v in t_ids)) - found,
                                 "recall": round(found / total, 5) if total else None}
            line["exact_over_traversal"] = round(line["exact"]["queries_per_sec"] / line["traversal"]["queries_per_sec"], 3)
            res["lines"][f"about_{target}_{name}"] = line
            print(f"about_{target}_{name}", line, flush=True)
            save()

    # the scan without its merges: a radius that admits nothing, beside exact_knn(k = 10)
    nothing = float(np.nextafter(pooled[0], np.float32(-np.inf))) - 1.0
    ix.reset_stats()
    r_walls = walls_of(lambda: ix.exact_range_query(q, nothing), a.steps)
    assert ix.exact_range_info()["results"] == 0
    k_walls = walls_of(lambda: ix.exact_knn_query(q, 10), a.steps)
    spread = lambda w: round(1e3 * (max(w) - min(w)), 3)   # noqa: E731
    res["empty_radius_against_exact_knn_k10"] = {
        "exact_range_ms": [round(1e3 * w, 3) for w in r_walls], "exact_knn_ms": [round(1e3 * w, 3) for w in k_walls],
        "exact_range_median_ms": round(1e3 * float(np.median(r_walls)), 3), "exact_knn_median_ms": round(1e3 * float(np.median(k_walls)), 3),
        "spread_ms": {"exact_range": spread(r_walls), "exact_knn": spread(k_walls)},
        "range_slower_by_more_than_the_spread": bool(np.median(r_walls) - np.median(k_walls) > max(max(r_walls) - min(r_walls), max(k_walls) - min(k_walls)))}
    print(res["empty_radius_against_exact_knn_k10"], flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
