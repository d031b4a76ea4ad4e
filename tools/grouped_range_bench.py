#!/usr/bin/env python3
"""range_query_grouped at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128: the index of
tools/grouped_knn_bench.py) beside the loop it replaces, in one session:
    grouped   Index.range_query_grouped(q, radius, row_group, query_group, G)
    loop      per group g: Index.range_query(q[sel_g], radius, allowed=mask_g), masks and selections built beforehand
16 384 queries assigned uniformly to G in {10, 100, 1 000} random groups; radii for about 10 and about 340 results per query
within a group, taken from the distribution of true distances (the share F(r) = target * G / n of all rows lies within r).  The
traversal's closure is the whole ball, n * F(r) ids per query, whatever the group: a case whose ball exceeds --max-closure ids per
query is not run and is recorded as such.  Per case: the median wall time of --steps calls after a warm-up for both, their ratio,
whether the bytes are equal, results per query, the grouped call's counters.  G = 1: the grouped call against the plain
range_query, with the spread of the plain call's own timings.
    python tools/grouped_range_bench.py [--out profiles/grouped_range_c2.json] [--steps 5]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(f, steps):
    out = f()   # warm-up (a first call allocates its scratch)
    walls = []
    for _ in range(steps):
        t = time.perf_counter()
        out = f()
        walls.append(1e3 * (time.perf_counter() - t))
    return out, walls


def same(a, b):
    return len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() and v.tobytes() == w.tobytes() for x, y, v, w in zip(a[0], b[0], a[1], b[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grouped_range_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--max-closure", type=int, default=4000)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, nq = 128, a.queries
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((nq, dim), dtype=np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": 16, "ef_construction": 200, "min_nn": 128, "queries": nq, "timed_calls": a.steps,
                      "statistic": "median wall ms per call after one warm-up call", "max_closure": a.max_closure},
           "build_seconds": round(time.perf_counter() - t0, 2), "cases": {}, "not_run": {}}
    rng = np.random.default_rng(11)
    sample = x[rng.choice(a.n, 20000, replace=False)]
    true_d = np.sort(np.concatenate([((sample - qq) ** 2).sum(1) for qq in q[:64]]).astype(np.float32))

    for n_groups in (10, 100, 1000):
        rg = rng.integers(0, n_groups, a.n).astype(np.int32)
        qg = rng.integers(0, n_groups, nq).astype(np.int32)
        groups = [int(g) for g in np.unique(qg)]
        masks = {g: rg == g for g in groups}
        sels = {g: np.flatnonzero(qg == g) for g in groups}
        for target in (10, 340):
            name = f"G{n_groups}_r{target}"
            share = target * n_groups / a.n
            if share * a.n > a.max_closure:
                res["not_run"][name] = f"the ball holds about {int(share * a.n)} ids per query, above max_closure"
                continue
            radius = float(true_d[int(share * true_d.size)])

            def grouped():
                return ix.range_query_grouped(q, radius, rg, qg, n_groups)

            def loop():
                ids, d = [None] * nq, [None] * nq
                for g in groups:
                    a_ids, a_d = ix.range_query(q[sels[g]], radius, allowed=masks[g])
                    for w, i, v in zip(sels[g], a_ids, a_d):
                        ids[w], d[w] = i, v
                return ids, d

            ix.reset_stats()
            got, walls = timed(grouped, a.steps)
            info, st = ix.range_grouped_info(), ix.stats()
            want, loop_walls = timed(loop, a.steps)
            ms, loop_ms = float(np.median(walls)), float(np.median(loop_walls))
            c = {"groups": n_groups, "radius": radius, "grouped_ms": round(ms, 3), "loop_ms": round(loop_ms, 3), "loop_over_grouped": round(loop_ms / ms, 2),
                 "same_bytes_as_loop": same(got, want), "results_per_query": round(float(np.mean([i.size for i in got[0]])), 2),
                 "grouped_info_over_all_calls": info, "range_kernel_ms_over_all_calls": st.get("range_kernel_ms"),
                 "closure_per_query": round(st.get("range_results", 0) / max(1, (a.steps + 1) * nq), 1) if "range_results" in st else None}
            res["cases"][name] = c
            print(name, c, flush=True)

    # one group: the descriptor path against the plain call
    radius = float(true_d[int(340 / a.n * true_d.size)])
    rg, qg = np.zeros(a.n, np.int32), np.zeros(nq, np.int32)
    plain, plain_walls = timed(lambda: ix.range_query(q, radius), a.steps)
    got, walls = timed(lambda: ix.range_query_grouped(q, radius, rg, qg, 1), a.steps)
    res["one_group"] = {"radius": radius, "plain_ms": [round(w, 3) for w in plain_walls], "plain_median_ms": round(float(np.median(plain_walls)), 3),
                        "plain_spread_ms": round(max(plain_walls) - min(plain_walls), 3), "grouped_ms": [round(w, 3) for w in walls],
                        "grouped_median_ms": round(float(np.median(walls)), 3), "same_bytes_as_plain": same(got, plain),
                        "results_per_query": round(float(np.mean([i.size for i in got[0]])), 2)}
    print("one_group", res["one_group"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
