#!/usr/bin/env python3
"""knn_query_grouped at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128, k = 10: the index of
tools/filtered_bench.py) beside what it replaces and beside the grouped flat scan, all in one session:
    grouped        Index.knn_query_grouped(q, k, row_group, query_group, G)
    loop           per group g: Index.knn_query(q[sel_g], k, allowed=mask_g), masks and selections built beforehand
    loop_build     the same loop with mask_g = (row_group == g) and sel_g = (query_group == g) built inside it
    exact_grouped  Index.exact_knn_query_grouped on the same inputs (exact answers: its recall is 1 by construction)
Cases: uniform random groups, G in {2, 4, 16}, at 1 024 and at 65 536 queries per call; one skewed labelling (one group with 70 %
of the rows, fifteen sharing the rest, queries distributed like the rows) at both sizes; G = 1 against the filtered call with
everything allowed.  Per case: the median wall time of --steps calls after a warm-up, device evaluations per query, hand-backs,
whether grouped and loop returned the same bytes, the recall@10 of the grouped call against the scan, and the label upload's
share: the wall time of staging the same bytes (row_group, query_group, order table) through pinned memory to the device, timed
apart with torch, over the grouped call's time.
    python tools/grouped_knn_bench.py [--out profiles/grouped_knn_c2.json] [--steps 5]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def median_ms(f, steps):
    out = f()   # warm-up (a first call allocates its scratch)
    walls = []
    for _ in range(steps):
        t = time.perf_counter()
        out = f()
        walls.append(time.perf_counter() - t)
    return out, round(1e3 * float(np.median(walls)), 3)


def same(a, b):
    return bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())


def upload_ms(n_labels, nq, steps):
    """The bytes a grouped call sends up (labels, the queries' groups, the order table), staged as the call stages them."""
    import torch
    src = np.zeros(n_labels + 2 * nq, np.int32)
    pin = torch.empty(src.size, dtype=torch.int32).pin_memory()
    dev = torch.empty(src.size, dtype=torch.int32, device="cuda")

    def go():
        np.copyto(pin.numpy(), src)
        dev.copy_(pin, non_blocking=True)
        torch.cuda.synchronize()
    return median_ms(go, steps)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "grouped_knn_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, k = 128, 10
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q_all = np.random.default_rng(65540).random((65536, dim), dtype=np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    build_s = time.perf_counter() - t0
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(), "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": 16, "ef_construction": 200,
           "min_nn": 128, "k": k, "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(build_s, 2), "cases": {}}
    rng = np.random.default_rng(11)
    labelings = {f"uniform_G{g}": (rng.integers(0, g, a.n).astype(np.int32), g, None) for g in (2, 4, 16)}
    p = np.array([0.7] + [0.3 / 15] * 15)
    labelings["skewed_G16_70pct"] = (rng.choice(16, a.n, p=p).astype(np.int32), 16, p)
    labelings["one_group_G1"] = (np.zeros(a.n, np.int32), 1, None)

    def evals_and_handbacks(f, nq):
        ix.reset_stats()
        f()
        st = ix.stats()
        return round(st["search_evals"] / nq, 1), int(st["search_overflows"])

    for name, (rg, n_groups, prob) in labelings.items():
        for nq in (1024, 65536):
            q = q_all[:nq]
            qg = (rng.integers(0, n_groups, nq) if prob is None else rng.choice(n_groups, nq, p=prob)).astype(np.int32)
            groups = [int(g) for g in np.unique(qg)]
            masks = {g: rg == g for g in groups}
            sels = {g: np.flatnonzero(qg == g) for g in groups}

            def grouped():
                return ix.knn_query_grouped(q, k, rg, qg, n_groups)

            def loop(build=False):
                ids, d = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32)
                for g in groups:
                    sel = np.flatnonzero(qg == g) if build else sels[g]
                    ids[sel], d[sel] = ix.knn_query(q[sel], k, allowed=(rg == g) if build else masks[g])
                return ids, d

            def exact():
                return ix.exact_knn_query_grouped(q, k, rg, qg, n_groups)

            got, ms = median_ms(grouped, a.steps)
            want, loop_ms = median_ms(loop, a.steps)
            _, build_ms = median_ms(lambda: loop(True), a.steps)
            truth, exact_ms = median_ms(exact, a.steps)
            c = {"groups": n_groups, "queries": nq, "grouped_ms": ms, "loop_ms": loop_ms, "loop_build_ms": build_ms, "exact_grouped_ms": exact_ms,
                 "loop_over_grouped": round(loop_ms / ms, 2), "loop_build_over_grouped": round(build_ms / ms, 2),
                 "exact_grouped_over_grouped": round(exact_ms / ms, 2), "same_bytes_as_loop": same(got, want)}
            c["evals_per_query"], c["handbacks"] = evals_and_handbacks(grouped, nq)
            c["loop_evals_per_query"], c["loop_handbacks"] = evals_and_handbacks(loop, nq)
            up = upload_ms(a.n, nq, a.steps)
            c["label_upload_ms"], c["label_upload_share"] = up, round(up / ms, 3)
            c["recall_at_10_vs_scan"] = round(float(np.mean([len(set(g.tolist()) & set(h.tolist())) / k for g, h in zip(truth[0], got[0])])), 4)
            if name == "one_group_G1":   # ... against the filtered call with everything allowed, on this build
                allowed = np.ones(a.n, dtype=bool)
                f_out, f_ms = median_ms(lambda: ix.knn_query(q, k, allowed=allowed), a.steps)
                c["filtered_all_allowed_ms"], c["same_bytes_as_filtered_all_allowed"] = f_ms, same(got, f_out)
            res["cases"][f"{name}_q{nq}"] = c
            print(name, nq, c, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
