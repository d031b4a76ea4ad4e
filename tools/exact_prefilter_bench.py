#!/usr/bin/env python3
"""A/B of the flat scan's MFMA prefilter on the device: exact_knn at C2 -- 1M x 128 uniform rows, 4 096 queries,
k = 10, unfiltered -- for sq_euclid and sq_euclid_f16, the plain kernel (diag exact_prefilter=0: exact_scan_kernel<M, ExactTopK>, the
code the parent commit runs, equal code hash in profiles/exact_prefilter_kernel_resources.json) and the default (1) alternating, five
runs each, a run = a warm-up call and `--calls` timed calls, its figure their median.  Then once each: the 1 % allow-set line of
3.14, the clustered table (rows = 100 + 0.1 noise: the tile turns nothing away), and the shapes around the picker's floors (forced
with exact_prefilter=2).  Per run: wall ms per call (host clock around the call, which ends in a synchronise), scan + merge ms from
exact_kernel_ms, pairs_remeasured / pairs_on_tile; ids and distance bytes of both forms are compared on every shape.
    python tools/exact_prefilter_bench.py [-o profiles/exact_prefilter_c2.json] [--rows 1000000] [--queries 4096] [--runs 5] [--calls 3]"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def set_mode(mode):
    os.environ["HNSW_MI355X_DIAG"] = f"exact_prefilter={mode}"   # read by the library on every use


def run(db, q, k, allowed, mode, calls):
    """One run: a warm-up call, then `calls` timed ones -> medians, the tile's ratio, the answer of the last call."""
    set_mode(mode)
    got = db.exact_knn(q, k, allowed=allowed)
    db.reset_stats()
    pf0 = db.exact_prefilter_stats()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        got = db.exact_knn(q, k, allowed=allowed)
        wall.append((time.perf_counter() - t0) * 1e3)
    st, pf1 = db.stats(), db.exact_prefilter_stats()
    on_tile = pf1["pairs_on_tile"] - pf0["pairs_on_tile"]
    return got, {"mode": mode, "wall_ms": statistics.median(wall), "kernel_ms": st["exact_kernel_ms"] / max(st["exact_timed_launches"], 1),
                 "launches_on_tile": pf1["launches"] - pf0["launches"], "exact_evals": st["exact_evals"],
                 "remeasured_over_on_tile": (pf1["pairs_remeasured"] - pf0["pairs_remeasured"]) / on_tile if on_tile else None}


def ab(db, q, k, allowed, runs, calls, new_mode=1):
    out, answers = [], {}
    for _ in range(runs):
        for mode in (0, new_mode):
            answers[mode], r = run(db, q, k, allowed, mode, calls)
            out.append(r)
    a, b = answers[0], answers[new_mode]
    same = bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())
    plain, new = [r for r in out if r["mode"] == 0], [r for r in out if r["mode"] != 0]
    return {"runs": out, "same_ids_and_bytes": same,
            "plain_kernel_ms": [r["kernel_ms"] for r in plain], "new_kernel_ms": [r["kernel_ms"] for r in new],
            "every_new_run_beats_every_plain_run": max(r["kernel_ms"] for r in new) < min(r["kernel_ms"] for r in plain)
            and max(r["wall_ms"] for r in new) < min(r["wall_ms"] for r in plain)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=str(ROOT / "profiles" / "exact_prefilter_c2.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    import hnswindex
    rng = np.random.default_rng(2024)
    n, nq, dim, k = args.rows, args.queries, 128, 10
    x, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
    clustered = (100.0 + 0.1 * rng.standard_normal((n, dim), dtype=np.float32)).astype(np.float32)
    cq = (100.0 + 0.1 * rng.standard_normal((nq, dim), dtype=np.float32)).astype(np.float32)
    mask = rng.random(n) < 0.01
    res = {"rows": n, "queries": nq, "dim": dim, "k": k, "runs": args.runs, "calls_per_run": args.calls, "cases": {}}
    for metric in ("sq_euclid", "sq_euclid_f16"):
        db = hnswindex.DeviceBackend(dim, metric, capacity=n)
        db.upload_rows(0, x)
        db.set_profiling(True)
        res["cases"][f"{metric} unfiltered"] = ab(db, q, k, None, args.runs, args.calls)
        res["cases"][f"{metric} unfiltered k=64"] = ab(db, q, 64, None, 1, args.calls)
        res["cases"][f"{metric} allow-set 1%"] = ab(db, q, k, mask, 1, args.calls, new_mode=2)
        for fq, fm in ((256, 65536), (256, n), (nq, 65536), (64, n)):      # around the picker's floors
            res["cases"][f"{metric} nq={fq} m={fm}"] = ab(db, q[:fq], k, np.arange(fm, dtype=np.int32) if fm < n else None, 1, args.calls, new_mode=2)
        db.upload_rows(0, clustered)
        res["cases"][f"{metric} clustered"] = ab(db, cq, k, None, 1, args.calls)
        del db
    for dim2 in (64, 256):                                                  # the other row lengths, a quarter of the rows
        x2, q2 = rng.random((n // 4, dim2), dtype=np.float32), rng.random((nq, dim2), dtype=np.float32)
        db = hnswindex.DeviceBackend(dim2, "sq_euclid", capacity=n // 4)
        db.upload_rows(0, x2)
        db.set_profiling(True)
        res["cases"][f"sq_euclid dim={dim2} m={n // 4}"] = ab(db, q2, k, None, 1, args.calls)
        del db
    os.environ.pop("HNSW_MI355X_DIAG", None)
    Path(args.o).parent.mkdir(parents=True, exist_ok=True)
    Path(args.o).write_text(json.dumps(res, indent=1) + "\n")
    for name, c in res["cases"].items():
        print(name, "same" if c["same_ids_and_bytes"] else "DIFFERENT", "plain", [round(v, 2) for v in c["plain_kernel_ms"]], "new", [round(v, 2) for v in c["new_kernel_ms"]],
              "remeasured/on_tile", c["runs"][-1]["remeasured_over_on_tile"])


if __name__ == "__main__":
    main()
