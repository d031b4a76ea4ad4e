#!/usr/bin/env python3
"""A/B of the int8 flat scan on the i8 MFMA tile on the device: exact_knn on sq_euclid_i8 -- 1M x 128 and 1M x 96
uniform rows, 4 096 queries, k = 10 -- the plain kernel (diag exact_prefilter=0: exact_scan_kernel<M_I8, ExactTopK>, the code the parent
commit runs) and the new form (exact_prefilter=2) alternating in one process, five runs each, a run = a warm-up call and `--calls`
timed calls, its figures the median wall time and the mean kernel time of those.  Then once each per row length: k = 64, a 1 % allow-set, a call below the picker's floors (64
queries), and at dim 128 the adverse tables: 32 768 equal rows, and 32 768 rows of four distinct vectors.  Per run: wall ms per call
(host clock around the call, which ends in a synchronise), scan + merge ms from exact_kernel_ms, pairs_remeasured / pairs_on_tile; ids
and distance bytes of both forms are compared on every shape.
    python tools/exact_i8_tile_bench.py [-o profiles/exact_i8_tile_c2.json] [--rows 1000000] [--queries 4096] [--runs 5] [--calls 3]"""
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


def run(db, q, k, allowed, mode, calls):
    """One run: a warm-up call, then `calls` timed ones -> medians, the tile's ratio, the answer of the last call."""
    os.environ["HNSW_MI355X_DIAG"] = f"exact_prefilter={mode}"   # read by the library on every use
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


def ab(db, q, k, allowed, runs, calls):
    out, answers = [], {}
    for _ in range(runs):
        for mode in (0, 2):
            answers[mode], r = run(db, q, k, allowed, mode, calls)
            out.append(r)
    a, b = answers[0], answers[2]
    same = bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())
    plain, new = [r for r in out if r["mode"] == 0], [r for r in out if r["mode"] != 0]
    return {"runs": out, "same_ids_and_bytes": same,
            "plain_kernel_ms": [r["kernel_ms"] for r in plain], "new_kernel_ms": [r["kernel_ms"] for r in new],
            "every_new_run_beats_every_plain_run": max(r["kernel_ms"] for r in new) < min(r["kernel_ms"] for r in plain)
            and max(r["wall_ms"] for r in new) < min(r["wall_ms"] for r in plain)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=str(ROOT / "profiles" / "exact_i8_tile_c2.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--dims", default="128,96")
    args = ap.parse_args()
    import hnswindex
    rng = np.random.default_rng(2024)
    n, nq, k = args.rows, args.queries, 10
    res = {"metric": "sq_euclid_i8", "rows": n, "queries": nq, "k": k, "runs": args.runs, "calls_per_run": args.calls, "cases": {}}
    out = Path(args.o)
    out.parent.mkdir(parents=True, exist_ok=True)

    def case(name, c):
        res["cases"][name] = c
        out.write_text(json.dumps(res, indent=1) + "\n")
        print(name, "same" if c["same_ids_and_bytes"] else "DIFFERENT", "plain", [round(v, 2) for v in c["plain_kernel_ms"]], "new", [round(v, 2) for v in c["new_kernel_ms"]],
              "remeasured/on_tile", c["runs"][-1]["remeasured_over_on_tile"], flush=True)

    def backend(x):
        db = hnswindex.DeviceBackend(x.shape[1], "sq_euclid_i8", capacity=x.shape[0])
        db.upload_rows(0, x)
        db.set_profiling(True)
        return db

    mask = rng.random(n) < 0.01
    for dim in (int(d) for d in args.dims.split(",")):
        x, q = rng.random((n, dim), dtype=np.float32), rng.random((nq, dim), dtype=np.float32)
        db = backend(x)
        case(f"dim {dim} unfiltered", ab(db, q, k, None, args.runs, args.calls))
        case(f"dim {dim} unfiltered k=64", ab(db, q, 64, None, 1, args.calls))
        case(f"dim {dim} allow-set 1%", ab(db, q, k, mask, 1, args.calls))
        case(f"dim {dim} below the floors: nq=64", ab(db, q[:64], k, None, 1, args.calls))
        del db
        if dim == 128:   # the adverse tables: equal distances everywhere, a bound alone turns nothing away
            for distinct in (1, 4):
                db = backend(x[:distinct][np.arange(32768) % distinct])
                case(f"dim {dim} adverse: 32768 rows, {distinct} distinct", ab(db, q, k, None, 1, args.calls))
                del db
        del x
    os.environ.pop("HNSW_MI355X_DIAG", None)


if __name__ == "__main__":
    main()
