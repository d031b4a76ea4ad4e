#!/usr/bin/env python3
"""A/B of the cosine family's MFMA prefilter on the device: exact_knn at C3 -- 1M x 768 unit rows, 4 096 queries,
k = 10, rows added only -- for ucosine and ucosine_f16, cosine on the unnormalised rows, the plain kernel (diag exact_prefilter=0:
exact_scan_kernel<M, ExactTopK>, the code the parent commit runs) and the new form alternating in one process, five runs each, a run =
a warm-up call and `--calls` timed calls, its figure their median.  Then once each: k = 50, the 4- against the 8-wave block at dim 768
(exact_prefilter=2 with exact_qtile=4 / 8), dims 64, 128, 256 and 1 024 for ucosine, 128 and 256 for the other two, and the adverse table at 32 768 x 768 (rows and queries
unit(v + 1e-4 noise): the tile turns nothing away).  Per run: wall ms per call, scan + merge ms from exact_kernel_ms,
pairs_remeasured / pairs_on_tile; ids and distance bytes of both forms are compared on every shape.
    python tools/exact_prefilter_cos_bench.py [-o profiles/exact_prefilter_cos_c3.json] [--rows 1000000] [--queries 4096] [--runs 5] [--calls 3]"""
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
    os.environ["HNSW_MI355X_DIAG"] = mode   # read by the library on every use


def run(db, q, k, mode, calls):
    """One run: a warm-up call, then `calls` timed ones -> medians, the tile's ratio, the answer of the last call."""
    set_mode(mode)
    got = db.exact_knn(q, k)
    db.reset_stats()
    pf0 = db.exact_prefilter_stats()
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        got = db.exact_knn(q, k)
        wall.append((time.perf_counter() - t0) * 1e3)
    st, pf1 = db.stats(), db.exact_prefilter_stats()
    on_tile = pf1["pairs_on_tile"] - pf0["pairs_on_tile"]
    return got, {"mode": mode, "wall_ms": statistics.median(wall), "kernel_ms": st["exact_kernel_ms"] / max(st["exact_timed_launches"], 1),
                 "launches_on_tile": pf1["launches"] - pf0["launches"], "exact_evals": st["exact_evals"],
                 "remeasured_over_on_tile": (pf1["pairs_remeasured"] - pf0["pairs_remeasured"]) / on_tile if on_tile else None}


def ab(db, q, k, runs, calls, new_mode="exact_prefilter=2", old_mode="exact_prefilter=0"):
    out, answers = [], {}
    for _ in range(runs):
        for mode in (old_mode, new_mode):
            answers[mode], r = run(db, q, k, mode, calls)
            out.append(r)
    a, b = answers[old_mode], answers[new_mode]
    same = bool((a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes())
    old, new = [r for r in out if r["mode"] == old_mode], [r for r in out if r["mode"] == new_mode]
    return {"runs": out, "same_ids_and_bytes": same, "old_mode": old_mode, "new_mode": new_mode,
            "old_kernel_ms": [r["kernel_ms"] for r in old], "new_kernel_ms": [r["kernel_ms"] for r in new],
            "every_new_run_beats_every_old_run": max(r["kernel_ms"] for r in new) < min(r["kernel_ms"] for r in old)
            and max(r["wall_ms"] for r in new) < min(r["wall_ms"] for r in old)}


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def backend(dim, metric, x):
    import hnswindex
    db = hnswindex.DeviceBackend(dim, metric, capacity=x.shape[0])
    db.upload_rows(0, x)
    db.set_profiling(True)
    return db


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=str(ROOT / "profiles" / "exact_prefilter_cos_c3.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated case prefixes; empty: all")
    args = ap.parse_args()
    want = lambda name: not args.only or any(name.startswith(p) for p in args.only.split(","))   # noqa: E731
    rng = np.random.default_rng(2024)
    n, nq, dim, k = args.rows, args.queries, 768, 10
    res = {"rows": n, "queries": nq, "dim": dim, "k": k, "runs": args.runs, "calls_per_run": args.calls, "cases": {}, "not_measured": []}
    out = Path(args.o)
    out.parent.mkdir(parents=True, exist_ok=True)
    if args.only and out.exists():   # a further visit adds its cases to the file
        res["cases"] = json.loads(out.read_text())["cases"]

    def case(name, fn):
        if not want(name):
            res["not_measured"].append(name)
            return
        c = res["cases"][name] = fn()
        out.write_text(json.dumps(res, indent=1) + "\n")
        print(name, "same" if c["same_ids_and_bytes"] else "DIFFERENT", "old", [round(v, 2) for v in c["old_kernel_ms"]], "new", [round(v, 2) for v in c["new_kernel_ms"]],
              "remeasured/on_tile", c["runs"][-1]["remeasured_over_on_tile"], flush=True)

    raw, q = rng.random((n, dim), dtype=np.float32), unit(rng.random((nq, dim), dtype=np.float32))
    x = unit(raw)
    for metric in ("ucosine", "ucosine_f16", "cosine"):
        if not want(metric + " "):
            res["not_measured"].append(metric + " *")
            continue
        db = backend(dim, metric, raw if metric == "cosine" else x)
        case(f"{metric} 768", lambda: ab(db, q, k, args.runs, args.calls))
        if metric == "ucosine":
            case("ucosine 768 k=50", lambda: ab(db, q, 50, 1, args.calls))
            case("ucosine 768 waves 4 (old) against 8 (new)",
                 lambda: ab(db, q, k, 2, args.calls, new_mode="exact_prefilter=2,exact_qtile=8", old_mode="exact_prefilter=2,exact_qtile=4"))
        del db
    del raw, x
    for metric, dim2 in (("ucosine", 64), ("ucosine", 128), ("ucosine", 256), ("ucosine", 1024), ("ucosine_f16", 128), ("ucosine_f16", 256),
                         ("cosine", 128), ("cosine", 256)):                 # the other row lengths, two runs each
        if not want(f"{metric} {dim2}"):
            res["not_measured"].append(f"{metric} {dim2}")
            continue
        raw2, q2 = rng.random((n, dim2), dtype=np.float32), unit(rng.random((nq, dim2), dtype=np.float32))
        db = backend(dim2, metric, raw2 if metric == "cosine" else unit(raw2))
        case(f"{metric} {dim2}", lambda: ab(db, q2, k, 2, args.calls))
        del db, raw2
    if want("ucosine adverse"):
        v, m = rng.random(dim, dtype=np.float32), 32768
        xa = unit(v + np.float32(1e-4) * rng.standard_normal((m, dim)).astype(np.float32))
        qa = unit(v + np.float32(1e-4) * rng.standard_normal((nq, dim)).astype(np.float32))
        db = backend(dim, "ucosine", xa)
        case("ucosine adverse 32768 x 768", lambda: ab(db, qa, k, 1, args.calls))
        del db
    else:
        res["not_measured"].append("ucosine adverse 32768 x 768")
    os.environ.pop("HNSW_MI355X_DIAG", None)
    res["not_measured"] = [name for name in res["not_measured"] if name not in res["cases"] and not any(c.startswith(name.rstrip("*")) for c in res["cases"])]
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
