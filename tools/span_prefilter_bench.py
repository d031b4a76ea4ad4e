#!/usr/bin/env python3
"""A/B of the spanning trees' MFMA prefilter on the device, one process: single_linkage_tree and
mutual_reachability_tree (min_samples 1 and 5) through DeviceBackend.exact_span_tree / exact_mreach_tree over C2's rows -- 128 uniform
elements, 1 % of the rows planted near-duplicates (tools/near_dup_bench.py's recipe), only the member rows uploaded -- for sq_euclid.
Per case a warm-up call of both forms, then the plain kernels (diag exact_prefilter=0: span_scan_kernel / mreach_scan_kernel, the code
the parent commit runs) and the new form (exact_prefilter=2) alternating, `--runs` calls each; per call the wall ms (host clock around
the call, which ends in a synchronise) and the scans' ms from exact_kernel_ms; edges, weights, core and info of both forms are compared
on every case.  Cases: 16 384, 49 152 and 131 072 members; the new form's chunk forced at 131 072 members; and the adverse table: rows
100 + 0.1 noise, 32 768 members, where the tile can turn nothing away.  The file is rewritten after every case.
    python tools/span_prefilter_bench.py [-o profiles/span_prefilter_c2.json] [--members 16384,49152,131072] [--runs 5]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from triangle_prefilter_bench import planted  # noqa: E402  (C2's rows with 1 % planted near-duplicates)

CALLS = {"single_linkage_tree": lambda db, n: db.exact_span_tree(n),
         "mutual_reachability_tree(1)": lambda db, n: db.exact_mreach_tree(n, 1),
         "mutual_reachability_tree(5)": lambda db, n: db.exact_mreach_tree(n, 5)}


def one(db, call, mode, chunk=0):
    os.environ["HNSW_MI355X_DIAG"] = f"exact_prefilter={mode},exact_chunk={chunk}"   # read by the library on every use
    db.reset_stats()
    t0, pf0 = time.perf_counter(), db.span_prefilter_stats()
    got = call()
    wall = (time.perf_counter() - t0) * 1e3
    st, pf1 = db.stats(), db.span_prefilter_stats()
    on_tile = pf1["pairs_on_tile"] - pf0["pairs_on_tile"]
    return got, {"mode": mode, "wall_ms": round(wall, 3), "kernel_ms": round(st["exact_kernel_ms"], 3), "launches_on_tile": pf1["launches"] - pf0["launches"],
                 "remeasured_over_on_tile": (pf1["pairs_remeasured"] - pf0["pairs_remeasured"]) / on_tile if on_tile else None}


def same(a, b):
    return all(u == v if isinstance(u, dict) else u.tobytes() == v.tobytes() for u, v in zip(a, b))


def ab(db, call, runs, chunk=0):
    out, ans = [], {}
    for mode in (0, 2):
        ans[mode], _ = one(db, call, mode, chunk if mode else 0)   # warm-up: a first call allocates its scratch
    for _ in range(runs):
        for mode in (0, 2):
            ans[mode], r = one(db, call, mode, chunk if mode else 0)
            out.append(r)
    plain, new = [r for r in out if r["mode"] == 0], [r for r in out if r["mode"] == 2]
    return {"same_edges_weights_core_info": bool(same(ans[0], ans[2])), "info": ans[2][-1],
            "plain_kernel_ms": [r["kernel_ms"] for r in plain], "new_kernel_ms": [r["kernel_ms"] for r in new],
            "plain_wall_ms": [r["wall_ms"] for r in plain], "new_wall_ms": [r["wall_ms"] for r in new],
            "launches_on_tile": new[-1]["launches_on_tile"], "remeasured_over_on_tile": new[-1]["remeasured_over_on_tile"],
            "every_new_run_beats_every_plain_run": max(r["kernel_ms"] for r in new) < min(r["kernel_ms"] for r in plain)
            and max(r["wall_ms"] for r in new) < min(r["wall_ms"] for r in plain)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=str(ROOT / "profiles" / "span_prefilter_c2.json"))
    ap.add_argument("--members", default="16384,49152,131072")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunks", default="1024,2048,8192,16384")
    args = ap.parse_args()
    import hnswindex
    sizes = [int(v) for v in args.members.split(",")]
    res = {"build_id": hnswindex.net_amd.lib.hnsw_mi355x_build_id().decode(), "members": sizes, "runs": args.runs, "cases": {}}

    def case(name, db, call, **kw):
        res["cases"][name] = c = ab(db, call, **kw)
        print(name, "same" if c["same_edges_weights_core_info"] else "DIFFERENT", "plain", c["plain_kernel_ms"], "new", c["new_kernel_ms"],
              "wall", c["plain_wall_ms"], c["new_wall_ms"], "remeasured/on_tile", c["remeasured_over_on_tile"], flush=True)
        Path(args.o).parent.mkdir(parents=True, exist_ok=True)
        Path(args.o).write_text(json.dumps(res, indent=1) + "\n")

    def backend(x):
        db = hnswindex.DeviceBackend(x.shape[1], "sq_euclid", capacity=x.shape[0])
        db.upload_rows(0, x)
        db.set_profiling(True)
        return db

    x = planted(max(sizes), 128, np.random.default_rng(65539))
    db = backend(x)
    for m in sizes:
        for name, f in CALLS.items():
            case(f"{name} m={m}", db, lambda: f(db, m), runs=args.runs)
    for chunk in [int(v) for v in args.chunks.split(",") if v]:     # beside the default of about 4 096 rows, against the same plain kernel
        case(f"single_linkage_tree m={max(sizes)} chunk={chunk}", db, lambda: CALLS["single_linkage_tree"](db, max(sizes)), runs=3, chunk=chunk)
    del db
    m = 32768
    db = backend((100.0 + 0.1 * np.random.default_rng(2024).standard_normal((m, 128), dtype=np.float32)).astype(np.float32))
    for name, f in CALLS.items():
        case(f"{name} m={m} rows 100 + 0.1 noise", db, lambda: f(db, m), runs=3)
    os.environ.pop("HNSW_MI355X_DIAG", None)


if __name__ == "__main__":
    main()
