#!/usr/bin/env python3
"""A/B of the triangle scans' MFMA prefilter on the device, one process: duplicate_groups, neighbor_counts and
density_clusters (min_samples 5) through DeviceBackend.exact_range_groups / exact_range_density over C2's rows -- 1M x 128 uniform, 1 %
of them planted near-duplicates (tools/near_dup_bench.py's recipe), radius 0.05 -- for sq_euclid and sq_euclid_f16.  Per case a warm-up
call of both forms, then the plain kernel (diag exact_prefilter=0: exact_scan_kernel with the call's sink, the code the parent commit
runs) and the new form (exact_prefilter=2) alternating, `--runs` calls each; per call the wall ms (host clock around the call, which
ends in a synchronise) and the scan's ms from exact_kernel_ms; labels, counts and info of both forms are compared on every case.
Cases: 16 384, 131 072 and 1M members (the plain side of 1M once); dims 64 and 256 at 65 536 members; the new form's chunk forced
at 131 072 members; and the two adverse tables: rows 100 + 0.1 noise, where the tile can turn nothing away, and a radius that holds
about 7 % of all pairs, where the density sinks pay one atomic per within pair.  The file is rewritten after every case.
    python tools/triangle_prefilter_bench.py [-o profiles/triangle_prefilter_c2.json] [--rows 1000000] [--runs 5]"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CALLS = {"duplicate_groups": lambda db, r, n, m: db.exact_range_groups(r, n, allowed=m),
         "neighbor_counts": lambda db, r, n, m: db.exact_range_density(r, 1, n, allowed=m, labels=False),
         "density_clusters": lambda db, r, n, m: db.exact_range_density(r, 5, n, allowed=m)}


def one(db, call, mode, chunk=0):
    os.environ["HNSW_MI355X_DIAG"] = f"exact_prefilter={mode},exact_chunk={chunk}"   # read by the library on every use
    db.reset_stats()
    t0, pf0 = time.perf_counter(), db.triangle_prefilter_stats()
    got = call()
    wall = (time.perf_counter() - t0) * 1e3
    st, pf1 = db.stats(), db.triangle_prefilter_stats()
    on_tile = pf1["pairs_on_tile"] - pf0["pairs_on_tile"]
    return got, {"mode": mode, "wall_ms": round(wall, 3), "kernel_ms": round(st["exact_kernel_ms"], 3), "launches_on_tile": pf1["launches"] - pf0["launches"],
                 "remeasured_over_on_tile": (pf1["pairs_remeasured"] - pf0["pairs_remeasured"]) / on_tile if on_tile else None}


def same(a, b):
    return all(u == v if u is None or isinstance(u, dict) else u.tobytes() == v.tobytes() for u, v in zip(a, b))


def ab(db, call, runs, plain_runs=None, chunk=0):
    out, ans = [], {}
    for mode in (0, 2):
        ans[mode], _ = one(db, call, mode, chunk if mode else 0)   # warm-up: a first call allocates its scratch
    for i in range(runs):
        for mode in (0, 2):
            if mode == 0 and plain_runs is not None and i >= plain_runs:
                continue
            ans[mode], r = one(db, call, mode, chunk if mode else 0)
            out.append(r)
    plain, new = [r for r in out if r["mode"] == 0], [r for r in out if r["mode"] == 2]
    return {"same_labels_counts_info": bool(same(ans[0], ans[2])), "info": ans[2][-1],
            "plain_kernel_ms": [r["kernel_ms"] for r in plain], "new_kernel_ms": [r["kernel_ms"] for r in new],
            "plain_wall_ms": [r["wall_ms"] for r in plain], "new_wall_ms": [r["wall_ms"] for r in new],
            "remeasured_over_on_tile": new[-1]["remeasured_over_on_tile"],
            "every_new_run_beats_every_plain_run": max(r["kernel_ms"] for r in new) < min(r["kernel_ms"] for r in plain)
            and max(r["wall_ms"] for r in new) < min(r["wall_ms"] for r in plain)}


def planted(n, dim, rng):
    x = rng.random((n, dim), dtype=np.float32)
    dup = rng.choice(n, n // 100, replace=False)
    src = rng.integers(0, n, dup.size)
    src = np.where(np.isin(src, dup), (src + 1) % n, src)
    x[dup] = x[src]
    x[dup[::2]] += rng.uniform(-1e-3, 1e-3, (dup[::2].size, dim)).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-o", default=str(ROOT / "profiles" / "triangle_prefilter_c2.json"))
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    import hnswindex
    n, radius = args.rows, 0.05
    res = {"build_id": hnswindex.net_amd.lib.hnsw_mi355x_build_id().decode(), "rows": n, "radius": radius, "runs": args.runs, "cases": {}}

    def case(name, db, call, **kw):
        res["cases"][name] = c = ab(db, call, **kw)
        print(name, "same" if c["same_labels_counts_info"] else "DIFFERENT", "plain", c["plain_kernel_ms"], "new", c["new_kernel_ms"],
              "wall", c["plain_wall_ms"], c["new_wall_ms"], "remeasured/on_tile", c["remeasured_over_on_tile"], flush=True)
        Path(args.o).parent.mkdir(parents=True, exist_ok=True)
        Path(args.o).write_text(json.dumps(res, indent=1) + "\n")

    def backend(metric, x):
        db = hnswindex.DeviceBackend(x.shape[1], metric, capacity=x.shape[0])
        db.upload_rows(0, x)
        db.set_profiling(True)
        return db

    x = planted(n, 128, np.random.default_rng(65539))
    for metric in ("sq_euclid", "sq_euclid_f16"):
        db = backend(metric, x)
        for m in (16384, 131072, n):
            members = np.arange(min(m, n), dtype=np.int32)
            for name, f in CALLS.items():
                big = m >= n
                case(f"{metric} {name} m={members.size}", db, lambda: f(db, radius, n, members), runs=3 if big else args.runs, plain_runs=1 if big else None)
        if metric == "sq_euclid":
            members = np.arange(min(131072, n), dtype=np.int32)
            for chunk in (1024, 2048, 8192, 16384):     # beside the default of about 4 096 rows, against the same plain kernel
                case(f"{metric} duplicate_groups m={members.size} chunk={chunk}", db, lambda: CALLS["duplicate_groups"](db, radius, n, members), runs=3, chunk=chunk)
            members = np.arange(min(16384, n), dtype=np.int32)
            for name in ("neighbor_counts", "density_clusters"):    # about 7 % of the pairs within: the per-pair atomics of the density sinks
                case(f"{metric} {name} m={members.size} radius=18", db, lambda: CALLS[name](db, 18.0, n, members), runs=3)
        del db
    m = min(65536, n)
    rng = np.random.default_rng(2024)
    for dim in (64, 256):
        db = backend("sq_euclid", planted(m, dim, rng))
        for name in ("duplicate_groups", "density_clusters"):
            case(f"sq_euclid dim={dim} {name} m={m}", db, lambda: CALLS[name](db, radius, m, None), runs=3)
        del db
    m = min(32768, n)
    db = backend("sq_euclid", (100.0 + 0.1 * rng.standard_normal((m, 128), dtype=np.float32)).astype(np.float32))
    case(f"sq_euclid duplicate_groups m={m} rows 100 + 0.1 noise", db, lambda: CALLS["duplicate_groups"](db, radius, m, None), runs=3)
    os.environ.pop("HNSW_MI355X_DIAG", None)


if __name__ == "__main__":
    main()
