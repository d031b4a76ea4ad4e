#!/usr/bin/env python3
"""The collapsed exact k-NN call (hnswdev_exact_knn_collapsed) at C2 rows (1M x 128, 4 096 queries, k = 10,
per_group = 1) beside the plain call and beside the workaround it replaces, in one session and one build.  The rows are uploaded to
a context (the scan reads no graph, so none is built).  Two labellings of the rows:
   even    100 000 documents of 10 chunks each, scattered over the ids
   skewed  the same, but one document holds 5 % of the rows
Per labelling: the wall time (warm-up, median of five) and the HIP-event time of scan + merge (hnswdev_stats.exact_kernel_ms, from
a profiling-on pass of its own) of
   collapsed    exact_knn_collapsed(q, 10, row_group, per_group = 1)
   plain        exact_knn(q, 10): the same scan with the plain sink -- the cost the collapse is measured over
   workaround   exact_knn(q, 100) and the collapse of its rows in numpy on the host (first row of every label, the first 10 of those)
and how many of the workaround's rows come out short (fewer than 10 results) or wrong (other ids than the collapsed call's), the
collapsed call's rows being checked against the walk over the complete order (exact_range at an infinite radius) for the first 8
queries.
    python tools/exact_collapsed_bench.py [--out profiles/exact_collapsed_c2.json] [--n 1000000] [--quick]
--quick: 100 000 rows, 512 queries (a check that the tool runs)."""
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


def host_collapse(ids, d, row_group, k):
    """The workaround's second half: per row the first entry of every label, the first k of those, padded."""
    out_i = np.full((ids.shape[0], k), -1, np.int32)
    out_d = np.full((ids.shape[0], k), np.nan, np.float32)
    for r in range(ids.shape[0]):
        valid = ids[r] >= 0
        lab = row_group[ids[r][valid]]
        first = np.sort(np.unique(lab, return_index=True)[1])[:k]
        out_i[r, :first.size] = ids[r][valid][first]
        out_d[r, :first.size] = d[r][valid][first]
    return out_i, out_d


def walk(ids, d, row_group, k):
    seen, keep = set(), []
    for p, i in enumerate(ids):
        g = int(row_group[i])
        if g not in seen:
            seen.add(g)
            keep.append(p)
            if len(keep) == k:
                break
    return ids[keep], d[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_collapsed_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.n, a.nq = min(a.n, 100_000), min(a.nq, 512)
    import hnswindex
    net = hnswindex.net_amd
    dim, k, wide = 128, 10, 100
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((a.nq, dim), dtype=np.float32)
    db = hnswindex.DeviceBackend(dim, "sq_euclid", capacity=a.n)
    db.upload_rows(0, x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "k": k, "per_group": 1, "workaround_k": wide, "queries_per_call": a.nq, "timed_calls": a.steps,
                      "metric": "sq_euclid"},
           "labellings": {}}

    def profiled(call):
        db.set_profiling(True)
        db.reset_stats()
        call()
        st = db.stats()
        db.set_profiling(False)
        return st

    p_wall, p_all = walls(lambda: db.exact_knn(q, k), a.steps)
    p_st = profiled(lambda: db.exact_knn(q, k))
    res["plain"] = {"ms_per_call": round(1e3 * p_wall, 3), "calls_ms": p_all, "kernel_ms_scan_plus_merge": round(p_st["exact_kernel_ms"], 3)}
    print("plain", res["plain"], flush=True)

    docs = a.n // 10
    for name in ("even", "skewed"):
        rng = np.random.default_rng(7 if name == "even" else 8)
        rg = (np.arange(a.n) % docs).astype(np.int32)[rng.permutation(a.n)]
        if name == "skewed":
            rg[rng.permutation(a.n)[: a.n // 20]] = docs   # one document of 5 % of the rows

        def collapsed():
            return db.exact_knn_collapsed(q, k, rg, per_group=1)

        def workaround():
            return host_collapse(*db.exact_knn(q, wide), rg, k)

        c_wall, c_all = walls(collapsed, a.steps)
        w_wall, w_all = walls(workaround, a.steps)
        wk_wall, _ = walls(lambda: db.exact_knn(q, wide), a.steps)
        c_st = profiled(collapsed)
        info = db.exact_collapsed_info()
        w_st = profiled(lambda: db.exact_knn(q, wide))
        c_out, w_out = collapsed(), workaround()
        short = int(((w_out[0] >= 0).sum(axis=1) < k).sum())
        wrong = int((w_out[0] != c_out[0]).any(axis=1).sum())
        n_chk = min(8, a.nq)
        full = db.exact_range(q[:n_chk], np.inf)
        exact = all((walk(full[0][i], full[1][i], rg, k)[0] == c_out[0][i]).all() and walk(full[0][i], full[1][i], rg, k)[1].tobytes() == c_out[1][i].tobytes()
                    for i in range(n_chk))
        line = {"labels": int(np.unique(rg).size), "largest_label_rows": int(np.bincount(rg).max()),
                "collapsed": {"ms_per_call": round(1e3 * c_wall, 3), "calls_ms": c_all, "kernel_ms_scan_plus_merge": round(c_st["exact_kernel_ms"], 3),
                              "keys_dropped": info["dropped"], "entries_evicted": info["evicted"], "equals_the_walk_first_queries": bool(exact), "checked_queries": n_chk},
                "workaround": {"ms_per_call": round(1e3 * w_wall, 3), "calls_ms": w_all, "ms_exact_knn_k100_alone": round(1e3 * wk_wall, 3),
                               "kernel_ms_scan_plus_merge": round(w_st["exact_kernel_ms"], 3), "rows_short": short, "rows_wrong": wrong},
                "collapsed_over_plain_wall": round(c_wall / p_wall, 4),
                "collapsed_over_plain_kernel": round(c_st["exact_kernel_ms"] / p_st["exact_kernel_ms"], 4) if p_st["exact_kernel_ms"] else None,
                "workaround_over_collapsed_wall": round(w_wall / c_wall, 3)}
        res["labellings"][name] = line
        print(name, line, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
