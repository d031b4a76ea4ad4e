#!/usr/bin/env python3
"""range_query_tagged / exact_range_query_tagged at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200,
MinNN = 128: the index and tag generator of tools/tagged_knn_bench.py) beside the loops they replace, all in one session:
    tagged   Index.range_query_tagged(q, radius, row_tags, query_tags, "any")            (16 384 queries)
    loop     per distinct mask m: Index.range_query(q[sel_m], radius, allowed=mask_m), masks and selections built beforehand
    long0    the tagged call again with diag range_sort_long=0: closures beyond the sort kernel's table go to the host
    scan     Index.exact_range_query_tagged on 65 536 queries beside the loop of Index.exact_range_query(..., allowed=mask_m)
Cases: 32 tags drawn independently per row at a density of 25 / 6 %; 4 / 16 / 256 distinct query masks of two tags each, assigned
uniformly to the queries; two radii, for about 10 and about 340 results per query within its mask, taken from the distribution of
true distances as tools/grouped_range_bench.py takes them (the share F(r) = target / (selectivity * n) of all rows lies within r).
The traversal's closure is the whole ball, whatever the mask: a case whose ball exceeds --max-closure ids per query is not run and
is recorded as such.  Per line: the median wall time of --steps calls after a warm-up, whether both sides returned the same bytes,
results per query, the info counters (lists left to the host with and without the long-closure path).  The partition guard: 16
tags, one per row, single-tag masks, beside range_query_grouped and exact_range_query_grouped on the same labelling.
    python tools/tagged_range_bench.py [--out profiles/tagged_range_c2.json] [--steps 5] [--quick]
The file is rewritten after every line, so a run that is cut short leaves what it measured.
--quick: 100 000 rows, 2 048 / 4 096 queries (a check that the tool runs)."""
import argparse
import itertools
import json
import os
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
    return out, round(float(np.median(walls)), 3)


def same(a, b):
    return len(a[0]) == len(b[0]) and all(x.tobytes() == y.tobytes() and v.tobytes() == w.tobytes() for x, y, v, w in zip(a[0], b[0], a[1], b[1]))


def with_diag(setting, f):
    """f() with HNSW_MI355X_DIAG set to `setting` (the library reads it on every use)."""
    old = os.environ.get("HNSW_MI355X_DIAG")
    os.environ["HNSW_MI355X_DIAG"] = setting
    try:
        return f()
    finally:
        if old is None:
            del os.environ["HNSW_MI355X_DIAG"]
        else:
            os.environ["HNSW_MI355X_DIAG"] = old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tagged_range_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=16384, help="queries of the traversal lines")
    ap.add_argument("--scan-queries", type=int, default=65536, help="queries of the scan lines")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--max-closure", type=int, default=4000)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.n, a.queries, a.scan_queries = min(a.n, 100_000), min(a.queries, 2048), min(a.scan_queries, 4096)
    import hnswindex
    net = hnswindex.net_amd
    dim = 128
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q_all = np.random.default_rng(65540).random((max(a.queries, a.scan_queries), dim), dtype=np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": 16, "ef_construction": 200, "min_nn": 128, "match": "any", "traversal_queries": a.queries,
                      "scan_queries": a.scan_queries, "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call",
                      "max_closure": a.max_closure},
           "build_seconds": round(time.perf_counter() - t0, 2), "traversal": {}, "scan": {}, "not_run": {}, "partition": {}}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    rng = np.random.default_rng(11)
    sample = x[rng.choice(a.n, 20000, replace=False)]
    true_d = np.sort(np.concatenate([((sample - qq) ** 2).sum(1) for qq in q_all[:64]]).astype(np.float32))
    pairs = [(1 << i) | (1 << j) for i, j in itertools.combinations(range(32), 2)]   # 496 masks of two tags

    def lines(rt, qt_of, name, selectivity, target, partition=None):
        """One (tags, masks, radius) case: the traversal lines, then the scan lines."""
        share = target / (selectivity * a.n)
        radius = float(true_d[min(true_d.size - 1, int(share * true_d.size))])
        # -- the traversal
        nq = a.queries
        q, qt = q_all[:nq], qt_of(nq)
        distinct = [int(m) for m in np.unique(qt)]
        allow = {m: (rt & np.uint32(m)) != 0 for m in distinct}
        sels = {m: np.flatnonzero(qt == m) for m in distinct}

        def loop_of(call, qq, sel_of):
            ids, d = [None] * qq.shape[0], [None] * qq.shape[0]
            for m in distinct:
                a_ids, a_d = call(qq[sel_of[m]], radius, allowed=allow[m])
                for w, i, v in zip(sel_of[m], a_ids, a_d):
                    ids[w], d[w] = i, v
            return ids, d
        if share * a.n > a.max_closure:
            res["not_run"][name] = f"traversal: the ball holds about {int(share * a.n)} ids per query, above max_closure"
        else:
            ix.reset_stats()
            got, ms = timed(lambda: ix.range_query_tagged(q, radius, rt, qt, "any"), a.steps)
            info = ix.range_tagged_info()
            ix.reset_stats()
            off, off_ms = with_diag("range_sort_long=0", lambda: timed(lambda: ix.range_query_tagged(q, radius, rt, qt, "any"), a.steps))
            info_off = ix.range_tagged_info()
            want, loop_ms = timed(lambda: loop_of(ix.range_query, q, sels), a.steps)
            calls = a.steps + 1
            c = {"distinct_masks": len(distinct), "queries": nq, "radius": radius, "mean_selectivity": round(float(np.mean([allow[m].mean() for m in distinct])), 4),
                 "tagged_ms": ms, "loop_ms": loop_ms, "loop_over_tagged": round(loop_ms / ms, 2), "tagged_long0_ms": off_ms,
                 "same_bytes_as_loop": same(got, want), "long0_same_bytes": same(off, got), "results_per_query": round(float(np.mean([i.size for i in got[0]])), 2),
                 "ball_per_query_expected": int(share * a.n), "left_to_host_per_call": info["host_finished"] // calls,
                 "long_finished_per_call": info["long_finished"] // calls, "left_to_host_per_call_long0": info_off["host_finished"] // calls,
                 "skipped_per_call": info["skipped"] // calls}
            if partition:
                label, n_groups = partition
                qg = np.log2(qt.astype(np.float64)).astype(np.int32)
                g_out, g_ms = timed(lambda: ix.range_query_grouped(q, radius, label, qg, n_groups), a.steps)
                c.update({"grouped_ms": g_ms, "tagged_over_grouped": round(ms / g_ms, 2), "same_bytes_as_grouped": same(got, g_out)})
            (res["partition"] if partition else res["traversal"])[name] = c
            print("traversal", name, c, flush=True)
            save()
        # -- the scan
        nq = a.scan_queries
        q, qt = q_all[:nq], qt_of(nq)
        distinct = [int(m) for m in np.unique(qt)]
        allow = {m: (rt & np.uint32(m)) != 0 for m in distinct}
        sels = {m: np.flatnonzero(qt == m) for m in distinct}
        ix.reset_stats()
        got, ms = timed(lambda: ix.exact_range_query_tagged(q, radius, rt, qt, "any"), a.steps)
        info = ix.exact_range_tagged_info()
        want, loop_ms = timed(lambda: loop_of(ix.exact_range_query, q, sels), a.steps)
        calls = a.steps + 1
        c = {"distinct_masks": len(distinct), "queries": nq, "radius": radius, "tagged_ms": ms, "loop_ms": loop_ms, "loop_over_tagged": round(loop_ms / ms, 2),
             "same_bytes_as_loop": same(got, want), "results_per_query": round(float(np.mean([i.size for i in got[0]])), 2),
             "batches_per_call": info["batches"] // calls, "ids_listed_per_call": info["ids_listed"] // calls, "repeated_pieces_per_call": info["repeated_pieces"] // calls,
             "host_sorted_per_call": info["host_sorted"] // calls}
        if partition:
            label, n_groups = partition
            qg = np.log2(qt.astype(np.float64)).astype(np.int32)
            g_out, g_ms = timed(lambda: ix.exact_range_query_grouped(q, radius, label, qg, n_groups), a.steps)
            c.update({"grouped_ms": g_ms, "tagged_over_grouped": round(ms / g_ms, 2), "same_bytes_as_grouped": same(got, g_out)})
        (res["partition"] if partition else res["scan"])[name + ("_scan" if partition else "")] = c
        print("scan", name, c, flush=True)
        save()

    for density in (0.25, 0.06):
        rt = np.zeros(a.n, np.uint32)
        for bit in range(32):
            rt |= np.where(rng.random(a.n) < density, np.uint32(1 << bit), np.uint32(0)).astype(np.uint32)
        selectivity = 1.0 - (1.0 - density) ** 2   # a mask of two tags under "any"
        for n_masks in (4, 16, 256):
            masks = np.array(pairs, np.uint32)[rng.choice(len(pairs), n_masks, replace=False)]
            pick = rng.integers(0, masks.size, max(a.queries, a.scan_queries))
            for target in (10, 340):
                lines(rt, lambda nq: masks[pick[:nq]], f"density{int(100 * density)}_D{n_masks}_r{target}", selectivity, target)

    # the partition guard: 16 tags, one per row -- the labelling of the grouped calls, which are timed beside
    label = rng.integers(0, 16, a.n).astype(np.int32)
    rt = (np.uint32(1) << label.astype(np.uint32)).astype(np.uint32)
    masks = (np.uint32(1) << np.arange(16, dtype=np.uint32)).astype(np.uint32)
    pick = rng.integers(0, 16, max(a.queries, a.scan_queries))
    for target in (10, 340):
        lines(rt, lambda nq: masks[pick[:nq]], f"G16_r{target}", 1.0 / 16, target, partition=(label, 16))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
