#!/usr/bin/env python3
"""knn_query_tagged / exact_knn_query_tagged at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128,
k = 10: the index of tools/grouped_knn_bench.py) beside what they replace, all in one session:
    tagged        Index.knn_query_tagged(q, k, row_tags, query_tags, "any")
    loop          per distinct mask m: Index.knn_query(q[sel_m], k, allowed=mask_m), masks and selections built beforehand
    exact_tagged  Index.exact_knn_query_tagged on the same inputs (exact answers: its recall is 1 by construction)
Cases: 32 tags drawn independently per row at a density of 50 / 25 / 6 %; 4 / 16 / 256 distinct query masks of two tags each,
assigned uniformly to 1 024 and to 65 536 queries.  One line where the tags are a partition (16 tags, one per row, single-tag
masks) beside knn_query_grouped and exact_knn_query_grouped on the same labelling: what overlap support costs.  And the list
builder on its own (dk_tag_lists.h: D x n predicate tests) at 256 and 4 096 distinct masks over the 1M words: the HIP-event time of
its kernels (hnswdev_tag_list_ms) in a scan of one query per mask, k = 1, on a context that holds 1M rows of 4 dimensions, with
short lists ("all") and, at 256 masks, with lists of nearly every row ("any").
Per case: the median wall time of --steps calls after one warm-up, whether tagged and loop returned the same bytes, hand-backs,
and the tagged call's recall@10 against the scan.
    python tools/tagged_knn_bench.py [--out profiles/tagged_knn_c2.json] [--steps 5]"""
import argparse
import itertools
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tagged_knn_c2.json"))
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
           "min_nn": 128, "k": k, "match": "any", "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(build_s, 2), "cases": {}, "partition": {}, "list_builder": {}}
    rng = np.random.default_rng(11)

    def save():   # after every case: a run that is cut short leaves what it measured
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    pairs = [(1 << i) | (1 << j) for i, j in itertools.combinations(range(32), 2)]   # 496 masks of two tags

    def one_case(rt, masks, nq, extra=None):
        q = q_all[:nq]
        qt = masks[rng.integers(0, masks.size, nq)]
        distinct = [int(m) for m in np.unique(qt)]
        allow = {m: (rt & np.uint32(m)) != 0 for m in distinct}
        sels = {m: np.flatnonzero(qt == m) for m in distinct}

        def tagged():
            return ix.knn_query_tagged(q, k, rt, qt, "any")

        def loop():
            ids, d = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32)
            for m in distinct:
                ids[sels[m]], d[sels[m]] = ix.knn_query(q[sels[m]], k, allowed=allow[m])
            return ids, d

        def exact():
            return ix.exact_knn_query_tagged(q, k, rt, qt, "any")

        got, ms = median_ms(tagged, a.steps)
        want, loop_ms = median_ms(loop, a.steps)
        truth, exact_ms = median_ms(exact, a.steps)
        ix.reset_stats()
        tagged()
        exact()
        c = {"distinct_masks": len(distinct), "queries": nq, "mean_selectivity": round(float(np.mean([allow[m].mean() for m in distinct])), 4),
             "tagged_ms": ms, "loop_ms": loop_ms, "exact_tagged_ms": exact_ms, "loop_over_tagged": round(loop_ms / ms, 2),
             "exact_tagged_over_tagged": round(exact_ms / ms, 2), "same_bytes_as_loop": same(got, want), "handbacks": ix.knn_tagged_info()["handbacks"],
             "scan_batches": ix.exact_tagged_info()["batches"], "scan_ids_listed": ix.exact_tagged_info()["ids_listed"],
             "recall_at_10_vs_scan": round(float(np.mean([len(set(g.tolist()) & set(h.tolist())) / k for g, h in zip(truth[0], got[0])])), 4)}
        if extra:
            c.update(extra(q, qt, got, truth))
        return c

    for density in (0.5, 0.25, 0.06):
        rt = np.zeros(a.n, np.uint32)
        for bit in range(32):
            rt |= np.where(rng.random(a.n) < density, np.uint32(1 << bit), np.uint32(0)).astype(np.uint32)
        for n_masks in (4, 16, 256):
            masks = np.array(pairs, np.uint32)[rng.choice(len(pairs), n_masks, replace=False)]
            for nq in (1024, 65536):
                name = f"density{int(100 * density)}_D{n_masks}_q{nq}"
                res["cases"][name] = one_case(rt, masks, nq)
                print(name, res["cases"][name], flush=True)
                save()

    # the tags as a partition: 16 tags, one per row -- the labelling of knn_query_grouped, which is timed beside
    label = rng.integers(0, 16, a.n).astype(np.int32)
    rt = (np.uint32(1) << label.astype(np.uint32)).astype(np.uint32)
    masks = (np.uint32(1) << np.arange(16, dtype=np.uint32)).astype(np.uint32)
    for nq in (1024, 65536):
        def beside(q, qt, got, truth):
            qg = np.log2(qt.astype(np.float64)).astype(np.int32)
            g_out, g_ms = median_ms(lambda: ix.knn_query_grouped(q, k, label, qg, 16), a.steps)
            x_out, x_ms = median_ms(lambda: ix.exact_knn_query_grouped(q, k, label, qg, 16), a.steps)
            return {"grouped_ms": g_ms, "exact_grouped_ms": x_ms, "same_bytes_as_grouped": same(got, g_out), "scan_same_bytes_as_exact_grouped": same(truth, x_out)}
        res["partition"][f"G16_q{nq}"] = c = one_case(rt, masks, nq, beside)
        c["tagged_over_grouped"] = round(c["tagged_ms"] / c["grouped_ms"], 2)
        c["exact_tagged_over_exact_grouped"] = round(c["exact_tagged_ms"] / c["exact_grouped_ms"], 2)
        print("partition", nq, c, flush=True)
        save()

    # the list builder alone: one query per mask, k = 1, rows of 4 dimensions -- the scan is next to nothing, the D x n tests are all there
    db = hnswindex.DeviceBackend(4, "sq_euclid", capacity=a.n)
    db.upload_rows(0, np.zeros((a.n, 4), np.float32))
    rt = rng.integers(0, 1 << 32, a.n, dtype=np.uint64).astype(np.uint32)          # 50 % density
    # "all" keeps the lists short (a mask of about ten tags matches one row in a thousand): the tests alone; "any" fills lists of
    # nearly every row: the tests and the writes
    for n_masks, match in ((256, "all"), (256, "any"), (4096, "all")):
        qt = rng.choice(1 << 20, n_masks, replace=False).astype(np.uint32) + np.uint32(1)
        qq = np.zeros((n_masks, 4), np.float32)
        _, wall = median_ms(lambda: db.exact_knn_tagged(qq, 1, rt, qt, match), a.steps)
        db.set_profiling(True)
        db.reset_stats()
        db.exact_knn_tagged(qq, 1, rt, qt, match)
        info = db.exact_tagged_info()
        res["list_builder"][f"D{n_masks}_{match}"] = {"distinct_masks": n_masks, "match": match, "rows": a.n, "predicate_tests": n_masks * a.n,
                                                      "ids_listed": info["ids_listed"], "batches": info["batches"], "list_kernels_ms": round(db.tag_list_ms(), 3),
                                                      "scan_kernels_ms": round(db.stats()["exact_kernel_ms"], 3), "call_wall_ms": wall}
        db.set_profiling(False)
        print("list_builder", n_masks, match, res["list_builder"][f"D{n_masks}_{match}"], flush=True)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
