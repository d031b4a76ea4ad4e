#!/usr/bin/env python3
"""The by-id calls at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128, k = 10: the index of
tools/tagged_knn_bench.py) beside what they replace, all in one session:
    traversal   Index.knn_query_by_id(ids, k) for 1 024 and 65 536 ids, against
                round_trip  the rows kept on the host + Index.knn_query(rows, k + 1), everything allowed: what a caller did before.
                            Cheaper, and NOT equivalent -- the first hit is dropped unseen (a duplicate under a smaller id is lost)
                loop        per id Index.knn_query(get_vectors([i]), k, allowed=<every id but i>): the equivalent, on 256 ids
    scan        Index.exact_knn_query_by_id(ids, k) for 4 096 ids against Index.exact_knn_query(host copies of the same rows, k):
                the sink's self test should cost nothing measurable; the ratio is recorded
    gather      Index.get_vectors of 65 536 random ids against Index.export_edges(0, 2 M + 2), the familiar yardstick of a copy-out
Per line: the median wall time of --steps calls after one warm-up call, and whether by-id and loop returned the same bytes.
    python tools/by_id_bench.py [--out profiles/by_id_c2.json] [--steps 5]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "by_id_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, k, m = 128, 10, 16
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(m); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(), "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": m, "ef_construction": 200,
           "min_nn": 128, "k": k, "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(time.perf_counter() - t0, 2), "traversal": {}, "scan": {}, "gather": {}}
    rng = np.random.default_rng(12)

    def save():   # after every line: a run that is cut short leaves what it measured
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    for nq in (1024, 65536):
        ids = rng.choice(a.n, nq, replace=False).astype(np.int32)
        host_rows = x[ids]
        got, ms = median_ms(lambda: ix.knn_query_by_id(ids, k), a.steps)
        trip, trip_ms = median_ms(lambda: ix.knn_query(host_rows, k + 1), a.steps)
        ix.reset_stats()
        ix.knn_query_by_id(ids, k)
        res["traversal"][f"q{nq}"] = c = {"ids": nq, "by_id_ms": ms, "round_trip_k_plus_1_ms": trip_ms, "by_id_over_round_trip": round(ms / trip_ms, 2),
                                          "round_trip_first_hit_is_self": round(float((trip[0][:, 0] == ids).mean()), 4),
                                          "same_ids_as_round_trip_minus_first": round(float((trip[0][:, 1:] == got[0]).all(axis=1).mean()), 4),
                                          "handbacks": ix.by_id_info()["handbacks"]}
        print("traversal", nq, c, flush=True)
        save()
    ids = rng.choice(a.n, 256, replace=False).astype(np.int32)

    def loop():
        out_ids, out_d = np.empty((ids.size, k), np.int32), np.empty((ids.size, k), np.float32)
        allowed = np.ones(a.n, bool)
        for i, own in enumerate(ids):
            allowed[own] = False
            out_ids[i], out_d[i] = (r[0] for r in ix.knn_query(ix.get_vectors([own]), k, allowed=allowed))
            allowed[own] = True
        return out_ids, out_d
    got, ms = median_ms(lambda: ix.knn_query_by_id(ids, k), a.steps)
    want, loop_ms = median_ms(loop, a.steps)
    res["traversal"]["loop_q256"] = c = {"ids": 256, "by_id_ms": ms, "per_id_filtered_loop_ms": loop_ms, "loop_over_by_id": round(loop_ms / ms, 2),
                                         "same_bytes_as_loop": same(got, want)}
    print("traversal loop", c, flush=True)
    save()

    ids = rng.choice(a.n, 4096, replace=False).astype(np.int32)
    host_rows = x[ids]
    got, ms = median_ms(lambda: ix.exact_knn_query_by_id(ids, k), a.steps)
    plain, plain_ms = median_ms(lambda: ix.exact_knn_query(host_rows, k + 1), a.steps)
    res["scan"]["q4096"] = c = {"ids": 4096, "by_id_ms": ms, "exact_knn_query_on_host_rows_k_plus_1_ms": plain_ms, "by_id_over_plain": round(ms / plain_ms, 3),
                                "rows_without_self_equal": bool(all(g.tolist() == [j for j in p.tolist() if j != own][:k] for g, p, own in zip(got[0], plain[0], ids)))}
    print("scan", c, flush=True)
    save()

    ids = rng.integers(0, a.n, 65536).astype(np.int32)
    rows, ms = median_ms(lambda: ix.get_vectors(ids), a.steps)
    _, edges_ms = median_ms(lambda: ix.export_edges(0, 2 * m + 2), a.steps)
    res["gather"]["q65536"] = c = {"ids": 65536, "bytes": int(rows.nbytes), "get_vectors_ms": ms, "gb_per_s": round(rows.nbytes / ms / 1e6, 2),
                                   "export_edges_layer0_ms": edges_ms, "export_edges_bytes": a.n * (2 * m + 3) * 4, "equals_host_rows": bool((rows == x[ids]).all())}
    print("gather", c, flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
