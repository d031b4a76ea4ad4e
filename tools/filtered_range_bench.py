"""Filtered RangeQuery throughput: the setup of tools/range_bench.py (100k x 128 sq_euclid, its seeds, 16 384
queries per call) at radii 15 and 16, over random allow-sets of selectivity 1.0 / 0.5 / 0.1 / 0.01 and one correlated set (a
threshold on one coordinate).  Three ways to answer, each measured through the export in steady state (best of the later calls):
  unfiltered  hnsw_range_query
  postfilter  hnsw_range_query, then the disallowed ids dropped on the host (what callers did without the filtered call)
  filtered    hnsw_mi355x_range_query_filtered
plus evaluations and results per query, lists ordered on the device / on the host and hand-backs of the filtered call.
usage: python tools/filtered_range_bench.py [-o profiles/filtered_range_100k.json] [--quick]"""
import argparse
import ctypes as ct
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import hnswindex  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("-o", "--out", default=None)
ap.add_argument("--quick", action="store_true", help="one radius, two sets, one call each (a kernel trace's workload)")
a = ap.parse_args()

n, nq, dim = 100_000, 16_384, 128
x = np.random.default_rng(65537).random((n, dim), dtype=np.float32)
q = np.random.default_rng(65538).random((nq, dim), dtype=np.float32)
ix = hnswindex.Index(dim, "sq_euclid")
ix.set_collection_size(n); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(128)
ix.add(x)
lib = hnswindex.net_amd.lib
F, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_uint32)
ids_pp, dists_pp, counts = (ct.c_void_p * nq)(), (ct.c_void_p * nq)(), (ct.c_int * nq)()
rng = np.random.default_rng(7)
masks = {f"random_{s}": rng.random(n) < s for s in (1.0, 0.5, 0.1, 0.01)}
masks["correlated_0.1"] = x[:, 0] < np.float32(0.1)
reps = 1 if a.quick else 4
if a.quick:
    masks = {k: masks[k] for k in ("random_1.0", "random_0.1")}


def timed(call):
    dts = []
    for _ in range(reps):
        t = time.perf_counter()
        assert call() == 0, hnswindex.net_amd.last_error()
        dts.append(time.perf_counter() - t)
        lib.hnsw_free_results(ids_pp, dists_pp, nq)
    return min(dts[1:] if len(dts) > 1 else dts), dts


def stats_of(call):
    ix.reset_stats()
    assert call() == 0
    lib.hnsw_free_results(ids_pp, dists_pp, nq)
    st = ix.stats()
    return {"evals_per_query": round(st["search_evals"] / nq, 1), "device_ordered": st["range_device_ordered"],
            "host_ordered": st["range_host_ordered"], "handbacks": st["range_handbacks"], "kernel_ms": round(st["range_kernel_ms"], 3)}


ix.set_profiling(True)
out = {"n": n, "nq": nq, "dim": dim, "metric": "sq_euclid", "build_id": lib.hnsw_mi355x_build_id().decode(), "radii": {}}
for radius in ((16.0,) if a.quick else (15.0, 16.0)):
    unf = lambda: lib.hnsw_range_query(ix._h, q.ctypes.data_as(F), nq, dim, radius, ids_pp, dists_pp, counts)  # noqa: E731
    dt_u, dts_u = timed(unf)
    su = stats_of(unf)
    u_ids, u_d = ix.range_query(q, radius)
    r = {"unfiltered": {"queries_per_sec": round(nq / dt_u, 1), "ms_per_call": [round(1e3 * v, 2) for v in dts_u],
                        "results_per_query": round(sum(len(v) for v in u_ids) / nq, 2), **su}, "sets": {}}
    for name, mask in masks.items():
        words, nbits = hnswindex.net_amd.allow_bits(mask)
        filt = lambda: lib.hnsw_mi355x_range_query_filtered(ix._h, q.ctypes.data_as(F), nq, dim, radius, words.ctypes.data_as(U), nbits,  # noqa: E731
                                                            ids_pp, dists_pp, counts)
        dt_f, dts_f = timed(filt)
        sf = stats_of(filt)
        # postfilter: the unfiltered export, then each query's disallowed ids dropped from its callee-allocated arrays
        drops = []
        for _ in range(reps):
            t = time.perf_counter()
            assert unf() == 0
            t1 = time.perf_counter()
            kept = 0
            for i in range(nq):
                m = counts[i]
                if m:
                    qi = np.ctypeslib.as_array(ct.cast(ids_pp[i], ct.POINTER(ct.c_int)), shape=(m,))
                    qd = np.ctypeslib.as_array(ct.cast(dists_pp[i], F), shape=(m,))
                    keep = mask[qi]
                    kept += int(qi[keep].size) + 0 * qd[keep].size
            t2 = time.perf_counter()
            lib.hnsw_free_results(ids_pp, dists_pp, nq)
            drops.append((t2 - t, t2 - t1))
        best = min(drops[1:] if len(drops) > 1 else drops)
        f_ids, f_d = ix.range_query(q, radius, allowed=mask)
        entry = {"selectivity": round(float(mask.mean()), 4), "filtered_queries_per_sec": round(nq / dt_f, 1),
                 "filtered_ms_per_call": [round(1e3 * v, 2) for v in dts_f], "results_per_query": round(sum(len(v) for v in f_ids) / nq, 2),
                 **{f"filtered_{k}": v for k, v in sf.items()},
                 "postfilter_queries_per_sec": round(nq / best[0], 1), "postfilter_drop_ms": round(1e3 * best[1], 2),
                 "filtered_over_unfiltered": round(dt_u / dt_f, 3), "evals_equal_unfiltered": sf["evals_per_query"] == su["evals_per_query"]}
        if name == "random_1.0":
            entry["identical_to_unfiltered"] = all(p.tolist() == s.tolist() and c.tobytes() == e.tobytes()
                                                   for p, s, c, e in zip(f_ids, u_ids, f_d, u_d))
        r["sets"][name] = entry
        print(json.dumps({"radius": radius, name: entry}), flush=True)
    out["radii"][str(radius)] = r
if a.out:
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
print(json.dumps({"radii": {k: v["unfiltered"] for k, v in out["radii"].items()}}))
