#!/usr/bin/env python3
"""MultiLayerKnnQuery and the `layer` argument at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, k = 10; 65 536 queries per
call): queries/s, kernel ms (profiling on) and device evaluations per query of Index.multilayer_knn_query over all layers, with
  (a) the same call on the lock-step path (device traversal off, the same graph imported) on a 1 024-query subset, and
  (b) the filtered KnnQuery with everything allowed and MinNN = k -- the same two-heap traversal at layer 0 alone --
for scale; the oracle's evaluation count for the same chains on a subset (the device launch keeps visited sets, so the two are
equal); and knn_query(layer = 1) against the layer-0 call.
    python tools/multilayer_bench.py [--out profiles/multilayer_c2.json] [--steps 3] [--quick]
--quick (the rocprofv3 --kernel-trace --stats run, kept apart from any counter collection): one timed call each, no lock-step path,
no oracle."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

PEAK_GBPS = 8000.0
ROW_BYTES = 128 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multilayer_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, k = 128, 10
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    q = np.random.default_rng(65540).random((a.nq, dim), dtype=np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(16); ix.set_max_candidates(200); ix.set_min_nn(k)   # MinNN = k: (b)'s beam is the chain's
    t0 = time.perf_counter()
    ix.add(x)
    build_s = time.perf_counter() - t0
    ix.set_profiling(True)
    everything = np.ones(a.n, dtype=bool)
    levels = ix.levels()
    top = ix.top_layer()

    def measure(call):
        out = call()   # warm-up (first calls allocate their scratch)
        ix.reset_stats()
        walls = []
        for _ in range(1 if a.quick else a.steps):
            t = time.perf_counter()
            out = call()
            walls.append(time.perf_counter() - t)
        st = ix.stats()
        calls = len(walls)
        kms = st["search_kernel_ms"] / calls
        evals = st["search_timed_evals"] / calls
        return out, {"queries_per_sec": round(a.nq / float(np.median(walls)), 1), "ms_per_call": round(1e3 * float(np.median(walls)), 3),
                     "kernel_ms": round(kms, 3), "evals_per_query": round(evals / a.nq, 2),
                     "GBps": round(evals * ROW_BYTES / (kms * 1e-3) / 1e9, 1) if kms > 0 else None,
                     "frac_of_peak": round(evals * ROW_BYTES / (kms * 1e-3) / 1e9 / PEAK_GBPS, 4) if kms > 0 else None,
                     "handbacks": int(st["search_overflows"] + st["multilayer_handbacks"]) // calls,
                     "multilayer_jobs_per_call": st["multilayer_jobs"] / calls, "search_launches_per_call": st["search_launches"] / calls,
                     "distance_launches": int(st["launches"])}
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(), "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": 16,
           "ef_construction": 200, "min_nn": k, "k": k, "queries_per_call": a.nq, "timed_calls": 1 if a.quick else a.steps},
           "build_seconds": round(build_s, 2), "peak_GBps": PEAK_GBPS, "bytes_per_eval": ROW_BYTES, "top_layer": int(top),
           "nodes_per_layer": [int((levels >= l).sum()) for l in range(top + 1)]}
    ml, res["multilayer_all_layers"] = measure(lambda: ix.multilayer_knn_query(q, k))
    print("multilayer", res["multilayer_all_layers"], flush=True)
    _, res["multilayer_layer0_only"] = measure(lambda: ix.multilayer_knn_query(q, k, 0, 0))   # descent + one step: (b)'s work, through the chain kernel
    print("multilayer 0..0", res["multilayer_layer0_only"], flush=True)
    _, res["filtered_all_allowed_layer0"] = measure(lambda: ix.knn_query(q, k, allowed=everything))
    print("filtered, everything allowed", res["filtered_all_allowed_layer0"], flush=True)
    _, res["knn_layer0"] = measure(lambda: ix.knn_query(q, k))
    _, res["knn_layer1"] = measure(lambda: ix.knn_query(q, k, layer=1))
    print("knn layer 0 / 1", res["knn_layer0"], res["knn_layer1"], flush=True)
    m, b = res["multilayer_all_layers"], res["filtered_all_allowed_layer0"]
    res["ratios_vs_filtered_layer0"] = {"time_per_query": round(b["queries_per_sec"] / m["queries_per_sec"], 3),
                                        "kernel_ms": round(m["kernel_ms"] / b["kernel_ms"], 3) if b["kernel_ms"] else None,
                                        "evals_per_query": round(m["evals_per_query"] / b["evals_per_query"], 3)}
    if not a.quick:
        import oracle
        from layer_query_model import multilayer_chain, multilayer_knn_batch
        layers = [ix.export_edges(l, 33) for l in range(int(levels.max()) + 1)]
        ref = oracle.OracleIndex(dim, max_edges=16, max_candidates=200, min_nn=k, collection_size=a.n)
        ref.import_graph(x, levels, ix.entry_point, layers)
        assert ref.graph_hash() == ix.graph_hash()
        sub = 2048
        ref.reset_n_eval()
        for qi in q[:sub]:
            multilayer_chain(ref, qi, k)
        want = ref.n_eval
        ix.reset_stats()
        got = ix.multilayer_knn_query(q[:sub], k)
        dev = int(ix.stats()["search_evals"])
        assert dev == want, (dev, want)   # the launch keeps visited sets: the same rows are measured
        ref_out = multilayer_knn_batch(ref, q[:sub], k)
        res["oracle_subset"] = {"queries": sub, "oracle_evals_per_query": round(want / sub, 2), "device_evals_per_query": round(dev / sub, 2),
                                "evals_equal": dev == want,
                                "answers_equal": bool((got[0] == ref_out[0]).all() and got[1].tobytes() == ref_out[1].tobytes())}
        print("oracle", res["oracle_subset"], flush=True)
        lsub = 1024
        iy = hnswindex.Index(dim)
        iy.set_collection_size(a.n); iy.set_max_edges(16); iy.set_max_candidates(200); iy.set_min_nn(k); iy.set_device_traversal(False)
        iy.import_graph(x, levels, ix.entry_point, layers)
        assert iy.graph_hash() == ix.graph_hash()
        t = time.perf_counter()
        ids, d = iy.multilayer_knn_query(q[:lsub], k)
        wall = time.perf_counter() - t
        res["lockstep_subset"] = {"queries": lsub, "queries_per_sec": round(lsub / wall, 1),
                                  "same_as_device": bool((ids == ml[0][:lsub]).all() and d.tobytes() == ml[1][:lsub].tobytes()),
                                  "device_speedup": round(m["queries_per_sec"] / (lsub / wall), 1)}
        print("lockstep", res["lockstep_subset"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
