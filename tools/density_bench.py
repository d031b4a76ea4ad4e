#!/usr/bin/env python3
"""density_clusters and neighbor_counts at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128) with the rows
and the plant of tools/near_dup_bench.py (1 % of the rows are near-duplicates of other rows: half exact copies, half with noise of 1e-3
per element), over the first 131 072 ids at radius 0.05, all in one session:
    density_clusters at min_samples 1 and 5             one scan, the within pairs kept in the arena
    duplicate_groups                                    the call density_clusters equals at min_samples 1
    density_clusters with density_pair_cap=1            the two-scan form, forced (min_samples 5)
    neighbor_counts                                     the counting scan alone
    the composition the call replaces                   exact_range_query_by_id in pieces of 65 536 ids with the members as the allow-set
                                                        (exact_radius_graph's loop) and the contract in numpy; labels and counts must be equal
Per line: the median wall time of --steps calls after one warm-up call.  The file is rewritten after every line.
    python tools/density_bench.py [--out profiles/density_c2.json] [--steps 5]"""
import argparse
import json
import os
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
    return out, round(1e3 * float(np.median(walls)), 3), [round(1e3 * w, 3) for w in walls]


def host_density(ix, members, n, radius, min_samples, piece=65536):
    """The composition that existed before: range lists over PCIe, then the contract in numpy -- counts, a union-find over the pairs
    between two cores, and for every other member the core neighbour of smallest (distance, id)."""
    allowed = np.zeros(n, bool)
    allowed[members] = True
    lo, hi, dist = [], [], []
    for at in range(0, members.size, piece):
        own = members[at:at + piece]
        ids, ds = ix.exact_range_query_by_id(own, radius, allowed=allowed)
        a, b, d = np.repeat(own, [l.size for l in ids]), np.concatenate(ids), np.concatenate(ds)
        keep = b > a                                             # a pair counts once, from its smaller id's list
        lo.append(a[keep]); hi.append(b[keep]); dist.append(d[keep])
    a, b, d = np.concatenate(lo), np.concatenate(hi), np.concatenate(dist)
    counts = np.full(n, -1, np.int32)
    counts[members] = 0
    counts += (np.bincount(a, minlength=n) + np.bincount(b, minlength=n)).astype(np.int32)
    core = counts + 1 >= min_samples
    core &= allowed
    both = core[a] & core[b]
    ca, cb = a[both], b[both]
    lab = np.arange(n, dtype=np.int32)                           # every id takes the smallest label around it until nothing changes
    while True:
        new = lab.copy()
        np.minimum.at(new, ca, lab[cb])
        np.minimum.at(new, cb, lab[ca])
        new = new[new]
        if (new == lab).all():
            break
        lab = new
    labels = np.full(n, -1, np.int32)
    labels[core] = lab[core]
    one = core[a] != core[b]
    c, v, dv = np.where(core[a], a, b)[one], np.where(core[a], b, a)[one], d[one]
    order = np.lexsort((c, np.where(dv == 0, np.float32(0), dv), v))
    v, c = v[order], c[order]
    first = np.r_[True, v[1:] != v[:-1]] if v.size else np.zeros(0, bool)
    labels[v[first]] = lab[c[first]]
    return labels, counts, int(a.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "density_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--subset", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, m_edges = 128, 16
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    rng = np.random.default_rng(14)
    dup = rng.choice(a.n, a.n // 100, replace=False)
    src = rng.integers(0, a.n, dup.size)
    src = np.where(np.isin(src, dup), (src + 1) % a.n, src)   # (a source that is itself replaced only makes a longer chain)
    x[dup] = x[src]
    x[dup[::2]] += rng.uniform(-1e-3, 1e-3, (dup[::2].size, dim)).astype(np.float32)
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(m_edges); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    radius = 0.05
    members = np.arange(min(a.subset, a.n), dtype=np.int32)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": m_edges, "ef_construction": 200, "min_nn": 128, "planted_duplicates": int(dup.size),
                      "members": int(members.size), "radius": radius, "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(time.perf_counter() - t0, 2)}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    def scan_kernel_ms(f):
        ix.set_profiling(True)
        ix.reset_stats()
        f()
        st = ix.stats()
        ix.set_profiling(False)
        return round(st["exact_kernel_ms"], 3), int(st["exact_launches"])

    got = {}
    for ms in (1, 5):
        call = lambda: ix.density_clusters(radius, ms, allowed=members)
        got[ms], wall, walls = median_ms(call, a.steps)
        k_ms, launches = scan_kernel_ms(call)
        res[f"density_clusters_min_samples_{ms}"] = c = {**got[ms][2], "ms": wall, "ms_repeats": walls, "scan_kernel_ms": k_ms, "scan_launches": launches}
        print("density_clusters", ms, c, flush=True)
        save()
    call = lambda: ix.duplicate_groups(radius, allowed=members)
    (groups, g_info), wall, walls = median_ms(call, a.steps)
    k_ms, launches = scan_kernel_ms(call)
    res["duplicate_groups"] = c = {**g_info, "ms": wall, "ms_repeats": walls, "scan_kernel_ms": k_ms, "scan_launches": launches,
                                   "labels_equal_min_samples_1": bool(groups.tobytes() == got[1][0].tobytes())}
    print("duplicate_groups", c, flush=True)
    save()
    os.environ["HNSW_MI355X_DIAG"] = "density_pair_cap=1"
    try:
        call = lambda: ix.density_clusters(radius, 5, allowed=members)
        two, wall2, walls = median_ms(call, a.steps)
        k_ms, launches = scan_kernel_ms(call)
    finally:
        os.environ.pop("HNSW_MI355X_DIAG")
    res["density_clusters_min_samples_5_two_scans"] = c = {**two[2], "ms": wall2, "ms_repeats": walls, "scan_kernel_ms": k_ms, "scan_launches": launches,
                                                          "labels_and_counts_equal": bool(two[0].tobytes() == got[5][0].tobytes() and two[1].tobytes() == got[5][1].tobytes())}
    print("two scans", c, flush=True)
    save()
    call = lambda: ix.neighbor_counts(radius, allowed=members)
    counts, wall, walls = median_ms(call, a.steps)
    k_ms, launches = scan_kernel_ms(call)
    res["neighbor_counts"] = c = {"ms": wall, "ms_repeats": walls, "scan_kernel_ms": k_ms, "scan_launches": launches,
                                  "counts_equal": bool(counts.tobytes() == got[5][1].tobytes())}
    print("neighbor_counts", c, flush=True)
    save()
    (want, want_counts, n_pairs), host_ms, host_walls = median_ms(lambda: host_density(ix, members, a.n, radius, 5), a.steps)
    one, group_ms = res["density_clusters_min_samples_5"]["ms"], res["duplicate_groups"]["ms"]
    res["exact_range_query_by_id_and_numpy_min_samples_5"] = c = {
        "ms": host_ms, "ms_repeats": host_walls, "labels_equal": bool(want.tobytes() == got[5][0].tobytes()),
        "counts_equal": bool(want_counts.tobytes() == got[5][1].tobytes()), "pairs_equal": bool(n_pairs == got[5][2]["pairs_within"])}
    res["ratios"] = {"composition_over_density_clusters": round(host_ms / one, 2), "density_clusters_over_duplicate_groups": round(one / group_ms, 3),
                     "two_scans_over_arena": round(wall2 / one, 3), "neighbor_counts_over_density_clusters": round(res["neighbor_counts"]["ms"] / one, 3)}
    print("composition", c, res["ratios"], flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
