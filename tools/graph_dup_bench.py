#!/usr/bin/env python3
"""The near-duplicate calls over the graph's edges at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200,
MinNN = 128, default Add) beside the exact call, all in one session.  The rows are tools/near_dup_bench.py's: 1 % of them are planted
near-duplicates of other rows (half exact copies, half with noise of 1e-3 per element), radius 0.05.
Per member set (the first 131 072 ids; every id):
    graph_duplicate_groups and near_edges: the median wall time of --steps calls after one warm-up call, edges measured and within;
    duplicate_groups: the same (every id: ONE call, no warm-up -- it takes seconds);
    agreement, from the two label arrays: groups each way, the share of members with the same label, pair recall (the sum over the
    graph's groups of C(size, 2) over the same sum over the exact groups; the graph's groups refine the exact ones, so every pair
    the graph joins is one the exact call joins), and the planted (duplicate, source) pairs the graph's groups hold together, by kind.
Then repair_reachability() and the agreement over every id once more.  The file is rewritten after every line.
    python tools/graph_dup_bench.py [--out profiles/graph_dup_c2.json] [--steps 5]"""
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
    return out, round(1e3 * float(np.median(walls)), 3), [round(1e3 * w, 3) for w in walls]


def pairs_in_groups(labels):
    sizes = np.bincount(labels[labels >= 0]).astype(np.int64)
    return int((sizes * (sizes - 1) // 2).sum())


def agreement(graph, exact, members, dup, src, noisy):
    """The two label arrays compared over `members`; the planted pairs whose two ends are members, by kind."""
    g, e = graph[members], exact[members]
    inside = np.isin(dup, members) & np.isin(src, members)
    out = {"groups_graph": int(np.unique(g).size), "groups_exact": int(np.unique(e).size),
           "members_with_equal_label_share": round(float((g == e).mean()), 6),
           "graph_groups_refine_exact": bool((exact[g] == e).all()),
           "pairs_graph": pairs_in_groups(g), "pairs_exact": pairs_in_groups(e)}
    out["pair_recall"] = round(out["pairs_graph"] / max(out["pairs_exact"], 1), 6)
    for kind, mask in (("exact_copies", inside & ~noisy), ("noisy_copies", inside & noisy)):
        a, b = dup[mask], src[mask]
        out["planted_" + kind] = {"pairs": int(mask.sum()), "together_graph": int((graph[a] == graph[b]).sum()), "together_exact": int((exact[a] == exact[b]).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "graph_dup_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--subset", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    import hnswindex
    net = hnswindex.net_amd
    dim, m_edges, radius = 128, 16, 0.05
    x = np.random.default_rng(65539).random((a.n, dim), dtype=np.float32)
    rng = np.random.default_rng(14)
    dup = rng.choice(a.n, a.n // 100, replace=False)
    src = rng.integers(0, a.n, dup.size)
    src = np.where(np.isin(src, dup), (src + 1) % a.n, src)   # (a source that is itself replaced only makes a longer chain)
    x[dup] = x[src]
    x[dup[::2]] += rng.uniform(-1e-3, 1e-3, (dup[::2].size, dim)).astype(np.float32)
    noisy = np.zeros(dup.size, bool)
    noisy[::2] = True
    ix = hnswindex.Index(dim)
    ix.set_collection_size(a.n); ix.set_max_edges(m_edges); ix.set_max_candidates(200); ix.set_min_nn(128)
    t0 = time.perf_counter()
    ix.add(x)
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": m_edges, "ef_construction": 200, "min_nn": 128, "planted_duplicates": int(dup.size),
                      "radius": radius, "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(time.perf_counter() - t0, 2)}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    every = np.arange(a.n, dtype=np.int32)
    exact_every = None
    for name, members in ((f"first_{min(a.subset, a.n)}", every[:a.subset]), ("every_id", every)):
        allowed = None if members.size == a.n else members
        (labels, info), ms, walls = median_ms(lambda: ix.graph_duplicate_groups(radius, allowed=allowed), a.steps)
        edges, e_ms, e_walls = median_ms(lambda: ix.near_edges(radius, allowed=allowed), a.steps)
        if allowed is None:
            t = time.perf_counter()
            exact, exact_info = ix.duplicate_groups(radius)
            x_ms, x_walls = round(1e3 * (time.perf_counter() - t), 1), "one call, no warm-up"
            exact_every = exact
        else:
            (exact, exact_info), x_ms, x_walls = median_ms(lambda: ix.duplicate_groups(radius, allowed=allowed), a.steps)
        res[name] = c = {"members": int(members.size), **{k: info[k] for k in ("groups", "edges_measured", "edges_within", "launches")},
                         "graph_duplicate_groups_ms": ms, "graph_duplicate_groups_ms_repeats": walls,
                         "near_edges_ms": e_ms, "near_edges_ms_repeats": e_walls, "near_edges_returned": int(edges[0].size),
                         "duplicate_groups_ms": x_ms, "duplicate_groups_ms_repeats": x_walls, "duplicate_groups_pairs_measured": exact_info["pairs_measured"],
                         "exact_over_graph": round(x_ms / ms, 1), "agreement": agreement(labels, exact, members, dup, src, noisy)}
        print(name, c, flush=True)
        save()
    lost = int(ix.unreachable_ids(0).size)
    t = time.perf_counter()
    rep = ix.repair_reachability()
    res["after_repair_reachability"] = c = {"unreachable_before": lost, "repair_ms": round(1e3 * (time.perf_counter() - t), 1), "unreachable_after": int(ix.unreachable_ids(0).size),
                                            "layers": json.loads(json.dumps(rep, default=float))}
    labels, info = ix.graph_duplicate_groups(radius)
    c.update({k: info[k] for k in ("groups", "edges_measured", "edges_within")})
    c["agreement"] = agreement(labels, exact_every, every, dup, src, noisy)   # (the rows did not change: the exact labels are those above)
    c["agreement_moved"] = bool(c["agreement"] != res["every_id"]["agreement"])
    print("after repair", c, flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
