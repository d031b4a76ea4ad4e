#!/usr/bin/env python3
"""The near-duplicate calls at C2 (1M x 128 sq_euclid, M = 16, efConstruction = 200, MinNN = 128) beside what they
replace, all in one session.  1 % of the rows are planted near-duplicates of other rows (half exact copies, half with noise of
1e-3 per element).
    (a) range   Index.exact_range_query_by_id for 4 096 ids at radii giving about 12 and about 380 results per id (order statistics
                of the oracle's distances of 64 of the rows to every other row), against Index.exact_range_query on host copies of the
                same rows plus the host-side drop of the own id; the lists must be equal
    (b) groups  Index.duplicate_groups(radius 0.05) over the first 131 072 ids against the composition that existed before: pieces
                of 4 096 ids through get_vectors + exact_range_query(allowed=the members) + a union-find on the host, identical
                labels required; then, with --full, one call over all 1M ids (no comparator: it would take minutes).
                The share of the scan's (tile, chunk) blocks that leave early is worked out here from the member list with the
                launch's tile (32 queries), chunk (device_backend.hip: about 2 048 rows) and round (65 536 members).
Per line: the median wall time of --steps calls after one warm-up call.  The file is rewritten after every line.
    python tools/near_dup_bench.py [--out profiles/near_dup_c2.json] [--steps 5] [--full]"""
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


def early_exit_share(members, qtile=32, chunk_rows=2048, round_q=65536, iter_rows=128, max_chunks=4096):
    """Blocks of duplicate_groups' launches whose chunk ends at or below their tile's first query id / all blocks."""
    m = members.size
    chunks = max(1, min(m // chunk_rows, max_chunks))
    chunk = -(-(-(-m // chunks)) // iter_rows) * iter_rows                          # ceil(ceil(m / chunks) / 128) * 128
    last = members[np.minimum(np.arange(chunk, m + chunk, chunk), m) - 1]          # the last id of every chunk
    left = total = 0
    for off in range(0, m, round_q):
        first = members[off:off + round_q:qtile]                                   # the first query id of every tile of the round
        left += int(np.searchsorted(last, first, side="right").sum())              # chunks whose last id is <= it
        total += first.size * last.size
    return left / total, chunk, int(last.size)


def host_groups(ix, members, n, radius, piece=4096):
    """The composition that existed before: rows back, range lists over PCIe, a union-find here."""
    allowed = np.zeros(n, bool)
    allowed[members] = True
    lo_ids, hi_ids = [], []
    for lo in range(0, members.size, piece):
        own = members[lo:lo + piece]
        ids, _ = ix.exact_range_query(ix.get_vectors(own), radius, allowed=allowed)
        a, b = np.repeat(own, [l.size for l in ids]), np.concatenate(ids)
        lo_ids.append(a[b > a])
        hi_ids.append(b[b > a])
    a, b = np.concatenate(lo_ids), np.concatenate(hi_ids)
    # the union-find in numpy: every id takes the smallest label of its neighbours and of its label's label until nothing changes
    lab = np.arange(n, dtype=np.int32)
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        new = new[new]
        if (new == lab).all():
            break
        lab = new
    out = np.full(n, -1, np.int32)
    out[members] = lab[members]
    return out, int(a.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "near_dup_c2.json"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--subset", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    import hnswindex
    import oracle
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
    res = {"build_id": net.lib.hnsw_mi355x_build_id().decode(),
           "config": {"n": a.n, "dim": dim, "metric": "sq_euclid", "M": m_edges, "ef_construction": 200, "min_nn": 128, "planted_duplicates": int(dup.size),
                      "timed_calls": a.steps, "statistic": "median wall ms per call after one warm-up call"},
           "build_seconds": round(time.perf_counter() - t0, 2), "range": {}, "groups": {}}

    def save():
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")

    # (a) the range scan by id
    ids = rng.choice(a.n, 4096, replace=False).astype(np.int32)
    host_rows = x[ids]
    every = np.arange(a.n, dtype=np.int32)
    pooled = np.sort(np.concatenate([np.delete(oracle.dist_query_rows("sq_euclid", x, x[i], every), i) for i in ids[:64]]))
    for target in (12, 380):
        radius = float(pooled[64 * target - 1])

        def plain():
            got = ix.exact_range_query(host_rows, radius)
            keep = [l != own for l, own in zip(got[0], ids)]
            return [l[k] for l, k in zip(got[0], keep)], [d[k] for d, k in zip(got[1], keep)]
        got, ms, walls = median_ms(lambda: ix.exact_range_query_by_id(ids, radius), a.steps)
        want, plain_ms, plain_walls = median_ms(plain, a.steps)
        res["range"][f"about_{target}"] = c = {
            "ids": 4096, "radius": radius, "results_per_id": round(sum(l.size for l in got[0]) / 4096, 2), "by_id_ms": ms, "by_id_ms_repeats": walls,
            "exact_range_query_on_host_rows_minus_self_ms": plain_ms, "plain_ms_repeats": plain_walls, "by_id_over_plain": round(ms / plain_ms, 3),
            "lists_equal": bool(all(g.tolist() == w.tolist() and u.tobytes() == v.tobytes() for g, w, u, v in zip(got[0], want[0], got[1], want[1])))}
        print("range", target, c, flush=True)
        save()

    # (b) the groups
    radius = 0.05
    members = np.arange(min(a.subset, a.n), dtype=np.int32)
    (labels, info), ms, walls = median_ms(lambda: ix.duplicate_groups(radius, allowed=members), a.steps)
    ix.set_profiling(True)
    ix.reset_stats()
    ix.duplicate_groups(radius, allowed=members)
    st = ix.stats()
    ix.set_profiling(False)
    (want, n_pairs), host_ms, host_walls = median_ms(lambda: host_groups(ix, members, a.n, radius), a.steps)
    share, chunk, n_chunks = early_exit_share(members)
    res["groups"][f"first_{members.size}"] = c = {
        "members": int(members.size), "radius": radius, **info, "duplicate_groups_ms": ms, "duplicate_groups_ms_repeats": walls,
        "scan_kernel_ms": round(st["exact_kernel_ms"], 3), "scan_launches": int(st["exact_launches"]),
        "get_vectors_exact_range_query_union_find_ms": host_ms, "host_ms_repeats": host_walls, "host_over_device": round(host_ms / ms, 2),
        "labels_identical": bool(labels.tobytes() == want.tobytes()), "pairs_identical": bool(n_pairs == info["pairs_within"]),
        "chunk_rows": chunk, "chunks": n_chunks, "blocks_leaving_early_share": round(share, 4)}
    print("groups", c, flush=True)
    save()
    # the same call with the chunk forced (the exact_chunk diagnostic): what the default of about 2 048 rows stands beside
    c["forced_chunk_ms"] = {}
    for rows in (512, 1024, 4096, 8192, 32768):
        os.environ["HNSW_MI355X_DIAG"] = f"exact_chunk={rows}"
        try:
            (forced, _), f_ms, _ = median_ms(lambda: ix.duplicate_groups(radius, allowed=members), a.steps)
        finally:
            os.environ.pop("HNSW_MI355X_DIAG")
        c["forced_chunk_ms"][str(rows)] = f_ms if forced.tobytes() == labels.tobytes() else None
    print("groups, chunk forced", c["forced_chunk_ms"], flush=True)
    save()
    if a.full:
        t = time.perf_counter()
        labels, info = ix.duplicate_groups(radius)
        wall = time.perf_counter() - t
        share, chunk, n_chunks = early_exit_share(np.arange(a.n, dtype=np.int32))
        in_group = int((np.bincount(labels[labels >= 0], minlength=a.n) > 1).sum())
        res["groups"]["every_id"] = c = {"members": a.n, "radius": radius, **info, "duplicate_groups_ms_one_call": round(1e3 * wall, 1), "groups_of_two_or_more": in_group,
                                         "chunk_rows": chunk, "chunks": n_chunks, "blocks_leaving_early_share": round(share, 4)}
        print("groups, every id", c, flush=True)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
