"""The reference of hnsw_mi355x_exact_knn_query / hnswdev_exact_knn: every candidate measured with the oracle's
metric (oracle.dist_query_rows -- the reference's arithmetic, bit for bit) and the k smallest taken in (distance, id) order,
np.lexsort((ids, dist)): distances as IEEE numbers (-0 == +0), NaN after +inf, equal distances and NaNs by id."""
import numpy as np

PAD_ID = -1


def select(dist, ids, k):
    """(ids [k], dists [k]) of the k candidates of smallest (distance, id), padded with -1 / NaN."""
    dist, ids = np.asarray(dist, dtype=np.float32), np.asarray(ids, dtype=np.int32)
    order = np.lexsort((ids, dist))[:k]
    out_ids = np.full(k, PAD_ID, dtype=np.int32)
    out_d = np.full(k, np.nan, dtype=np.float32)
    out_ids[:order.size] = ids[order]
    out_d[:order.size] = dist[order]
    return out_ids, out_d


def select_rows(dist, ids, k):
    """select() for every row of dist [nq, len(ids)] at once: (ids [nq, k], dists [nq, k]), the same lexsort along the last axis."""
    dist, ids = np.atleast_2d(np.asarray(dist, dtype=np.float32)), np.asarray(ids, dtype=np.int32)
    order = np.lexsort((np.broadcast_to(ids, dist.shape), dist), axis=-1)[:, :k]
    out_ids = np.full((dist.shape[0], k), PAD_ID, dtype=np.int32)
    out_d = np.full((dist.shape[0], k), np.nan, dtype=np.float32)
    out_ids[:, :order.shape[1]] = ids[order]
    out_d[:, :order.shape[1]] = np.take_along_axis(dist, order, axis=1)
    return out_ids, out_d


def stored(metric, x):
    """(base metric, rows as the index stores them): X_f16 is X on the rows rounded to binary16."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if metric.endswith("_f16"):
        with np.errstate(over="ignore"):
            return metric[:-4], x.astype(np.float16).astype(np.float32)
    return metric, x


def candidates(n, mask=None, live=None):
    """Candidate ids: live (None: 0 .. n-1) and allowed by the bool mask indexed by id (ids past its end are not allowed)."""
    ids = np.arange(n, dtype=np.int32) if live is None else np.sort(np.asarray(live, dtype=np.int32))
    if mask is not None:
        mask = np.asarray(mask, dtype=bool)
        ids = ids[ids < mask.size]
        ids = ids[mask[ids]]
    return ids


def distances(metric, x, q, ids):
    """[nq, len(ids)] distances of the candidates, from the oracle."""
    import oracle
    base, rows = stored(metric, x)
    q = np.atleast_2d(np.asarray(q, dtype=np.float32))
    out = np.empty((q.shape[0], ids.size), dtype=np.float32)
    for i in range(q.shape[0]):
        if ids.size:
            out[i] = oracle.dist_query_rows(base, rows, q[i], ids)
    return out


def exact_knn(metric, x, q, k, mask=None, live=None):
    """(ids [nq, k] int32, dists [nq, k] float32): the model's answer."""
    ids = candidates(np.shape(x)[0], mask, live)
    d = distances(metric, x, q, ids)
    out = [select(d[i], ids, k) for i in range(d.shape[0])]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def plan(nq, m, k, pitch, forced_qtile=0, forced_chunk=0, num_cu=256):
    """The host-side plan of a call (exact_plan, csrc/device_backend.hip), restated: nq queries over m candidate ids, lists of k,
    `pitch` 32-bit words per resident query (dim; the int8 record's words, ((dim + 3) // 4 + 2 + 15) & ~15, for sq_euclid_i8);
    forced_qtile / forced_chunk are the exact_qtile / exact_chunk diagnostics.  Returns qtile (queries per block), piece (query
    words staged at a time: pitch, or a multiple of 16 below it), chunk (ids per chunk), n_chunks and round (queries per launch).

    The chip enters through ceil(2 * num_cu / tiles) alone, and only where that is below m // 1024.  The tests that use this
    restatement have tiles <= 3, where 2 * CU / tiles exceeds m // 1024 (at most 19 there) on any chip of more than 30 CUs: the
    values do not depend on the CU count, and num_cu is a default argument, not something the tests read from the device.  A test
    asserts its own precondition with it (n_chunks >= 2, ceil(nq / round) == 2, piece < pitch) and ties it to the product where
    the product shows it: stats()["exact_launches"] == ceil(nq / round)."""
    RQ, MAX_QTILE, ITER_ROWS, MAX_CHUNKS = 4, 32, 128, 4096   # kExactRQ, kExactMaxQTile, kExactIterRows (csrc/dk_exact.h)
    tile_rows = lambda q: (q + RQ - 1) // RQ * RQ   # noqa: E731
    qt = min(forced_qtile, MAX_QTILE) if forced_qtile > 0 else MAX_QTILE
    while qt > RQ and (tile_rows(qt) * k * 8 > 32768 or (forced_qtile <= 0 and (qt * pitch * 4 > 16384 or qt // 2 >= nq))):
        qt >>= 1
    qtr = tile_rows(qt)
    piece = pitch if qtr * pitch * 4 <= 16384 else max(16, (16384 // 4 // qtr) & ~15)
    tiles = (min(nq, 65536) + qt - 1) // qt
    if forced_chunk > 0:
        chunks = (m + forced_chunk - 1) // forced_chunk
    else:
        chunks = max(1, min((2 * num_cu + tiles - 1) // tiles, m // 1024))
    chunks = min(chunks, MAX_CHUNKS)
    chunk = (m + chunks - 1) // chunks
    if forced_chunk <= 0:
        chunk = (chunk + ITER_ROWS - 1) // ITER_ROWS * ITER_ROWS
    n_chunks = (m + chunk - 1) // chunk
    by_lists, by_out = (1 << 30) // (n_chunks * k * 8), (1 << 24) // k   # 1 GiB of lists, 2^24 output entries per round
    return {"qtile": qt, "piece": piece, "chunk": chunk, "n_chunks": n_chunks, "round": max(1, min(nq, by_lists, by_out))}


def boundary_tie(metric, x, q, k, mask=None, live=None):
    """True when, for some query, the candidates of rank k-1 and k (0-based) have equal distances: the tie the id order decides."""
    ids = candidates(np.shape(x)[0], mask, live)
    if ids.size <= k:
        return False
    d = distances(metric, x, q, ids)
    for row in d:
        s = row[np.lexsort((ids, row))]
        if s[k - 1] == s[k]:
            return True
    return False
