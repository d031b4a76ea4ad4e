"""The contract of knn_query_tagged (include/hnsw_mi355x.h hnsw_mi355x_knn_query_tagged) in plain Python, on the CPU oracle's graph: for
every distinct mask m the queries with query_tags == m are answered by the filtered KnnQuery of tests/filtered_model.py with the
allow-set of the ids whose tag word matches m, and their rows are scattered back to the queries' places.  row_tags[id] is a uint32 of
tag bits; an id past the array's end has the word 0, and the word 0 matches no mask."""
import numpy as np

from filtered_model import filtered_knn_batch

MODES = ("any", "all")


def tag_mask(row_tags, m, match, n):
    """The allow-set of mask m as a bool mask over ids 0 .. n - 1.  any: the word shares a bit with m; all: m != 0 and the word
    holds every bit of m."""
    if match not in MODES:
        raise ValueError(f"match = {match!r} is neither 'any' nor 'all'")
    w = np.zeros(n, dtype=np.uint64)
    rt = np.asarray(row_tags).astype(np.uint64).ravel()[:n]
    w[:rt.size] = rt
    m = np.uint64(int(m) & 0xFFFFFFFF)
    hit = w & m
    return hit != 0 if match == "any" else (hit == m) & (m != 0)


def check_tag_args(query_tags, match, nq):
    if match not in MODES:
        raise ValueError(f"match = {match!r} is neither 'any' nor 'all'")
    qt = np.asarray(query_tags).astype(np.uint64).ravel()
    if qt.size != nq:
        raise ValueError(f"query_tags has {qt.size} entries for {nq} queries")
    if np.unique(qt).size > 65536:
        raise ValueError("more than 65536 distinct masks")
    return qt


def tagged_knn_batch(ix, rows, metric, queries, k, min_nn, row_tags, query_tags, match="any"):
    """(ids[nq, k], dists[nq, k]).  ix: an oracle.OracleIndex holding `rows` (metric and rows as tests/filtered_model.py takes
    them); a query whose mask matches no id gets a row of padding."""
    queries = np.asarray(queries, dtype=np.float32)
    qt = check_tag_args(query_tags, match, queries.shape[0])
    ids = np.full((queries.shape[0], max(k, 0)), -1, dtype=np.int32)
    dists = np.full((queries.shape[0], max(k, 0)), np.nan, dtype=np.float32)
    if k < 1:
        return ids, dists
    for m in np.unique(qt):
        mask = tag_mask(row_tags, int(m), match, rows.shape[0])
        sel = qt == m
        if mask.any():
            ids[sel], dists[sel] = filtered_knn_batch(ix, rows, metric, queries[sel], k, min_nn, mask)
    return ids, dists
