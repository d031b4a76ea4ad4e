"""The contracts of the by-id calls (include/hnsw_mi355x.h, hnsw_mi355x_exact_knn_query_by_id / hnsw_mi355x_knn_query_by_id) in numpy.

The flat scan: query i is the stored row of ids[i]; its candidates are the live ids (those of `allowed`, when one is given) except
ids[i] itself; the answer is the k candidates of smallest (distance, id), padded with -1 / NaN where they run out.  A duplicate of
the row under another id is a candidate like any other.  Distances come from the caller (dist_to(id) -> the float32 distances of the
stored row of `id` to every candidate, in the candidates' order), so the model says nothing about arithmetic.

The traversal: the per-id loop over the existing filtered call, which is the contract itself."""
import numpy as np


def top_k_by_distance_and_id(d, cand, k):
    """(ids[k], dists[k]): the k entries of smallest (distance, id), NaN distances last, padded with -1 / NaN."""
    d, cand = np.asarray(d, np.float32), np.asarray(cand, np.int32)
    key = np.where(d == 0, np.float32(0), d)                 # -0 and +0 are equal: the id decides
    order = np.lexsort((cand, key))                          # (NaN sorts last)
    ids = np.full(max(k, 0), -1, np.int32)
    out = np.full(max(k, 0), np.nan, np.float32)
    m = min(max(k, 0), order.size)
    ids[:m], out[:m] = cand[order[:m]], d[order[:m]]
    return ids, out


def candidates(live_ids, allowed=None):
    """The candidate ids of a call, ascending: the live ids, of which `allowed` (a bool mask over ids, or an id list) keeps some."""
    live = np.sort(np.asarray(live_ids, np.int32))
    if allowed is None:
        return live
    a = np.asarray(allowed)
    if a.dtype == bool:
        return live[(live < a.size) & a[np.minimum(live, a.size - 1)]] if a.size else live[:0]
    return live[np.isin(live, a)]


def exact_knn_by_id(dist_to, live_ids, ids, k, allowed=None):
    """(ids[n, k], dists[n, k]) of the contract.  dist_to(id, cand) -> float32[len(cand)]."""
    cand = candidates(live_ids, allowed)
    out_ids = np.full((len(ids), max(k, 0)), -1, np.int32)
    out_d = np.full((len(ids), max(k, 0)), np.nan, np.float32)
    for i, own in enumerate(np.asarray(ids, np.int32)):
        c = cand[cand != own]
        out_ids[i], out_d[i] = top_k_by_distance_and_id(dist_to(int(own), c), c, k)
    return out_ids, out_d


def drop_first_of_k_plus_1(dist_to, live_ids, ids, k):
    """The shortcut the calls do NOT take: ask for k + 1 with the query's own id among the candidates, drop the first hit."""
    cand = candidates(live_ids)
    out_ids = np.full((len(ids), k), -1, np.int32)
    out_d = np.full((len(ids), k), np.nan, np.float32)
    for i, own in enumerate(np.asarray(ids, np.int32)):
        a, b = top_k_by_distance_and_id(dist_to(int(own), cand), cand, k + 1)
        out_ids[i], out_d[i] = a[1:], b[1:]
    return out_ids, out_d


def all_but(n, own):
    """The allow-set "every id below n except `own`" as a bool mask."""
    m = np.ones(n, bool)
    m[own] = False
    return m


def knn_by_id_loop(ix, ids, k, layer=0, n=None):
    """knn_query_by_id's contract on an Index, by the calls it replaces: one get_vectors and one filtered knn_query per id."""
    n = ix.length if n is None else n
    out_ids = np.full((len(ids), k), -1, np.int32)
    out_d = np.full((len(ids), k), np.nan, np.float32)
    for i, own in enumerate(np.asarray(ids, np.int32)):
        out_ids[i], out_d[i] = (a[0] for a in ix.knn_query(ix.get_vectors([own]), k, allowed=all_but(n, int(own)), layer=layer))
    return out_ids, out_d


def exact_by_id_loop(ix, ids, k, allowed=None, n=None):
    """exact_knn_query_by_id's contract on an Index, by the calls it replaces."""
    n = ix.length if n is None else n
    live = np.zeros(n, bool)
    live[ix.ids()] = True
    base = live if allowed is None else live & np.isin(np.arange(n), candidates(np.arange(n), allowed))
    out_ids = np.full((len(ids), k), -1, np.int32)
    out_d = np.full((len(ids), k), np.nan, np.float32)
    for i, own in enumerate(np.asarray(ids, np.int32)):
        m = base.copy()
        m[own] = False
        out_ids[i], out_d[i] = (a[0] for a in ix.exact_knn_query(ix.get_vectors([own]), k, allowed=m))
    return out_ids, out_d
