"""CPU tier: filtered RangeQuery (include/hnsw_mi355x.h hnsw_mi355x_range_query_filtered).  The plain-Python restatement of
SearchLayerRange with a filter (tests/filtered_range_model.py) pinned to the oracle with everything allowed, its empty-heap rule
against the closed form, the host replay over a closure (csrc/range_replay.h) against the restatement, and the new exports'
argument errors."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from common import normalize_f32, uniform
from filtered_range_model import HeapEmpty, filtered_range, filtered_range_batch, heap_empty_closed_form

ROOT = Path(__file__).resolve().parent.parent
F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)


@pytest.fixture(scope="module")
def net():
    import hnswindex
    return hnswindex.net_amd


def _data(metric, kind, n, dim, seed):
    if kind == "grid":
        x = np.random.default_rng(seed).integers(0, 3, (n, dim)).astype(np.float32)
    else:
        x = uniform(n, dim, seed)
    return normalize_f32(x) if metric == "ucosine" else x


def _radii(metric, x, q):
    """Three radii at small quantiles of the query-row distances: lists of a few to a few dozen results."""
    import oracle
    d = np.concatenate([oracle.dist_query_rows(metric, x, qq, np.arange(x.shape[0], dtype=np.int32)) for qq in q[:5]])
    return [float(np.quantile(d, p)) for p in (0.005, 0.03, 0.1)]


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8"])
@pytest.mark.parametrize("kind", ["random", "grid"])
def test_restatement_with_everything_allowed_is_range_query(metric, kind):
    import oracle
    n, dim = 400, 8
    x = _data(metric, kind, n, dim, 21)
    q = _data(metric, kind, 25, dim, 22)
    ix = oracle.OracleIndex(dim, metric, max_edges=6, max_candidates=20, collection_size=n)
    ix.add(x)
    for radius in _radii(metric, x, q):
        want_ids, want_d = ix.range_query(q, radius)
        for mask in (None, np.ones(n, dtype=bool), np.ones(n + 100, dtype=bool)):
            got_ids, got_d = filtered_range_batch(ix, x, metric, q, radius, mask)
            for a, b, c, e in zip(got_ids, want_ids, got_d, want_d):
                assert a.tolist() == b.tolist(), (metric, kind, radius)
                assert c.tobytes() == e.tobytes(), (metric, kind, radius)


def test_restatement_with_a_filter_returns_allowed_members_of_the_closure():
    import oracle
    n, dim = 400, 8
    x = _data("sq_euclid", "random", n, dim, 23)
    q = _data("sq_euclid", "random", 25, dim, 24)
    ix = oracle.OracleIndex(dim, "sq_euclid", max_edges=6, max_candidates=20, collection_size=n)
    ix.add(x)
    mask = np.random.default_rng(5).random(n) < 0.4
    radius = _radii("sq_euclid", x, q)[2]
    full, _ = ix.range_query(q, radius)
    got, _ = filtered_range_batch(ix, x, "sq_euclid", q, radius, mask)
    for a, b in zip(got, full):
        assert sorted(a.tolist()) == sorted(i for i in b.tolist() if mask[i])


def _unnormalised_ucosine(n, dim, seed):
    # ucosine assumes unit rows; on raw rows 1 - dot goes negative, so a negative range has results
    return np.random.default_rng(seed).normal(size=(n, dim)).astype(np.float32)


def test_heap_empty_closed_form_agrees_with_the_restatement():
    import oracle
    n, dim = 300, 6
    x = _unnormalised_ucosine(n, dim, 31)
    q = _unnormalised_ucosine(60, dim, 32)
    ix = oracle.OracleIndex(dim, "ucosine", max_edges=6, max_candidates=20, collection_size=n)
    ix.add(x)
    rng = np.random.default_rng(33)
    raised = kept = 0
    for radius in (-0.5, -2.0, -5.0, 0.5):
        for sel in (0.1, 0.5, 0.9):
            mask = rng.random(n) < sel
            for qq in q:
                closed = heap_empty_closed_form(ix, x, "ucosine", qq, radius, mask)
                try:
                    filtered_range(ix, x, "ucosine", qq, radius, mask)
                    model = False
                except HeapEmpty:
                    model = True
                assert closed == model, (radius, sel)
                raised += model
                kept += not model
    assert raised > 20 and kept > 20


def _adjacency(ix, n, m):
    stride = 2 * m + 2
    adj = np.zeros((n, stride), dtype=np.int32)
    for i in range(n):
        e = ix.edges(i, 0)
        adj[i, 0] = e.size
        adj[i, 1:1 + e.size] = e
    return adj, stride


def _words(mask):
    b = np.packbits(np.asarray(mask, dtype=np.uint8), bitorder="little")
    b = np.concatenate([b, np.zeros((-b.size) % 4, np.uint8)])
    return b.view(np.uint32) if b.size else np.zeros(1, np.uint32)


@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_host_replay_over_a_closure_equals_the_restatement(net, metric):
    """hnswhost_test_range_replay_filtered: the unfiltered result (the closure), shuffled, replayed with a filter -- on
    integer-grid data, where most distances tie; and for ucosine on raw rows with negative radii, the empty-heap code (-2)."""
    import oracle
    lib = net.lib
    lib.hnswhost_test_range_replay_filtered.argtypes = [I, ct.c_int, ct.c_int, ct.c_int, ct.c_float, I, F, ct.c_int, U, ct.c_longlong, I, F]
    rng = np.random.default_rng(41)
    n, dim, m = 900, 5, 8
    if metric == "ucosine":
        x = _unnormalised_ucosine(n, dim, 42)
        q = _unnormalised_ucosine(60, dim, 43)
        radii = (-0.5, -2.0, 0.3)
    else:
        x = rng.integers(0, 3, (n, dim)).astype(np.float32)
        q = rng.integers(0, 3, (60, dim)).astype(np.float32) + np.float32(0.25)
        radii = (0.9, 2.0, 3.5)
    ix = oracle.OracleIndex(dim, metric, max_edges=m, max_candidates=40, collection_size=n)
    ix.add(x)
    adj, stride = _adjacency(ix, n, m)
    masks = [rng.random(n) < s for s in (1.0, 0.5, 0.1)] + [np.zeros(n, dtype=bool), rng.random(n // 2) < 0.5]
    tied = empties = 0
    for radius in radii:
        closure_ids, closure_d = ix.range_query(q, radius)
        for mask in masks:
            words = _words(mask)
            for qi in range(q.shape[0]):
                try:
                    want_ids, want_d = filtered_range(ix, x, metric, q[qi], radius, mask)
                    want_rc = want_ids.size
                except HeapEmpty:
                    want_rc = -2
                ids, d = closure_ids[qi], closure_d[qi]
                perm = rng.permutation(ids.size)
                f_ids, f_d = np.ascontiguousarray(ids[perm]), np.ascontiguousarray(d[perm])
                out_ids = np.empty(max(ids.size, 1), np.int32)
                out_d = np.empty(max(ids.size, 1), np.float32)
                entry = ix.find_entry_point(0, q[qi])
                rc = lib.hnswhost_test_range_replay_filtered(adj.ctypes.data_as(I), stride, 2 * m, entry, radius, f_ids.ctypes.data_as(I),
                                                             f_d.ctypes.data_as(F), ids.size, words.ctypes.data_as(U), len(mask),
                                                             out_ids.ctypes.data_as(I), out_d.ctypes.data_as(F))
                assert rc == want_rc, (radius, qi)
                if rc == -2:
                    empties += 1
                    continue
                assert out_ids[:rc].tolist() == want_ids.tolist() and out_d[:rc].tobytes() == want_d.tobytes(), (radius, qi)
                tied += int(rc > 1 and (np.diff(want_d) == 0).any())
    if metric == "ucosine":
        assert empties > 5
    else:
        assert tied > 50


def test_new_symbols_are_declared_and_exported(net):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)
    for s in ("hnsw_mi355x_range_query_filtered", "hnswdev_range_search_filtered"):
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert hasattr(net.lib, s), s
    assert hasattr(net.lib, "hnswhost_test_range_replay_filtered")


def test_filtered_range_argument_errors_without_a_gpu(net):
    """Null handle: 0 for the index call (the hnsw_range_query rule), -1 for the context call; a NULL bitset or nbits < 0: -1,
    checked before the handle is used (a stand-in handle here: nothing opens a device)."""
    lib = net.lib
    v = np.zeros((2, 4), dtype=np.float32)
    pp_i, pp_d = (ct.c_void_p * 2)(), (ct.c_void_p * 2)()
    counts = (ct.c_int * 2)()
    c2, f2 = np.zeros(2, np.int32), np.zeros(2, np.int32)
    w = np.ones(1, dtype=np.uint32)
    assert lib.hnsw_mi355x_range_query_filtered(None, v.ctypes.data_as(F), 2, 4, 1.0, w.ctypes.data_as(U), 32, pp_i, pp_d, counts) == 0
    assert lib.hnswdev_range_search_filtered(None, v.ctypes.data_as(F), 2, 0, 1.0, w.ctypes.data_as(U), 32, c2.ctypes.data_as(I),
                                             f2.ctypes.data_as(I)) == -1
    stand_in = ct.create_string_buffer(64)
    h = ct.cast(stand_in, ct.c_void_p)
    assert lib.hnsw_mi355x_range_query_filtered(h, v.ctypes.data_as(F), 2, 4, 1.0, None, 32, pp_i, pp_d, counts) == -1
    assert "allow_bits" in net.last_error()
    assert lib.hnsw_mi355x_range_query_filtered(h, v.ctypes.data_as(F), 2, 4, 1.0, w.ctypes.data_as(U), -1, pp_i, pp_d, counts) == -1
