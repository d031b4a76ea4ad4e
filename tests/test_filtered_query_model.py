"""CPU tier: filtered KnnQuery (an allow-set over ids, include/hnsw_mi355x.h hnsw_mi355x_knn_query_filtered).  The packing
helper against hand-computed words, the two new exports, and the plain-Python restatement of the filtered SearchLayerQuery
(tests/filtered_model.py) pinned to the oracle: its heaps to oracle.heap_script, and with everything allowed its answers to
OracleIndex.knn_query bit for bit."""
import re
from pathlib import Path

import numpy as np
import pytest

from common import normalize_f32, uniform
from filtered_model import BinaryHeap, closer_first, farther_first, filtered_knn_batch

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def net():
    import hnswindex
    return hnswindex.net_amd


def test_allow_bits_packs_a_bool_mask(net):
    mask = np.zeros(70, dtype=bool)
    mask[[0, 5, 31, 32, 63, 69]] = True
    words, nbits = net.allow_bits(mask)
    assert nbits == 70
    assert words.dtype == np.uint32 and words.tolist() == [(1 << 0) | (1 << 5) | (1 << 31), (1 << 0) | (1 << 31), 1 << 5]


def test_allow_bits_packs_an_id_list(net):
    words, nbits = net.allow_bits(np.array([3, 33, 3, 64], dtype=np.int64))
    assert nbits == 65                                  # ids past the largest listed one are not allowed
    assert words.tolist() == [1 << 3, 1 << 1, 1 << 0]
    words, nbits = net.allow_bits([0])
    assert (words.tolist(), nbits) == ([1], 1)


def test_allow_bits_of_an_empty_set(net):
    for empty in (np.zeros(0, dtype=bool), np.zeros(0, dtype=np.int32), []):
        words, nbits = net.allow_bits(empty)
        assert words.size == 0 and nbits == 0
    words, nbits = net.allow_bits(np.zeros(40, dtype=bool))
    assert words.tolist() == [0, 0] and nbits == 40


def test_allow_bits_rejects_negative_ids_and_floats(net):
    with pytest.raises(ValueError):
        net.allow_bits([1, -2])
    with pytest.raises(TypeError):
        net.allow_bits(np.array([0.5]))


def test_new_symbols_are_declared_and_exported(net):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)
    for s in ("hnsw_mi355x_knn_query_filtered", "hnswdev_knn_search_filtered"):
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert hasattr(net.lib, s), s


def test_filtered_query_argument_errors_without_a_gpu(net):
    """Null handle: 0 for the index call (the hnsw_knn_query rule), -1 for the context call (the hnswdev_* rule)."""
    import ctypes as ct
    lib = net.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), dtype=np.float32)
    ids = np.zeros((2, 3), dtype=np.int32)
    d = np.zeros((2, 3), dtype=np.float32)
    w = np.ones(1, dtype=np.uint32)
    assert lib.hnsw_mi355x_knn_query_filtered(None, v.ctypes.data_as(F), 2, 4, 3, w.ctypes.data_as(U), 32, ids.ctypes.data_as(I), d.ctypes.data_as(F)) == 0
    assert lib.hnswdev_knn_search_filtered(None, v.ctypes.data_as(F), 2, 0, 3, 3, w.ctypes.data_as(U), 32, ids.ctypes.data_as(I),
                                           d.ctypes.data_as(F), ids.ctypes.data_as(I)) == -1


def test_restated_heaps_equal_the_oracle_heap_script():
    """Tie-heavy scripts: few distinct distances, pushes and pops interleaved -- heap ARRAYS and pop order equal."""
    import oracle
    rng = np.random.default_rng(7)
    for trial in range(40):
        n = int(rng.integers(5, 120))
        ops = np.where(rng.random(n) < 0.3, -1, np.arange(n)).astype(np.int32)
        dists = rng.integers(0, 4, n).astype(np.float32)
        for closer in (False, True):
            want_ids, want_d, want_pop = oracle.heap_script(closer, ops, dists)
            h = BinaryHeap(closer_first if closer else farther_first)
            popped = []
            for o, dd in zip(ops.tolist(), dists.tolist()):
                if o >= 0:
                    h.push((o, dd))
                elif len(h):
                    popped.append(h.pop()[0])
            assert [e[0] for e in h.buf] == want_ids.tolist(), (trial, closer)
            assert [e[1] for e in h.buf] == want_d.tolist()
            assert popped == want_pop.tolist()


def _data(metric, kind, n, dim, seed):
    if kind == "grid":   # integer grid: many equal distances (heap layout decides ids)
        x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32)
    else:
        x = uniform(n, dim, seed)
    return normalize_f32(x) if metric == "ucosine" else x


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8"])
@pytest.mark.parametrize("kind", ["random", "grid"])
def test_restatement_with_everything_allowed_is_knn_query(metric, kind):
    import oracle
    n, dim, min_nn = 400, 8, 12
    x = _data(metric, kind, n, dim, 11)
    q = _data(metric, kind, 30, dim, 12)
    ix = oracle.OracleIndex(dim, metric, max_edges=6, min_nn=min_nn, max_candidates=20, collection_size=n)
    ix.add(x)
    for k in (5, 20):
        want_ids, want_d = ix.knn_query(q, k)
        for mask in (None, np.ones(n, dtype=bool), np.ones(n + 100, dtype=bool)):
            got_ids, got_d = filtered_knn_batch(ix, x, metric, q, k, min_nn, mask)
            assert (got_ids == want_ids).all(), (metric, kind, k)
            assert got_d.tobytes() == want_d.tobytes(), (metric, kind, k)


def test_restatement_with_a_filter_keeps_out_what_is_not_allowed():
    """Every result is allowed, and with fewer allowed ids than the beam the search covers all of layer 0 it reaches -- on this
    connected graph, brute force over the allowed rows.  Nothing allowed: padding."""
    import oracle
    n, dim = 300, 8
    x = uniform(n, dim, 3)
    q = uniform(10, dim, 4)
    ix = oracle.OracleIndex(dim, max_edges=6, min_nn=10, max_candidates=20, collection_size=n)
    ix.add(x)
    mask = np.zeros(n, dtype=bool)
    mask[np.random.default_rng(5).choice(n, 6, replace=False)] = True
    ids, d = filtered_knn_batch(ix, x, "sq_euclid", q, 4, 10, mask)
    allowed = np.flatnonzero(mask)
    for i in range(q.shape[0]):
        bd = oracle.dist_query_rows("sq_euclid", x, q[i], allowed)
        order = np.argsort(bd, kind="stable")[:4]
        assert ids[i].tolist() == allowed[order].tolist()
        assert d[i].tobytes() == bd[order].astype(np.float32).tobytes()
    none_ids, none_d = filtered_knn_batch(ix, x, "sq_euclid", q[:2], 4, 10, np.zeros(n, dtype=bool))
    assert (none_ids == -1).all() and np.isnan(none_d).all()
