"""GPU tier: the exact k-NN call (hnsw_mi355x_exact_knn_query / hnswdev_exact_knn) against its reference
(tests/exact_knn_model.py: the oracle's distances, np.lexsort((ids, dist))): ids and distance BYTES, at the six metrics, on data
with and without equal distances, at row shapes that take every path of the lane arithmetic, at forced chunk lengths and query
tiles (byte-identical output), with allow-sets, removals, NaN / inf rows -- and independent of the graph.

The issue's list names "k = 1600 > N pads" beside the contract's 1 <= k <= 1024; the padding of a k above the number of
candidates is covered with k = 1024 on 300 rows and with allow-sets of fewer than k ids, k = 1025 by the error it must return."""
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_knn_model import boundary_tie, candidates, distances, exact_knn, select

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
N, DIM = 1500, 16
GRID_SEED = 2   # data seed of the grid sets: the reference meets a tie across rank k-1 / k at every metric (asserted below)


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _backend(metric, x):
    import hnswindex
    db = hnswindex.DeviceBackend(x.shape[1], metric, capacity=max(x.shape[0], 1))
    db.upload_rows(0, x)
    return db


def _same(got, want):
    return (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()


def _model(dist, ids, nq, k):
    out = [select(dist[i], ids, k) for i in range(nq)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.fixture(scope="module")
def sets():
    """(x, q, backend, the model's distance matrix) per (metric, grid): computed once, shared, never written."""
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            x = _data(metric, N, DIM, GRID_SEED if grid else 1, grid)
            q = _data(metric, 67, DIM, (GRID_SEED if grid else 1) + 100, grid)
            d = distances(metric, x, q, np.arange(N, dtype=np.int32))
            for a in (x, q, d):
                a.setflags(write=False)
            cache[(metric, grid)] = (x, q, _backend(metric, x), d)
        return cache[(metric, grid)]
    return get


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("metric", METRICS)
def test_ids_and_distance_bytes_are_the_models(sets, metric, grid):
    x, q, db, d = sets(metric, grid)
    ids = np.arange(N, dtype=np.int32)
    for nq in (1, 9, 67):
        for k in (1, 10, 64, 1024):
            db.reset_stats()
            got = db.exact_knn(q[:nq], k)
            assert _same(got, _model(d, ids, nq, k)), (metric, grid, nq, k)
            st = db.stats()
            assert st["exact_evals"] == nq * N and st["exact_launches"] == 1 and st["search_launches"] == 0, st
    if grid:   # the condition: the reference itself must meet a tie across the boundary, or the id order is never exercised
        assert any(boundary_tie(metric, x, q[:9], k) for k in (1, 10, 64)), metric


SHAPES = [(m, dim) for m in METRICS if m != "sq_euclid_i8" for dim in (5, 13, 24, 120, 264)] + [("sq_euclid_i8", dim) for dim in (5, 13, 96)]


@pytest.mark.parametrize("metric,dim", SHAPES)
def test_row_shapes(metric, dim):
    """dim 5: no 8-block; 13: a tail; 24, 120: odd block counts of the f16 record; 264: beyond 256 elements; 96: the int8 record of two lines."""
    n = 300
    x, q = _data(metric, n, dim, 11), _data(metric, 9, dim, 12)
    db = _backend(metric, x)
    for k in (10, 1024):   # 1024 > n: padded
        got = db.exact_knn(q, k)
        assert _same(got, exact_knn(metric, x, q, k)), (metric, dim, k)
        if k > n:
            assert (got[0][:, n:] == -1).all() and np.isnan(got[1][:, n:]).all()


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8", "ucosine_f16"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3 * 64 + 7])
def test_chunks_and_tiles_give_identical_bytes(monkeypatch, metric, n):
    x, q = _data(metric, n, 24, 21, grid=True), _data(metric, 9, 24, 22, grid=True)
    db = _backend(metric, x)
    want = exact_knn(metric, x, q, 10)
    for chunk in (64, 1000, 0):
        for qtile in (1, 0):
            set_diag(monkeypatch, exact_chunk=chunk, exact_qtile=qtile)
            assert _same(db.exact_knn(q, 10), want), (metric, n, chunk, qtile)
    set_diag(monkeypatch, exact_chunk=64, exact_qtile=3)   # a tile that is no multiple of the register tile, k above the rows
    assert _same(db.exact_knn(q, 300), exact_knn(metric, x, q, 300)), (metric, n)


def _masks(x, seed):
    rng = np.random.default_rng(seed)
    out = {f"sel{s}": rng.random(x.shape[0]) < s for s in (1.0, 0.5, 0.1, 0.02)}
    out["correlated"] = x[:, 0] < np.quantile(x[:, 0], 0.15)
    out["nbits1111"] = (rng.random(x.shape[0]) < 0.5)[:1111]      # nbits < N and no multiple of 32: ids >= 1111 are not allowed
    one = np.zeros(x.shape[0], bool); one[777] = True
    out["one"] = one
    few = np.zeros(x.shape[0], bool); few[[3, 64, 65, 900, 1499]] = True
    out["few"] = few                                              # fewer allowed ids than k
    return out


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_allow_sets(sets, metric):
    x, q, db, d = sets(metric, False)   # uniform data: the correlated mask is a threshold on a continuous coordinate
    nq, k = 9, 10
    for name, mask in _masks(x, 3).items():
        ids = candidates(N, mask)
        assert ids.size > 0, name
        db.reset_stats()
        got = db.exact_knn(q[:nq], k, allowed=mask)
        assert _same(got, _model(d[:, ids], ids, nq, k)), (metric, name)
        st = db.stats()
        assert st["exact_evals"] == nq * ids.size and st["exact_launches"] == 1, (metric, name, st)
        assert np.isin(got[0][got[0] >= 0], ids).all()
    # ids passed as an integer array; n_rows below the uploaded rows
    ids = np.array([5, 1200, 31, 32], np.int32)
    assert _same(db.exact_knn(q[:nq], k, allowed=ids), _model(d[:, np.sort(ids)], np.sort(ids), nq, k))
    head = np.arange(1000, dtype=np.int32)
    assert _same(db.exact_knn(q[:nq], k, n_rows=1000), _model(d[:, head], head, nq, k))
    # nothing allowed: padding, and no launch
    db.reset_stats()
    got = db.exact_knn(q[:nq], k, allowed=np.zeros(N, bool))
    assert (got[0] == -1).all() and np.isnan(got[1]).all()
    st = db.stats()
    assert st["exact_launches"] == 0 and st["exact_evals"] == 0, st
    # a bitset that reaches past the uploaded rows: clamped, never dereferenced
    wide = np.ones(N + 5000, bool)
    assert _same(db.exact_knn(q[:nq], k, allowed=wide), _model(d, np.arange(N, dtype=np.int32), nq, k))


def test_duplicates_and_self_query():
    x = uniform(N, DIM, 31).copy()
    x[700] = x[10]
    db = _backend("sq_euclid", x)
    ids, d = db.exact_knn(x[10:11], 5)
    assert ids[0, :2].tolist() == [10, 700] and d[0, :2].tolist() == [0.0, 0.0]
    assert _same((ids, d), exact_knn("sq_euclid", x, x[10:11], 5))


def test_nan_and_inf_rows_order_last():
    n = 200
    x = uniform(n, DIM, 41).copy()
    x[5, 2] = np.nan
    x[9, 3] = np.inf
    x[150, 0] = np.nan
    q = uniform(4, DIM, 42)
    db = _backend("sq_euclid", x)
    ids, d = db.exact_knn(q, n)
    w_ids, w_d = exact_knn("sq_euclid", x, q, n)
    assert (ids == w_ids).all()
    assert d[:, :n - 2].tobytes() == w_d[:, :n - 2].tobytes()       # every number, +inf included, bit for bit
    assert (ids[:, n - 3:] == [9, 5, 150]).all()                    # the inf row before the NaN rows, those by id
    assert np.isfinite(d[:, :n - 3]).all() and np.isinf(d[:, n - 3]).all() and np.isnan(d[:, n - 2:]).all()
    ids10, d10 = db.exact_knn(q, 10)                                # and they never displace a number
    assert (ids10 == w_ids[:, :10]).all() and d10.tobytes() == w_d[:, :10].tobytes()


def _index(metric, x, **knobs):
    import hnswindex
    ix = hnswindex.Index(x.shape[1], metric)
    ix.set_collection_size(2048); ix.set_min_nn(20)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    return ix


@pytest.fixture(scope="module")
def built(sets):
    x, q, _, d = sets("sq_euclid", False)
    return x, q, d, _index("sq_euclid", x)


def test_removals_and_slot_reuse():
    x = uniform(N, DIM, 51).copy()
    q = uniform(9, DIM, 52)
    ix = _index("sq_euclid", x)
    rng = np.random.default_rng(53)
    gone = np.unique(np.concatenate([[ix.entry_point], rng.choice(N, 99, replace=False)])).astype(np.int32)
    ix.remove(gone)
    live = np.sort(ix.ids())
    assert not np.isin(gone, live).any()
    mask = rng.random(N) < 0.3
    for k in (10, 64):
        got = ix.exact_knn_query(q, k)
        assert not np.isin(got[0], gone).any()
        assert _same(got, exact_knn("sq_euclid", x, q, k, live=live)), k
        assert _same(ix.exact_knn_query(q, k, allowed=mask), exact_knn("sq_euclid", x, q, k, mask=mask, live=live)), k
    fresh = uniform(50, DIM, 54)
    new_ids = ix.add(fresh)
    assert np.isin(new_ids, gone).all()          # vacated slots are reused
    x[new_ids] = fresh
    live = np.sort(ix.ids())
    ix.reset_stats()
    assert _same(ix.exact_knn_query(q, 10), exact_knn("sq_euclid", x, q, 10, live=live))
    assert ix.stats()["exact_evals"] == 9 * live.size


@pytest.mark.parametrize("metric", ["cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_index_call_at_other_metrics(sets, metric):
    x, q, _, d = sets(metric, True)
    ix = _index(metric, x)
    mask = np.random.default_rng(61).random(N) < 0.1
    ids = np.arange(N, dtype=np.int32)
    assert _same(ix.exact_knn_query(q[:9], 10), _model(d, ids, 9, 10))
    assert _same(ix.exact_knn_query(q[:9], 10, allowed=mask), _model(d[:, mask], ids[mask], 9, 10))


def test_no_graph_dependence(built, tmp_path):
    import hnswindex
    x, q, d, ix = built
    want = _model(d, np.arange(N, dtype=np.int32), 67, 10)
    assert _same(ix.exact_knn_query(q, 10), want)
    ix.serialize(tmp_path / "ix.bin")
    back = hnswindex.Index.deserialize(tmp_path / "ix.bin")
    assert _same(back.exact_knn_query(q, 10), want)
    seq = _index("sq_euclid", x, set_insert_batch=1)     # another graph over the same rows
    assert _same(seq.exact_knn_query(q, 10), want)
    host = _index("sq_euclid", x, set_device_traversal=False)   # no host form: the scan still runs on the device
    host.reset_stats()
    assert _same(host.exact_knn_query(q, 10), want)
    assert host.stats()["exact_launches"] == 1
    h0 = ix.graph_hash()
    ix.exact_knn_query(q, 10)
    assert ix.graph_hash() == h0


def test_against_the_traversal(built):
    x, q, d, ix = built
    k = 10
    e_ids, e_d = ix.exact_knn_query(q, k)
    t_ids, t_d = ix.knn_query(q, k)
    assert (e_d <= t_d).all()            # rank by rank the exact answer is no farther
    m_ids, _ = _model(d, np.arange(N, dtype=np.int32), 67, k)
    recall = lambda truth: np.mean([np.isin(t_ids[i], truth[i]).mean() for i in range(q.shape[0])])   # noqa: E731
    assert recall(e_ids) == recall(m_ids)


def test_k_above_the_limit_is_an_error(built, sets):
    x, q, d, ix = built
    with pytest.raises(RuntimeError, match="1024"):
        ix.exact_knn_query(q[:2], 1025)
    db = sets("sq_euclid", False)[2]
    with pytest.raises(RuntimeError, match="1024"):
        db.exact_knn(q[:2], 1025)
    ids, dd = ix.exact_knn_query(q[:2], 0)      # k < 1: nothing to write, success (as the filtered call)
    assert ids.shape == (2, 0)


def test_beside_the_traversal_from_two_threads(built):
    x, q, d, ix = built
    mask = np.random.default_rng(71).random(N) < 0.2
    want_e, want_t = ix.exact_knn_query(q, 10, allowed=mask), ix.knn_query(q, 10)
    got, errs = {}, []

    def worker(name, call):
        try:
            for _ in range(6):
                got[name] = call()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=("e", lambda: ix.exact_knn_query(q, 10, allowed=mask))),
          threading.Thread(target=worker, args=("t", lambda: ix.knn_query(q, 10)))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    assert _same(got["e"], want_e) and _same(got["t"], want_t)
    ids = np.flatnonzero(mask).astype(np.int32)
    assert _same(want_e, _model(d[:, ids], ids, 67, 10))


def test_two_contexts_on_one_gpu(sets):
    x, q, _, d = sets("sq_euclid", False)
    ix = _index("sq_euclid", x, set_devices=2)
    ids = np.arange(N, dtype=np.int32)
    assert _same(ix.exact_knn_query(q, 10), _model(d, ids, 67, 10))
    t = ix.knn_query(q, 10)                      # the sharded traversal before and after: the scan leaves it working
    assert _same(ix.exact_knn_query(q[:9], 64), _model(d, ids, 9, 64))
    assert _same(ix.knn_query(q, 10), t)


def _raw_index_call(ix, q, k, bits, nbits):
    """hnsw_mi355x_exact_knn_query through ctypes, as a host that is not the Python class calls it."""
    import ctypes as ct
    import hnswindex
    lib = hnswindex.net_amd.lib
    q = np.ascontiguousarray(q, np.float32)
    ids = np.empty((q.shape[0], k), np.int32)
    d = np.empty((q.shape[0], k), np.float32)
    rc = lib.hnsw_mi355x_exact_knn_query(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), q.shape[0], q.shape[1], k, bits, nbits,
                                         ids.ctypes.data_as(ct.POINTER(ct.c_int)), d.ctypes.data_as(ct.POINTER(ct.c_float)))
    return rc, (ids, d)


def _raw_context_call(db, q, k, n_rows, bits, nbits):
    import ctypes as ct
    import hnswindex
    lib = hnswindex.net_amd.lib
    q = np.ascontiguousarray(q, np.float32)
    ids = np.empty((q.shape[0], k), np.int32)
    d = np.empty((q.shape[0], k), np.float32)
    rc = lib.hnswdev_exact_knn(db._ctx, q.ctypes.data_as(ct.POINTER(ct.c_float)), q.shape[0], n_rows, k, bits, nbits,
                               ids.ctypes.data_as(ct.POINTER(ct.c_int)), d.ctypes.data_as(ct.POINTER(ct.c_float)))
    return rc, (ids, d)


def test_a_null_bitset_means_no_filter_whatever_nbits_says(sets):
    """INTEGRATION.md writes the call as (bitsOrNull, Length): NULL with nbits = Length, a small nbits or a negative one is the
    unfiltered call -- at both entry points, before and after removals (when the index layer supplies the live set itself)."""
    x, q, db, d = sets("sq_euclid", False)
    k = 10
    all_ids = np.arange(N, dtype=np.int32)
    want = _model(d, all_ids, 9, k)
    ix = _index("sq_euclid", x)
    for nbits in (N, 7, 0, -5):
        rc, got = _raw_index_call(ix, q[:9], k, None, nbits)
        assert rc == 0 and _same(got, want), nbits
        rc, got = _raw_context_call(db, q[:9], k, N, None, nbits)
        assert rc == 0 and _same(got, want), nbits
    gone = np.array([0, 31, 32, 700, 1499], np.int32)
    ix.remove(gone)
    live = np.setdiff1d(all_ids, gone).astype(np.int32)
    want = _model(d[:, live], live, 9, k)
    for nbits in (N, 7, 0, -5):
        rc, got = _raw_index_call(ix, q[:9], k, None, nbits)
        assert rc == 0 and _same(got, want), nbits
    # with a bitset nbits counts: negative is an error, 7 allows ids below 7 only
    import ctypes as ct
    words = np.full((N + 31) // 32, 0xFFFFFFFF, np.uint32)
    wp = words.ctypes.data_as(ct.POINTER(ct.c_uint32))
    assert _raw_index_call(ix, q[:9], k, wp, -5)[0] == -1 and _raw_context_call(db, q[:9], k, N, wp, -5)[0] == -1
    rc, got = _raw_context_call(db, q[:9], k, N, wp, 7)
    head = np.arange(7, dtype=np.int32)
    assert rc == 0 and _same(got, _model(d[:, head], head, 9, k))
    rc, got = _raw_index_call(ix, q[:9], k, wp, 7)
    head = np.arange(1, 7, dtype=np.int32)      # id 0 was removed
    assert rc == 0 and _same(got, _model(d[:, head], head, 9, k))


def test_the_resident_query_set_is_not_touched(sets):
    x, q, db, d = sets("sq_euclid", False)
    import hnswindex
    lib = hnswindex.net_amd.lib
    ix = _index("sq_euclid", x)
    ix.set_resident_queries(q[:20])
    before = ix.knn_query_resident(10)
    other = uniform(33, DIM, 91)
    assert _same(ix.exact_knn_query(other, 10), exact_knn("sq_euclid", x, other, 10))
    ix.exact_knn_query(other[:5], 10, allowed=np.zeros(N, bool))      # the no-launch path
    assert lib.hnsw_mi355x_resident_count(ix._h) == 20
    assert _same(ix.knn_query_resident(10), before)
    # the inner boundary: the set hnswdev_set_queries uploaded still answers hnswdev_dist_query_batch(NULL)
    fresh = _backend("cosine", x)                  # cosine: the cached query norms must survive too
    fresh.set_queries(q[:4])
    cand = np.arange(50, dtype=np.int32)
    off = np.arange(5, dtype=np.int32) * 50
    want = fresh.dist_query_batch(None, off, np.tile(cand, 4))
    fresh.exact_knn(other, 10)
    assert fresh.dist_query_batch(None, off, np.tile(cand, 4)).tobytes() == want.tobytes()
    assert want.tobytes() == distances("cosine", x, q[:4], cand).tobytes()


PIECES = [(m, 264) for m in METRICS if m != "sq_euclid_i8"] + [("sq_euclid_i8", 520)]


@pytest.mark.parametrize("metric,dim", PIECES)
def test_rows_walked_in_pieces(monkeypatch, metric, dim):
    """A forced tile of 32 queries leaves 16 KB / 32 = 128 staged words per query: rows of 264 elements (int8: the 144-word record
    of 520 elements) are walked in 3 (2) pieces, the accumulators carried across and the tail in the last one.  40 queries: a full
    tile and a ragged one."""
    n = 300
    x, q = _data(metric, n, dim, 13), _data(metric, 40, dim, 14)
    db = _backend(metric, x)
    want = exact_knn(metric, x, q, 10)
    set_diag(monkeypatch, exact_qtile=32)
    db.reset_stats()
    assert _same(db.exact_knn(q, 10), want), (metric, dim)
    assert db.stats()["exact_evals"] == 40 * n
    set_diag(monkeypatch, exact_qtile=32, exact_chunk=70)
    assert _same(db.exact_knn(q, 10), want), (metric, dim)
