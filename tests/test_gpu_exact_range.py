"""GPU tier: the exact range call (hnsw_mi355x_exact_range_query / hnswdev_exact_range) against its reference
(tests/exact_range_model.py: the oracle's distances, d <= radius, np.lexsort((ids, dist))): counts, ids and distance BYTES per
query, at the six metrics, on data with and without equal distances, at row shapes that take every path of the lane arithmetic,
at forced chunk lengths, query tiles, capacities, arena sizes and sort limits (byte-identical output), with allow-sets, removals,
NaN / inf rows -- and independent of the graph.

The radii come from the model's own distance matrix, never from a guess: the distance of a chosen (query, id) pair, a value
several ids hold, the float below the minimum, order statistics for a wanted mean length.  Every test asserts from the model that
its radius meets what it is about (an empty list, a tie at the boundary, lengths on both sides of a threshold)."""
import ctypes as ct

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_knn_model import candidates, distances, exact_knn
from exact_range_model import exact_range, within

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
N, DIM = 1500, 16
GRID_SEED = 2
INF = float("inf")


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _backend(metric, x):
    import hnswindex
    db = hnswindex.DeviceBackend(x.shape[1], metric, capacity=max(x.shape[0], 1))
    db.upload_rows(0, x)
    return db


def _same(got, want):
    """counts, ids and distance bytes, query by query"""
    if len(got[0]) != len(want[0]) or len(got[1]) != len(want[1]):
        return False
    for gi, gd, wi, wd in zip(got[0], got[1], want[0], want[1]):
        if gi.shape != wi.shape or not (gi == wi).all() or np.asarray(gd, np.float32).tobytes() != wd.tobytes():
            return False
    return True


def _model(dist, ids, nq, radius):
    out = [within(dist[i], ids, radius) for i in range(nq)]
    return [o[0] for o in out], [o[1] for o in out]


def _lens(want):
    return np.array([a.size for a in want[0]])


def _radius_for_mean(dist, mean_len):
    """the order statistic of the matrix that leaves about mean_len entries per row within it"""
    flat = np.sort(dist, axis=None)
    return float(flat[min(flat.size, int(dist.shape[0] * mean_len)) - 1])


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
def test_counts_ids_and_distance_bytes_are_the_models(sets, metric, grid):
    x, q, db, d = sets(metric, grid)
    ids = np.arange(N, dtype=np.int32)
    for nq in (1, 9, 67):
        dn = d[:nq]
        order0 = np.lexsort((ids, dn[0]))
        radii = {}
        # the distance of one (query, id) pair -- query 0 and its 5th candidate: that pair is on the boundary and must be in
        pair_id = int(order0[4])
        radii["pair"] = float(dn[0, pair_id])
        # the float below the smallest distance of the call: every list empty; below query 0's alone: some are, where nq > 1
        radii["below_all"] = float(np.nextafter(dn.min(), np.float32(-np.inf)))
        radii["below_q0"] = float(np.nextafter(dn[0].min(), np.float32(-np.inf)))
        for mean in (3, 50, 700):
            radii[f"mean{mean}"] = _radius_for_mean(dn, mean)
        radii.update(inf=INF, nan=float("nan"), negzero=-0.0)
        if grid:   # a value that several ids of query 0 hold: all of them are in, in id order
            vals, cnts = np.unique(dn[0], return_counts=True)
            assert (cnts >= 3).any(), metric
            radii["tied"] = float(vals[np.flatnonzero(cnts >= 3)[0]])
        for name, radius in radii.items():
            want = _model(d, ids, nq, radius)
            db.reset_stats()
            got = db.exact_range(q[:nq], radius)
            assert _same(got, want), (metric, grid, nq, name)
            st, info = db.stats(), db.exact_range_info()
            assert st["exact_evals"] == nq * N and st["exact_launches"] == 1 and st["search_launches"] == 0, (name, st)
            lens = _lens(want)
            assert info["results"] == lens.sum() and info["repeated_rounds"] == 0 and info["host_sorted"] == 0, (name, info)
            assert info["device_sorted"] == (lens >= 2).sum(), (name, info)
            # the preconditions, from the model
            if name == "pair":
                assert pair_id in want[0][0].tolist() and want[1][0][-1] == np.float32(radius)
            elif name in ("below_all", "nan"):
                assert lens.sum() == 0
            elif name == "below_q0":
                assert lens[0] == 0 and (nq < 9 or lens.sum() > 0 or not grid)
            elif name.startswith("mean"):
                assert abs(lens.mean() - int(name[4:])) <= max(2, 0.2 * int(name[4:])) or grid   # grid data: whole tie groups enter at once
                assert lens.mean() >= int(name[4:]) * 0.9
            elif name == "inf":
                assert (lens == N).all()
            elif name == "tied":
                tail = want[1][0] == np.float32(radius)
                assert tail.sum() >= 3 and (np.diff(want[0][0][tail]) > 0).all()
    if grid:   # ties across the boundary of a list: the last distance of some list is held by more than one id
        want = _model(d, ids, 67, _radius_for_mean(d, 50))
        assert any(w.size >= 2 and w[-1] == w[-2] for w in want[1]), metric


def test_a_negative_radius_is_an_ordinary_one():
    """ucosine distances of a row to itself round below zero: a negative radius admits exactly those."""
    x = _data("ucosine", N, DIM, 1)
    q = x[:67]
    d = distances("ucosine", x, q, np.arange(N, dtype=np.int32))
    neg = np.sort(d[d < 0])
    assert neg.size >= 2, "the data holds no negative distance"
    db = _backend("ucosine", x)
    for radius in (float(neg[-1]), float(neg[0]), -0.5):
        want = _model(d, np.arange(N, dtype=np.int32), 67, radius)
        assert _same(db.exact_range(q, radius), want), radius
    lens = _lens(_model(d, np.arange(N, dtype=np.int32), 67, float(neg[-1])))
    assert lens.sum() == neg.size and (lens == 0).any()


SHAPES = [(m, dim) for m in METRICS if m != "sq_euclid_i8" for dim in (5, 13, 24, 120, 264)] + [("sq_euclid_i8", dim) for dim in (5, 13, 96)]


@pytest.mark.parametrize("metric,dim", SHAPES)
def test_row_shapes(metric, dim):
    """dim 5: no 8-block; 13: a tail; 24, 120: odd block counts of the f16 record; 264: beyond 256 elements; 96: the int8 record of two lines."""
    n = 300
    x, q = _data(metric, n, dim, 11), _data(metric, 9, dim, 12)
    ids = np.arange(n, dtype=np.int32)
    d = distances(metric, x, q, ids)
    db = _backend(metric, x)
    for radius in (_radius_for_mean(d, 10), INF):
        want = _model(d, ids, 9, radius)
        assert _lens(want).sum() >= 90
        assert _same(db.exact_range(q, radius), want), (metric, dim, radius)


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8", "ucosine_f16"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3 * 64 + 7])
def test_chunks_and_tiles_give_identical_bytes(monkeypatch, metric, n):
    """radius = +inf: every measured pair is a result, so every pending list of a full step fills to its 128 entries"""
    x, q = _data(metric, n, 24, 21, grid=True), _data(metric, 9, 24, 22, grid=True)
    db = _backend(metric, x)
    want = exact_range(metric, x, q, INF)
    assert (_lens(want) == n).all()
    for chunk in (64, 1000, 0):
        for qtile in (1, 3, 0):
            set_diag(monkeypatch, exact_chunk=chunk, exact_qtile=qtile)
            db.reset_stats()
            assert _same(db.exact_range(q, INF), want), (metric, n, chunk, qtile)
            assert db.stats()["exact_evals"] == 9 * n


def test_capacities(monkeypatch, sets):
    x, q, db, d = sets("sq_euclid", False)
    ids = np.arange(N, dtype=np.int32)
    radius = _radius_for_mean(d, 50)
    want = _model(d, ids, 67, radius)
    lens = _lens(want)
    top = int(lens.max())
    assert 8 < lens.min() and (lens == top).sum() >= 1 and (lens < top).any()
    # the largest list fits exactly: one pass
    set_diag(monkeypatch, exact_range_cap=top)
    db.reset_stats()
    assert _same(db.exact_range(q, radius), want)
    assert db.exact_range_info()["repeated_rounds"] == 0 and db.stats()["exact_evals"] == 67 * N and db.stats()["exact_launches"] == 1
    # one entry short, and far short: the round is repeated with exact capacities, and its pairs count again
    for cap in (top - 1, 8):
        set_diag(monkeypatch, exact_range_cap=cap)
        db.reset_stats()
        assert _same(db.exact_range(q, radius), want), cap
        info, st = db.exact_range_info(), db.stats()
        assert info["repeated_rounds"] >= 1 and info["results"] == lens.sum(), (cap, info)
        assert st["exact_evals"] == 2 * 67 * N and st["exact_launches"] == 1 + info["repeated_rounds"], (cap, st)
    # an arena of 20 full-length segments: four rounds of pass A
    set_diag(monkeypatch, exact_range_cap=0, exact_range_arena=20 * N)
    db.reset_stats()
    assert _same(db.exact_range(q, radius), want)
    assert db.stats()["exact_launches"] == 4 and db.exact_range_info()["repeated_rounds"] == 0
    # pass B cut by the arena: 8 entries per query in pass A, then pieces of the round whose counts fit 600 entries
    assert top <= 600 < lens.sum()
    set_diag(monkeypatch, exact_range_cap=8, exact_range_arena=600)
    db.reset_stats()
    assert _same(db.exact_range(q, radius), want)
    assert db.exact_range_info()["repeated_rounds"] >= -(-int(lens.sum()) // 600)
    # an arena below one query's count: an error that names the limit, nothing returned; the next call is answered
    set_diag(monkeypatch, exact_range_cap=0, exact_range_arena=top - 1)
    with pytest.raises(RuntimeError, match=rf"arena.*\b{top - 1}\b"):
        db.exact_range(q, radius)
    counts = np.full(67, 5, np.int32)
    lib = _lib()
    qq = np.ascontiguousarray(q, np.float32)
    assert lib.hnswdev_exact_range(db._ctx, qq.ctypes.data_as(ct.POINTER(ct.c_float)), 67, N, ct.c_float(radius), None, 0,
                                   counts.ctypes.data_as(ct.POINTER(ct.c_int))) == -1
    assert (counts == 0).all()
    set_diag(monkeypatch, exact_range_arena=0)
    assert _same(db.exact_range(q, radius), want)


def _line(metric, n=200):
    """rows i * e0 and queries p * e0: the squared distance is (i - p)^2 exactly, so a radius of 32^2 gives a query at p the
    rows of [p - 32, p + 32] that exist -- list lengths by construction, equal distances on both sides of p"""
    x = np.zeros((n, 8), np.float32)
    x[:, 0] = np.arange(n)
    q = np.zeros((8, 8), np.float32)
    q[:, 0] = [-100, -32, -31, 30, 31, 32, 100, 199]
    return x, q, float(32 * 32)


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_f16"])
def test_the_sort_limit_splits_the_lists_between_device_and_host(monkeypatch, metric):
    x, q, radius = _line(metric)
    want = exact_range(metric, x, q, radius)
    lens = _lens(want)
    assert lens.tolist() == [0, 1, 2, 63, 64, 65, 65, 33]
    assert any(w.size >= 2 and (np.diff(w) == 0).any() for w in want[1])     # equal distances inside the lists
    db = _backend(metric, x)
    results = {}
    for limit in (64, 0, 1, 2):
        set_diag(monkeypatch, exact_range_sort=limit)
        db.reset_stats()
        got = db.exact_range(q, radius)
        assert _same(got, want), (metric, limit)
        cut = limit if limit else 4096
        info = db.exact_range_info()
        assert info["device_sorted"] == ((lens >= 2) & (lens <= cut)).sum() and info["host_sorted"] == (lens > cut).sum(), (limit, info)
        results[limit] = info
    assert results[64]["device_sorted"] == 4 and results[64]["host_sorted"] == 2


@pytest.mark.parametrize("n,on_device", [(4096, True), (4200, False)])
def test_the_real_sort_limit(n, on_device):
    """4096 keys are what the device orders in LDS; one more and the host does"""
    x, q = uniform(n, 8, 61), uniform(9, 8, 62)
    want = exact_range("sq_euclid", x, q, INF)
    db = _backend("sq_euclid", x)
    db.reset_stats()
    assert _same(db.exact_range(q, INF), want)
    info = db.exact_range_info()
    assert (info["device_sorted"], info["host_sorted"]) == ((9, 0) if on_device else (0, 9)), info
    assert info["repeated_rounds"] == 0 and info["results"] == 9 * n and db.stats()["exact_evals"] == 9 * n


def _masks(x, seed):
    rng = np.random.default_rng(seed)
    out = {f"sel{s}": rng.random(x.shape[0]) < s for s in (1.0, 0.5, 0.1, 0.02)}
    out["correlated"] = x[:, 0] < np.quantile(x[:, 0], 0.15)
    out["nbits1111"] = (rng.random(x.shape[0]) < 0.5)[:1111]      # nbits < N and no multiple of 32: ids >= 1111 are not allowed
    one = np.zeros(x.shape[0], bool); one[777] = True
    out["one"] = one
    few = np.zeros(x.shape[0], bool); few[[3, 64, 65, 900, 1499]] = True
    out["few"] = few
    return out


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_allow_sets(sets, metric):
    x, q, db, d = sets(metric, False)
    nq = 9
    radius = _radius_for_mean(d[:nq], 200)
    for name, mask in _masks(x, 3).items():
        ids = candidates(N, mask)
        assert ids.size > 0, name
        want = _model(d[:, ids], ids, nq, radius)
        db.reset_stats()
        got = db.exact_range(q[:nq], radius, allowed=mask)
        assert _same(got, want), (metric, name)
        st = db.stats()
        assert st["exact_evals"] == nq * ids.size and st["exact_launches"] == 1, (metric, name, st)
        if name.startswith("sel") or name == "correlated":
            assert _lens(want).sum() > 0, name
    # ids passed as an integer array; n_rows below the uploaded rows
    ids = np.array([5, 1200, 31, 32], np.int32)
    assert _same(db.exact_range(q[:nq], INF, allowed=ids), _model(d[:, np.sort(ids)], np.sort(ids), nq, INF))
    head = np.arange(1000, dtype=np.int32)
    assert _same(db.exact_range(q[:nq], radius, n_rows=1000), _model(d[:, head], head, nq, radius))
    # nothing allowed: empty lists, and no launch
    db.reset_stats()
    got = db.exact_range(q[:nq], INF, allowed=np.zeros(N, bool))
    assert len(got[0]) == nq and all(a.size == 0 for a in got[0]) and all(a.size == 0 for a in got[1])
    st = db.stats()
    assert st["exact_launches"] == 0 and st["exact_evals"] == 0 and db.exact_range_info()["results"] == 0, st
    # a bitset that reaches past the uploaded rows: clamped, never dereferenced
    wide = np.ones(N + 5000, bool)
    assert _same(db.exact_range(q[:nq], radius, allowed=wide), _model(d, np.arange(N, dtype=np.int32), nq, radius))


def test_nan_and_inf_rows():
    n = 200
    x = uniform(n, DIM, 41).copy()
    x[5, 2] = np.nan
    x[9, 3] = np.inf
    x[150, 0] = np.nan
    q = uniform(4, DIM, 42)
    db = _backend("sq_euclid", x)
    want = exact_range("sq_euclid", x, q, INF)
    assert all(w.size == n - 2 and w[-1] == 9 for w in want[0]) and all(np.isinf(w[-1]) for w in want[1])   # +inf is in, last; a NaN never
    got = db.exact_range(q, INF)
    assert _same(got, want)
    assert not np.isin([5, 150], np.concatenate(got[0])).any()
    big = float(np.finfo(np.float32).max)
    want = exact_range("sq_euclid", x, q, big)
    assert all(w.size == n - 3 for w in want[0])
    assert _same(db.exact_range(q, big), want)
    assert all(a.size == 0 for a in db.exact_range(q, float("nan"))[0])


def test_f16_rows_that_overflow_to_inf():
    n = 120
    x = uniform(n, 24, 43).copy()
    x[7, 1] = 1e6            # beyond binary16: stored as +inf
    x[30, 23] = -7e4
    q = uniform(5, 24, 44)
    for metric in ("sq_euclid_f16", "ucosine_f16"):
        want = exact_range(metric, x, q, INF)
        if metric == "sq_euclid_f16":
            assert all(w[-2:].tolist() == [7, 30] for w in want[0]) and all(np.isinf(w[-2:]).all() for w in want[1])
        assert _same(_backend(metric, x).exact_range(q, INF), want), metric


def _index(metric, x, **knobs):
    """x = None: an empty index of DIM columns (for import_graph)"""
    import hnswindex
    ix = hnswindex.Index(DIM if x is None else x.shape[1], metric)
    ix.set_collection_size(2048); ix.set_min_nn(20); ix.set_max_edges(12)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    if x is not None:
        ix.add(x)
    return ix


@pytest.fixture(scope="module")
def built(sets):
    x, q, _, d = sets("sq_euclid", False)
    return x, q, d, _index("sq_euclid", x)


def test_removals_leave_the_live_set():
    x = uniform(N, DIM, 51).copy()
    q = uniform(9, DIM, 52)
    ix = _index("sq_euclid", x)
    rng = np.random.default_rng(53)
    gone = np.unique(np.concatenate([[ix.entry_point], rng.choice(N, 99, replace=False)])).astype(np.int32)
    ix.remove(gone)
    live = np.sort(ix.ids())
    mask = rng.random(N) < 0.3
    d = distances("sq_euclid", x, q, np.arange(N, dtype=np.int32))
    radius = _radius_for_mean(d, 100)
    got = ix.exact_range_query(q, radius)
    want = exact_range("sq_euclid", x, q, radius, live=live)
    assert np.isin(gone, np.concatenate(_model(d, np.arange(N, dtype=np.int32), 9, radius)[0])).any()   # a removed id would have been in
    assert not np.isin(np.concatenate(got[0]), gone).any() and _same(got, want)
    assert _same(ix.exact_range_query(q, radius, allowed=mask), exact_range("sq_euclid", x, q, radius, mask=mask, live=live))
    ix.reset_stats()
    assert _same(ix.exact_range_query(q, INF), exact_range("sq_euclid", x, q, INF, live=live))
    assert ix.stats()["exact_evals"] == 9 * live.size and ix.exact_range_info()["results"] == 9 * live.size
    # a set that allows removed ids only: no live id, no launch
    only_gone = np.zeros(N, bool); only_gone[gone] = True
    ix.reset_stats()
    got = ix.exact_range_query(q, INF, allowed=only_gone)
    assert all(a.size == 0 for a in got[0]) and ix.stats()["exact_launches"] == 0


@pytest.mark.parametrize("metric", ["cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_index_call_at_other_metrics(sets, metric):
    x, q, _, d = sets(metric, True)
    ix = _index(metric, x)
    mask = np.random.default_rng(61).random(N) < 0.1
    ids = np.arange(N, dtype=np.int32)
    radius = _radius_for_mean(d[:9], 50)
    assert _same(ix.exact_range_query(q[:9], radius), _model(d, ids, 9, radius))
    assert _same(ix.exact_range_query(q[:9], radius, allowed=mask), _model(d[:, mask], ids[mask], 9, radius))


def test_no_graph_dependence(built):
    import hnswindex
    x, q, d, ix = built
    radius = _radius_for_mean(d, 50)
    want = _model(d, np.arange(N, dtype=np.int32), 67, radius)
    assert _same(ix.exact_range_query(q, radius), want)
    seq = _index("sq_euclid", x, set_insert_batch=1)            # a graph built one item at a time over the same rows ...
    lv = seq.levels()
    rep = _index("sq_euclid", None)                              # ... and that graph imported instead of built
    rep.import_graph(x, lv, seq.entry_point, [seq.export_edges(L, 26 if L == 0 else 14) for L in range(int(lv.max()) + 1)])
    assert rep.graph_hash() == seq.graph_hash()
    assert _same(seq.exact_range_query(q, radius), want) and _same(rep.exact_range_query(q, radius), want)
    host = _index("sq_euclid", x, set_device_traversal=False)   # no host form: the scan still runs on the device
    host.reset_stats()
    assert _same(host.exact_range_query(q, radius), want)
    assert host.stats()["exact_launches"] == 1
    h0 = ix.graph_hash()
    ix.exact_range_query(q, radius)
    assert ix.graph_hash() == h0
    empty = hnswindex.Index(DIM, "sq_euclid")                    # an index nothing was added to: empty lists
    got = empty.exact_range_query(q[:3], INF)
    assert len(got[0]) == 3 and all(a.size == 0 for a in got[0])


def test_against_the_traversal_and_the_exact_knn_call(built):
    x, q, d, ix = built
    radius = _radius_for_mean(d, 8)                              # short lists
    e_ids, e_d = ix.exact_range_query(q, radius)
    t_ids, t_d = ix.range_query(q, radius)
    assert sum(a.size for a in t_ids) > 0
    for i in range(q.shape[0]):   # whatever the traversal found is within the radius: in the exact list, with the same distance bits
        pos = {int(v): j for j, v in enumerate(e_ids[i])}
        assert all(int(v) in pos for v in t_ids[i]), i
        assert np.array([e_d[i][pos[int(v)]] for v in t_ids[i]], np.float32).tobytes() == t_d[i].tobytes()
    a_ids, a_d = ix.exact_range_query(q, INF)
    for k in (1, 10, 64):
        k_ids, k_d = ix.exact_knn_query(q, k)
        assert (np.stack([a[:k] for a in a_ids]) == k_ids).all() and np.stack([a[:k] for a in a_d]).tobytes() == k_d.tobytes()


def _lib():
    import hnswindex
    return hnswindex.net_amd.lib


def _raw_index_call(ix, q, radius, bits, nbits):
    """hnsw_mi355x_exact_range_query through ctypes, as a host that is not the Python class calls it: the arrays are left allocated"""
    q = np.ascontiguousarray(q, np.float32)
    n = q.shape[0]
    pp_i, pp_d = (ct.c_void_p * n)(*([0x1234] * n)), (ct.c_void_p * n)(*([0x1234] * n))
    counts = np.full(n, 77, np.int32)
    rc = _lib().hnsw_mi355x_exact_range_query(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), n, q.shape[1], ct.c_float(radius), bits, nbits,
                                              pp_i, pp_d, counts.ctypes.data_as(ct.POINTER(ct.c_int)))
    return rc, pp_i, pp_d, counts


def test_the_c_call_allocates_frees_and_fails_as_the_range_query_does(monkeypatch, built):
    x, q, d, ix = built
    ids = np.arange(N, dtype=np.int32)
    radius = float(np.nextafter(d[0].min(), np.float32(-np.inf)))            # query 0's list is empty, others are not
    want = _model(d, ids, 9, radius)
    lens = _lens(want)
    assert lens[0] == 0 and lens.sum() > 0
    for nbits in (N, 7, 0, -5):                                               # a NULL bitset: no filter, whatever nbits says
        rc, pp_i, pp_d, counts = _raw_index_call(ix, q[:9], radius, None, nbits)
        assert rc == 0 and counts.tolist() == lens.tolist()
        for i in range(9):
            if lens[i] == 0:
                assert pp_i[i] is None and pp_d[i] is None                    # NULL where the count is 0
            else:
                got_i = np.ctypeslib.as_array(ct.cast(pp_i[i], ct.POINTER(ct.c_int)), shape=(int(lens[i]),))
                got_d = np.ctypeslib.as_array(ct.cast(pp_d[i], ct.POINTER(ct.c_float)), shape=(int(lens[i]),))
                assert (got_i == want[0][i]).all() and got_d.tobytes() == want[1][i].tobytes()
        _lib().hnsw_free_results(pp_i, pp_d, 9)
        assert all(p is None for p in pp_i) and all(p is None for p in pp_d)  # released and cleared
    # nbits < 0 with a bitset: -1, every pointer NULL, every count 0
    words = np.full((N + 31) // 32, 0xFFFFFFFF, np.uint32)
    wp = words.ctypes.data_as(ct.POINTER(ct.c_uint32))
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q[:9], INF, wp, -5)
    assert rc == -1 and all(p is None for p in pp_i) and all(p is None for p in pp_d) and (counts == 0).all()
    # ... a device-side failure (an arena below a list) leaves the same
    set_diag(monkeypatch, exact_range_arena=100)
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q[:9], INF, None, 0)
    set_diag(monkeypatch, exact_range_arena=0)
    assert rc == -1 and all(p is None for p in pp_i) and all(p is None for p in pp_d) and (counts == 0).all()
    # with a bitset nbits counts: 7 allows ids below 7 only
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q[:9], INF, wp, 7)
    assert rc == 0 and (counts == 7).all()
    assert np.ctypeslib.as_array(ct.cast(pp_i[3], ct.POINTER(ct.c_int)), shape=(7,)).tolist() == within(d[3, :7], ids[:7], INF)[0].tolist()
    _lib().hnsw_free_results(pp_i, pp_d, 9)
    info = (ct.c_uint64 * 4)()
    assert _lib().hnsw_mi355x_exact_range_info(ix._h, info) == 0 and list(info) == [ix.exact_range_info()[k] for k in ("device_sorted", "host_sorted", "repeated_rounds", "results")]
    ix.reset_stats()
    assert sum(ix.exact_range_info().values()) == 0


def test_the_resident_query_set_and_pending_range_results_are_not_touched(sets):
    x, q, db, d = sets("sq_euclid", False)
    lib = _lib()
    ix = _index("sq_euclid", x)
    ix.set_resident_queries(q[:20])
    before = ix.knn_query_resident(10)
    other = uniform(33, DIM, 91)
    radius = _radius_for_mean(d, 20)
    assert _same(ix.exact_range_query(other, radius), exact_range("sq_euclid", x, other, radius))
    ix.exact_range_query(other[:5], radius, allowed=np.zeros(N, bool))      # the no-launch path
    assert lib.hnsw_mi355x_resident_count(ix._h) == 20
    after = ix.knn_query_resident(10)
    assert (after[0] == before[0]).all() and after[1].tobytes() == before[1].tobytes()
    # the inner boundary: the set hnswdev_set_queries uploaded still answers hnswdev_dist_query_batch(NULL) and
    # hnswdev_exact_range(NULL); the traversal's pending results are still there after an exact range call
    fresh = _backend("cosine", x)                  # cosine: the cached query norms must survive too
    dc = distances("cosine", x, q[:4], np.arange(N, dtype=np.int32))
    rc_radius = _radius_for_mean(dc, 30)
    fresh.set_queries(q[:4])
    cand = np.arange(50, dtype=np.int32)
    off = np.arange(5, dtype=np.int32) * 50
    want = fresh.dist_query_batch(None, off, np.tile(cand, 4))
    fresh.exact_range(other, rc_radius)
    assert fresh.dist_query_batch(None, off, np.tile(cand, 4)).tobytes() == want.tobytes()
    assert want.tobytes() == dc[:, :50].tobytes()
    counts = np.zeros(4, np.int32)
    assert lib.hnswdev_exact_range(fresh._ctx, None, 4, 1 << 62, ct.c_float(rc_radius), None, 0, counts.ctypes.data_as(ct.POINTER(ct.c_int))) == 0
    w = _model(dc, np.arange(N, dtype=np.int32), 4, rc_radius)
    assert counts.tolist() == _lens(w).tolist() and counts.sum() > 0
    out_i, out_d = np.empty(counts.sum(), np.int32), np.empty(counts.sum(), np.float32)
    assert lib.hnswdev_exact_range_results(fresh._ctx, out_i.ctypes.data_as(ct.POINTER(ct.c_int)), out_d.ctypes.data_as(ct.POINTER(ct.c_float))) == 0
    assert (out_i == np.concatenate(w[0])).all() and out_d.tobytes() == np.concatenate(w[1]).tobytes()
    assert lib.hnswdev_exact_range(fresh._ctx, None, 5, 1 << 62, ct.c_float(rc_radius), None, 0, counts.ctypes.data_as(ct.POINTER(ct.c_int))) == -1   # 4 resident rows
    # a traversal's results wait in the context while an exact range call comes and goes
    lv = ix.levels()
    dev = _backend("sq_euclid", x)
    dev.set_graph(lv, [ix.export_edges(L, 26 if L == 0 else 14) for L in range(int(lv.max()) + 1)], 12)
    qq = np.ascontiguousarray(q[:9], np.float32)
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    t_counts, t_flags = np.zeros(9, np.int32), np.zeros(9, np.int32)
    t_radius = _radius_for_mean(d, 8)
    assert lib.hnswdev_range_search(dev._ctx, qq.ctypes.data_as(F), 9, int(ix.entry_point), ct.c_float(t_radius), t_counts.ctypes.data_as(I),
                                    t_flags.ctypes.data_as(I)) == 0
    assert t_counts.sum() > 0
    e = dev.exact_range(other, radius)
    assert _same(e, exact_range("sq_euclid", x, other, radius))
    t_i, t_d = np.empty(t_counts.sum(), np.int32), np.empty(t_counts.sum(), np.float32)
    assert lib.hnswdev_range_results(dev._ctx, t_i.ctypes.data_as(I), t_d.ctypes.data_as(F)) == 0
    again = dev.range_search(q[:9], int(ix.entry_point), t_radius)
    assert (t_i == np.concatenate(again[0])).all() and t_d.tobytes() == np.concatenate(again[1]).tobytes()


def test_two_contexts_on_one_gpu(sets):
    x, q, _, d = sets("sq_euclid", False)
    ix = _index("sq_euclid", x, set_devices=2)
    ids = np.arange(N, dtype=np.int32)
    radius = _radius_for_mean(d, 50)
    assert _same(ix.exact_range_query(q, radius), _model(d, ids, 67, radius))
    t = ix.knn_query(q, 10)                      # the sharded traversal before and after: the scan leaves it working
    assert _same(ix.exact_range_query(q[:9], INF), _model(d, ids, 9, INF))
    t2 = ix.knn_query(q, 10)
    assert (t[0] == t2[0]).all() and t[1].tobytes() == t2[1].tobytes()
    assert ix.stats_at(0)["exact_launches"] == 2 and ix.stats_at(1)["exact_launches"] == 0   # context 0 alone
