"""GPU tier: exact_knn_query_by_id and exact_knn_graph -- the flat scan whose queries are stored rows and whose sink
drops the pair (query, its own row).  Byte for byte the per-id loop of existing calls it replaces --
exact_knn_query(get_vectors([id]), k, allowed=<allowed, or every live id, minus id>) -- for every row kind, and on float32 rows the
numpy statement of the contract (tests/by_id_model.py) over the oracle's distances.  3 000 rows x dim 20, 48 query ids; the
exact_chunk / exact_qtile diagnostics cut the rows into five chunks and the queries into six tiles, and the query ids sit in the first
chunk, in the last one and on both sides of a chunk's edge."""
import gc

import numpy as np
import pytest

from by_id_model import all_but, exact_by_id_loop, exact_knn_by_id
from common import normalize_f32, set_diag, uniform

pytestmark = pytest.mark.gpu

N, DIM, NQ = 3000, 20, 48
CHUNK, QTILE = 700, 8                          # chunks [0, 700) .. [2800, 3000): five; 48 queries: six tiles
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
A, DUP_LO, DUP_HI = 1500, 100, 2900            # the row of id A is stored under ids DUP_LO < A < DUP_HI as well
MUST = [0, 1, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, A, DUP_LO, DUP_HI, 7, 7, 2800, N - 1]


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _rows(metric):
    x = _data(metric, N, DIM, 1).copy()
    x[DUP_LO] = x[A]
    x[DUP_HI] = x[A]
    return x


def _index(dim, metric, n):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(8); ix.set_insert_batch(0)
    return ix


def _query_ids():
    rest = [i for i in np.random.default_rng(5).permutation(N).tolist() if i not in MUST][:NQ - len(MUST)]
    return np.array(MUST + rest, np.int32)


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _oracle_dist(metric, rows):
    """dist_to of tests/by_id_model.py from the oracle: the distances of the stored row `own` to the candidates (float32 rows)."""
    import oracle
    return lambda own, cand: oracle.dist_query_rows(metric, rows, rows[own], cand) if cand.size else np.zeros(0, np.float32)


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x = _rows(metric)
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        self.qids = _query_ids()
        self._want = {}

    def want(self, k):
        if k not in self._want:
            w = exact_by_id_loop(self.ix, self.qids, k)
            w[0].setflags(write=False); w[1].setflags(write=False)
            self._want[k] = w
        return self._want[k]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


def test_the_query_ids_sit_where_the_chunks_begin_and_end():
    q = _query_ids()
    assert q.size == NQ > QTILE and -(-N // CHUNK) == 5
    chunk_of = q // CHUNK
    assert {0, 4} <= set(chunk_of.tolist()) and {CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, 2800, N - 1} <= set(q.tolist())
    assert (q == 7).sum() == 2 and {A, DUP_LO, DUP_HI} <= set(q.tolist())


@pytest.mark.parametrize("metric", METRICS)
def test_exact_by_id_is_the_per_id_loop(cases, monkeypatch, metric):
    c = cases(metric)
    for knobs in ({}, dict(exact_chunk=CHUNK, exact_qtile=QTILE)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for k in (1, 10, 100):
            c.ix.reset_stats()
            got = c.ix.exact_knn_query_by_id(c.qids, k)
            st, info = c.ix.stats(), c.ix.by_id_info()
            assert _same(got, c.want(k)), (metric, knobs, k)
            assert not (got[0] == c.qids[:, None]).any() and (got[0] >= 0).all()
            # every pair but the 48 (query, own row) pairs was turned into a key
            assert st["exact_evals"] == NQ * N - NQ and st["exact_launches"] == 1 and st["search_launches"] == 0, (metric, knobs, k, st)
            assert info == {"calls": 1, "traversed": 0, "handbacks": 0, "scanned": NQ, "rows_gathered": NQ, "self_skipped": NQ}, info
    ids, d = c.ix.exact_knn_query_by_id(c.qids, 10)
    at = {int(q): i for i, q in enumerate(c.qids)}
    for own, others in ((A, [DUP_LO, DUP_HI]), (DUP_LO, [A, DUP_HI]), (DUP_HI, [DUP_LO, A])):
        row = at[own]                                                                    # the duplicates first, by id, at one distance
        assert ids[row, :2].tolist() == others and d[row, 0].tobytes() == d[row, 1].tobytes() and d[row, 1] <= d[row, 2], (metric, own)
    rep = np.flatnonzero(c.qids == 7)
    assert (ids[rep[0]] == ids[rep[1]]).all() and d[rep[0]].tobytes() == d[rep[1]].tobytes()


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine"])
def test_exact_by_id_is_the_numpy_model_on_float32_rows(cases, monkeypatch, metric):
    c = cases(metric)
    want = exact_knn_by_id(_oracle_dist(metric, c.x), np.arange(N), c.qids, 100)
    assert _same(c.ix.exact_knn_query_by_id(c.qids, 100), want), metric
    set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE)
    assert _same(c.ix.exact_knn_query_by_id(c.qids, 100), want), metric
    assert _same(c.ix.exact_knn_query_by_id(c.qids, 10), (want[0][:, :10], want[1][:, :10])), metric


def test_allowed_sets(cases, monkeypatch):
    c = cases("sq_euclid_i8")
    set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE)
    allowed = np.zeros(N, bool)
    allowed[np.random.default_rng(8).choice(N, 900, replace=False)] = True
    allowed[[0, A, DUP_LO, N - 1]] = True                                                 # some query ids are in the set ...
    allowed[[1, CHUNK, DUP_HI]] = False                                                   # ... and some are not: they answer normally
    inside = int(allowed[c.qids].sum())
    assert 4 <= inside < NQ
    c.ix.reset_stats()
    got = c.ix.exact_knn_query_by_id(c.qids, 20, allowed=allowed)
    # the pairs of every query with every allowed id, but for the queries whose own id is allowed
    assert c.ix.stats()["exact_evals"] == NQ * int(allowed.sum()) - inside and c.ix.by_id_info()["self_skipped"] == inside
    assert _same(got, exact_by_id_loop(c.ix, c.qids, 20, allowed))
    as_ids = c.ix.exact_knn_query_by_id(c.qids, 20, allowed=np.flatnonzero(allowed))      # the set as an id list
    assert _same(as_ids, got)
    # a set that holds only the id itself: padding; beside a query whose id is not in it
    ids, d = c.ix.exact_knn_query_by_id([A, 5, A], 3, allowed=[A])
    assert (ids[[0, 2]] == -1).all() and np.isnan(d[[0, 2]]).all() and ids[1].tolist() == [A, -1, -1]
    ids, d = c.ix.exact_knn_query_by_id([A], 3, allowed=np.zeros(N, bool))                # a set that allows nothing: no launch
    assert (ids == -1).all() and np.isnan(d).all()


def test_k_1024_on_1100_rows():
    n = 1100
    x = _data("cosine", n, DIM, 21)
    ix = _index(DIM, "cosine", n)
    ix.add(x)
    qids = np.array([0, n - 1, 550, 7, 7] + list(range(40, 51)), np.int32)
    got = ix.exact_knn_query_by_id(qids, 1024)
    assert _same(got, exact_by_id_loop(ix, qids, 1024)) and (got[0] >= 0).all()
    assert _same(got, exact_knn_by_id(_oracle_dist("cosine", x), np.arange(n), qids, 1024))
    with pytest.raises(RuntimeError, match="k = 1025 is above the limit of 1024"):
        ix.exact_knn_query_by_id(qids, 1025)


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_f16"])
def test_padding_where_k_reaches_the_other_items(metric):
    n = 50
    x = _data(metric, n, DIM, 23)
    ix = _index(DIM, metric, n)
    ix.add(x)
    qids = np.arange(n, dtype=np.int32)
    for k in (n - 2, n - 1, n, 64):
        ids, d = ix.exact_knn_query_by_id(qids, k)
        valid = min(k, n - 1)                                                             # n live items: at most n - 1 results
        assert (ids[:, :valid] >= 0).all() and not np.isnan(d[:, :valid]).any() and (ids[:, valid:] == -1).all() and np.isnan(d[:, valid:]).all()
        assert _same((ids, d), exact_by_id_loop(ix, qids, k)), k
        if k >= n - 1:
            assert all(sorted(ids[i, :n - 1].tolist()) == [j for j in range(n) if j != i] for i in range(n))


def test_more_queries_than_a_round(monkeypatch):
    """exact_chunk = 1 on 4 097 rows: 2 049 chunks x 128 keys x 8 B of lists per query, so 1 GiB holds 511 queries and 600 ids take two
    rounds -- the second reads its own ids at self + 511.  Grid rows: most rows have a duplicate, many under a smaller id."""
    import hnswindex
    n, nq, k, dim = 4097, 600, 128, 8
    x = _data("sq_euclid", n, dim, 2, grid=True)
    qids = np.random.default_rng(3).choice(n, nq, replace=False).astype(np.int32)
    qids[[0, 510, 511, 512, nq - 1]] = [0, 4096, 4095, 1, 2048]
    assert sum(bool((x[:q] == x[q]).all(axis=1).any()) for q in qids[:100]) > 5           # duplicates under smaller ids
    want = exact_knn_by_id(_oracle_dist("sq_euclid", x), np.arange(n), qids, k)
    set_diag(monkeypatch, exact_chunk=1)
    db = hnswindex.DeviceBackend(dim, "sq_euclid", capacity=n)     # (the call allocates the full list workspace: dropped below)
    try:
        db.upload_rows(0, x)
        got = db.exact_knn_by_id(qids, k)
        st, info = db.stats(), db.by_id_info()
        assert st["exact_launches"] == 2 and st["exact_evals"] == nq * n - nq and info["self_skipped"] == nq and info["scanned"] == nq, (st, info)
        assert _same((got[0][:511], got[1][:511]), (want[0][:511], want[1][:511]))
        assert _same((got[0][511:], got[1][511:]), (want[0][511:], want[1][511:]))
    finally:
        del db
        gc.collect()


def test_exact_knn_graph_on_700_rows():
    n, k = 700, 12
    x = _data("sq_euclid", n, DIM, 31).copy()
    x[650] = x[30]
    x[40] = x[660]
    ix = _index(DIM, "sq_euclid", n)
    ix.add(x)
    ids, d = ix.exact_knn_graph(k)
    assert ids.shape == d.shape == (n, k) and ids.dtype == np.int32 and d.dtype == np.float32
    assert _same((ids, d), exact_knn_by_id(_oracle_dist("sq_euclid", x), np.arange(n), np.arange(n), k))
    assert not (ids == np.arange(n)[:, None]).any()                                       # row i lacks i
    assert ids[30, 0] == 650 and ids[650, 0] == 30 and ids[40, 0] == 660 and ids[660, 0] == 40 and d[30, 0] == d[650, 0] == 0.0
    some = np.array([699, 30, 30, 0], np.int32)
    assert _same(ix.exact_knn_graph(k, some), (ids[some], d[some]))
    # after removals the default is every live id, ascending, and no row holds a removed id
    ix.remove([5, 650])
    live = np.delete(np.arange(n), [5, 650])
    g_ids, g_d = ix.exact_knn_graph(k)
    assert _same((g_ids, g_d), exact_knn_by_id(_oracle_dist("sq_euclid", x), live, live, k))
    assert not np.isin(g_ids, [5, 650]).any() and g_ids[29, 0] != 650                     # (live[29] == 30: its duplicate is gone)
    with pytest.raises(RuntimeError, match=r"hnsw_mi355x_exact_knn_query_by_id: ids\[1\] = 650 is not a live id"):
        ix.exact_knn_graph(k, [3, 650])


def test_device_backend_exact_knn_by_id():
    """The inner boundary: rows a host uploaded itself; row by row hnswdev_exact_knn for the gathered row with the id taken out."""
    import hnswindex
    n = 900
    x = _data("ucosine_f16", n, 33, 41)
    dev = hnswindex.DeviceBackend(33, "ucosine_f16", capacity=n)
    dev.upload_rows(0, x)
    qids = np.array([0, 899, 450, 450, 17], np.int32)
    dev.reset_stats()
    ids, d = dev.exact_knn_by_id(qids, 15)
    assert dev.stats()["exact_evals"] == 5 * n - 5
    for i, own in enumerate(qids):
        want = dev.exact_knn(dev.gather_rows([own]), 15, allowed=all_but(n, int(own)))
        assert _same((ids[i:i + 1], d[i:i + 1]), want), own
    half = dev.exact_knn_by_id(qids, 15, n_rows=400)                                      # rows [0, 400): ids 899 and 450 are outside, and answer
    for i, own in enumerate(qids):
        m = all_but(n, int(own))
        m[400:] = False
        assert _same((half[0][i:i + 1], half[1][i:i + 1]), dev.exact_knn(dev.gather_rows([own]), 15, allowed=m)), own
    launches = dev.stats()["exact_launches"]
    with pytest.raises(RuntimeError, match=r"exact_knn_by_id: ids\[1\] = 900 is no uploaded row"):
        dev.exact_knn_by_id([0, n], 15)
    with pytest.raises(RuntimeError, match="exact_knn_by_id: k = 2000 is above the limit of 1024"):
        dev.exact_knn_by_id(qids, 2000)
    with pytest.raises(RuntimeError, match="exact_knn_by_id: bad argument"):
        dev.exact_knn_by_id(qids, 0)
    assert dev.stats()["exact_launches"] == launches
