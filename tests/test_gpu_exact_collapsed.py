"""GPU tier: exact_knn_query_collapsed (hnsw_mi355x_exact_knn_query_collapsed / hnswdev_exact_knn_collapsed) -- the flat
scan whose sink keeps at most per_group results per label.  The reference is the library's own complete order,
exact_range_query(q, inf, allowed=...), walked by tests/collapse_model.py: ids equal, distances equal as bytes.  3 000 rows x dim 20,
48 queries; the exact_chunk / exact_qtile diagnostics cut the rows into five chunks and the queries into six tiles."""
import gc

import numpy as np
import pytest

from collapse_model import collapsed_rows
from common import normalize_f32, set_diag, uniform

pytestmark = pytest.mark.gpu

N, DIM, NQ = 3000, 20, 48
CHUNK, QTILE = 700, 8                          # chunks [0, 700) .. [2800, 3000): five; 48 queries: six tiles
KNOBS = dict(exact_chunk=CHUNK, exact_qtile=QTILE)
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
A, DUP_LO, DUP_HI = 1500, 100, 2900            # the row of id A is stored under ids DUP_LO < A < DUP_HI as well


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _index(dim, metric, n):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(8); ix.set_insert_batch(0)
    return ix


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _threes(n=N, seed=3):
    """n / 3 labels of 3 rows each, scattered over the ids; the values are negative and positive."""
    return (np.repeat(np.arange(n // 3), 3)[np.random.default_rng(seed).permutation(n)] - 400).astype(np.int32)


def _heavy(n=N, seed=4):
    """Three labels: -1 holds 90 % of the rows, 2^31 - 1 and 0 share the rest."""
    lab = np.full(n, -1, np.int32)
    rest = np.random.default_rng(seed).permutation(n)[: n // 10]
    lab[rest[::2]] = 2 ** 31 - 1
    lab[rest[1::2]] = 0
    return lab


LAYOUTS = {"threes": _threes, "heavy": _heavy, "own": lambda n=N: np.arange(n, dtype=np.int32)[::-1].copy()}


class Case:
    """An index of N rows of one metric, its queries, and per allow-set the complete order of every query (computed once)."""

    def __init__(self, metric):
        self.metric = metric
        self.x = _data(metric, N, DIM, 1).copy()
        self.x[DUP_LO] = self.x[A]
        self.x[DUP_HI] = self.x[A]
        self.q = _data(metric, NQ, DIM, 2).copy()
        self.q[0] = self.x[A]                                                             # query 0 is the stored row of A, DUP_LO, DUP_HI
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        self._order = {}

    def order(self, allowed=None):
        key = None if allowed is None else allowed.tobytes()
        if key not in self._order:
            ids, d = self.ix.exact_range_query(self.q, np.inf, allowed=allowed)
            assert all(i.size == (N if allowed is None else int(allowed.sum())) for i in ids)
            self._order[key] = (ids, d)
        return self._order[key]

    def want(self, row_group, k, m, allowed=None):
        return collapsed_rows(*self.order(allowed), row_group, k, m)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


@pytest.mark.parametrize("metric", METRICS)
def test_per_group_equal_to_k_is_exact_knn_query(cases, monkeypatch, metric):
    c = cases(metric)
    for knobs in ({}, KNOBS):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for k in (1, 10, 65):
            for name in ("threes", "heavy"):
                got = c.ix.exact_knn_query_collapsed(c.q, k, LAYOUTS[name](), per_group=k)
                assert _same(got, c.ix.exact_knn_query(c.q, k)), (metric, knobs, k, name)


@pytest.mark.parametrize("metric", METRICS)
def test_label_layouts(cases, monkeypatch, metric):
    c = cases(metric)
    for knobs in ({}, KNOBS):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for name, make in LAYOUTS.items():
            rg = make()
            for m in (1, 3):
                got = c.ix.exact_knn_query_collapsed(c.q, 10, rg, per_group=m)
                assert _same(got, c.want(rg, 10, m)), (metric, knobs, name, m)
                lab = np.where(got[0] >= 0, rg[got[0].clip(0)].astype(np.int64), np.arange(10) + (1 << 40))   # padding: a label of its own
                assert all(np.unique(r, return_counts=True)[1].max() <= m for r in lab)
                if name == "heavy":                                                        # three labels: 3 results and 7 paddings, 9 and 1
                    assert ((got[0] >= 0).sum(axis=1) == 3 * m).all() and (got[0][:, 3 * m:] == -1).all() and np.isnan(got[1][:, 3 * m:]).all()
                if name == "own":                                                          # every row its own label: the cap never binds
                    assert _same(got, c.ix.exact_knn_query(c.q, 10))
    # the default is one result per label
    rg = _threes()
    assert _same(c.ix.exact_knn_query_collapsed(c.q, 10, rg), c.want(rg, 10, 1))


@pytest.mark.parametrize("metric", METRICS)
def test_one_row_under_three_ids(cases, monkeypatch, metric):
    """Query 0 is the row stored under ids 100, 1 500 and 2 900: three keys at one distance, in three chunks."""
    c = cases(metric)
    set_diag(monkeypatch, **KNOBS)
    same = _threes()
    same[[DUP_LO, A, DUP_HI]] = 12345
    other = _threes()
    other[[DUP_LO, A, DUP_HI]] = [-9, 12345, 12346]
    for m, n_same in ((1, 1), (2, 2), (3, 3)):
        got = c.ix.exact_knn_query_collapsed(c.q, 10, same, per_group=m)
        assert _same(got, c.want(same, 10, m)), (metric, m)
        assert got[0][0, :n_same].tolist() == [DUP_LO, A, DUP_HI][:n_same] and not np.isin(got[0][0, n_same:], [DUP_LO, A, DUP_HI]).any()
        got = c.ix.exact_knn_query_collapsed(c.q, 10, other, per_group=m)
        assert _same(got, c.want(other, 10, m)) and got[0][0, :3].tolist() == [DUP_LO, A, DUP_HI], (metric, m)
        assert got[1][0, 0].tobytes() == got[1][0, 2].tobytes()


@pytest.fixture(scope="module")
def grid():
    """Grid rows (integers 1..3) on a context of uploaded rows: dozens of candidates tie, and the id decides which member of a
    label survives.  (db, rows, queries, the complete order per query)."""
    import hnswindex
    made = {}

    def get(metric):
        if metric not in made:
            x, q = _data(metric, N, DIM, 6, grid=True), _data(metric, NQ, DIM, 7, grid=True)
            db = hnswindex.DeviceBackend(DIM, metric, capacity=N)
            db.upload_rows(0, x)
            order = db.exact_range(q, np.inf)
            d0 = order[1][0]
            if metric == "sq_euclid":
                assert (np.diff(d0) == 0).sum() > 30                                      # dozens of ties
            made[metric] = (db, q, order)
        return made[metric]
    yield get
    made.clear()
    gc.collect()


@pytest.mark.parametrize("metric", METRICS)
def test_ties_on_grid_rows(grid, monkeypatch, metric):
    db, q, order = grid(metric)
    for knobs in ({}, KNOBS):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for name in ("threes", "heavy"):
            rg = LAYOUTS[name]()
            for k, m in ((10, 1), (10, 2), (65, 3)):
                got = db.exact_knn_collapsed(q, k, rg, per_group=m)
                assert _same(got, collapsed_rows(*order, rg, k, m)), (metric, knobs, name, k, m)


@pytest.mark.parametrize("metric", METRICS)
def test_a_labels_nearest_members_across_chunks(monkeypatch, metric):
    """One label whose three nearest members are ids 699, 700 and 1 400 -- the last and the first entry of two chunks and the first
    of a third -- with farther members in every chunk."""
    import hnswindex
    x = uniform(N, DIM, 8).copy()
    q = uniform(NQ, DIM, 9).copy()
    x[1400], x[700], x[699] = q[0] + np.float32(0.02), q[0] + np.float32(0.04), q[0] + np.float32(0.06)
    if metric.startswith("ucosine"):
        x, q = normalize_f32(x), normalize_f32(q)
    rg = np.arange(N, dtype=np.int32) + 10
    rg[[5, 650, 699, 700, 1399, 1400, 2000, 2999]] = 7
    db = hnswindex.DeviceBackend(DIM, metric, capacity=N)
    db.upload_rows(0, x)
    set_diag(monkeypatch, **KNOBS)
    order = db.exact_range(q, np.inf)
    near = order[0][0][:3].tolist()                                                       # (int8 rows may tie: then the id orders them)
    assert sorted(near) == [699, 700, 1400]
    for m in (1, 2, 3):
        got = db.exact_knn_collapsed(q, 10, rg, per_group=m)
        assert _same(got, collapsed_rows(*order, rg, 10, m)), (metric, m)
        assert got[0][0, :m].tolist() == near[:m] and (rg[got[0][0]] == 7).sum() == m, (metric, m)
    del db
    gc.collect()


@pytest.mark.parametrize("metric", METRICS)
def test_lists_longer_than_a_piece(cases, monkeypatch, metric):
    c = cases(metric)
    rg = _threes()
    for knobs in ({}, KNOBS):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for k in (65, 130):
            assert _same(c.ix.exact_knn_query_collapsed(c.q, k, rg, per_group=3), c.want(rg, k, 3)), (metric, knobs, k)
            assert _same(c.ix.exact_knn_query_collapsed(c.q, k, rg, per_group=1), c.want(rg, k, 1)), (metric, knobs, k)
        heavy = _heavy()
        assert _same(c.ix.exact_knn_query_collapsed(c.q, 130, heavy, per_group=64), c.want(heavy, 130, 64)), (metric, knobs)
        own = LAYOUTS["own"]()
        got = c.ix.exact_knn_query_collapsed(c.q, 1024, own, per_group=1)
        assert _same(got, c.ix.exact_knn_query(c.q, 1024)) and (got[0] >= 0).all(), (metric, knobs)
    got = c.ix.exact_knn_query_collapsed(c.q, 1024, rg, per_group=1)                    # 1 000 labels: 1 000 results and 24 paddings
    assert _same(got, c.want(rg, 1024, 1)) and ((got[0] >= 0).sum(axis=1) == 1000).all()


def test_allowed_and_removed_ids(monkeypatch):
    """A removed id is no candidate and counts towards no label's cap: the label's next member takes its place.  The same under a
    10 % allow-set."""
    x, q = uniform(N, DIM, 1), uniform(NQ, DIM, 2)
    ix = _index(DIM, "sq_euclid", N)
    ix.add(x)
    rg = _threes()
    set_diag(monkeypatch, **KNOBS)
    allowed = np.zeros(N, bool)
    allowed[np.random.default_rng(8).choice(N, N // 10, replace=False)] = True
    before = ix.exact_knn_query_collapsed(q, 10, rg)
    a_before = ix.exact_knn_query_collapsed(q, 10, rg, allowed=allowed)
    assert _same(a_before, collapsed_rows(*ix.exact_range_query(q, np.inf, allowed=allowed), rg, 10, 1)) and allowed[a_before[0][a_before[0] >= 0]].all()
    gone = np.unique(np.concatenate([before[0][:24, 0], a_before[0][:24, 1]]))            # the nearest member of some labels
    ix.remove(gone)
    assert ix.count == N - gone.size and ix.length == N
    for al in (None, allowed):
        got = ix.exact_knn_query_collapsed(q, 10, rg, allowed=al)
        assert _same(got, collapsed_rows(*ix.exact_range_query(q, np.inf, allowed=al), rg, 10, 1)), al is None
        assert not np.isin(got[0], gone).any()
    got = ix.exact_knn_query_collapsed(q, 10, rg)
    # where the removed id's label has another member, that member is in the row now or lies behind the row's last result
    full = ix.exact_range_query(q[:1], np.inf)
    lab0 = int(rg[before[0][0, 0]])
    heirs = [int(i) for i in full[0][0] if rg[i] == lab0]
    assert heirs and before[0][0, 0] not in heirs and (heirs[0] in got[0][0] or full[1][0][list(full[0][0]).index(heirs[0])] >= got[1][0, -1])
    assert (np.array([(rg[r] == lab0).sum() for r in got[0]]) <= 1).all()


def test_errors_leave_the_next_call_correct(cases):
    import hnswindex
    c = cases("sq_euclid")
    rg = _threes()
    want = c.want(rg, 10, 1)
    c.ix.reset_stats()
    with pytest.raises(ValueError, match=f"row_group has {N - 1} entries, the index's length is {N}"):
        c.ix.exact_knn_query_collapsed(c.q, 10, rg[:-1])
    with pytest.raises(ValueError, match=r"per_group = 0 is outside \[1, k = 10\]"):
        c.ix.exact_knn_query_collapsed(c.q, 10, rg, per_group=0)
    with pytest.raises(ValueError, match=r"per_group = 11 is outside \[1, k = 10\]"):
        c.ix.exact_knn_query_collapsed(c.q, 10, rg, per_group=11)
    with pytest.raises(ValueError, match="k = 1025 is above the limit of 1024"):
        c.ix.exact_knn_query_collapsed(c.q, 1025, rg)
    # the C ABI says the same to a caller that comes without the bindings
    import ctypes as ct
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    ids, d = np.full((NQ, 10), 7, np.int32), np.full((NQ, 10), 7.0, np.float32)
    big_ids, big_d = np.full((NQ, 1025), 7, np.int32), np.full((NQ, 1025), 7.0, np.float32)

    def call(k, n_rg, m, oi=ids, od=d):
        return lib.hnsw_mi355x_exact_knn_query_collapsed(c.ix._h, c.q.ctypes.data_as(F), NQ, DIM, k, rg.ctypes.data_as(I), n_rg, m, None, 0,
                                                         oi.ctypes.data_as(I), od.ctypes.data_as(F))
    for args, msg in (((10, N - 1, 1), f"hnsw_mi355x_exact_knn_query_collapsed: row_group has {N - 1} entries, the index's length is {N}"),
                      ((10, N, 0), "hnsw_mi355x_exact_knn_query_collapsed: per_group = 0 is outside [1, k = 10]"),
                      ((10, N, 11), "hnsw_mi355x_exact_knn_query_collapsed: per_group = 11 is outside [1, k = 10]"),
                      ((1025, N, 1, big_ids, big_d), "hnsw_mi355x_exact_knn_query_collapsed: k = 1025 is above the limit of 1024")):
        assert call(*args) == -1 and msg in hnswindex.net_amd.last_error(), (args, hnswindex.net_amd.last_error())
    assert (ids == 7).all() and (d == 7.0).all() and (big_ids == 7).all()
    assert c.ix.stats()["exact_launches"] == 0 and c.ix.exact_collapsed_info()["calls"] == 0      # nothing was launched
    assert call(10, N, 1) == 0 and _same((ids, d), want)
    assert _same(c.ix.exact_knn_query_collapsed(c.q, 10, rg), want)
    # the inner boundary checks the labels against the rows it holds
    db = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=N)
    db.upload_rows(0, c.x)
    with pytest.raises(RuntimeError, match=f"exact_knn_collapsed: row_group has {N - 1} entries, the scan's {N} ids need one each"):
        db.exact_knn_collapsed(c.q, 10, rg[:-1])
    assert db.stats()["exact_launches"] == 0
    assert _same(db.exact_knn_collapsed(c.q, 10, rg[:-1], n_rows=N - 1), collapsed_rows(*db.exact_range(c.q, np.inf, n_rows=N - 1), rg, 10, 1))
    assert _same(db.exact_knn_collapsed(c.q, 10, rg), want)
    del db
    gc.collect()


def test_counters(cases, monkeypatch):
    c = cases("sq_euclid")
    set_diag(monkeypatch, **KNOBS)
    allowed = np.zeros(N, bool)
    allowed[::3] = True
    c.ix.reset_stats()
    assert c.ix.exact_collapsed_info() == {"calls": 0, "queries": 0, "dropped": 0, "evicted": 0}
    c.ix.exact_knn_query_collapsed(c.q, 10, LAYOUTS["own"]())                             # every row its own label: the cap never acts
    st, info = c.ix.stats(), c.ix.exact_collapsed_info()
    assert info == {"calls": 1, "queries": NQ, "dropped": 0, "evicted": 0}, info
    assert st["exact_evals"] == NQ * N and st["exact_launches"] == 1 and st["search_launches"] == 0, st
    c.ix.exact_knn_query_collapsed(c.q[:5], 10, LAYOUTS["own"](), allowed=allowed)
    st, info = c.ix.stats(), c.ix.exact_collapsed_info()
    assert st["exact_evals"] == NQ * N + 5 * 1000 and info["calls"] == 2 and info["queries"] == NQ + 5
    # one label for every row, one result: a list never fills, so every key reaches an insert, and every key but the first of a
    # list is dropped or evicts -- in the five chunk lists of a query, and then four of those five in the merge
    c.ix.reset_stats()
    ids, d = c.ix.exact_knn_query_collapsed(c.q, 10, np.full(N, -3, np.int32))
    info = c.ix.exact_collapsed_info()
    assert info["calls"] == 1 and info["dropped"] + info["evicted"] == NQ * (N - 5) + NQ * 4, info
    assert info["evicted"] >= 0 and (ids[:, 1:] == -1).all() and _same((ids[:, :1], d[:, :1]), c.ix.exact_knn_query(c.q, 1))
    c.ix.reset_stats()
    assert c.ix.exact_collapsed_info()["calls"] == 0
