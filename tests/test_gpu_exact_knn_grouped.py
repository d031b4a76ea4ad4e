"""GPU tier: the grouped exact k-NN call (hnsw_mi355x_exact_knn_query_grouped / hnswdev_exact_knn_grouped) against its
two references -- the model (tests/exact_grouped_model.py: exact_knn_model one group at a time) and the product's own ungrouped call
with the group as its allow-set.  Every comparison is ids equal and distance BYTES equal; every call that launches is also held to
the exact number of (query, row) pairs it must measure."""
import ctypes as ct
import re

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_grouped_model import evals, exact_knn_grouped, group_mask, info
from exact_knn_model import boundary_tie, distances, exact_knn

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
N, DIM, NQ = 1500, 16, 67
GRID_SEED = 2


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _backend(metric, x):
    import hnswindex
    db = hnswindex.DeviceBackend(x.shape[1], metric, capacity=max(x.shape[0], 1))
    db.upload_rows(0, x)
    return db


def _index(metric, x, **knobs):
    import hnswindex
    ix = hnswindex.Index(x.shape[1], metric)
    ix.set_collection_size(2048); ix.set_min_nn(20)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    return ix


def _same(got, want):
    return (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()


def _per_group_calls(db, q, k, rg, qg, ng):
    """The parent's way: one ungrouped call per group that a query names, the group as its allow-set."""
    qg = np.asarray(qg)
    ids = np.empty((q.shape[0], k), np.int32)
    d = np.empty((q.shape[0], k), np.float32)
    for g in np.unique(qg):
        sel = np.flatnonzero(qg == g)
        ids[sel], d[sel] = db.exact_knn(q[sel], k, allowed=group_mask(rg, int(g), ng))
    return ids, d


def _check(db, metric, x, q, k, rg, qg, ng, tag=None, product=True, want=None):
    """One grouped call on a backend holding x: the model's answer, the per-group calls' answer, the pairs measured."""
    n = x.shape[0]
    db.reset_stats()
    got = db.exact_knn_grouped(q, k, rg, qg, ng)
    st = db.stats()
    want = exact_knn_grouped(metric, x, q, k, rg, qg, ng) if want is None else want
    assert _same(got, want), (metric, tag)
    pairs = evals(n, rg, qg, ng)
    assert st["exact_evals"] == pairs and st["exact_launches"] == (1 if pairs else 0) and st["search_launches"] == 0, (metric, tag, st, pairs)
    if product:
        assert _same(got, _per_group_calls(db, q, k, rg, qg, ng)), (metric, tag)
    return got


def _base_groups():
    rg = (np.arange(N) % 7).astype(np.int32)
    rg[rg == 5] = 2            # group 5 is empty, group 2 has 425 members
    rg[100:110] = -1
    qg = np.random.default_rng(7).integers(0, 7, NQ).astype(np.int32)   # 5 to 14 queries per group, in scrambled order
    return rg, qg


@pytest.fixture(scope="module")
def sets():
    """(x, q, backend) per (metric, grid): computed once, shared, never written."""
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            x = _data(metric, N, DIM, GRID_SEED if grid else 1, grid)
            q = _data(metric, NQ, DIM, (GRID_SEED if grid else 1) + 100, grid)
            for a in (x, q):
                a.setflags(write=False)
            cache[(metric, grid)] = (x, q, _backend(metric, x))
        return cache[(metric, grid)]
    return get


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("metric", METRICS)
def test_the_base_case_is_the_model_and_the_per_group_calls(sets, metric, grid):
    x, q, db = sets(metric, grid)
    rg, qg = _base_groups()
    per = np.bincount(qg, minlength=7)
    assert per.min() >= 5 and per.max() <= 14 and (np.diff(qg) < 0).any()
    assert (rg == 5).sum() == 0 and (rg == 2).sum() == 425
    db.reset_stats()
    got = _check(db, metric, x, q, 10, rg, qg, 7, grid)
    sel5 = qg == 5
    assert sel5.any() and (got[0][sel5] == -1).all() and np.isnan(got[1][sel5]).all()      # the empty group: padding
    assert not np.isin(got[0], np.arange(100, 110)).any()
    gi = db.exact_grouped_info()
    scanned, listed = info(N, rg, qg, 7)
    assert gi["calls"] == 1 and gi["groups_scanned"] == scanned == 6 and gi["ids_listed"] == listed == N - 10 and gi["scan_blocks"] >= scanned, gi
    if grid:   # the condition: the model itself meets a tie across rank k-1 / k inside a group, or the id order is never exercised
        for g in (0, 4, 6):
            assert boundary_tie(metric, x, q[qg == g], 10, mask=rg == g), (metric, g)


SHAPES = [(m, dim) for m in METRICS if m != "sq_euclid_i8" for dim in (5, 13, 24, 120, 264)] + [("sq_euclid_i8", 96)]


@pytest.mark.parametrize("metric,dim", SHAPES)
def test_row_shapes(metric, dim):
    """Three groups of very different size -- 1 row, 40 rows, the rest -- at the row shapes that take every path of the lane arithmetic."""
    n = 300
    x, q = _data(metric, n, dim, 11), _data(metric, 9, dim, 12)
    rg = np.full(n, 2, np.int32)
    rg[7] = 0
    rg[50:90] = 1
    qg = np.array([0, 1, 2, 2, 1, 0, 2, 1, 2], np.int32)
    db = _backend(metric, x)
    for k in (10, 64):
        got = _check(db, metric, x, q, k, rg, qg, 3, (dim, k))
        assert (got[0][qg == 0, 0] == 7).all() and (got[0][qg == 0, 1:] == -1).all()
        if k == 64:
            assert (got[0][qg == 1, 40:] == -1).all() and (got[0][qg == 1, :40] >= 50).all()


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_k_and_padding(metric):
    n = 300
    x, q = _data(metric, n, 24, 21, grid=True), _data(metric, 12, 24, 22, grid=True)
    rg = np.full(n, 2, np.int32)         # 226 rows
    rg[:64] = 0                          # 64 rows
    rg[100:110] = 1                      # 10 rows
    qg = np.arange(12, dtype=np.int32)[::-1] % 3
    db = _backend(metric, x)
    for k in (1, 63, 64, 65, 1024):
        got = _check(db, metric, x, q, k, rg, qg, 3, k)
        for g, m in ((0, 64), (1, 10), (2, 226)):
            assert (got[0][qg == g, :min(k, m)] >= 0).all() and (got[0][qg == g, m:] == -1).all() and np.isnan(got[1][qg == g, m:]).all(), (k, g)


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8"])
def test_tiles(metric):
    """A group of 33 queries -- two tiles, the second of one query, which shadows itself three times --, a group of one query and a
    group that no query names."""
    n = 600
    x, q = _data(metric, n, DIM, 31), _data(metric, 34, DIM, 32)
    rg = (np.arange(n) % 3).astype(np.int32)
    qg = np.zeros(34, np.int32)
    qg[17] = 1                           # the single query sits in the middle of the caller's order
    db = _backend(metric, x)
    _check(db, metric, x, q, 10, rg, qg, 3)
    gi = db.exact_grouped_info()
    assert gi["groups_scanned"] == 2 and gi["scan_blocks"] == 3 and gi["ids_listed"] == n, gi   # tiles of 32 + 1 and of 1; one chunk each


def test_row_group_edges(sets):
    x, q, db = sets("sq_euclid", False)
    rg, qg = _base_groups()
    rg = rg.copy()
    rg[200:220] = 7                      # >= n_groups
    rg[300:310] = -5
    rg[400] = np.iinfo(np.int32).max
    rg[401] = np.iinfo(np.int32).min
    _check(db, "sq_euclid", x, q, 10, rg, qg, 7, "values")
    # n_row_group shorter than the rows: ids past its end are in no group
    got = _check(db, "sq_euclid", x, q, 10, rg[:1000], qg, 7, "short")
    assert got[0].max() < 1000
    # ... and beyond them: clamped, a row that does not exist is never dereferenced
    wide = np.concatenate([rg, np.tile(np.arange(7, dtype=np.int32), 1000)])
    want = exact_knn_grouped("sq_euclid", x, q, 10, rg, qg, 7)
    db.reset_stats()
    assert _same(db.exact_knn_grouped(q, 10, wide, qg, 7), want)
    assert db.stats()["exact_evals"] == evals(N, rg, qg, 7)
    # n_rows below the uploaded rows
    head = db.exact_knn_grouped(q, 10, rg, qg, 7, n_rows=700)
    assert _same(head, exact_knn_grouped("sq_euclid", x[:700], q, 10, rg[:700], qg, 7))
    # the index layer clamps to Length in the same way
    ix = _index("sq_euclid", x)
    for arr in (rg, rg[:1000], wide):
        assert _same(ix.exact_knn_query_grouped(q, 10, arr, qg, 7), exact_knn_grouped("sq_euclid", x, q, 10, arr[:N], qg, 7))
    # no id in any group that a query names: padding and no scan
    db.reset_stats()
    ids, d = db.exact_knn_grouped(q, 10, np.full(N, -1, np.int32), qg, 7)
    assert (ids == -1).all() and np.isnan(d).all()
    assert db.stats()["exact_launches"] == 0
    assert db.exact_grouped_info() == {"calls": 0, "groups_scanned": 0, "scan_blocks": 0, "ids_listed": 0}   # a call that scans nothing counts nowhere
    ids, d = db.exact_knn_grouped(q, 10, np.zeros(0, np.int32), qg, 7)
    assert (ids == -1).all() and np.isnan(d).all()


BIG_N, BIG_DIM = 20000, 8


@pytest.fixture(scope="module")
def big():
    """20 000 x 8 rows per metric with one group of about 15 000 rows beside groups of 3 and of 200; the model's answer, computed once."""
    cache = {}

    def get(metric):
        if metric not in cache:
            x, q = _data(metric, BIG_N, BIG_DIM, 41, grid=True), _data(metric, 9, BIG_DIM, 42, grid=True)
            rg = np.full(BIG_N, -1, np.int32)
            rng = np.random.default_rng(43)
            perm = rng.permutation(BIG_N)
            rg[perm[:15001]] = 0
            rg[perm[15001:15004]] = 1
            rg[perm[15004:15204]] = 2
            qg = np.array([0, 2, 0, 1, 0, 2, 0, 1, 0], np.int32)
            want = exact_knn_grouped(metric, x, q, 10, rg, qg, 3)
            for a in (x, q, rg, qg, *want):
                a.setflags(write=False)
            cache[metric] = (x, q, rg, qg, want, _backend(metric, x))
        return cache[metric]
    return get


@pytest.mark.parametrize("metric", METRICS)
def test_chunks_and_tiles_give_identical_bytes(monkeypatch, big, metric):
    x, q, rg, qg, want, db = big(metric)
    blocks = {}
    for chunk in (64, 1000, 0):
        for qtile in (1, 3, 0):
            set_diag(monkeypatch, exact_chunk=chunk, exact_qtile=qtile)
            _check(db, metric, x, q, 10, rg, qg, 3, (chunk, qtile), product=(chunk, qtile) == (0, 0), want=want)
            blocks[(chunk, qtile)] = db.exact_grouped_info()["scan_blocks"]
    # the large group gets more chunks than the small ones: 5 queries x 235 chunks of 64, 2 x 1 (3 rows), 2 x 4 (200 rows)
    assert blocks[(64, 1)] == 5 * 235 + 2 * 1 + 2 * 4 and blocks[(64, 0)] == 235 + 1 + 4, blocks
    assert blocks[(1000, 3)] == 2 * 16 + 1 + 1 and blocks[(0, 0)] > 3, blocks


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_one_row_chunks_and_the_chunk_cap(monkeypatch, big, metric):
    """exact_chunk=1: a 4 096-row group is 4 096 chunks of one row (every block shadows its row 127 times), a 5 000-row group meets
    the cap of 4 096 chunks and gets 2 500 chunks of two."""
    x, q, _, _, _, db = big(metric)
    rg = np.full(BIG_N, -1, np.int32)
    rg[1000:5096] = 0
    rg[10000:15000] = 1
    qg = np.array([1, 0, 0, 1, 0], np.int32)
    want = exact_knn_grouped(metric, x, q[:5], 10, rg, qg, 2)
    set_diag(monkeypatch, exact_chunk=1)
    _check(db, metric, x, q[:5], 10, rg, qg, 2, "chunk1", product=False, want=want)
    assert db.exact_grouped_info()["scan_blocks"] == 4096 + 2500
    set_diag(monkeypatch, exact_chunk=0)
    _check(db, metric, x, q[:5], 10, rg, qg, 2, "picker", product=False, want=want)


def test_many_tiny_groups():
    """n_groups = n = 4 096: every row its own group, query i in group i -- offsets over thousands of groups, thousands of one-query
    work items of one row."""
    n = 4096
    x, q = uniform(n, DIM, 51), uniform(n, DIM, 52)
    rg = np.random.default_rng(53).permutation(n).astype(np.int32)     # row j is group rg[j]
    qg = np.arange(n, dtype=np.int32)                                  # query i wants the one row whose group is i
    row_of = np.argsort(rg).astype(np.int32)
    db = _backend("sq_euclid", x)
    db.reset_stats()
    ids, d = db.exact_knn_grouped(q, 3, rg, qg, n)
    st, gi = db.stats(), db.exact_grouped_info()
    assert (ids[:, 0] == row_of).all() and (ids[:, 1:] == -1).all() and np.isnan(d[:, 1:]).all()
    want = np.array([distances("sq_euclid", x, q[i], row_of[i:i + 1])[0, 0] for i in range(n)], np.float32)
    assert d[:, 0].tobytes() == want.tobytes()
    assert st["exact_evals"] == n and st["exact_launches"] == 1, st
    assert gi == {"calls": 1, "groups_scanned": n, "scan_blocks": n, "ids_listed": n}, gi


def test_a_row_group_of_more_than_4_mib():
    """1.1M ids are 4.4 MB of row_group: above 4 MiB the array goes up in pieces from several threads, not through the one pinned
    stage.  Two small groups whose members lie in every piece, the last id included; everything else in no group."""
    n = 1_100_000
    x, q = uniform(n, 8, 55), uniform(6, 8, 56)
    rg = np.full(n, -1, np.int32)
    picks = np.random.default_rng(57).choice(n - 1, 600, replace=False)
    rg[picks[:500]] = 0
    rg[picks[500:]] = 3
    rg[n - 1] = 3
    qg = np.array([3, 0, 0, 3, 1, 0], np.int32)      # group 1 is empty
    assert rg.nbytes > 4 << 20
    db = _backend("sq_euclid", x)
    got = _check(db, "sq_euclid", x, q, 10, rg, qg, 4, product=False)
    assert (got[0][4] == -1).all() and db.exact_grouped_info()["ids_listed"] == 601
    db.set_profiling(True)                           # the list-building kernels' event time is kept apart from the scan's
    db.reset_stats()
    db.exact_knn_grouped(q, 10, rg, qg, 4)
    st, ms = db.stats(), db.exact_grouped_list_ms()
    db.set_profiling(False)
    assert ms > 0.0 and st["exact_kernel_ms"] > 0.0 and st["exact_timed_launches"] == 1
    db.reset_stats()
    assert db.exact_grouped_list_ms() == 0.0


def test_a_single_group_and_the_cap_on_groups(sets):
    x, q, db = sets("sq_euclid", False)
    rg, qg = _base_groups()
    zeros = np.zeros(N, np.int32)
    db.reset_stats()
    assert _same(db.exact_knn_grouped(q, 10, zeros, np.zeros(NQ, np.int32), 1), db.exact_knn(q, 10))
    assert db.stats()["exact_evals"] == 2 * NQ * N
    want = exact_knn_grouped("sq_euclid", x, q, 10, rg, qg, 7)
    assert _same(db.exact_knn_grouped(q, 10, rg, qg, 65536), want)      # the largest number of groups is accepted
    top = rg.copy()
    top[rg == 6] = 65535
    assert _same(db.exact_knn_grouped(q, 10, top, np.where(qg == 6, 65535, qg), 65536), want)
    ix = _index("sq_euclid", x)
    assert _same(ix.exact_knn_query_grouped(q, 10, rg, qg, 65536), want)
    assert _same(ix.exact_knn_query_grouped(q, 10, rg, qg), want)       # n_groups worked out from the arrays
    for call in (db.exact_knn_grouped, ix.exact_knn_query_grouped):
        for bad in (65537, 0, -1):
            with pytest.raises(RuntimeError, match="65536"):
                call(q, 10, rg, np.zeros(NQ, np.int32), bad)


def test_two_rounds_by_the_output_budget():
    """k = 1024 leaves 2^24 / 1024 = 16 384 queries per round: 16 384 + 16 queries are two rounds.  64 groups of 64 rows: every row
    of the result is padded from rank 64.  Rounds are ranges of the caller's order, the sort is inside a round."""
    n, nq, k = 4096, 16384 + 16, 1024
    x, q = uniform(n, 8, 61), uniform(nq, 8, 62)
    rg = (np.arange(n) % 64).astype(np.int32)
    qg = np.random.default_rng(63).integers(0, 64, nq).astype(np.int32)
    db = _backend("sq_euclid", x)
    db.reset_stats()
    got = db.exact_knn_grouped(q, k, rg, qg, 64)
    st = db.stats()
    assert st["exact_launches"] == 2 and st["exact_evals"] == nq * 64, st
    assert (got[0][:, :64] >= 0).all() and (got[0][:, 64:] == -1).all() and np.isnan(got[1][:, 64:]).all()
    assert (got[0][:, 0] % 64 == qg).all()
    assert _same(got, _per_group_calls(db, q, k, rg, qg, 64))
    sel = np.r_[0:8, 16380:16400]       # the model, across the boundary of the rounds
    assert _same((got[0][sel], got[1][sel]), exact_knn_grouped("sq_euclid", x, q[sel], k, rg, qg[sel], 64))


def test_nan_and_inf_rows_order_last_inside_their_group():
    n = 200
    x = uniform(n, DIM, 71).copy()
    x[5, 2] = np.nan
    x[9, 3] = np.inf
    x[151, 0] = np.nan
    x[8, 1] = np.nan                      # in the other group
    q = uniform(4, DIM, 72)
    rg = (np.arange(n) % 2).astype(np.int32)     # 5, 9, 151 are in group 1
    qg = np.array([1, 0, 1, 1], np.int32)
    db = _backend("sq_euclid", x)
    ids, d = db.exact_knn_grouped(q, 100, rg, qg, 2)
    w_ids, w_d = exact_knn_grouped("sq_euclid", x, q, 100, rg, qg, 2)
    assert (ids == w_ids).all()
    odd = qg == 1
    assert d[odd][:, :98].tobytes() == w_d[odd][:, :98].tobytes()       # every number, +inf included, bit for bit
    assert (ids[odd][:, 97:] == [9, 5, 151]).all()                      # the inf row before the NaN rows, those by id
    assert np.isinf(d[odd][:, 97]).all() and np.isnan(d[odd][:, 98:]).all()
    assert d[odd][:, 98:].view(np.uint32).tolist() == [[0x7fc00000] * 2] * 3
    assert ids[1, 99] == 8 and np.isnan(d[1, 99]) and d[1, :99].tobytes() == w_d[1, :99].tobytes()
    ids10, d10 = db.exact_knn_grouped(q, 10, rg, qg, 2)                 # and they never displace a number
    assert (ids10 == w_ids[:, :10]).all() and d10.tobytes() == w_d[:, :10].tobytes()


def test_removals_and_slot_reuse():
    x = uniform(N, DIM, 81).copy()
    q = uniform(12, DIM, 82)
    rg, _ = _base_groups()
    qg = (np.arange(12) % 7).astype(np.int32)[::-1].copy()
    ix = _index("sq_euclid", x)
    assert _same(ix.exact_knn_query_grouped(q, 10, rg, qg, 7), exact_knn_grouped("sq_euclid", x, q, 10, rg, qg, 7))
    rng = np.random.default_rng(83)
    gone = np.unique(np.concatenate([[ix.entry_point], rng.choice(N, 99, replace=False)])).astype(np.int32)
    before = rg.copy()
    ix.remove(gone)
    live = np.sort(ix.ids())
    for k in (10, 300):
        ix.reset_stats()
        got = ix.exact_knn_query_grouped(q, k, rg, qg, 7)
        assert not np.isin(got[0], gone).any()
        assert _same(got, exact_knn_grouped("sq_euclid", x, q, k, rg, qg, 7, live=live)), k
        assert ix.stats()["exact_evals"] == evals(N, rg, qg, 7, live=live)
        for g in np.unique(qg):
            sel = qg == g
            assert _same((got[0][sel], got[1][sel]), ix.exact_knn_query(q[sel], k, allowed=rg == g)), (k, g)
    assert (rg == before).all()                  # the caller's array is not written
    fresh = uniform(50, DIM, 84)
    new_ids = ix.add(fresh)
    assert np.isin(new_ids, gone).all()          # vacated slots are reused
    x[new_ids] = fresh
    live = np.sort(ix.ids())
    got = ix.exact_knn_query_grouped(np.concatenate([q, fresh[:3]]), 10, rg, np.concatenate([qg, rg[new_ids[:3]].clip(0)]), 7)
    want = exact_knn_grouped("sq_euclid", x, np.concatenate([q, fresh[:3]]), 10, rg, np.concatenate([qg, rg[new_ids[:3]].clip(0)]), 7, live=live)
    assert _same(got, want)
    for j in range(3):                           # a re-added id is returned, with its new row: distance 0 to itself
        if rg[new_ids[j]] >= 0:
            assert got[0][12 + j, 0] == new_ids[j] and got[1][12 + j, 0] == 0.0


def _raw(lib_call, handle, q, k, rg, n_rg, qg, ng, n_rows=None):
    q = np.ascontiguousarray(q, np.float32)
    ids = np.full((q.shape[0], max(k, 1)), 77, np.int32)
    d = np.full((q.shape[0], max(k, 1)), 77.0, np.float32)
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    rgp = None if rg is None else rg.ctypes.data_as(I)
    qgp = None if qg is None else qg.ctypes.data_as(I)
    mid = (q.shape[0], q.shape[1], k) if n_rows is None else (q.shape[0], n_rows, k)
    rc = lib_call(handle, q.ctypes.data_as(F), *mid, rgp, n_rg, qgp, ng, ids.ctypes.data_as(I), d.ctypes.data_as(F))
    return rc, ids, d


def test_argument_errors_write_nothing(sets):
    import hnswindex
    lib = hnswindex.net_amd.lib
    x, q, db = sets("sq_euclid", False)
    rg, qg = _base_groups()
    ix = _index("sq_euclid", x)
    bad = qg.copy()
    bad[41] = 7
    bad[60] = -1
    for call, handle, n_rows, err in ((lib.hnsw_mi355x_exact_knn_query_grouped, ix._h, None, hnswindex.net_amd.last_error),
                                      (lib.hnswdev_exact_knn_grouped, db._ctx, N, db.last_error)):
        for args, word in (((q, 10, rg, N, bad, 7), r"query_group\[41\]"), ((q, 1025, rg, N, qg, 7), "1024"), ((q, 10, None, N, qg, 7), "row_group"),
                           ((q, 10, rg, -1, qg, 7), "n_row_group"), ((q, 10, rg, N, qg, 65537), "65536")):
            rc, ids, d = _raw(call, handle, *args, n_rows=n_rows)
            assert rc == -1 and (ids == 77).all() and (d == 77.0).all(), word
            assert re.search(word, err()), (word, err())
        rc, ids, d = _raw(call, handle, q, 10, rg, N, qg, 7, n_rows=n_rows)      # and the same call with good arguments answers
        assert rc == 0 and _same((ids, d), exact_knn_grouped("sq_euclid", x, q, 10, rg, qg, 7))
    with pytest.raises(RuntimeError, match=r"query_group\[41\]"):
        ix.exact_knn_query_grouped(q, 10, rg, bad, 7)
    with pytest.raises(RuntimeError, match="1024"):
        db.exact_knn_grouped(q, 1025, rg, qg, 7)
    ids, d = ix.exact_knn_query_grouped(q[:2], 0, rg, qg[:2], 7)       # k < 1: nothing to write, success (as the ungrouped call)
    assert ids.shape == (2, 0)


def test_the_grouped_counters(sets):
    x, q, db = sets("sq_euclid", False)
    rg, qg = _base_groups()
    db.reset_stats()
    assert db.exact_grouped_info() == {"calls": 0, "groups_scanned": 0, "scan_blocks": 0, "ids_listed": 0}
    db.exact_knn_grouped(q, 10, rg, qg, 7)
    db.exact_knn_grouped(q[:3], 10, rg[:700], np.array([5, 1, 1], np.int32), 7)    # group 5 has no member; one group scanned
    gi = db.exact_grouped_info()
    a, b = info(N, rg, qg, 7), info(700, rg[:700], [5, 1, 1], 7)
    assert gi["calls"] == 2 and gi["groups_scanned"] == a[0] + b[0] == 7 and gi["ids_listed"] == a[1] + b[1], gi
    assert gi["scan_blocks"] == 6 + 1, gi                               # 1 500 x 16 rows: one tile and one chunk per group
    assert db.stats()["exact_evals"] == evals(N, rg, qg, 7) + evals(700, rg[:700], [5, 1, 1], 7)
    ix = _index("sq_euclid", x)
    ix.exact_knn_query_grouped(q, 10, rg, qg, 7)
    gi = ix.exact_grouped_info()
    assert gi["calls"] == 1 and gi["groups_scanned"] == 6 and gi["ids_listed"] == a[1], gi
    ix.reset_stats()
    assert ix.exact_grouped_info()["calls"] == 0


def test_the_resident_query_set_is_not_touched_and_can_be_the_queries(sets):
    import hnswindex
    lib = hnswindex.net_amd.lib
    x, q, _ = sets("sq_euclid", False)
    rg, qg = _base_groups()
    ix = _index("sq_euclid", x)
    ix.set_resident_queries(q[:20])
    before = ix.knn_query_resident(10)
    other = uniform(33, DIM, 91)
    og = (np.arange(33) % 7).astype(np.int32)
    assert _same(ix.exact_knn_query_grouped(other, 10, rg, og, 7), exact_knn_grouped("sq_euclid", x, other, 10, rg, og, 7))
    ix.exact_knn_query_grouped(other[:5], 10, np.full(N, -1, np.int32), og[:5], 7)      # the no-scan path
    assert lib.hnsw_mi355x_resident_count(ix._h) == 20
    assert _same(ix.knn_query_resident(10), before)
    # the inner boundary, where the cached query norms (cosine) and the quantised records (int8) must survive and be gathered too
    for metric in ("cosine", "sq_euclid_i8"):
        xm, qm, _ = sets(metric, False)
        fresh = _backend(metric, xm)
        fresh.set_queries(qm[:40])
        cand = np.arange(50, dtype=np.int32)
        off = np.arange(41, dtype=np.int32) * 50
        want = fresh.dist_query_batch(None, off, np.tile(cand, 40))
        fresh.exact_knn_grouped(other, 10, rg, og, 7)
        assert fresh.dist_query_batch(None, off, np.tile(cand, 40)).tobytes() == want.tobytes()
        # queries == NULL: the resident set is the query set, gathered into the call's order on the device
        res = fresh.exact_knn_grouped(None, 10, rg, qg[:40], 7)
        assert _same(res, exact_knn_grouped(metric, xm, qm[:40], 10, rg, qg[:40], 7)), metric
        assert fresh.dist_query_batch(None, off, np.tile(cand, 40)).tobytes() == want.tobytes()
        with pytest.raises(RuntimeError, match="resident"):
            fresh.exact_knn_grouped(None, 10, rg, qg[:41], 7)


def test_other_contexts_and_the_host_traversal_setting(sets):
    x, q, _ = sets("sq_euclid", False)
    rg, qg = _base_groups()
    want = exact_knn_grouped("sq_euclid", x, q, 10, rg, qg, 7)
    two = _index("sq_euclid", x, set_devices=2)          # the primary context alone
    t = two.knn_query(q, 10)
    assert _same(two.exact_knn_query_grouped(q, 10, rg, qg, 7), want)
    assert _same(two.knn_query(q, 10), t)
    host = _index("sq_euclid", x, set_device_traversal=False)   # no host form: the scan still runs on the device
    host.reset_stats()
    assert _same(host.exact_knn_query_grouped(q, 10, rg, qg, 7), want)
    assert host.stats()["exact_launches"] == 1
    h0 = host.graph_hash()
    host.exact_knn_query_grouped(q, 10, rg, qg, 7)
    assert host.graph_hash() == h0
