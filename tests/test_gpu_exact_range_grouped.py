"""GPU tier: the grouped exact range call (hnsw_mi355x_exact_range_query_grouped / hnswdev_exact_range_grouped)
against its two references -- the model (tests/exact_range_grouped_model.py: exact_range_model one group at a time) and the product's
own loop of ungrouped calls with the group as the allow-set.  Every comparison is counts, ids and distance BYTES per query, in the
caller's order.  The radii come from the model's own distance matrix, and every test asserts from the model that its case is what it
is about (a list longer than the capacity, lengths on both sides of a limit, a tie at the boundary)."""
import ctypes as ct
import re

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_grouped_model import evals, group_mask, members
from exact_knn_model import distances
from exact_range_grouped_model import exact_range_grouped, from_matrix

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
N, NG = 600, 7
INF = float("inf")
EMPTY = {"calls": 0, "device_sorted": 0, "host_sorted": 0, "repeated_pieces": 0}


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
    ix.set_collection_size(2048); ix.set_min_nn(20); ix.set_max_edges(12)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    return ix


def _lib():
    import hnswindex
    return hnswindex.net_amd.lib


def _same(got, want):
    """counts, ids and distance bytes, query by query"""
    if len(got[0]) != len(want[0]) or len(got[1]) != len(want[1]):
        return False
    for gi, gd, wi, wd in zip(got[0], got[1], want[0], want[1]):
        if gi.shape != wi.shape or not (gi == wi).all() or np.asarray(gd, np.float32).tobytes() != wd.tobytes():
            return False
    return True


def _lens(want):
    return np.array([a.size for a in want[0]])


def _per_group_calls(call, q, radius, rg, qg, ng):
    """The parent's way: one ungrouped call per group that a query names, the group as its allow-set, the lists put back in the
    caller's order.  call(queries, radius, allowed=mask) is DeviceBackend.exact_range or Index.exact_range_query."""
    qg = np.asarray(qg)
    ids, d = [None] * qg.size, [None] * qg.size
    for g in np.unique(qg):
        sel = np.flatnonzero(qg == g)
        g_ids, g_d = call(q[sel], radius, allowed=group_mask(rg, int(g), ng))
        for j, i in enumerate(sel):
            ids[i], d[i] = g_ids[j], g_d[j]
    return ids, d


def _check(db, q, radius, rg, qg, ng, want, tag=None, product=True, pairs=None):
    """One grouped call on a backend: the model's answer, the per-group calls' answer, the pairs measured (None: not held)."""
    db.reset_stats()
    got = db.exact_range_grouped(q, radius, rg, qg, ng)
    st = db.stats()
    assert _same(got, want), tag
    assert st["search_launches"] == 0, (tag, st)
    if pairs is not None:
        assert st["exact_evals"] == pairs and st["exact_launches"] == (1 if pairs else 0), (tag, st, pairs)
    if product:
        assert _same(got, _per_group_calls(db.exact_range, q, radius, rg, qg, ng)), tag
    return got


def _base_groups():
    """Seven groups of unequal size over 600 ids: group 3 is one row, group 4 has no row; 55 queries in a scrambled order with the
    33 queries of group 0 around the single query of group 1, which sits in the middle of the caller's order."""
    rg = np.random.default_rng(7).choice([0, 2, 5, 6], N, p=[0.45, 0.3, 0.15, 0.1]).astype(np.int32)
    rg[300:340] = 1
    rg[77] = 3
    rg[100:110] = -1
    qg = np.concatenate([np.zeros(33, np.int32), [2] * 5, [3] * 3, [4] * 2, [5] * 7, [6] * 4]).astype(np.int32)
    qg = qg[np.random.default_rng(8).permutation(qg.size)]
    qg = np.concatenate([qg[:27], [1], qg[27:]]).astype(np.int32)
    return rg, qg


NQ = 55


def _in_group(d, rg, qg):
    """the model's distances of every (query, candidate of its group) pair, flattened and sorted"""
    return np.sort(np.concatenate([d[i, group_mask(rg, int(g), NG)[:N]] for i, g in enumerate(qg)]))


@pytest.fixture(scope="module")
def sets():
    """(x, q, backend, the model's distance matrix) per (metric, dim, grid): computed once, shared, never written."""
    cache = {}

    def get(metric, dim, grid=False):
        key = (metric, dim, grid)
        if key not in cache:
            x = _data(metric, N, dim, 2 if grid else 1, grid)
            q = _data(metric, NQ, dim, 102 if grid else 101, grid)
            d = distances(metric, x, q, np.arange(N, dtype=np.int32))
            for a in (x, q, d):
                a.setflags(write=False)
            cache[key] = (x, q, _backend(metric, x), d)
        return cache[key]
    return get


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("dim", [20, 21])
@pytest.mark.parametrize("metric", METRICS)
def test_the_base_case_is_the_model_and_the_per_group_calls(sets, metric, dim, grid):
    x, q, db, d = sets(metric, dim, grid)
    rg, qg = _base_groups()
    per = np.bincount(qg, minlength=NG)
    mem = members(N, rg, NG)
    assert per.tolist() == [33, 1, 5, 3, 2, 7, 4] and qg[27] == 1 and (np.diff(qg) < 0).any()
    assert mem[3] == 1 and mem[4] == 0 and len(set(mem.tolist())) == NG          # a one-row group, an empty one, all sizes unequal
    flat = _in_group(d, rg, qg)
    i0 = int(np.flatnonzero(qg == 0)[0])                                          # a query of the large group
    c0 = np.flatnonzero(rg == 0)
    pair_id = int(c0[np.lexsort((c0, d[i0, c0]))[4]])                             # ... and its 5th candidate: that pair is on the boundary
    radii = {"pair": float(d[i0, pair_id]), "below_all": float(np.nextafter(flat[0], np.float32(-np.inf))),
             "mean3": float(flat[3 * NQ - 1]), "mean50": float(flat[50 * NQ - 1]), "inf": INF, "nan": float("nan"), "negzero": -0.0}
    if grid:   # a value that several ids of query i0's group hold: all of them are in, in id order
        vals, cnts = np.unique(d[i0, c0], return_counts=True)
        assert cnts.max() >= 2, metric
        radii["tied"] = float(vals[np.argmax(cnts)])
    pairs = evals(N, rg, qg, NG)
    for name, radius in radii.items():
        want = from_matrix(d, radius, rg, qg, NG)
        got = _check(db, q, radius, rg, qg, NG, want, (metric, dim, grid, name), pairs=pairs)
        lens = _lens(want)
        info = db.exact_range_grouped_info()      # (read after _check's per-group calls: they do not count here)
        assert info == {"calls": 1, "device_sorted": int((lens >= 2).sum()), "host_sorted": 0, "repeated_pieces": 0}, (name, info)
        assert (lens[qg == 4] == 0).all() and not np.isin(np.arange(100, 110), np.concatenate(got[0])).any()
        # the preconditions, from the model
        if name == "pair":
            assert pair_id in want[0][i0].tolist() and want[1][i0][-1] == np.float32(radius)
        elif name in ("below_all", "nan"):
            assert lens.sum() == 0
        elif name.startswith("mean"):
            assert lens.mean() >= int(name[4:]) and (grid or lens.mean() <= int(name[4:]) + 1) and (lens == 0).any()
        elif name == "inf":
            assert (lens == mem[qg]).all() and (lens[qg == 3] == 1).all()
        elif name == "negzero":
            assert lens.sum() == 0 or (np.concatenate(want[1]) <= 0).all()
        elif name == "tied":
            tail = want[1][i0] == np.float32(radius)
            assert tail.sum() >= 2 and (np.diff(want[0][i0][tail]) > 0).all()
    # the model from the matrix is the model
    assert _same(from_matrix(d, radii["mean3"], rg, qg, NG), exact_range_grouped(metric, x, q, radii["mean3"], rg, qg, NG))


def test_a_negative_radius_is_an_ordinary_one():
    """ucosine distances of a row to itself round below zero: a negative radius admits exactly those, inside the query's group."""
    x = _data("ucosine", N, 20, 1)
    rg, _ = _base_groups()
    qi = np.r_[0:40, 300:310].astype(np.int32)               # the queries are rows, asked of their own group or of another
    q = x[qi]
    qg = rg[qi].clip(0).astype(np.int32)
    qg[5] = (qg[5] + 2) % 3                                  # this one's own row is not in the group it asks
    d = distances("ucosine", x, q, np.arange(N, dtype=np.int32))
    neg = _in_group(d, rg, qg)
    neg = neg[neg < 0]
    assert neg.size >= 2, "the data holds no negative distance inside a group"
    db = _backend("ucosine", x)
    for radius in (float(neg[-1]), float(neg[0]), -0.5):
        want = from_matrix(d, radius, rg, qg, NG)
        _check(db, q, radius, rg, qg, NG, want, radius)
    lens = _lens(from_matrix(d, float(neg[-1]), rg, qg, NG))
    assert lens.sum() == neg.size and (lens == 0).any() and (lens == 1).any()


BIG_N = 2000


@pytest.fixture(scope="module")
def big():
    """2 000 x 8 grid rows per metric in groups of 1 000 / 635 / 257 / 1 / 0 rows (107 in none), 40 queries; the distance matrix once."""
    cache = {}

    def get(metric):
        if metric not in cache:
            x, q = _data(metric, BIG_N, 8, 41, grid=True), _data(metric, 40, 8, 42, grid=True)
            rg = np.full(BIG_N, -1, np.int32)
            perm = np.random.default_rng(43).permutation(BIG_N)
            rg[perm[:1000]] = 0
            rg[perm[1000:1635]] = 1
            rg[perm[1635:1892]] = 2
            rg[perm[1892]] = 3
            qg = np.concatenate([[0] * 33, [1] * 3, [2] * 2, [3], [4]]).astype(np.int32)[np.random.default_rng(44).permutation(40)]
            d = distances(metric, x, q, np.arange(BIG_N, dtype=np.int32))
            for a in (x, q, rg, qg, d):
                a.setflags(write=False)
            cache[metric] = (x, q, rg, qg, d, _backend(metric, x))
        return cache[metric]
    return get


@pytest.mark.parametrize("metric", METRICS)
def test_forced_chunks_and_tiles_give_identical_bytes_and_shadows_add_nothing(monkeypatch, big, metric):
    """One-row chunks (every block shadows its row 127 times), chunks of 127 / 128 / 129 rows (a step short of, equal to and one row
    past the 128 rows of a step), tiles of 1, 3 and 5 queries (shadow queries in every tile but the first form).  At +inf every
    measured pair is a result, so a shadow that offered anything would show in a count."""
    x, q, rg, qg, d, db = big(metric)
    mem = members(BIG_N, rg, 5)
    want_inf = from_matrix(d, INF, rg, qg, 5)
    flat = np.sort(np.concatenate([d[i, rg == g] for i, g in enumerate(qg)]))
    mid = float(flat[flat.size // 20])
    want_mid = from_matrix(d, mid, rg, qg, 5)
    assert (_lens(want_inf) == mem[qg]).all() and 0 < _lens(want_mid).sum() < _lens(want_inf).sum()
    pairs = evals(BIG_N, rg, qg, 5)
    for chunk, qtile in ((1, 0), (127, 1), (128, 3), (129, 5), (1000, 0), (0, 1), (0, 0)):
        set_diag(monkeypatch, exact_chunk=chunk, exact_qtile=qtile)
        got = _check(db, q, INF, rg, qg, 5, want_inf, (metric, chunk, qtile), product=(chunk, qtile) == (0, 0), pairs=pairs)
        assert [a.size for a in got[0]] == mem[qg].tolist()                    # exactly the group's size: no shadow was counted
        _check(db, q, mid, rg, qg, 5, want_mid, (metric, chunk, qtile, "mid"), product=False, pairs=pairs)


def _rounds(caps, arena):
    """pass A's rounds as the contract states them: ranges of the caller's order whose capacities fit the arena"""
    n, keys = 1, 0
    for c in caps:
        if keys + c > arena and keys > 0:
            n, keys = n + 1, 0
        keys += c
    return n


def test_capacities_and_the_arena(monkeypatch, big):
    x, q, rg, qg, d, db = big("sq_euclid")
    mem = members(BIG_N, rg, 5)
    flat = np.sort(np.concatenate([d[i, rg == g] for i, g in enumerate(qg)]))
    radius = float(flat[flat.size // 10])
    want = from_matrix(d, radius, rg, qg, 5)
    lens = _lens(want)
    top = int(lens.max())
    assert top > 40 and (lens == top).sum() >= 1 and (lens < top - 1).sum() >= 10 and (lens == 0).any()
    pairs = evals(BIG_N, rg, qg, 5)
    # the largest list fits exactly: one pass
    set_diag(monkeypatch, exact_range_cap=top)
    _check(db, q, radius, rg, qg, 5, want, "cap=top", pairs=pairs)
    assert db.exact_range_grouped_info()["repeated_pieces"] == 0
    # one entry short: only the tiles of the queries with `top` results are scanned again; far short: most are
    for cap in (top - 1, 8):
        over = lens > np.minimum(cap, mem[qg])
        assert over.any() and not over.all()
        set_diag(monkeypatch, exact_range_cap=cap)
        db.reset_stats()
        got = db.exact_range_grouped(q, radius, rg, qg, 5)
        info, st = db.exact_range_grouped_info(), db.stats()
        assert _same(got, want), cap
        assert info["repeated_pieces"] == 1 and st["exact_launches"] == 2 and pairs < st["exact_evals"] <= 2 * pairs, (cap, info, st)
        assert info["device_sorted"] == (lens >= 2).sum() and info["host_sorted"] == 0, (cap, info)
    # (cap = top - 1: the queries of the groups whose tiles hold no such query are not measured a second time)
    set_diag(monkeypatch, exact_range_cap=top - 1, exact_qtile=1)
    db.reset_stats()
    assert _same(db.exact_range_grouped(q, radius, rg, qg, 5), want)
    assert db.stats()["exact_evals"] == pairs + int(mem[qg][lens == top].sum())
    # a small group costs a small segment: capacities are min(cap, members), so an arena of 2 100 keys holds groups 1 .. 4 whole
    # and two queries of group 0 per round
    set_diag(monkeypatch, exact_range_cap=0, exact_qtile=0, exact_range_arena=2100)
    caps = np.minimum(8192, mem[qg])
    db.reset_stats()
    assert _same(db.exact_range_grouped(q, radius, rg, qg, 5), want)
    n_rounds = _rounds(caps.tolist(), 2100)
    assert 10 <= n_rounds and db.exact_range_grouped_info()["repeated_pieces"] == 0
    assert db.stats()["exact_launches"] == n_rounds and db.stats()["exact_evals"] == pairs
    # pass B cut by the arena: 8 entries per query in pass A, then pieces whose exact counts fit 300 entries
    over8 = lens > np.minimum(8, mem[qg])
    assert top <= 300 < lens[over8].sum()
    set_diag(monkeypatch, exact_range_cap=8, exact_range_arena=300)
    db.reset_stats()
    assert _same(db.exact_range_grouped(q, radius, rg, qg, 5), want)
    assert db.exact_range_grouped_info()["repeated_pieces"] >= -(-int(lens[over8].sum()) // 300)
    # an arena below one query's count: an error that names the limit, nothing returned; the next call is answered
    set_diag(monkeypatch, exact_range_cap=0, exact_range_arena=top - 1)
    with pytest.raises(RuntimeError, match=rf"arena.*\b{top - 1}\b"):
        db.exact_range_grouped(q, radius, rg, qg, 5)
    counts = np.full(40, 5, np.int32)
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    qq = np.ascontiguousarray(q, np.float32)
    assert _lib().hnswdev_exact_range_grouped(db._ctx, qq.ctypes.data_as(F), 40, BIG_N, ct.c_float(radius), rg.ctypes.data_as(I), BIG_N,
                                              qg.ctypes.data_as(I), 5, counts.ctypes.data_as(I)) == -1
    assert (counts == 0).all()
    none_i, none_d = np.full(4, 77, np.int32), np.full(4, 77.0, np.float32)
    assert _lib().hnswdev_exact_range_results(db._ctx, none_i.ctypes.data_as(I), none_d.ctypes.data_as(F)) == 0 and (none_i == 77).all()   # nothing kept
    set_diag(monkeypatch, exact_range_arena=0)
    assert _same(db.exact_range_grouped(q, radius, rg, qg, 5), want)


def _line():
    """group 0: rows i * e0, i < 200, and queries p * e0 -- the squared distance is (i - p)^2 exactly, so a radius of 32^2 gives the
    query at p the rows of [p - 32, p + 32] that exist: list lengths by construction.  group 1: 70 rows at 1 000 + i, two queries
    (every value is a binary16 number)."""
    x = np.zeros((270, 8), np.float32)
    x[:200, 0] = np.arange(200)
    x[200:, 0] = 1000 + np.arange(70)
    rg = np.concatenate([np.zeros(200, np.int32), np.ones(70, np.int32)])
    q = np.zeros((10, 8), np.float32)
    q[:, 0] = [-100, -32, 1031, -31, 30, 31, 1000, 32, 100, 199]
    qg = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.int32)
    return x, q, rg, qg, float(32 * 32)


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_f16"])
def test_the_sort_limit_splits_the_lists_between_device_and_host(monkeypatch, metric):
    x, q, rg, qg, radius = _line()
    want = exact_range_grouped(metric, x, q, radius, rg, qg, 2)
    lens = _lens(want)
    assert lens.tolist() == [0, 1, 64, 2, 63, 64, 33, 65, 65, 33]
    assert any(w.size >= 2 and (np.diff(w) == 0).any() for w in want[1])     # equal distances inside the lists
    db = _backend(metric, x)
    for limit in (64, 0, 1, 2):
        set_diag(monkeypatch, exact_range_sort=limit)
        _check(db, q, radius, rg, qg, 2, want, (metric, limit), product=False)
        cut = limit if limit else 4096
        info = db.exact_range_grouped_info()
        assert info["device_sorted"] == ((lens >= 2) & (lens <= cut)).sum() and info["host_sorted"] == (lens > cut).sum(), (limit, info)
        if limit == 64:
            assert info["device_sorted"] == 6 and info["host_sorted"] == 2


def test_the_real_sort_limit():
    """4 096 keys are what the device orders in LDS; one more and the host does: groups of 4 096 and of 4 200 members at +inf"""
    n = 4096 + 4200
    x, q = uniform(n, 8, 61), uniform(9, 8, 62)
    rg = np.ones(n, np.int32)
    rg[np.random.default_rng(63).choice(n, 4096, replace=False)] = 0
    qg = np.array([0, 1, 1, 0, 0, 1, 0, 1, 0], np.int32)
    want = exact_range_grouped("sq_euclid", x, q, INF, rg, qg, 2)
    assert sorted(set(_lens(want).tolist())) == [4096, 4200]
    db = _backend("sq_euclid", x)
    _check(db, q, INF, rg, qg, 2, want, pairs=5 * 4096 + 4 * 4200)
    info = db.exact_range_grouped_info()
    assert info == {"calls": 1, "device_sorted": 5, "host_sorted": 4, "repeated_pieces": 0}, info


def test_row_group_edges(sets):
    x, q, db, d = sets("sq_euclid", 20, False)
    rg, qg = _base_groups()
    rg = rg.copy()
    rg[200:220] = NG                     # at n_groups
    rg[230:240] = -5
    rg[400] = np.iinfo(np.int32).max
    rg[401] = np.iinfo(np.int32).min
    radius = float(_in_group(d, rg, qg)[20 * NQ])
    want = from_matrix(d, radius, rg, qg, NG)
    got = _check(db, q, radius, rg, qg, NG, want, "values", pairs=evals(N, rg, qg, NG))
    assert not np.isin(np.r_[200:220, 230:240, 400, 401], np.concatenate(got[0])).any()
    assert np.isin(np.r_[200:220, 230:240], np.concatenate(from_matrix(d, radius, np.zeros(N, np.int32), np.zeros(NQ, np.int32), 1)[0])).any()
    # row_group shorter than the rows: ids past its end are in no group
    short = _check(db, q, radius, rg[:400], qg, NG, from_matrix(d, radius, rg[:400], qg, NG), "short", pairs=evals(400, rg, qg, NG))
    assert np.concatenate(short[0]).max() < 400 <= np.concatenate(got[0]).max()
    # ... and beyond them: clamped, a row that does not exist is never dereferenced
    wide = np.concatenate([rg, np.tile(np.arange(NG, dtype=np.int32), 1000)])
    _check(db, q, radius, wide, qg, NG, want, "wide", product=False, pairs=evals(N, rg, qg, NG))
    # n_rows below the uploaded rows
    assert _same(db.exact_range_grouped(q, radius, rg, qg, NG, n_rows=350), from_matrix(d[:, :350], radius, rg[:350], qg, NG))
    # the index layer clamps to Length in the same way
    ix = _index("sq_euclid", x)
    for arr in (rg, rg[:400], wide):
        assert _same(ix.exact_range_query_grouped(q, radius, arr, qg, NG), from_matrix(d, radius, arr[:N], qg, NG))
    # no id in any group that a query names: empty lists and no scan
    db.reset_stats()
    got = db.exact_range_grouped(q, INF, np.full(N, -1, np.int32), qg, NG)
    assert len(got[0]) == NQ and all(a.size == 0 for a in got[0]) and all(a.size == 0 for a in got[1])
    assert db.stats()["exact_launches"] == 0 and db.exact_range_grouped_info() == EMPTY     # a call that scans nothing counts nowhere
    got = db.exact_range_grouped(q, INF, np.zeros(0, np.int32), qg, NG)
    assert all(a.size == 0 for a in got[0])


def test_a_single_group_and_the_cap_on_groups(sets):
    x, q, db, d = sets("sq_euclid", 20, False)
    rg, qg = _base_groups()
    radius = float(_in_group(d, rg, qg)[20 * NQ])
    ix = _index("sq_euclid", x)
    zeros_r, zeros_q = np.zeros(N, np.int32), np.zeros(NQ, np.int32)
    for r in (radius, INF):              # one group: the call without a set
        assert _same(db.exact_range_grouped(q, r, zeros_r, zeros_q, 1), db.exact_range(q, r))
        assert _same(ix.exact_range_query_grouped(q, r, zeros_r, zeros_q, 1), ix.exact_range_query(q, r))
    want = from_matrix(d, radius, rg, qg, NG)
    assert _lens(want).sum() > 0
    assert _same(db.exact_range_grouped(q, radius, rg, qg, 65536), want)          # the largest number of groups is accepted
    top = rg.copy()
    top[rg == 6] = 65535
    assert _same(db.exact_range_grouped(q, radius, top, np.where(qg == 6, 65535, qg).astype(np.int32), 65536), want)
    assert _same(ix.exact_range_query_grouped(q, radius, rg, qg, 65536), want)
    assert _same(ix.exact_range_query_grouped(q, radius, rg, qg), want)           # n_groups worked out from the arrays
    for call in (db.exact_range_grouped, ix.exact_range_query_grouped):
        for bad in (65537, 0, -1):
            with pytest.raises(RuntimeError, match="65536"):
                call(q, radius, rg, zeros_q, bad)


def test_a_row_group_of_more_than_4_mib():
    """1.1M ids are 4.4 MB of row_group: above 4 MiB the array goes up in pieces, not through the one pinned stage.  Two small groups
    whose members lie in every piece, the last id included; everything else in no group."""
    n = 1_100_000
    x, q = uniform(n, 4, 55), uniform(6, 4, 56)
    rg = np.full(n, -1, np.int32)
    picks = np.random.default_rng(57).choice(n - 1, 600, replace=False)
    rg[picks[:500]] = 0
    rg[picks[500:]] = 3
    rg[n - 1] = 3
    qg = np.array([3, 0, 0, 3, 1, 0], np.int32)      # group 1 is empty
    assert rg.nbytes > 4 << 20
    db = _backend("sq_euclid", x)
    want = exact_range_grouped("sq_euclid", x, q, 0.25, rg, qg, 4)
    assert 0 < _lens(want)[0] < 101 and _lens(want)[4] == 0 and _lens(want).sum() > 50
    _check(db, q, 0.25, rg, qg, 4, want, product=False, pairs=2 * 101 + 3 * 500)
    got = _check(db, q, INF, rg, qg, 4, exact_range_grouped("sq_euclid", x, q, INF, rg, qg, 4), product=False)
    assert n - 1 in got[0][0].tolist() and [a.size for a in got[0]] == [101, 500, 500, 101, 0, 500]
    db.set_profiling(True)                           # the list-building kernels' event time is kept apart from the scan's
    db.reset_stats()
    db.exact_range_grouped(q, 0.25, rg, qg, 4)
    st, ms = db.stats(), db.exact_grouped_list_ms()
    db.set_profiling(False)
    assert ms > 0.0 and st["exact_kernel_ms"] > 0.0 and st["exact_timed_launches"] == 1


def test_nan_and_inf_rows_and_f16_overflow():
    n = 200
    x = uniform(n, 16, 71).copy()
    x[5, 2] = np.nan
    x[9, 3] = np.inf
    x[151, 0] = np.nan
    x[8, 1] = np.nan                      # in the other group
    q = uniform(4, 16, 72)
    rg = (np.arange(n) % 2).astype(np.int32)     # 5, 9, 151 are in group 1
    qg = np.array([1, 0, 1, 1], np.int32)
    db = _backend("sq_euclid", x)
    want = exact_range_grouped("sq_euclid", x, q, INF, rg, qg, 2)
    assert [w.size for w in want[0]] == [98, 99, 98, 98] and all(want[0][i][-1] == 9 and np.isinf(want[1][i][-1]) for i in (0, 2, 3))   # +inf is in, last; a NaN never
    got = _check(db, q, INF, rg, qg, 2, want)
    assert not np.isin([5, 8, 151], np.concatenate(got[0])).any()
    big = float(np.finfo(np.float32).max)
    want = exact_range_grouped("sq_euclid", x, q, big, rg, qg, 2)
    assert [w.size for w in want[0]] == [97, 99, 97, 97]
    _check(db, q, big, rg, qg, 2, want)
    assert all(a.size == 0 for a in db.exact_range_grouped(q, float("nan"), rg, qg, 2)[0])
    y = uniform(120, 24, 43).copy()
    y[7, 1] = 1e6            # beyond binary16: stored as +inf
    y[30, 23] = -7e4
    qy = uniform(5, 24, 44)
    rgy = (np.arange(120) % 3 == 1).astype(np.int32)          # 7 is in group 1, 30 in group 0
    qgy = np.array([1, 0, 1, 0, 1], np.int32)
    for metric in ("sq_euclid_f16", "ucosine_f16"):
        want = exact_range_grouped(metric, y, qy, INF, rgy, qgy, 2)
        if metric == "sq_euclid_f16":
            assert want[0][0][-1] == 7 and want[0][1][-1] == 30 and np.isinf(want[1][0][-1]) and np.isinf(want[1][1][-1])
        _check(_backend(metric, y), qy, INF, rgy, qgy, 2, want, metric)


def test_removals_and_slot_reuse():
    n, dim = 1500, 16
    x = uniform(n, dim, 81).copy()
    q = uniform(12, dim, 82)
    rg = (np.arange(n) % 7).astype(np.int32)
    rg[rg == 5] = 2
    rg[100:110] = -1
    qg = (np.arange(12) % 7).astype(np.int32)[::-1].copy()
    ix = _index("sq_euclid", x)
    d = distances("sq_euclid", x, q, np.arange(n, dtype=np.int32))
    radius = float(np.sort(d, axis=None)[12 * 300])
    assert _same(ix.exact_range_query_grouped(q, radius, rg, qg, 7), from_matrix(d, radius, rg, qg, 7))
    rng = np.random.default_rng(83)
    gone = np.unique(np.concatenate([[ix.entry_point], rng.choice(n, 99, replace=False)])).astype(np.int32)
    assert np.isin(gone, np.concatenate(from_matrix(d, radius, rg, qg, 7)[0])).any()    # a removed id would have been in
    before = rg.copy()
    ix.remove(gone)
    live = np.sort(ix.ids())
    for r in (radius, INF):
        ix.reset_stats()
        got = ix.exact_range_query_grouped(q, r, rg, qg, 7)
        assert not np.isin(np.concatenate(got[0]), gone).any()
        assert _same(got, from_matrix(d, r, rg, qg, 7, live=live)), r
        assert ix.stats()["exact_evals"] == evals(n, rg, qg, 7, live=live)
        assert _same(got, _per_group_calls(ix.exact_range_query, q, r, rg, qg, 7)), r
    assert (rg == before).all()                  # the caller's array is not written
    # labels on vacant slots only: no candidate, no scan
    only_gone = np.full(n, -1, np.int32)
    only_gone[gone] = 0
    ix.reset_stats()
    got = ix.exact_range_query_grouped(q, INF, only_gone, np.zeros(12, np.int32), 1)
    assert all(a.size == 0 for a in got[0]) and ix.stats()["exact_launches"] == 0
    fresh = uniform(50, dim, 84)
    new_ids = ix.add(fresh)
    assert np.isin(new_ids, gone).all()          # vacated slots are reused
    x[new_ids] = fresh
    live = np.sort(ix.ids())
    q2, qg2 = np.concatenate([q, fresh[:3]]), np.concatenate([qg, rg[new_ids[:3]].clip(0)]).astype(np.int32)
    got = ix.exact_range_query_grouped(q2, radius, rg, qg2, 7)
    assert _same(got, exact_range_grouped("sq_euclid", x, q2, radius, rg, qg2, 7, live=live))
    for j in range(3):                           # a re-added id is returned, with its new row: distance 0 to itself
        if rg[new_ids[j]] >= 0:
            assert got[0][12 + j][0] == new_ids[j] and got[1][12 + j][0] == 0.0


def _raw_index_call(ix, q, radius, rg, n_rg, qg, ng):
    """hnsw_mi355x_exact_range_query_grouped through ctypes, as a host that is not the Python class calls it: the arrays are left allocated"""
    q = np.ascontiguousarray(q, np.float32)
    n = q.shape[0]
    I = ct.POINTER(ct.c_int)
    pp_i, pp_d = (ct.c_void_p * n)(*([0x1234] * n)), (ct.c_void_p * n)(*([0x1234] * n))
    counts = np.full(n, 77, np.int32)
    rc = _lib().hnsw_mi355x_exact_range_query_grouped(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), n, q.shape[1], ct.c_float(radius),
                                                      None if rg is None else rg.ctypes.data_as(I), n_rg, None if qg is None else qg.ctypes.data_as(I), ng,
                                                      pp_i, pp_d, counts.ctypes.data_as(I))
    return rc, pp_i, pp_d, counts


def test_the_c_calls_allocate_free_and_fail_as_the_ungrouped_ones(monkeypatch, sets):
    import hnswindex
    lib = _lib()
    x, q, db, d = sets("sq_euclid", 20, False)
    rg, qg = _base_groups()
    ix = _index("sq_euclid", x)
    radius = float(_in_group(d, rg, qg)[3 * NQ])
    want = from_matrix(d, radius, rg, qg, NG)
    lens = _lens(want)
    assert (lens == 0).any() and lens.sum() > 0
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q, radius, rg, N, qg, NG)
    assert rc == 0 and counts.tolist() == lens.tolist()
    for i in range(NQ):
        if lens[i] == 0:
            assert pp_i[i] is None and pp_d[i] is None                    # NULL where the count is 0
        else:
            got_i = np.ctypeslib.as_array(ct.cast(pp_i[i], ct.POINTER(ct.c_int)), shape=(int(lens[i]),))
            got_d = np.ctypeslib.as_array(ct.cast(pp_d[i], ct.POINTER(ct.c_float)), shape=(int(lens[i]),))
            assert (got_i == want[0][i]).all() and got_d.tobytes() == want[1][i].tobytes()
    lib.hnsw_free_results(pp_i, pp_d, NQ)
    assert all(p is None for p in pp_i) and all(p is None for p in pp_d)  # released and cleared
    # argument errors: -1 with a message, every pointer NULL, every count 0
    bad = qg.copy()
    bad[41] = NG
    bad[50] = -1
    for args, word in (((rg, N, bad, NG), r"query_group\[41\]"), ((None, N, qg, NG), "row_group"), ((rg, -1, qg, NG), "n_row_group"),
                       ((rg, N, qg, 65537), "65536"), ((rg, N, None, NG), "ArgumentNullException")):
        rc, pp_i, pp_d, counts = _raw_index_call(ix, q, radius, *args)
        assert rc == -1 and all(p is None for p in pp_i) and all(p is None for p in pp_d) and (counts == 0).all(), word
        assert re.search(word, hnswindex.net_amd.last_error()), (word, hnswindex.net_amd.last_error())
    # ... a device-side failure (an arena below a list) leaves the same
    set_diag(monkeypatch, exact_range_arena=10)
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q, INF, rg, N, qg, NG)
    set_diag(monkeypatch, exact_range_arena=0)
    assert rc == -1 and all(p is None for p in pp_i) and all(p is None for p in pp_d) and (counts == 0).all()
    assert "arena" in hnswindex.net_amd.last_error()
    # the inner call: the same rules, the counts zeroed
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    qq = np.ascontiguousarray(q, np.float32)
    for args, word in (((rg.ctypes.data_as(I), N, bad.ctypes.data_as(I), NG), r"query_group\[41\]"), ((None, N, qg.ctypes.data_as(I), NG), "row_group"),
                       ((rg.ctypes.data_as(I), -1, qg.ctypes.data_as(I), NG), "n_row_group"), ((rg.ctypes.data_as(I), N, qg.ctypes.data_as(I), 0), "65536"),
                       ((rg.ctypes.data_as(I), N, None, NG), "query_group")):
        counts = np.full(NQ, 5, np.int32)
        assert lib.hnswdev_exact_range_grouped(db._ctx, qq.ctypes.data_as(F), NQ, N, ct.c_float(radius), *args, counts.ctypes.data_as(I)) == -1, word
        assert (counts == 0).all() and re.search(word, db.last_error()), (word, db.last_error())
    with pytest.raises(RuntimeError, match=r"query_group\[41\]"):
        ix.exact_range_query_grouped(q, radius, rg, bad, NG)
    # the counters of both layers, and their reset
    ix.reset_stats()
    ix.exact_range_query_grouped(q, radius, rg, qg, NG)
    info = (ct.c_uint64 * 4)()
    assert lib.hnsw_mi355x_exact_range_grouped_info(ix._h, info) == 0
    assert list(info) == [ix.exact_range_grouped_info()[k] for k in ("calls", "device_sorted", "host_sorted", "repeated_pieces")] == [1, int((lens >= 2).sum()), 0, 0]
    ix.reset_stats()
    assert ix.exact_range_grouped_info() == EMPTY


def test_the_resident_query_set_and_pending_range_results_are_not_touched(sets):
    lib = _lib()
    x, q, _, d = sets("sq_euclid", 20, False)
    rg, qg = _base_groups()
    radius = float(_in_group(d, rg, qg)[20 * NQ])
    ix = _index("sq_euclid", x)
    ix.set_resident_queries(q[:20])
    before = ix.knn_query_resident(10)
    other = uniform(33, 20, 91)
    og = (np.arange(33) % NG).astype(np.int32)
    assert _same(ix.exact_range_query_grouped(other, radius, rg, og, NG), exact_range_grouped("sq_euclid", x, other, radius, rg, og, NG))
    ix.exact_range_query_grouped(other[:5], radius, np.full(N, -1, np.int32), og[:5], NG)      # the no-scan path
    assert lib.hnsw_mi355x_resident_count(ix._h) == 20
    after = ix.knn_query_resident(10)
    assert (after[0] == before[0]).all() and after[1].tobytes() == before[1].tobytes()
    # the inner boundary, where the cached query norms (cosine) and the quantised records (int8) must survive and be gathered too
    for metric in ("cosine", "sq_euclid_i8"):
        xm, qm, _, dm = sets(metric, 20, False)
        r_m = float(_in_group(dm, rg, qg)[20 * NQ])
        fresh = _backend(metric, xm)
        fresh.set_queries(qm[:40])
        cand = np.arange(50, dtype=np.int32)
        off = np.arange(41, dtype=np.int32) * 50
        kept = fresh.dist_query_batch(None, off, np.tile(cand, 40))
        fresh.exact_range_grouped(other, r_m, rg, og, NG)
        assert fresh.dist_query_batch(None, off, np.tile(cand, 40)).tobytes() == kept.tobytes()
        # queries == NULL: the resident set is the query set, gathered into the call's order on the device
        res = fresh.exact_range_grouped(None, r_m, rg, qg[:40], NG)
        want = from_matrix(dm[:40], r_m, rg, qg[:40], NG)
        assert _lens(want).sum() > 100 and _same(res, want), metric
        assert fresh.dist_query_batch(None, off, np.tile(cand, 40)).tobytes() == kept.tobytes()
        with pytest.raises(RuntimeError, match="resident"):
            fresh.exact_range_grouped(None, r_m, rg, qg[:41], NG)
    # a traversal's results wait in the context while a grouped exact range call comes and goes
    lv = ix.levels()
    dev = _backend("sq_euclid", x)
    dev.set_graph(lv, [ix.export_edges(L, 26 if L == 0 else 14) for L in range(int(lv.max()) + 1)], 12)
    qq = np.ascontiguousarray(q[:9], np.float32)
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    t_counts, t_flags = np.zeros(9, np.int32), np.zeros(9, np.int32)
    t_radius = float(np.sort(d[:9], axis=None)[9 * 8])
    assert lib.hnswdev_range_search(dev._ctx, qq.ctypes.data_as(F), 9, int(ix.entry_point), ct.c_float(t_radius), t_counts.ctypes.data_as(I),
                                    t_flags.ctypes.data_as(I)) == 0
    assert t_counts.sum() > 0
    assert _same(dev.exact_range_grouped(other, radius, rg, og, NG), exact_range_grouped("sq_euclid", x, other, radius, rg, og, NG))
    t_i, t_d = np.empty(t_counts.sum(), np.int32), np.empty(t_counts.sum(), np.float32)
    assert lib.hnswdev_range_results(dev._ctx, t_i.ctypes.data_as(I), t_d.ctypes.data_as(F)) == 0
    again = dev.range_search(q[:9], int(ix.entry_point), t_radius)
    assert (t_i == np.concatenate(again[0])).all() and t_d.tobytes() == np.concatenate(again[1]).tobytes()


def test_other_contexts_and_the_host_traversal_setting(sets):
    x, q, _, d = sets("sq_euclid", 20, False)
    rg, qg = _base_groups()
    radius = float(_in_group(d, rg, qg)[20 * NQ])
    want = from_matrix(d, radius, rg, qg, NG)
    two = _index("sq_euclid", x, set_devices=2)          # the primary context alone
    t = two.knn_query(q, 10)
    assert _same(two.exact_range_query_grouped(q, radius, rg, qg, NG), want)
    t2 = two.knn_query(q, 10)
    assert (t[0] == t2[0]).all() and t[1].tobytes() == t2[1].tobytes()
    assert two.stats_at(0)["exact_launches"] == 1 and two.stats_at(1)["exact_launches"] == 0
    host = _index("sq_euclid", x, set_device_traversal=False)   # no host form: the scan still runs on the device
    host.reset_stats()
    h0 = host.graph_hash()
    assert _same(host.exact_range_query_grouped(q, radius, rg, qg, NG), want)
    assert host.stats()["exact_launches"] == 1 and host.graph_hash() == h0
