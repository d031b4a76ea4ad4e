"""GPU tier: the tagged exact range call (hnsw_mi355x_exact_range_query_tagged / hnswdev_exact_range_tagged)
against its two references -- the model (tests/tagged_range_model.py: exact_range_model one mask at a time, here from a distance
matrix computed once) and the product's own loop of unfiltered-scan calls with the mask's ids as the allow-set -- in both modes.
Every comparison is counts, ids and distance BYTES per query, in the caller's order.  The radii come from the model's own distance
matrix, and every test asserts from the model that its case is what it is about (the batches a cap makes, a list longer than the
capacity, lengths on both sides of a limit)."""
import ctypes as ct
import re

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_knn_model import distances
from exact_range_model import within
from tagged_range_model import exact_range_tagged, tag_mask

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
MODES = ("any", "all")
N = 600
N_TAGS = N - 50                      # row_tags is shorter than the rows: the last 50 ids carry no tag
B31 = 0x80000000
MASKS = np.array([1, 2, 4, 8, 16, 32, B31, 0b101, 0b11, B31 | 1, 0xFFFFFFFF, 0, 1 | 1 << 4], np.uint32)   # 16: on no row; 32: on one
NQ = 4 * MASKS.size
INF = float("inf")
EMPTY = {"calls": 0, "masks": 0, "scanned": 0, "skipped": 0, "ids_listed": 0, "batches": 0, "device_sorted": 0, "host_sorted": 0, "repeated_pieces": 0}


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _tags(seed, n_tags=N_TAGS):
    rng = np.random.default_rng(seed)
    rt = np.zeros(n_tags, np.uint32)
    for bit, share in ((0, 0.6), (1, 0.3), (2, 0.1), (31, 0.05)):
        rt |= np.where(rng.random(n_tags) < share, np.uint32(1 << bit), np.uint32(0)).astype(np.uint32)
    picked = rng.choice(n_tags, 7 + 40 + 1, replace=False)
    rt[picked[:7]] |= np.uint32(8)
    rt[picked[7:47]] = 0
    rt[picked[47]] |= np.uint32(32)
    return rt


def _query_tags(nq, seed):
    """The masks shuffled over the batch: the queries of any two masks are interleaved in the caller's order."""
    return MASKS[np.random.default_rng(seed).permutation(np.arange(nq) % MASKS.size)]


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


def from_matrix(d, radius, rt, qt, match, live=None):
    """The model from a distance matrix d[nq, n] computed once: per query the ids of its mask (of `live`) within the radius."""
    n = d.shape[1]
    out = []
    for i in range(d.shape[0]):
        keep = tag_mask(rt, int(qt[i]), match, n)
        if live is not None:
            keep &= np.isin(np.arange(n), live)
        ids = np.flatnonzero(keep).astype(np.int32)
        out.append(within(d[i, ids], ids, radius))
    return [o[0] for o in out], [o[1] for o in out]


def _per_mask_calls(call, q, radius, rt, qt, match, n):
    """The loop the call replaces: one call per distinct mask, the mask's ids as its allow-set, the lists put back in the caller's
    order.  call(queries, radius, allowed=mask) is DeviceBackend.exact_range or Index.exact_range_query."""
    ids, d = [None] * qt.size, [None] * qt.size
    for m in np.unique(qt):
        sel = np.flatnonzero(qt == m)
        g_ids, g_d = call(q[sel], radius, allowed=tag_mask(rt, int(m), match, n))
        for j, i in enumerate(sel):
            ids[i], d[i] = g_ids[j], g_d[j]
    return ids, d


def _counts(rt, qt, match, n=N):
    """Per distinct mask in the order it first appears: its candidates; and the queries of masks without one."""
    first = [int(m) for m in dict.fromkeys(qt.tolist())]
    cnt = [int(tag_mask(rt, m, match, n).sum()) for m in first]
    none = np.array([not tag_mask(rt, int(m), match, n).any() for m in qt])
    return cnt, none


def _batches(cnt, cap):
    """(batches scanned, ids listed) as the call documents them: masks in the order they first appear, a batch closed when the
    next list would take it past `cap`; a batch whose lists are all empty is not scanned."""
    out, i = 0, 0
    while i < len(cnt):
        total, j = cnt[i], i + 1
        while j < len(cnt) and total + cnt[j] <= cap:
            total += cnt[j]
            j += 1
        out += total > 0
        i = j
    return out, sum(cnt)


def _check(db, q, radius, rt, qt, match, want, tag=None, product=True, n=N):
    db.reset_stats()
    got = db.exact_range_tagged(q, radius, rt, qt, match)
    st = db.stats()
    assert _same(got, want), tag
    assert st["search_launches"] == 0, (tag, st)
    info = db.exact_range_tagged_info()
    if product:
        assert _same(got, _per_mask_calls(db.exact_range, q, radius, rt, qt, match, n)), tag
    return got, info


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


def _in_mask(d, rt, qt, match):
    """the model's distances of every (query, candidate of its mask) pair, flattened and sorted"""
    return np.sort(np.concatenate([d[i, tag_mask(rt, int(m), match, d.shape[1])] for i, m in enumerate(qt)]))


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("dim", [20, 21])
@pytest.mark.parametrize("metric", METRICS)
def test_the_base_case_is_the_model_and_the_per_mask_calls(sets, metric, dim, grid):
    x, q, db, d = sets(metric, dim, grid)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    assert all((qt == m).sum() == 4 for m in MASKS) and ((rt & 32) != 0).sum() == 1 and ((rt & 16) != 0).sum() == 0 and (rt == 0).sum() >= 40
    for match in MODES:
        cnt, none = _counts(rt, qt, match)
        flat = _in_mask(d, rt, qt, match)
        radii = {"below_all": float(np.nextafter(flat[0], np.float32(-np.inf))), "mean3": float(flat[3 * NQ - 1]), "mean30": float(flat[30 * NQ - 1]),
                 "inf": INF, "nan": float("nan"), "negzero": -0.0, "negative": -0.5}
        for name, radius in radii.items():
            want = from_matrix(d, radius, rt, qt, match)
            got, info = _check(db, q, radius, rt, qt, match, want, (metric, dim, grid, match, name))
            lens = _lens(want)
            assert info == {"calls": 1, "masks": MASKS.size, "scanned": NQ - int(none.sum()), "skipped": int(none.sum()), "ids_listed": sum(cnt), "batches": 1,
                            "device_sorted": int((lens >= 2).sum()), "host_sorted": 0, "repeated_pieces": 0}, (name, info)
            assert (lens[none] == 0).all() and (lens.sum() == 0 or np.concatenate(got[0]).max() < N_TAGS)
            # the preconditions, from the model
            if name in ("below_all", "nan"):
                assert lens.sum() == 0
            elif name.startswith("mean"):
                assert lens.mean() >= int(name[4:]) and (grid or lens.mean() <= int(name[4:]) + 1) and (lens == 0).any()
            elif name == "inf":
                assert lens.tolist() == [int(tag_mask(rt, int(m), match, N).sum()) for m in qt] and (lens[qt == 32] == 1).all()   # a mask with one candidate
            elif name in ("negzero", "negative"):
                assert lens.sum() == 0 or (np.concatenate(want[1]) <= 0).all()
        # the model from the matrix is the model
        assert _same(from_matrix(d, radii["mean3"], rt, qt, match), exact_range_tagged(metric, x, q, radii["mean3"], rt, qt, match))
    single = np.isin(qt, [1, 2, 4, 8, 32, B31])
    a, b = from_matrix(d, INF, rt, qt, "any"), from_matrix(d, INF, rt, qt, "all")
    assert all(a[0][i].tolist() == b[0][i].tolist() for i in np.flatnonzero(single)) and _lens(b)[~single].sum() < _lens(a)[~single].sum()


def test_a_negative_radius_is_an_ordinary_one():
    """ucosine distances of a row to itself round below zero: a negative radius admits exactly those, inside the query's mask."""
    x = _data("ucosine", N, 20, 1)
    rt = _tags(3)
    qi = np.arange(60, dtype=np.int32)                       # the queries are rows, asked for a tag of their own or for another
    q = x[qi]
    qt = np.where(rt[qi] != 0, rt[qi] & (~rt[qi] + np.uint32(1)), np.uint32(1)).astype(np.uint32)   # the row's lowest tag
    qt[5] = 16                                               # this one's own row does not match
    d = distances("ucosine", x, q, np.arange(N, dtype=np.int32))
    neg = _in_mask(d, rt, qt, "any")
    neg = neg[neg < 0]
    assert neg.size >= 2, "the data holds no negative distance inside a mask"
    db = _backend("ucosine", x)
    for radius in (float(neg[-1]), float(neg[0]), -0.5):
        _check(db, q, radius, rt, qt, "any", from_matrix(d, radius, rt, qt, "any"), radius)
    lens = _lens(from_matrix(d, float(neg[-1]), rt, qt, "any"))
    assert lens.sum() == neg.size and (lens == 0).any() and (lens == 1).any()


@pytest.mark.parametrize("match", MODES)
def test_batches_of_masks_keep_the_callers_order(monkeypatch, sets, match):
    """tag_list_cap below one list's length (that mask is a batch alone), just above the longest (batches of several masks) and 1
    (every mask with a candidate alone).  The masks are shuffled over the queries, so the queries of different batches alternate in
    the caller's order: lists concatenated batch by batch would come back in the wrong places."""
    x, q, db, d = sets("sq_euclid", 20, False)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    cnt, none = _counts(rt, qt, match)
    radius = float(_in_mask(d, rt, qt, match)[30 * NQ])
    want = from_matrix(d, radius, rt, qt, match)
    lens = _lens(want)
    longest = max(cnt)
    assert longest > 100 and sorted(cnt)[-2] < longest and (lens > 0).sum() > NQ // 3
    assert (np.diff(np.array([list(dict.fromkeys(qt.tolist())).index(int(m)) for m in qt])) < 0).sum() > 10   # interleaved
    for cap in (longest - 1, longest + 1, 1, 0):
        set_diag(monkeypatch, tag_list_cap=cap)
        n_batches, listed = _batches(cnt, cap if cap else 1 << 28)
        got, info = _check(db, q, radius, rt, qt, match, want, (match, cap), product=cap == 0)
        assert info["batches"] == n_batches and info["ids_listed"] == listed and info["scanned"] == NQ - none.sum(), (cap, info)
        assert info["device_sorted"] == (lens >= 2).sum() and info["host_sorted"] == 0, (cap, info)
        if cap == 1:
            assert n_batches == sum(c > 0 for c in cnt) >= 5
        elif cap == longest + 1:
            assert 1 < n_batches < sum(c > 0 for c in cnt)
        elif cap == 0:
            assert n_batches == 1
    # the index layer runs the same batches
    ix = _index("sq_euclid", x)
    set_diag(monkeypatch, tag_list_cap=longest + 1)
    ix.reset_stats()
    assert _same(ix.exact_range_query_tagged(q, radius, rt, qt, match), want)
    assert ix.exact_range_tagged_info()["batches"] == _batches(cnt, longest + 1)[0]


def test_capacities_and_the_arena(monkeypatch, sets):
    x, q, db, d = sets("sq_euclid", 20, True)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    match = "any"
    cnt, none = _counts(rt, qt, match)
    mem = np.array([int(tag_mask(rt, int(m), match, N).sum()) for m in qt])
    radius = float(_in_mask(d, rt, qt, match)[40 * NQ])
    want = from_matrix(d, radius, rt, qt, match)
    lens = _lens(want)
    top = int(lens.max())
    assert top > 40 and (lens < top - 1).sum() >= 10 and (lens == 0).any()
    # the largest list fits exactly: one pass
    set_diag(monkeypatch, exact_range_cap=top)
    _, info = _check(db, q, radius, rt, qt, match, want, "cap=top")
    assert info["repeated_pieces"] == 0
    # one entry short, and far short: pass B
    for cap in (top - 1, 8):
        over = lens > np.minimum(cap, mem)
        assert over.any() and not over.all()
        set_diag(monkeypatch, exact_range_cap=cap)
        got, info = _check(db, q, radius, rt, qt, match, want, cap, product=False)
        assert info["repeated_pieces"] == 1 and db.stats()["exact_launches"] == 2, (cap, info)
        assert info["device_sorted"] == (lens >= 2).sum() and info["host_sorted"] == 0, (cap, info)
    # ... in every batch that holds such a query
    set_diag(monkeypatch, exact_range_cap=8, tag_list_cap=1)
    _, info = _check(db, q, radius, rt, qt, match, want, "cap 8, a batch per mask", product=False)
    first = [int(m) for m in dict.fromkeys(qt.tolist())]
    assert info["repeated_pieces"] == sum(int((lens[qt == m] > min(8, c)).any()) for m, c in zip(first, cnt)) >= 3, info
    # a small arena: a query's pass-A capacity is bounded by its mask's candidate count, rounds follow the caller's order
    set_diag(monkeypatch, exact_range_cap=0, tag_list_cap=0, exact_range_arena=2100)
    _, info = _check(db, q, radius, rt, qt, match, want, "arena 2100", product=False)
    assert info["repeated_pieces"] == 0 and db.stats()["exact_launches"] >= -(-int(np.minimum(8192, mem).sum()) // 2100)
    # pass B cut by the arena
    over8 = lens > np.minimum(8, mem)
    assert top <= 300 < lens[over8].sum()
    set_diag(monkeypatch, exact_range_cap=8, exact_range_arena=300)
    _, info = _check(db, q, radius, rt, qt, match, want, "arena 300", product=False)
    assert info["repeated_pieces"] >= -(-int(lens[over8].sum()) // 300)
    # an arena below one query's count: an error that names the limit, nothing returned; the next call is answered
    set_diag(monkeypatch, exact_range_cap=0, exact_range_arena=top - 1)
    with pytest.raises(RuntimeError, match=rf"arena.*\b{top - 1}\b"):
        db.exact_range_tagged(q, radius, rt, qt, match)
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    counts = np.full(NQ, 5, np.int32)
    qq = np.ascontiguousarray(q, np.float32)
    assert _lib().hnswdev_exact_range_tagged(db._ctx, qq.ctypes.data_as(F), NQ, N, ct.c_float(radius), rt.ctypes.data_as(U), N_TAGS, qt.ctypes.data_as(U), 0,
                                             counts.ctypes.data_as(I)) == -1
    assert (counts == 0).all()
    none_i, none_d = np.full(4, 77, np.int32), np.full(4, 77.0, np.float32)
    assert _lib().hnswdev_exact_range_results(db._ctx, none_i.ctypes.data_as(I), none_d.ctypes.data_as(F)) == 0 and (none_i == 77).all()   # nothing kept
    set_diag(monkeypatch, exact_range_arena=0)
    assert _same(db.exact_range_tagged(q, radius, rt, qt, match), want)


def _line():
    """tag 1: rows i * e0, i < 200, and queries p * e0 -- the squared distance is (i - p)^2 exactly, so a radius of 32^2 gives the
    query at p the rows of [p - 32, p + 32] that exist: list lengths by construction.  tag 2: 70 rows at 1 000 + i, two queries.
    Both carry bit 31, which no mask names."""
    x = np.zeros((270, 8), np.float32)
    x[:200, 0] = np.arange(200)
    x[200:, 0] = 1000 + np.arange(70)
    rt = np.concatenate([np.full(200, B31 | 1, np.uint32), np.full(70, B31 | 2, np.uint32)])
    q = np.zeros((10, 8), np.float32)
    q[:, 0] = [-100, -32, 1031, -31, 30, 31, 1000, 32, 100, 199]
    qt = np.array([1, 1, 2, 1, 1, 1, 2, 1, 1, 1], np.uint32)
    return x, q, rt, qt, float(32 * 32)


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_f16"])
def test_the_sort_limit_splits_the_lists_between_device_and_host(monkeypatch, metric):
    x, q, rt, qt, radius = _line()
    want = exact_range_tagged(metric, x, q, radius, rt, qt)
    lens = _lens(want)
    assert lens.tolist() == [0, 1, 64, 2, 63, 64, 33, 65, 65, 33]                # 63 / 64 / 65 among them
    db = _backend(metric, x)
    for limit, batch_cap in ((64, 0), (64, 1), (0, 0), (2, 0)):
        set_diag(monkeypatch, exact_range_sort=limit, tag_list_cap=batch_cap)
        _, info = _check(db, q, radius, rt, qt, "any", want, (metric, limit, batch_cap), product=False, n=270)
        cut = limit if limit else 4096
        assert info["device_sorted"] == ((lens >= 2) & (lens <= cut)).sum() and info["host_sorted"] == (lens > cut).sum(), (limit, info)
        assert info["batches"] == (2 if batch_cap else 1)
        if limit == 64:
            assert info["device_sorted"] == 6 and info["host_sorted"] == 2


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8"])
def test_forced_chunks_and_tiles_give_identical_bytes(monkeypatch, metric):
    """Chunks of 127 / 128 / 129 rows (a step short of, equal to and one row past the 128 rows of a step) and of one row, tiles of 1,
    3 and 5 queries.  At +inf every measured pair is a result, so a shadow row or query that offered anything would show in a count."""
    n = 2000
    x, q = _data(metric, n, 8, 41, grid=True), _data(metric, 40, 8, 42, grid=True)
    rt = _tags(43, n)
    qt = _query_tags(40, 44)
    d = distances(metric, x, q, np.arange(n, dtype=np.int32))
    want_inf = from_matrix(d, INF, rt, qt, "any")
    mid = float(_in_mask(d, rt, qt, "any")[2000])
    want_mid = from_matrix(d, mid, rt, qt, "any")
    assert 0 < _lens(want_mid).sum() < _lens(want_inf).sum() and _lens(want_inf).max() > 1000
    db = _backend(metric, x)
    for chunk, qtile in ((1, 0), (127, 1), (128, 3), (129, 5), (0, 0)):
        set_diag(monkeypatch, exact_chunk=chunk, exact_qtile=qtile)
        got, _ = _check(db, q, INF, rt, qt, "any", want_inf, (metric, chunk, qtile), product=(chunk, qtile) == (0, 0), n=n)
        assert [a.size for a in got[0]] == [int(tag_mask(rt, int(m), "any", n).sum()) for m in qt]   # exactly the mask's ids: no shadow was counted
        _check(db, q, mid, rt, qt, "any", want_mid, (metric, chunk, qtile, "mid"), product=False, n=n)


def test_row_tags_shorter_and_longer_than_the_rows(sets):
    x, q, db, d = sets("sq_euclid", 20, False)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    radius = float(_in_mask(d, rt, qt, "any")[20 * NQ])
    want = from_matrix(d, radius, rt, qt, "any")
    got, _ = _check(db, q, radius, rt, qt, "any", want, "550 words")
    short, _ = _check(db, q, radius, rt[:400], qt, "any", from_matrix(d, radius, rt[:400], qt, "any"), "short")
    assert np.concatenate(short[0]).max() < 400 <= np.concatenate(got[0]).max()
    # ... and beyond the rows: clamped, a row that does not exist is never dereferenced
    wide = np.concatenate([rt, np.zeros(50, np.uint32), np.full(5000, 0xFFFFFFFF, np.uint32)])
    _check(db, q, radius, wide, qt, "any", want, "wide", product=False)
    # n_rows below the uploaded rows
    assert _same(db.exact_range_tagged(q, radius, rt, qt, "any", n_rows=350), from_matrix(d[:, :350], radius, rt[:350], qt, "any"))
    # the index layer clamps to Length in the same way
    ix = _index("sq_euclid", x)
    for arr in (rt, rt[:400], wide):
        assert _same(ix.exact_range_query_tagged(q, radius, arr, qt, "any"), from_matrix(d, radius, arr[:N], qt, "any"))
    # no mask has a candidate: empty lists and nothing launched
    for words, masks in ((np.zeros(N, np.uint32), qt), (rt, np.where(qt == 0, qt, np.uint32(16)).astype(np.uint32)), (np.zeros(0, np.uint32), qt)):
        db.reset_stats()
        got = db.exact_range_tagged(q, INF, words, masks, "any")
        assert len(got[0]) == NQ and all(a.size == 0 for a in got[0]) and all(a.size == 0 for a in got[1])
        info = db.exact_range_tagged_info()
        assert db.stats()["exact_launches"] == 0 and info["batches"] == 0 and info["scanned"] == 0 and info["ids_listed"] == 0, info


def test_the_limit_on_distinct_masks():
    n = 4096
    x = uniform(n, 4, 55)
    rt = np.arange(1, n + 1, dtype=np.uint32)                # every word differs
    db = _backend("sq_euclid", x)
    qt = np.arange(1, 65537, dtype=np.uint32)                # 65 536 distinct masks; those of 4 096 and above name a tag no row carries
    q = x[np.arange(65536) % n] + np.float32(0.001)
    got = db.exact_range_tagged(q, 0.01, rt, qt, "all")
    info = db.exact_range_tagged_info()
    assert len(got[0]) == 65536 and info["masks"] == 65536 and info["skipped"] >= 65536 - n and info["scanned"] >= n - 1, info
    found = 0
    for i in list(range(0, n, 97)) + [n - 1, n, 65535]:     # row i carries the word i + 1, the mask of query i; a mask above 4 096 names a tag beside bit 12, which only the word 4 096 has
        want = exact_range_tagged("sq_euclid", x, q[i:i + 1], 0.01, rt, qt[i:i + 1], "all")
        assert got[0][i].tolist() == want[0][0].tolist() and got[1][i].tobytes() == want[1][0].tobytes(), i
        assert (i in got[0][i].tolist()) == (i < n), i
        found += got[0][i].size
    assert found > 40
    counts = np.full(65537, 5, np.int32)
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    many = np.arange(65537, dtype=np.uint32)
    qq = np.ascontiguousarray(q[np.arange(65537) % 65536])
    assert _lib().hnswdev_exact_range_tagged(db._ctx, qq.ctypes.data_as(F), 65537, n, ct.c_float(1.0), rt.ctypes.data_as(U), n, many.ctypes.data_as(U), 0,
                                             counts.ctypes.data_as(I)) == -1
    assert (counts == 0).all() and "more than 65536 distinct masks" in db.last_error() and "index 65536" in db.last_error(), db.last_error()
    ix = _index("sq_euclid", x[:100])
    pp_i, pp_d = (ct.c_void_p * 65537)(), (ct.c_void_p * 65537)()
    assert _lib().hnsw_mi355x_exact_range_query_tagged(ix._h, qq.ctypes.data_as(F), 65537, 4, ct.c_float(1.0), rt.ctypes.data_as(U), n, many.ctypes.data_as(U), 0,
                                                       pp_i, pp_d, counts.ctypes.data_as(I)) == -1
    import hnswindex
    assert "more than 65536 distinct masks" in hnswindex.net_amd.last_error()


def test_a_partition_of_tags_is_the_grouped_call(sets):
    x, q, db, d = sets("cosine", 21, False)
    rg = np.random.default_rng(7).integers(-1, 6, N).astype(np.int32)          # -1: in no group / no tag
    qg = (np.arange(NQ) % 7).astype(np.int32)                                  # group 6: empty
    rt = np.where(rg >= 0, np.uint32(1) << rg.clip(0).astype(np.uint32), np.uint32(0)).astype(np.uint32)
    qt = (np.uint32(1) << qg.astype(np.uint32)).astype(np.uint32)
    radius = float(np.sort(d, axis=None)[NQ * 100])
    ix = _index("cosine", x)
    for match in MODES:   # one tag per row: the modes agree, and the groups' lists come back
        got = db.exact_range_tagged(q, radius, rt, qt, match)
        assert _same(got, db.exact_range_grouped(q, radius, rg, qg, 7)) and _lens(got).sum() > 300 and (_lens(got)[qg == 6] == 0).all()
        assert _same(ix.exact_range_query_tagged(q, radius, rt, qt, match), ix.exact_range_query_grouped(q, radius, rg, qg, 7))


def test_removals_and_slot_reuse():
    n, dim = 1500, 16
    x = uniform(n, dim, 81).copy()
    q = uniform(26, dim, 82)
    rt, qt = _tags(3, n), _query_tags(26, 4)
    ix = _index("sq_euclid", x)
    d = distances("sq_euclid", x, q, np.arange(n, dtype=np.int32))
    radius = float(np.sort(d, axis=None)[26 * 300])
    assert _same(ix.exact_range_query_tagged(q, radius, rt, qt), from_matrix(d, radius, rt, qt, "any"))
    gone = np.unique(np.concatenate([[ix.entry_point], np.random.default_rng(83).choice(n, 99, replace=False)])).astype(np.int32)
    assert np.isin(gone, np.concatenate(from_matrix(d, radius, rt, qt, "any")[0])).any()    # a removed id would have been in
    before = rt.copy()
    ix.remove(gone)
    live = np.sort(ix.ids())
    for match in MODES:
        for r in (radius, INF):
            got = ix.exact_range_query_tagged(q, r, rt, qt, match)
            assert not np.isin(np.concatenate(got[0]), gone).any()
            assert _same(got, from_matrix(d, r, rt, qt, match, live=live)), (match, r)
            assert _same(got, _per_mask_calls(ix.exact_range_query, q, r, rt, qt, match, n)), (match, r)
    assert (rt == before).all()                  # the caller's array is not written
    # tags on vacant slots only: no candidate, no scan
    only_gone = np.zeros(n, np.uint32)
    only_gone[gone] = 1
    ix.reset_stats()
    got = ix.exact_range_query_tagged(q, INF, only_gone, np.ones(26, np.uint32))
    assert all(a.size == 0 for a in got[0]) and ix.stats()["exact_launches"] == 0
    fresh = uniform(50, dim, 84)
    new_ids = ix.add(fresh)
    assert np.isin(new_ids, gone).all()          # vacated slots are reused, and their words count again
    x[new_ids] = fresh
    got = ix.exact_range_query_tagged(q, radius, rt, qt)
    assert _same(got, exact_range_tagged("sq_euclid", x, q, radius, rt, qt, live=np.sort(ix.ids())))


def _raw_index_call(ix, q, radius, rt, n_rt, qt, match):
    """hnsw_mi355x_exact_range_query_tagged through ctypes, as a host that is not the Python class calls it: the arrays are left allocated"""
    q = np.ascontiguousarray(q, np.float32)
    n = q.shape[0]
    I, U = ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    pp_i, pp_d = (ct.c_void_p * n)(*([0x1234] * n)), (ct.c_void_p * n)(*([0x1234] * n))
    counts = np.full(n, 77, np.int32)
    rc = _lib().hnsw_mi355x_exact_range_query_tagged(ix._h, q.ctypes.data_as(ct.POINTER(ct.c_float)), n, q.shape[1], ct.c_float(radius),
                                                     None if rt is None else rt.ctypes.data_as(U), n_rt, None if qt is None else qt.ctypes.data_as(U), match,
                                                     pp_i, pp_d, counts.ctypes.data_as(I))
    return rc, pp_i, pp_d, counts


def test_the_c_calls_allocate_free_and_fail_as_the_grouped_ones(monkeypatch, sets):
    import hnswindex
    lib = _lib()
    x, q, db, d = sets("sq_euclid", 20, False)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    ix = _index("sq_euclid", x)
    radius = float(_in_mask(d, rt, qt, "all")[3 * NQ])
    want = from_matrix(d, radius, rt, qt, "all")
    lens = _lens(want)
    assert (lens == 0).any() and lens.sum() > 0
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q, radius, rt, N_TAGS, qt, 1)
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
    for args, word in (((None, N_TAGS, qt, 0), "row_tags"), ((rt, -1, qt, 0), "n_row_tags"), ((rt, N_TAGS, qt, 2), "match = 2"), ((rt, N_TAGS, qt, -1), "match = -1"),
                       ((rt, N_TAGS, None, 0), "ArgumentNullException")):
        rc, pp_i, pp_d, counts = _raw_index_call(ix, q, radius, *args)
        assert rc == -1 and all(p is None for p in pp_i) and all(p is None for p in pp_d) and (counts == 0).all(), word
        assert re.search(word, hnswindex.net_amd.last_error()), (word, hnswindex.net_amd.last_error())
    # ... a device-side failure (an arena below a list) leaves the same
    set_diag(monkeypatch, exact_range_arena=10)
    rc, pp_i, pp_d, counts = _raw_index_call(ix, q, INF, rt, N_TAGS, qt, 0)
    set_diag(monkeypatch, exact_range_arena=0)
    assert rc == -1 and all(p is None for p in pp_i) and all(p is None for p in pp_d) and (counts == 0).all()
    assert "arena" in hnswindex.net_amd.last_error()
    # the inner call: the same rules, the counts zeroed
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    qq = np.ascontiguousarray(q, np.float32)
    rt_p, qt_p = rt.ctypes.data_as(U), qt.ctypes.data_as(U)
    for args, word in (((None, N_TAGS, qt_p, 0), "row_tags"), ((rt_p, -1, qt_p, 0), "n_row_tags"), ((rt_p, N_TAGS, qt_p, 2), "match = 2"),
                       ((rt_p, N_TAGS, None, 0), "query_tags")):
        counts = np.full(NQ, 5, np.int32)
        assert lib.hnswdev_exact_range_tagged(db._ctx, qq.ctypes.data_as(F), NQ, N, ct.c_float(radius), *args, counts.ctypes.data_as(I)) == -1, word
        assert (counts == 0).all() and re.search(word, db.last_error()), (word, db.last_error())
    counts = np.full(NQ, 5, np.int32)
    assert lib.hnswdev_exact_range_tagged(db._ctx, qq.ctypes.data_as(F), NQ, -1, ct.c_float(radius), rt_p, N_TAGS, qt_p, 0, counts.ctypes.data_as(I)) == -1
    assert (counts == 0).all() and "bad argument" in db.last_error()
    # the counters of both layers, and their reset
    ix.reset_stats()
    ix.exact_range_query_tagged(q, radius, rt, qt, "all")
    info = (ct.c_uint64 * 9)()
    assert lib.hnsw_mi355x_exact_range_tagged_info(ix._h, info) == 0
    cnt, none = _counts(rt, qt, "all")
    assert list(info) == list(ix.exact_range_tagged_info().values()) == [1, MASKS.size, NQ - none.sum(), none.sum(), sum(cnt), 1, int((lens >= 2).sum()), 0, 0]
    ix.reset_stats()
    assert ix.exact_range_tagged_info() == EMPTY


def test_the_resident_query_set_and_pending_range_results_are_not_touched(monkeypatch, sets):
    lib = _lib()
    x, q, _, d = sets("sq_euclid", 20, False)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    radius = float(_in_mask(d, rt, qt, "any")[20 * NQ])
    ix = _index("sq_euclid", x)
    ix.set_resident_queries(q[:20])
    before = ix.knn_query_resident(10)
    other = uniform(33, 20, 91)
    ot = _query_tags(33, 92)
    assert _same(ix.exact_range_query_tagged(other, radius, rt, ot), exact_range_tagged("sq_euclid", x, other, radius, rt, ot))
    ix.exact_range_query_tagged(other[:5], radius, np.zeros(N, np.uint32), ot[:5])      # the no-scan path
    assert lib.hnsw_mi355x_resident_count(ix._h) == 20
    after = ix.knn_query_resident(10)
    assert (after[0] == before[0]).all() and after[1].tobytes() == before[1].tobytes()
    # the inner boundary, where the cached query norms (cosine) and the quantised records (int8) must survive and be gathered too:
    # queries == NULL with several batches -- every batch gathers its own queries out of the resident set
    cnt, _ = _counts(rt, qt[:40], "any")
    set_diag(monkeypatch, tag_list_cap=max(cnt) + 1)
    assert _batches(cnt, max(cnt) + 1)[0] >= 3
    for metric in ("cosine", "sq_euclid_i8"):
        xm, qm, _, dm = sets(metric, 20, False)
        r_m = float(_in_mask(dm, rt, qt, "any")[20 * NQ])
        fresh = _backend(metric, xm)
        fresh.set_queries(qm[:40])
        cand = np.arange(50, dtype=np.int32)
        off = np.arange(41, dtype=np.int32) * 50
        kept = fresh.dist_query_batch(None, off, np.tile(cand, 40))
        fresh.exact_range_tagged(other, r_m, rt, ot)
        assert fresh.dist_query_batch(None, off, np.tile(cand, 40)).tobytes() == kept.tobytes()
        res = fresh.exact_range_tagged(None, r_m, rt, qt[:40])
        want = from_matrix(dm[:40], r_m, rt, qt[:40], "any")
        assert _lens(want).sum() > 100 and _same(res, want), metric
        assert fresh.exact_range_tagged_info()["batches"] >= 3
        assert fresh.dist_query_batch(None, off, np.tile(cand, 40)).tobytes() == kept.tobytes()
        with pytest.raises(RuntimeError, match="resident"):
            fresh.exact_range_tagged(None, r_m, rt, qt[:41])
    set_diag(monkeypatch, tag_list_cap=0)
    # a traversal's results wait in the context while a tagged exact range call comes and goes
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
    assert _same(dev.exact_range_tagged(other, radius, rt, ot), exact_range_tagged("sq_euclid", x, other, radius, rt, ot))
    t_i, t_d = np.empty(t_counts.sum(), np.int32), np.empty(t_counts.sum(), np.float32)
    assert lib.hnswdev_range_results(dev._ctx, t_i.ctypes.data_as(I), t_d.ctypes.data_as(F)) == 0
    again = dev.range_search(q[:9], int(ix.entry_point), t_radius)
    assert (t_i == np.concatenate(again[0])).all() and t_d.tobytes() == np.concatenate(again[1]).tobytes()
