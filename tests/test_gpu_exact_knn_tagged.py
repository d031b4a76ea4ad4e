"""GPU tier: exact_knn_query_tagged (hnsw_mi355x_exact_knn_query_tagged / hnswdev_exact_knn_tagged) -- the flat scan
with a tag mask per query -- against the per-mask loop of exact_knn_query calls it replaces and against numpy: per query the
candidates of its mask ordered by np.lexsort((ids, dist)) over the distances exact_knn_query itself reports.  Every comparison is ids
equal and distance BYTES equal.  Shapes and tags are those of tests/test_gpu_tagged_query.py, plus bit 5 on a single row."""
import ctypes as ct
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from tagged_query_model import tag_mask

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 1200, 16, 8, 20
N_TAGS = N - 50                      # row_tags is shorter than the rows: the last 50 ids carry no tag
B31 = 0x80000000
MASKS = np.array([1, 2, 4, 8, 16, 32, B31, 0b101, 0b11, B31 | 1, 0xFFFFFFFF, 0, 1 | 1 << 4], np.uint32)   # 16: on no row; 32: on one
MODES = ("any", "all")
NQ = 2 * MASKS.size


def _data(metric, n, seed):
    x = uniform(n, DIM, seed)
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
    return MASKS[np.random.default_rng(seed).permutation(np.arange(nq) % MASKS.size)]


def _index(metric, x, **knobs):
    import hnswindex
    ix = hnswindex.Index(DIM, metric)
    ix.set_collection_size(N + 64); ix.set_max_edges(M); ix.set_min_nn(MIN_NN)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    return ix


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _per_mask(call, q, k, rt, qt, match, n=N):
    """The loop the call replaces: one exact_knn_query-style call per distinct mask, the mask's ids as its allow-set."""
    ids = np.full((q.shape[0], k), -1, np.int32)
    d = np.full((q.shape[0], k), np.nan, np.float32)
    for m in np.unique(qt):
        sel = qt == m
        ids[sel], d[sel] = call(q[sel], k, tag_mask(rt, int(m), match, n))
    return ids, d


def _all_distances(ix, q, n):
    """dist[nq, n] as exact_knn_query reports them (NaN: not a live id), from calls of at most 1 024 results each."""
    out = np.full((q.shape[0], n), np.nan, np.float32)
    for lo in range(0, n, 1024):
        allowed = np.zeros(n, bool)
        allowed[lo:lo + 1024] = True
        ids, d = ix.exact_knn_query(q, min(1024, n - lo), allowed=allowed)
        for i in range(q.shape[0]):
            have = ids[i] >= 0
            out[i, ids[i][have]] = d[i][have]
    return out


def _by_lexsort(dist, k, rt, qt, match):
    """Per query the candidates of its mask that have a distance, ascending by (distance, id), padded."""
    nq, n = dist.shape
    ids = np.full((nq, k), -1, np.int32)
    d = np.full((nq, k), np.nan, np.float32)
    for i in range(nq):
        cand = np.flatnonzero(tag_mask(rt, int(qt[i]), match, n) & ~np.isnan(dist[i]))
        order = np.lexsort((cand, dist[i, cand]))[:k]
        ids[i, :order.size] = cand[order]
        d[i, :order.size] = dist[i, cand[order]]
    return ids, d


def _counts(rt, qt, match, n=N):
    """Per distinct mask in the order it first appears: its candidates; and the queries of masks without one."""
    first = [int(m) for m in dict.fromkeys(qt.tolist())]
    cnt = [int(tag_mask(rt, m, match, n).sum()) for m in first]
    none = np.array([not tag_mask(rt, int(m), match, n).any() for m in qt])
    return cnt, none


def _batches(cnt, cap):
    """The batches the call documents: masks in the order they first appear, a batch closed when the next list would take it past
    `cap`; a batch whose lists are all empty is not scanned."""
    out, i = 0, 0
    while i < len(cnt):
        total, j = cnt[i], i + 1
        while j < len(cnt) and total + cnt[j] <= cap:
            total += cnt[j]
            j += 1
        out += total > 0
        i = j
    return out


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x = _data(metric, N, 1)
        self.ix = _index(metric, self.x)
        self.q = _data(metric, NQ, 9)
        self.rt, self.qt = _tags(3), _query_tags(NQ, 4)
        self.dist = _all_distances(self.ix, self.q, N)
        self.dist.setflags(write=False)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


def test_the_tags_cover_every_branch_of_the_predicate():
    rt, qt = _tags(3), _query_tags(NQ, 4)
    assert ((rt & 8) != 0).sum() == 7 and ((rt & 16) != 0).sum() == 0 and ((rt & 32) != 0).sum() == 1
    assert 40 <= (rt == 0).sum() and rt.size == N - 50 and ((rt & B31) != 0).sum() > 20
    assert all((qt == m).sum() == 2 for m in MASKS)
    assert sum(c == 0 for c in _counts(rt, qt, "any")[0]) == 2 and sum(c == 0 for c in _counts(rt, qt, "all")[0]) == 4


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_tagged_scan_is_the_per_mask_loop_and_the_lexsort_of_the_candidates(cases, metric):
    c = cases(metric)
    for match in MODES:
        cnt, none = _counts(c.rt, c.qt, match)
        for k in (1, 10, 40, 1024):   # 40: past the 7 ids of bit 3 and the one of bit 5 (padding tails); 1 024: past most lists
            c.ix.reset_stats()
            got = c.ix.exact_knn_query_tagged(c.q, k, c.rt, c.qt, match)
            info = c.ix.exact_tagged_info()
            assert _same(got, _by_lexsort(c.dist, k, c.rt, c.qt, match)), (metric, match, k)
            assert _same(got, _per_mask(lambda q, kk, a: c.ix.exact_knn_query(q, kk, allowed=a), c.q, k, c.rt, c.qt, match)), (metric, match, k)
            assert info == {"calls": 1, "masks": MASKS.size, "scanned": NQ - int(none.sum()), "skipped": int(none.sum()), "ids_listed": sum(cnt), "batches": 1}, info
            assert (got[0][none] == -1).all() and np.isnan(got[1][none]).all()
            one = c.qt == 32
            assert ((got[0][one] >= 0).sum(axis=1) == 1).all() and (got[0][one][:, 0] == np.flatnonzero(c.rt & 32)[0]).all()
            if k == 40:
                assert ((got[0][c.qt == 8] >= 0).sum(axis=1) == 7).all() and (got[0][c.qt == 8][:, 7:] == -1).all()


def test_several_chunks_and_tiles_per_list(cases, monkeypatch):
    c = cases("sq_euclid")
    nq = 8 * MASKS.size
    q, qt = _data("sq_euclid", nq, 41), _query_tags(nq, 42)
    dist = _all_distances(c.ix, q, N)
    for knobs in (dict(exact_chunk=100), dict(exact_qtile=3), dict(exact_chunk=64, exact_qtile=2)):
        set_diag(monkeypatch, **knobs)
        for match in MODES:
            c.ix.reset_stats()
            got = c.ix.exact_knn_query_tagged(q, 12, c.rt, qt, match)
            assert _same(got, _by_lexsort(dist, 12, c.rt, qt, match)), (knobs, match)
            assert c.ix.stats()["exact_launches"] == 1


def test_masks_in_several_batches(cases, monkeypatch):
    """tag_list_cap below one list's length, just above the longest, and at one entry: the masks run in several batches, a list
    longer than the cap is a batch alone, the answers do not change and exact_tagged_info says it happened."""
    c = cases("cosine")
    for match in MODES:
        cnt, none = _counts(c.rt, c.qt, match)
        want = _by_lexsort(c.dist, 10, c.rt, c.qt, match)
        longest = max(cnt)
        for cap in (longest - 1, longest + 1, 300, 1, 0):
            set_diag(monkeypatch, tag_list_cap=cap)
            c.ix.reset_stats()
            got = c.ix.exact_knn_query_tagged(c.q, 10, c.rt, c.qt, match)
            info = c.ix.exact_tagged_info()
            assert _same(got, want), (match, cap)
            expect = _batches(cnt, cap if cap > 0 else 1 << 28)
            assert info["batches"] == expect and info["ids_listed"] == sum(cnt) and info["scanned"] == NQ - int(none.sum()), (match, cap, info)
            assert c.ix.stats()["exact_launches"] == expect
        assert _batches(cnt, longest - 1) >= 3 and _batches(cnt, 1) == sum(x > 0 for x in cnt) and _batches(cnt, 1 << 28) == 1


def test_many_queries_per_mask(cases):
    c = cases("sq_euclid")
    nq = 4096
    q = _data("sq_euclid", nq, 17)
    live = np.array([1, 2, 4, 8, 32, B31, 0b11, 0b101, B31 | 1], np.uint32)
    qt = live[np.random.default_rng(19).integers(0, live.size, nq)]
    for match in MODES:
        got = c.ix.exact_knn_query_tagged(q, 10, c.rt, qt, match)
        assert _same(got, _per_mask(lambda qq, kk, a: c.ix.exact_knn_query(qq, kk, allowed=a), q, 10, c.rt, qt, match)), match


def test_argument_errors_and_nothing_to_scan(cases):
    import hnswindex
    c = cases("sq_euclid")
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    for match in MODES:
        c.ix.reset_stats()
        nothing = c.ix.exact_knn_query_tagged(c.q, 5, c.rt, np.where(np.arange(NQ) % 2, 16, 0), match)
        assert (nothing[0] == -1).all() and np.isnan(nothing[1]).all() and c.ix.stats()["exact_launches"] == 0
        assert c.ix.exact_tagged_info()["batches"] == 0 and c.ix.exact_tagged_info()["skipped"] == NQ
        nothing = c.ix.exact_knn_query_tagged(c.q, 5, np.zeros(0, np.uint32), c.qt, match)      # no word at all
        assert (nothing[0] == -1).all()
        for k in (0, -2):
            assert c.ix.exact_knn_query_tagged(c.q, k, c.rt, c.qt, match)[0].shape == (NQ, 0)
    with pytest.raises(RuntimeError, match="k = 1025 is above the limit of 1024"):
        c.ix.exact_knn_query_tagged(c.q, 1025, c.rt, c.qt)
    ids, d = np.full((NQ, 5), 7, np.int32), np.full((NQ, 5), 7.0, np.float32)
    rt, qt = np.ascontiguousarray(c.rt), np.ascontiguousarray(c.qt)
    c.ix.reset_stats()

    def call(q=c.q.ctypes.data_as(F), row=rt.ctypes.data_as(U), n_row=rt.size, qtags=qt.ctypes.data_as(U), match=0):
        return lib.hnsw_mi355x_exact_knn_query_tagged(c.ix._h, q, NQ, DIM, 5, row, n_row, qtags, match, ids.ctypes.data_as(I), d.ctypes.data_as(F))
    for kwargs, message in ((dict(match=2), "match = 2 is neither 0 (any) nor 1 (all)"), (dict(row=None), "row_tags must not be NULL"),
                            (dict(n_row=-1), "n_row_tags must be >= 0"), (dict(qtags=None), "ArgumentNullException"), (dict(q=None), "ArgumentNullException")):
        assert call(**kwargs) == -1, kwargs
        assert message in hnswindex.net_amd.last_error(), (kwargs, hnswindex.net_amd.last_error())
    assert (ids == 7).all() and (d == 7.0).all()
    assert c.ix.stats()["exact_launches"] == 0 and c.ix.exact_tagged_info()["calls"] == 0


def test_after_removals_a_vacant_slot_s_tags_count_for_nothing_until_it_is_filled_again():
    x = _data("sq_euclid", N, 1)
    ix = _index("sq_euclid", x, set_allow_removals=True)
    rt, qt = _tags(3), _query_tags(NQ, 4)
    q = _data("sq_euclid", NQ, 9)
    rng = np.random.default_rng(21)
    gone = np.unique(np.concatenate([[ix.entry_point]] + [rng.choice(np.flatnonzero(rt & bit), n, replace=False) for bit, n in ((1, 60), (2, 28), (4, 10), (8, 2), (B31, 6))]))
    before = ix.exact_knn_query_tagged(q, 40, rt, qt, "any")
    ix.remove(gone)
    assert np.isin(before[0], gone).any() and (rt[gone[gone < N_TAGS]] != 0).any()   # the removed ids were results, and their slots stay tagged
    for match in MODES:
        dist = _all_distances(ix, q, N)
        assert np.isnan(dist[:, gone]).all()
        for k in (5, 40):
            got = ix.exact_knn_query_tagged(q, k, rt, qt, match)
            assert _same(got, _by_lexsort(dist, k, rt, qt, match)), (match, k)
            assert _same(got, _per_mask(lambda qq, kk, a: ix.exact_knn_query(qq, kk, allowed=a), q, k, rt, qt, match)), (match, k)
            assert not np.isin(got[0], gone).any()
    ix.remove(np.flatnonzero(rt & 32))    # the one row of bit 5: its mask has no candidate left
    ix.reset_stats()
    got = ix.exact_knn_query_tagged(q, 5, rt, qt, "any")
    assert (got[0][qt == 32] == -1).all() and ix.exact_tagged_info()["skipped"] == int(np.isin(qt, [32, 16, 0]).sum())
    new_ids = ix.add(x[:40] + np.float32(0.25))   # rows added after the removals: a slot filled again answers under the tags the array holds for it
    n_now = max(N, int(new_ids.max()) + 1)
    dist = _all_distances(ix, q, n_now)
    assert not np.isnan(dist[:, new_ids]).any()
    for match in MODES:
        got = ix.exact_knn_query_tagged(q, 40, rt, qt, match)
        assert _same(got, _by_lexsort(dist, 40, rt, qt, match)), match
    reused = new_ids[new_ids < N_TAGS]
    if reused.size:
        every = ix.exact_knn_query_tagged(q[:2], 1024, rt, [0xFFFFFFFF, 0xFFFFFFFF], "any")[0]
        assert np.isin(reused[rt[reused] != 0], every[0]).all() and not np.isin(reused[rt[reused] == 0], every[0]).any()


def test_device_backend_exact_knn_tagged(cases):
    """The inner boundary: rows a host uploaded itself, queries given or resident (queries == NULL), n_rows below the upload."""
    import hnswindex
    c = cases("ucosine")
    db = hnswindex.DeviceBackend(DIM, "ucosine", capacity=N)
    db.upload_rows(0, c.x)
    for match in MODES:
        cnt, none = _counts(c.rt, c.qt, match)
        db.reset_stats()
        got = db.exact_knn_tagged(c.q, 10, c.rt, c.qt, match)
        assert _same(got, _per_mask(lambda q, k, a: db.exact_knn(q, k, allowed=a), c.q, 10, c.rt, c.qt, match)), match
        assert _same(got, _by_lexsort(c.dist, 10, c.rt, c.qt, match)), match
        assert db.exact_tagged_info() == {"calls": 1, "masks": MASKS.size, "scanned": NQ - int(none.sum()), "skipped": int(none.sum()), "ids_listed": sum(cnt),
                                          "batches": 1}
        db.set_queries(c.q)
        assert _same(db.exact_knn_tagged(None, 10, c.rt, c.qt, match), got), match
        short = db.exact_knn_tagged(c.q, 10, c.rt, c.qt, match, n_rows=500)
        assert _same(short, _per_mask(lambda q, k, a: db.exact_knn(q, k, n_rows=500, allowed=a), c.q, 10, c.rt, c.qt, match)) and short[0].max() < 500
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    ids, d = np.full((NQ, 5), 7, np.int32), np.full((NQ, 5), 7.0, np.float32)
    rt, qt = np.ascontiguousarray(c.rt), np.ascontiguousarray(c.qt)
    launches = db.stats()["exact_launches"]
    good = dict(q=c.q.ctypes.data_as(F), rt=rt.ctypes.data_as(U), n_rt=rt.size, qt=qt.ctypes.data_as(U), match=0, k=5, ids=ids.ctypes.data_as(I), d=d.ctypes.data_as(F))
    for change, message in ((dict(rt=None), "row_tags must not be NULL"), (dict(n_rt=-1), "n_row_tags must be >= 0"), (dict(qt=None), "query_tags must not be NULL"),
                            (dict(match=3), "match = 3 is neither 0 (any) nor 1 (all)"), (dict(k=0), "bad argument"), (dict(k=1025), "k = 1025 is above the limit of 1024"),
                            (dict(ids=None), "bad argument"), (dict(d=None), "bad argument")):
        a = dict(good, **change)
        assert lib.hnswdev_exact_knn_tagged(db._ctx, a["q"], NQ, N, a["k"], a["rt"], a["n_rt"], a["qt"], a["match"], a["ids"], a["d"]) == -1, change
        assert db.last_error().startswith("exact_knn_tagged: ") and message in db.last_error(), (change, db.last_error())
    db2 = hnswindex.DeviceBackend(DIM, "ucosine", capacity=N)
    db2.upload_rows(0, c.x)
    with pytest.raises(RuntimeError, match="queries == NULL needs a resident query set"):
        db2.exact_knn_tagged(None, 5, c.rt, c.qt)
    assert (ids == 7).all() and (d == 7.0).all() and db.stats()["exact_launches"] == launches


def test_resident_queries_with_several_batches(cases, monkeypatch):
    """queries == NULL and more than one batch: a batch's queries are gathered from the resident set by their own indices."""
    import hnswindex
    c = cases("cosine")
    db = hnswindex.DeviceBackend(DIM, "cosine", capacity=N)
    db.upload_rows(0, c.x)
    db.set_queries(c.q)
    for match in MODES:
        want = _by_lexsort(c.dist, 10, c.rt, c.qt, match)
        set_diag(monkeypatch, tag_list_cap=300)
        db.reset_stats()
        assert _same(db.exact_knn_tagged(None, 10, c.rt, c.qt, match), want), match
        assert db.exact_tagged_info()["batches"] == _batches(_counts(c.rt, c.qt, match)[0], 300) > 2
        assert _same(db.exact_knn_tagged(c.q, 10, c.rt, c.qt, match), want), match
        monkeypatch.undo()


def test_threads_mixing_tagged_grouped_and_filtered_scans(cases):
    c = cases("sq_euclid")
    masks = [tag_mask(c.rt, m, "any", N) for m in (1, 2, B31)]
    rg = (c.rt & 3).astype(np.int32)
    qg = (np.arange(NQ) % 4).astype(np.int32)
    want_t = {match: _by_lexsort(c.dist, 5, c.rt, c.qt, match) for match in MODES}
    want_f = [c.ix.exact_knn_query(c.q, 5, allowed=m) for m in masks]
    want_g = c.ix.exact_knn_query_grouped(c.q, 5, rg, qg, 4)
    errors = []

    def work(t):
        try:
            for r in range(6):
                which = (t + r) % 4
                if which < 2:
                    assert _same(c.ix.exact_knn_query_tagged(c.q, 5, c.rt, c.qt, MODES[which]), want_t[MODES[which]])
                elif which == 2:
                    assert _same(c.ix.exact_knn_query(c.q, 5, allowed=masks[r % 3]), want_f[r % 3])
                else:
                    assert _same(c.ix.exact_knn_query_grouped(c.q, 5, rg, qg, 4), want_g)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
