"""GPU tier: range_query_tagged (hnsw_mi355x_range_query_tagged / Index.range_query_tagged) -- a tag mask per query, every mask in
one device traversal -- against the plain-Python statement of its contract (tests/tagged_range_model.py: the filtered RangeQuery of
the reference, one mask at a time) on graphs whose hash equals the CPU oracle's, and against the product's own loop of per-mask
filtered calls, in both modes: counts, ids, distance bits and the order among equal distances.  The shapes are those of
tests/test_gpu_grouped_range.py, the tags those of tests/test_gpu_tagged_query.py.  Every case asserts its precondition from the
model before it compares.

The model restates layer 0 only, so the layer-1 case is held to the product's per-mask loop alone.  The last three tests are
about closures beyond the sort kernel's table (kRangeSortMax = 2048 entries): range_sort_tagged_kernel finishes one on the device
when its allowed entries fit the table and no two of them tie (diag range_sort_long=0: as the other two sorts, on the host)."""
import ctypes as ct

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from tagged_range_model import HeapEmpty, heap_empty_closed_form, tag_mask, tagged_range

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 2000, 16, 8, 20
N_TAGS = N - 50                      # row_tags is shorter than the graph: the last 50 ids carry no tag
B31 = 0x80000000
# single bits 0 .. 4 and 31; 0b101 and 0b11, where "any" and "all" differ; bit 31 with bit 0; every bit; no bit; and 1 | 1 << 4, which
# selects the rows of 1 under "any" and none under "all"
MASKS = np.array([1, 2, 4, 8, 16, B31, 0b101, 0b11, B31 | 1, 0xFFFFFFFF, 0, 1 | 1 << 4], np.uint32)
MODES = ("any", "all")
F16 = {"sq_euclid_f16": "sq_euclid", "ucosine_f16": "ucosine"}
NQ = 24
TABLE = 2048                         # kRangeSortMax


def _data(metric, n, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, DIM)).astype(np.float32) if grid else uniform(n, DIM, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _tags(seed, n_tags=N_TAGS):
    rng = np.random.default_rng(seed)
    rt = np.zeros(n_tags, np.uint32)
    for bit, share in ((0, 0.6), (1, 0.3), (2, 0.1), (31, 0.05)):
        rt |= np.where(rng.random(n_tags) < share, np.uint32(1 << bit), np.uint32(0)).astype(np.uint32)
    picked = rng.choice(n_tags, 7 + 40, replace=False)
    rt[picked[:7]] |= np.uint32(8)
    rt[picked[7:]] = 0
    return rt


def _query_tags(nq, seed):
    return MASKS[np.random.default_rng(seed).permutation(np.arange(nq) % MASKS.size)]


def _build(metric, x, n=N, **knobs):
    import hnswindex
    import oracle
    ix = hnswindex.Index(x.shape[1], metric)
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    base = F16.get(metric, metric)
    rows = x.astype(np.float16).astype(np.float32) if metric in F16 else x
    ref = oracle.OracleIndex(x.shape[1], base, max_edges=M, min_nn=MIN_NN, collection_size=n)
    ref.add(rows)
    assert ix.graph_hash() == ref.graph_hash(), metric
    return ix, ref, base, rows


def _same(got, want):
    return len(got[0]) == len(want[0]) and all(a.tolist() == b.tolist() and c.tobytes() == e.tobytes()
                                               for a, b, c, e in zip(got[0], want[0], got[1], want[1]))


def _per_mask(ix, q, radius, rt, qt, match, n, layer=0):
    """The loop the call replaces: one filtered call per distinct mask, lists put back in the caller's order."""
    ids, d = [None] * q.shape[0], [None] * q.shape[0]
    for m in np.unique(qt):
        sel = np.flatnonzero(qt == m)
        a, b = ix.range_query(q[sel], radius, allowed=tag_mask(rt, int(m), match, n), layer=layer)
        for w, ai, bi in zip(sel, a, b):
            ids[w], d[w] = ai, bi
    return ids, d


def _no_candidate(rt, qt, match, n=N):
    return np.array([not tag_mask(rt, int(m), match, n).any() for m in qt])


TARGETS = (0.4, 24, 340)


def _radii(ref, base, rows, q):
    """Radii at which the unfiltered closure (the oracle's RangeQuery) holds about 0.4, 24 and 340 ids on average: a bisection over
    the quantiles of the true distances, on the oracle's own closure sizes."""
    import oracle
    d = np.sort(np.concatenate([oracle.dist_query_rows(base, rows, qq, np.arange(rows.shape[0], dtype=np.int32)) for qq in q[:6]]))
    out = []
    for target in TARGETS:
        lo, hi = 0, d.size // 2
        for _ in range(16):
            mid = (lo + hi) // 2
            if np.mean([a.size for a in ref.range_query(q, float(d[mid]))[0]]) < target:
                lo = mid
            else:
                hi = mid
        out.append(float(d[hi]))
    return out


class Case:
    """One metric's data, index, oracle, tags and queries, and the model's answers (computed once, shared by the tests)."""

    def __init__(self, metric, grid=False):
        self.metric = metric
        self.x = _data(metric, N, 2 if grid else 1, grid)
        self.ix, self.ref, self.base, self.rows = _build(metric, self.x)
        self.q = np.random.default_rng(8).integers(1, 4, (NQ, DIM)).astype(np.float32) if grid else _data(metric, NQ, 9)
        self.rt, self.qt = _tags(3), _query_tags(NQ, 4)
        self._want = {}
        self.radii = None if grid else _radii(self.ref, self.base, self.rows, self.q)

    def want(self, radius, match):
        if (radius, match) not in self._want:
            self._want[radius, match] = tagged_range(self.ref, self.rows, self.base, self.q, radius, self.rt, self.qt, match)
        return self._want[radius, match]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            cache[(metric, grid)] = Case(metric, grid)
        return cache[(metric, grid)]
    return get


def test_the_tags_cover_every_branch_of_the_predicate():
    rt, qt = _tags(3), _query_tags(NQ, 4)
    share = [float(((rt >> b) & 1).sum()) / N for b in (0, 1, 2, 31)]
    assert 0.5 < share[0] < 0.65 and 0.2 < share[1] < 0.35 and 0.05 < share[2] < 0.15 and 0.02 < share[3] < 0.08
    assert ((rt & 8) != 0).sum() == 7 and ((rt & 16) != 0).sum() == 0
    assert 40 <= (rt == 0).sum() and rt.size == N - 50 and rt.dtype == np.uint32
    assert all((qt == m).sum() == 2 for m in MASKS)
    for m in (0b101, 0b11, B31 | 1, 0xFFFFFFFF, 1 | 1 << 4):      # the modes differ on these
        assert tag_mask(rt, m, "all", N).sum() < tag_mask(rt, m, "any", N).sum(), m
    assert not tag_mask(rt, 1 | 1 << 4, "all", N).any() and not tag_mask(rt, 0xFFFFFFFF, "all", N).any()


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"])
def test_tagged_range_is_the_model_and_the_per_mask_filtered_calls(cases, metric):
    c = cases(metric)
    means = [np.mean([a.size for a in c.ref.range_query(c.q, radius)[0]]) for radius in c.radii]
    # the closures the radii were chosen for: about 0.4, 24 and 340 ids (within a factor of two)
    assert all(t / 2 < m < t * 2 for t, m in zip(TARGETS, means)), means
    for match in MODES:
        none = _no_candidate(c.rt, c.qt, match)
        assert none.sum() >= (4 if match == "any" else 8)               # the tag on no row, the mask 0; under "all" 1 | 1 << 4 and every bit too
        for radius in c.radii:
            want = c.want(radius, match)
            c.ix.reset_stats()
            got = c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, match)
            info, st = c.ix.range_tagged_info(), c.ix.stats()
            assert _same(got, want), (metric, match, radius)
            assert info["calls"] == 1 and info["masks"] == MASKS.size and info["launched"] == NQ - none.sum() and info["skipped"] == none.sum(), info
            assert st["range_launches"] >= 1 and info["long_finished"] == 0, (info, st)
            assert _same(got, _per_mask(c.ix, c.q, radius, c.rt, c.qt, match, N)), (metric, match, radius)
            assert all(got[0][i].size == 0 for i in np.flatnonzero(none))
        assert sum(a.size for a in c.want(c.radii[2], match)[0]) > (200 if match == "any" else 100)
    differ = np.isin(c.qt, [0b101, 0b11, B31 | 1, 0xFFFFFFFF, 1 | 1 << 4])
    a, b = c.want(c.radii[2], "any"), c.want(c.radii[2], "all")
    assert all(a[0][i].tolist() == b[0][i].tolist() for i in np.flatnonzero(~differ)) and any(a[0][i].tolist() != b[0][i].tolist() for i in np.flatnonzero(differ))


@pytest.mark.parametrize("match", MODES)
def test_ties_among_allowed_results_are_replayed_on_the_device(cases, match):
    c = cases("sq_euclid", grid=True)
    radius = 8.0
    want = c.want(radius, match)
    tied = sum(int(a.size >= 2 and (np.diff(d) == 0).any()) for a, d in zip(*want))
    closures = [a.size for a in c.ref.range_query(c.q, radius)[0]]
    assert tied >= (5 if match == "any" else 2) and max(closures) <= TABLE   # two allowed results tie; every closure fits a wave's table
    c.ix.reset_stats()
    got = c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, match)
    info, st = c.ix.range_tagged_info(), c.ix.stats()
    assert _same(got, want)
    assert st["range_device_ordered"] >= tied and st["range_host_ordered"] == 0 and info["host_finished"] == 0 and info["long_finished"] == 0, (info, st)
    assert _same(got, _per_mask(c.ix, c.q, radius, c.rt, c.qt, match, N))


def test_every_other_path_gives_the_same_answers(cases, monkeypatch):
    c = cases("sq_euclid", grid=True)
    radius = 8.0
    for match in MODES:
        want = c.want(radius, match)
        with_results = sum(int(a.size >= 2) for a in want[0])
        for finish in ("0", "1"):
            set_diag(monkeypatch, range_finish=finish)
            c.ix.reset_stats()
            assert _same(c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, match), want), (match, finish)
            assert c.ix.range_tagged_info()["host_finished"] >= (with_results if finish == "0" else 1), (match, finish)
            monkeypatch.undo()
    # device_traversal = 0: every query goes the lock-step way with its own predicate (a smaller graph: its Add is lock-step too)
    n = 600
    iy, ref, base, rows = _build("sq_euclid", c.x[:n], n=n, set_device_traversal=False)
    for match in MODES:
        want = tagged_range(ref, rows, base, c.q, radius, c.rt, c.qt, match)
        assert sum(int(a.size >= 2 and (np.diff(d) == 0).any()) for a, d in zip(*want)) >= 1      # ties among the results here too
        iy.reset_stats()
        assert _same(iy.range_query_tagged(c.q, radius, c.rt, c.qt, match), want), match
        assert iy.stats()["range_launches"] == 0 and iy.range_tagged_info()["calls"] == 0


def test_a_nan_radius_runs_and_finds_nothing(cases):
    c = cases("sq_euclid")
    for match in MODES:
        c.ix.reset_stats()
        got = c.ix.range_query_tagged(c.q, float("nan"), c.rt, c.qt, match)
        info = c.ix.range_tagged_info()
        assert all(a.size == 0 for a in got[0]) and _same(got, _per_mask(c.ix, c.q, float("nan"), c.rt, c.qt, match, N))
        assert info["launched"] == NQ and info["skipped"] == 0, info        # !(radius >= 0): nothing is skipped


def test_layer_one_equals_the_per_mask_loop(cases):
    c = cases("sq_euclid")
    assert c.ix.top_layer() >= 1
    radius = c.radii[2]
    for match in MODES:
        got = c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, match, layer=1)
        loop = _per_mask(c.ix, c.q, radius, c.rt, c.qt, match, N, layer=1)
        assert _same(got, loop) and sum(a.size for a in got[0]) > 0
        assert not _same(got, c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, match))   # layer 0 answers otherwise
    with pytest.raises(RuntimeError, match="layer"):
        c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, "any", layer=c.ix.top_layer() + 1)


def _raw_ucosine(n, seed):
    return np.random.default_rng(seed).normal(size=(n, DIM)).astype(np.float32)   # unnormalised: 1 - dot goes negative


def test_negative_radius_runs_every_query_and_fails_where_the_reference_throws():
    n = 1200
    x = _raw_ucosine(n, 21)
    ix, ref, base, rows = _build("ucosine", x, n=n)
    q = _raw_ucosine(24, 22)
    rt = (1 << np.random.default_rng(23).choice(3, n, p=[0.5, 0.3, 0.2])).astype(np.uint32)   # the tag 8: on no id
    qt = (1 << (np.arange(24) % 4)).astype(np.uint32)
    radius = -1.0
    throws = np.array([heap_empty_closed_form(ref, rows, base, q[i], radius, tag_mask(rt, int(qt[i]), "any", n)) for i in range(24)])
    assert throws.any() and not throws.all() and throws[qt == 8].any()   # a candidate-less mask's query throws too: it must not be skipped
    with pytest.raises(HeapEmpty):
        tagged_range(ref, rows, base, q, radius, rt, qt)
    ix.reset_stats()
    with pytest.raises(RuntimeError, match="Heap is empty"):
        ix.range_query_tagged(q, radius, rt, qt)
    assert ix.range_tagged_info()["skipped"] == 0 and ix.range_tagged_info()["launched"] == 24
    # the queries the loop completes: equal lists, the candidate-less mask's queries launched, not skipped
    keep = np.flatnonzero(~throws)
    for match in MODES:
        want = tagged_range(ref, rows, base, q[keep], radius, rt, qt[keep], match)
        assert sum(a.size for a in want[0]) > 0
        ix.reset_stats()
        got = ix.range_query_tagged(q[keep], radius, rt, qt[keep], match)
        assert _same(got, want) and _same(got, _per_mask(ix, q[keep], radius, rt, qt[keep], match, n))
        assert ix.range_tagged_info()["skipped"] == 0 and ix.range_tagged_info()["launched"] == keep.size
    # the C ABI: -1, the message, every array NULL and every count 0
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    qq = np.ascontiguousarray(q)
    counts = np.full(24, 7, np.int32)
    pp_i, pp_d = (ct.c_void_p * 24)(*[0x1234] * 24), (ct.c_void_p * 24)(*[0x1234] * 24)
    assert lib.hnsw_mi355x_range_query_tagged(ix._h, qq.ctypes.data_as(F), 24, DIM, ct.c_float(radius), 0, rt.ctypes.data_as(U), n, qt.ctypes.data_as(U), 0,
                                              pp_i, pp_d, counts.ctypes.data_as(I)) == -1
    assert "Heap is empty" in hnswindex.net_amd.last_error() and (counts == 0).all() and all(p is None for p in pp_i) and all(p is None for p in pp_d)
    # ... and its argument errors
    for args, word in (((None, n, qt.ctypes.data_as(U), 0), "row_tags"), ((rt.ctypes.data_as(U), -1, qt.ctypes.data_as(U), 0), "n_row_tags"),
                       ((rt.ctypes.data_as(U), n, qt.ctypes.data_as(U), 2), "match = 2"), ((rt.ctypes.data_as(U), n, None, 0), "query_tags")):
        counts[:] = 7
        for j in range(24):
            pp_i[j] = pp_d[j] = 0x1234
        assert lib.hnsw_mi355x_range_query_tagged(ix._h, qq.ctypes.data_as(F), 24, DIM, ct.c_float(1.0), 0, *args, pp_i, pp_d, counts.ctypes.data_as(I)) == -1, word
        assert (counts == 0).all() and all(p is None for p in pp_i) and all(p is None for p in pp_d), word
        assert word in hnswindex.net_amd.last_error(), (word, hnswindex.net_amd.last_error())


def test_removals_leave_vacant_slots_untagged_and_rows_added_again_count(cases):
    x = _data("sq_euclid", N, 1)
    import hnswindex
    import oracle
    ix = hnswindex.Index(DIM, "sq_euclid")
    ix.set_collection_size(N); ix.set_max_edges(M); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1); ix.set_allow_removals(True)
    ix.add(x)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=M, min_nn=MIN_NN, collection_size=N, allow_removals=True)
    ref.add(x)
    gone = np.random.default_rng(41).choice(N, 60, replace=False).astype(np.int32)
    ix.remove(gone); ref.remove(gone)
    assert ix.graph_hash() == ref.graph_hash()
    c = cases("sq_euclid")
    radius = c.radii[2]
    assert (c.rt[gone[gone < N_TAGS]] != 0).any()                          # removed slots are still tagged in the caller's array
    for match in MODES:
        want = tagged_range(ref, x, "sq_euclid", c.q, radius, c.rt, c.qt, match)
        assert sum(a.size for a in want[0]) > 50 and not np.isin(np.concatenate(want[0]), gone).any()
        got = ix.range_query_tagged(c.q, radius, c.rt, c.qt, match)
        assert _same(got, want) and _same(got, _per_mask(ix, c.q, radius, c.rt, c.qt, match, N))
    # rows added again: the freed slots are taken, and their words count once more
    again = ix.add(x[gone[:30]])
    assert (ref.add(x[gone[:30]]) == again).all() and ix.graph_hash() == ref.graph_hash() and np.isin(again, gone).all()
    rows_now = x.copy()
    rows_now[again] = x[gone[:30]]
    want = tagged_range(ref, rows_now, "sq_euclid", c.q, radius, c.rt, c.qt, "any")
    got = ix.range_query_tagged(c.q, radius, c.rt, c.qt, "any")
    assert _same(got, want) and _same(got, _per_mask(ix, c.q, radius, c.rt, c.qt, "any", N))


def test_a_partition_of_tags_is_range_query_grouped_and_the_results_lie_in_the_tagged_scan(cases):
    c = cases("cosine")
    radius = c.radii[2]
    rg = np.random.default_rng(51).integers(0, 5, N).astype(np.int32)
    qg = (np.arange(NQ) % 5).astype(np.int32)
    for match in MODES:   # one tag per row: the modes agree, and the groups' lists come back
        part = c.ix.range_query_tagged(c.q, radius, (1 << rg).astype(np.uint32), (1 << qg).astype(np.uint32), match)
        assert _same(part, c.ix.range_query_grouped(c.q, radius, rg, qg, 5)) and sum(a.size for a in part[0]) > 200
    every = c.ix.range_query_tagged(c.q, radius, np.full(N, B31, np.uint32), np.full(NQ, B31 | 1, np.uint32), "any")
    assert _same(every, c.ix.range_query(c.q, radius))                       # every id tagged: the unfiltered call
    for match in MODES:
        got = c.ix.range_query_tagged(c.q, radius, c.rt, c.qt, match)
        scan = c.ix.exact_range_query_tagged(c.q, radius, c.rt, c.qt, match)
        found = 0
        for i in range(NQ):   # every id the traversal returns is in the scan's list, with the same distance bits
            by_id = {int(a): b.tobytes() for a, b in zip(scan[0][i], scan[1][i])}
            assert all(int(a) in by_id and by_id[int(a)] == b.tobytes() for a, b in zip(got[0][i], got[1][i])), i
            found += got[0][i].size
        assert found > 50


def _layers(ref, lv):
    out = []
    for layer in range(int(lv.max()) + 1):
        counts = np.full(lv.size, -1, np.int32)
        edges = np.zeros((lv.size, 2 * M + 2), np.int32)
        for i in np.nonzero(lv >= layer)[0]:
            e = ref.edges(int(i), layer)
            counts[i] = e.size
            edges[i, :e.size] = e
        out.append((counts, edges))
    return out


def test_device_backend_range_search_tagged(cases):
    import hnswindex
    c = cases("sq_euclid", grid=True)
    lv = c.ref.levels()
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=N)
    dev.upload_rows(0, c.x)
    dev.set_graph(lv, _layers(c.ref, lv), M)
    for n_call, match in enumerate(MODES, 1):
        want = c.want(8.0, match)
        dev.reset_stats()
        ids, d, flags = dev.range_search_tagged(c.q, c.ref.entry_point, 8.0, c.rt, c.qt, match)
        assert not flags.any() and _same((ids, d), want)
        none = int(_no_candidate(c.rt, c.qt, match).sum())
        assert dev.range_tagged_info() == {"calls": 1, "masks": MASKS.size, "launched": NQ - none, "skipped": none, "host_finished": 0, "long_finished": 0}
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    counts, flags = np.full(NQ, 7, np.int32), np.full(NQ, 7, np.int32)
    many = np.arange(65537, dtype=np.uint32)
    qmany = np.zeros((65537, DIM), np.float32)
    big_c, big_f = np.zeros(65537, np.int32), np.zeros(65537, np.int32)
    call = lambda q, nq, rt, n_rt, qt, match, cc, ff: lib.hnswdev_range_search_tagged(   # noqa: E731
        dev._ctx, q.ctypes.data_as(F), nq, int(c.ref.entry_point), ct.c_float(8.0), 0, rt, n_rt, qt, match, cc.ctypes.data_as(I), ff.ctypes.data_as(I))
    rt_p, qt_p = c.rt.ctypes.data_as(U), c.qt.ctypes.data_as(U)
    for args, word in (((c.q, NQ, None, N_TAGS, qt_p, 0, counts, flags), "row_tags"), ((c.q, NQ, rt_p, -1, qt_p, 0, counts, flags), "n_row_tags"),
                       ((c.q, NQ, rt_p, N_TAGS, None, 0, counts, flags), "query_tags"), ((c.q, NQ, rt_p, N_TAGS, qt_p, 2, counts, flags), "match = 2"),
                       ((qmany, 65537, rt_p, N_TAGS, many.ctypes.data_as(U), 0, big_c, big_f), "more than 65536 distinct masks")):
        assert call(*args) == -1, word
        assert word in dev.last_error(), (word, dev.last_error())


# ---- closures beyond the sort kernel's table ------------------------------------------------------------------------------------

N_LONG = 4000


def _long_tags(share, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(N_LONG) < share, np.uint32(4), np.uint32(0)).astype(np.uint32) | np.uint32(B31) * (rng.random(N_LONG) < 0.5).astype(np.uint32)


def _long_case(grid, share, radius=None):
    x = _data("sq_euclid", N_LONG, 31, grid)
    ix, ref, base, rows = _build("sq_euclid", x, n=N_LONG)
    q = np.random.default_rng(33).integers(1, 4, (3, DIM)).astype(np.float32) if grid else _data("sq_euclid", 3, 32)
    rt = _long_tags(share, 34)
    qt = np.array([4, 4 | 16, 4], np.uint32)             # the tag 4 decides under "any"; bit 31, on half the rows, is in no mask
    radius = radius or (24.0 if grid else 3.0)
    closures = [a.size for a in ref.range_query(q, radius)[0]]
    want = tagged_range(ref, rows, base, q, radius, rt, qt, "any")
    assert min(closures) > TABLE, closures                # every closure is beyond kRangeSortMax
    return ix, q, rt, qt, radius, want


def test_a_long_closure_whose_allowed_entries_fit_the_table_is_finished_on_the_device(monkeypatch):
    ix, q, rt, qt, radius, want = _long_case(False, 0.05)
    assert all(2 <= a.size <= TABLE for a in want[0]), [a.size for a in want[0]]        # between 2 and kRangeSortMax allowed results
    assert all((np.diff(d) > 0).all() for d in want[1])                                # no two of them tie
    ix.reset_stats()
    got = ix.range_query_tagged(q, radius, rt, qt)
    info, st = ix.range_tagged_info(), ix.stats()
    assert _same(got, want)
    assert info["long_finished"] == 3 and info["host_finished"] == 0 and st["range_device_ordered"] == 3 and st["range_host_ordered"] == 0, (info, st)
    loop = _per_mask(ix, q, radius, rt, qt, "any", N_LONG)
    assert _same(got, loop)
    set_diag(monkeypatch, range_sort_long="0")           # as the other two sorts: handed to the host
    ix.reset_stats()
    back = ix.range_query_tagged(q, radius, rt, qt)
    info, st = ix.range_tagged_info(), ix.stats()
    assert info["long_finished"] == 0 and info["host_finished"] == 3 and st["range_host_ordered"] == 3, (info, st)
    assert _same(back, got) and _same(back, loop)


def test_a_long_closure_whose_allowed_entries_tie_is_handed_back_whole():
    ix, q, rt, qt, radius, want = _long_case(True, 0.05)
    assert all(2 <= a.size <= TABLE for a in want[0]) and all((np.diff(d) == 0).any() for d in want[1])   # allowed results tie in every list
    ix.reset_stats()
    got = ix.range_query_tagged(q, radius, rt, qt)
    info = ix.range_tagged_info()
    assert _same(got, want) and _same(got, _per_mask(ix, q, radius, rt, qt, "any", N_LONG))
    assert info["long_finished"] == 0 and info["host_finished"] == 3, info


def test_a_long_closure_with_more_allowed_entries_than_the_table_goes_to_the_host():
    ix, q, rt, qt, radius, want = _long_case(False, 0.6, 4.0)
    assert all(a.size > TABLE for a in want[0]), [a.size for a in want[0]]
    ix.reset_stats()
    got = ix.range_query_tagged(q, radius, rt, qt)
    info = ix.range_tagged_info()
    assert _same(got, want) and _same(got, _per_mask(ix, q, radius, rt, qt, "any", N_LONG))
    assert info["long_finished"] == 0 and info["host_finished"] == 3, info
    # the same tags at the first test's radius: allowed counts on both sides of the table's size in one call -- each list goes where
    # the model says (on the device: at most kRangeSortMax allowed results and no tie among them)
    ref_r = 3.0
    import oracle
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=M, min_nn=MIN_NN, collection_size=N_LONG)
    x = _data("sq_euclid", N_LONG, 31)
    ref.add(x)
    want = tagged_range(ref, x, "sq_euclid", q, ref_r, rt, qt, "any")
    sizes = [a.size for a in want[0]]
    on_device = sum(int(2 <= a.size <= TABLE and (np.diff(d) > 0).all()) for a, d in zip(*want))
    assert min(a.size for a in ref.range_query(q, ref_r)[0]) > TABLE and max(sizes) > TABLE and 1500 < min(sizes) <= TABLE and 1 <= on_device <= 2, sizes
    ix.reset_stats()
    got = ix.range_query_tagged(q, ref_r, rt, qt)
    info = ix.range_tagged_info()
    assert _same(got, want) and _same(got, _per_mask(ix, q, ref_r, rt, qt, "any", N_LONG))
    assert info["long_finished"] == on_device and info["host_finished"] == 3 - on_device, info


def test_jobs_launched_again_for_a_full_arena_keep_their_own_masks():
    """range_batch's second pass: 320 closures of 4 096 entries exceed the arena's floor of 2^20, so the jobs that found it full run
    again as a proper subset of the call's -- and the sort kernel's per-job mask table must name THEIR masks.  Expected: the
    per-mask filtered calls, 80 queries each (one launch: 80 x 4 096 < 2^20)."""
    import hnswindex
    n, dim, nq = 4096, 8, 320
    masks = np.array([1, 2, 0b110, B31 | 1], np.uint32)
    x, q = uniform(n, dim, 51), uniform(nq, dim, 52)
    ix = hnswindex.Index(dim, "sq_euclid")
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    ix.add(x)
    rng = np.random.default_rng(53)
    rt = np.zeros(n, np.uint32)
    for bit, share in ((0, 0.4), (1, 0.3), (2, 0.2), (31, 0.1)):
        rt |= np.where(rng.random(n) < share, np.uint32(1 << bit), np.uint32(0)).astype(np.uint32)
    qt = masks[np.random.default_rng(54).permutation(np.arange(nq) % masks.size)]
    radius = float(dim) + 1.0            # rows and queries lie in [0, 1)^8: no squared distance exceeds 8
    assert nq * n > 1 << 20 and (nq // masks.size) * n < 1 << 20
    ix.reset_stats()
    got = ix.range_query_tagged(q, radius, rt, qt, "any")   # first: the arena is sized by the call before, and there is none
    assert ix.stats()["range_launches"] > 1 and ix.range_tagged_info()["launched"] == nq
    for m in masks:
        sel = np.flatnonzero(qt == m)
        allowed = tag_mask(rt, int(m), "any", n)
        ix.reset_stats()
        want = ix.range_query(q[sel], radius, allowed=allowed)
        assert sel.size == 80 and ix.stats()["range_launches"] == 1, m
        assert all(a.size == int(allowed.sum()) for a in want[0]), m            # every candidate of the mask: the closure is the graph
        assert _same(([got[0][i] for i in sel], [got[1][i] for i in sel]), want), m
