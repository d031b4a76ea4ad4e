"""GPU tier: range_query_grouped (hnsw_mi355x_range_query_grouped / Index.range_query_grouped) -- a group filter per query, every
group in one device traversal -- against the plain-Python statement of its contract (tests/grouped_range_model.py: the filtered
RangeQuery of the reference, one group at a time) on graphs whose hash equals the CPU oracle's, and against the product's own
loop of per-group filtered calls: counts, ids, distance bits and the order among equal distances.  Every case asserts its
precondition from the model before it compares.

The model restates layer 0 only, so the layer-1 case is held to the product's per-group loop alone.  No input of the six row
kinds gives a -0 distance inside a closure (sq_euclid sums squares, the cosine kinds return 1 - x, which rounds to +0), so the
"-0 anywhere" hand-back of range_sort_grouped_kernel is reached here only through range_finish=0 and radius < 0, which take the
same host finish."""
import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from grouped_range_model import HeapEmpty, group_mask, grouped_range, heap_empty_closed_form

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 2000, 16, 8, 20
N_GROUPS, SMALL, EMPTY = 5, 3, 4     # groups 0 .. 2 hold about 60 / 30 / 10 %, group 3 seven ids, group 4 none
N_LABELS = N - 50                    # row_group is shorter than the graph: the last 50 ids have no group
F16 = {"sq_euclid_f16": "sq_euclid", "ucosine_f16": "ucosine"}
NQ = 20


def _data(metric, n, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, DIM)).astype(np.float32) if grid else uniform(n, DIM, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _labels(seed, n_labels=N_LABELS):
    rng = np.random.default_rng(seed)
    rg = rng.choice(3, n_labels, p=[0.6, 0.3, 0.1]).astype(np.int32)
    picked = rng.choice(n_labels, 7 + 40 + 10, replace=False)
    rg[picked[:7]] = SMALL
    rg[picked[7:47]] = -1
    rg[picked[47:]] = N_GROUPS + 2    # past n_groups: no group either
    return rg


def _query_groups(nq, seed):
    return np.random.default_rng(seed).permutation(np.arange(nq) % N_GROUPS).astype(np.int32)


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


def _per_group(ix, q, radius, rg, qg, n, layer=0):
    """The loop the call replaces: one filtered call per group, lists put back in the caller's order."""
    ids, d = [None] * q.shape[0], [None] * q.shape[0]
    for g in np.unique(qg):
        sel = np.flatnonzero(qg == g)
        a, b = ix.range_query(q[sel], radius, allowed=group_mask(rg, int(g), n), layer=layer)
        for w, ai, bi in zip(sel, a, b):
            ids[w], d[w] = ai, bi
    return ids, d


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
    """One metric's data, index, oracle, labels and queries, and the model's answers (computed once, shared by the tests)."""

    def __init__(self, metric, grid=False):
        self.metric = metric
        self.x = _data(metric, N, 2 if grid else 1, grid)
        self.ix, self.ref, self.base, self.rows = _build(metric, self.x)
        self.q = np.random.default_rng(8).integers(1, 4, (NQ, DIM)).astype(np.float32) if grid else _data(metric, NQ, 9)
        self.rg, self.qg = _labels(3), _query_groups(NQ, 4)
        self._want = {}
        self.radii = None if grid else _radii(self.ref, self.base, self.rows, self.q)

    def want(self, radius):
        if radius not in self._want:
            self._want[radius] = grouped_range(self.ref, self.rows, self.base, self.q, radius, self.rg, self.qg, N_GROUPS)
        return self._want[radius]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            cache[(metric, grid)] = Case(metric, grid)
        return cache[(metric, grid)]
    return get


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"])
def test_grouped_range_is_the_model_and_the_per_group_filtered_calls(cases, metric):
    c = cases(metric)
    n_empty = int((c.qg == EMPTY).sum())
    assert n_empty >= 2 and (c.rg == EMPTY).sum() == 0 and (c.rg == SMALL).sum() == 7 and c.rg.size < N
    means = []
    for radius in c.radii:
        means.append(np.mean([a.size for a in c.ref.range_query(c.q, radius)[0]]))
        want = c.want(radius)
        c.ix.reset_stats()
        got = c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS)
        info, st = c.ix.range_grouped_info(), c.ix.stats()
        assert _same(got, want), (metric, radius)
        assert info["calls"] == 1 and info["launched"] == NQ - n_empty and info["skipped"] == n_empty and st["range_launches"] >= 1, (info, st)
        assert _same(got, _per_group(c.ix, c.q, radius, c.rg, c.qg, N)), (metric, radius)
        assert all(got[0][i].size == 0 for i in np.flatnonzero(c.qg == EMPTY))
    # the closures the radii were chosen for: about 0.4, 24 and 340 ids (within a factor of two)
    assert all(t / 2 < m < t * 2 for t, m in zip(TARGETS, means)), means
    assert sum(a.size for a in c.want(c.radii[2])[0]) > 200


def test_ties_among_allowed_results_are_replayed_on_the_device(cases):
    c = cases("sq_euclid", grid=True)
    radius = 8.0
    want = c.want(radius)
    tied = sum(int(a.size >= 2 and (np.diff(d) == 0).any()) for a, d in zip(*want))
    closures = [a.size for a in c.ref.range_query(c.q, radius)[0]]
    assert tied >= 5 and max(closures) <= 2048                         # two allowed results tie; every closure fits a wave's table
    c.ix.reset_stats()
    got = c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS)
    info, st = c.ix.range_grouped_info(), c.ix.stats()
    assert _same(got, want)
    assert st["range_device_ordered"] >= tied and st["range_host_ordered"] == 0 and info["host_finished"] == 0, (info, st)
    assert _same(got, _per_group(c.ix, c.q, radius, c.rg, c.qg, N))


def test_every_other_path_gives_the_same_answers(cases, monkeypatch):
    c = cases("sq_euclid", grid=True)
    radius = 8.0
    want = c.want(radius)
    with_results = sum(int(a.size >= 2) for a in want[0])
    for finish in ("0", "1"):
        set_diag(monkeypatch, range_finish=finish)
        c.ix.reset_stats()
        assert _same(c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS), want), finish
        assert c.ix.range_grouped_info()["host_finished"] >= (with_results if finish == "0" else 1), finish
        monkeypatch.undo()
    iy, _, _, _ = _build("sq_euclid", c.x, set_device_traversal=False)
    iy.reset_stats()
    assert _same(iy.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS), want)
    assert iy.stats()["range_launches"] == 0 and iy.range_grouped_info()["calls"] == 0


def test_layer_one_equals_the_per_group_loop(cases):
    c = cases("sq_euclid")
    assert c.ix.top_layer() >= 1
    radius = c.radii[2]
    got = c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS, layer=1)
    loop = _per_group(c.ix, c.q, radius, c.rg, c.qg, N, layer=1)
    assert _same(got, loop) and sum(a.size for a in got[0]) > 0
    assert not _same(got, c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS))   # layer 0 answers otherwise
    with pytest.raises(RuntimeError, match="layer"):
        c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS, layer=c.ix.top_layer() + 1)


def test_a_closure_beyond_the_device_table_is_finished_on_the_host():
    n = 4000
    x = _data("sq_euclid", n, 31)
    ix, ref, base, rows = _build("sq_euclid", x, n=n)
    q = _data("sq_euclid", 3, 32)
    rg = (np.arange(n) % 2).astype(np.int32)
    qg = np.array([0, 1, 0], np.int32)
    radius = 3.0
    closures = [a.size for a in ref.range_query(q, radius)[0]]
    want = grouped_range(ref, rows, base, q, radius, rg, qg, 2)
    assert min(closures) > 2048 and min(a.size for a in want[0]) >= 2, closures   # beyond kRangeSortMax, two or more allowed
    ix.reset_stats()
    got = ix.range_query_grouped(q, radius, rg, qg, 2)
    assert _same(got, want)
    assert ix.range_grouped_info()["host_finished"] == 3 and ix.stats()["range_host_ordered"] == 3
    assert _same(got, _per_group(ix, q, radius, rg, qg, n))


def _raw_ucosine(n, seed):
    return np.random.default_rng(seed).normal(size=(n, DIM)).astype(np.float32)   # unnormalised: 1 - dot goes negative


def test_negative_radius_runs_every_query_and_fails_where_the_reference_throws():
    n = 1200
    x = _raw_ucosine(n, 21)
    ix, ref, base, rows = _build("ucosine", x, n=n)
    q = _raw_ucosine(24, 22)
    rg = np.random.default_rng(23).choice(3, n, p=[0.5, 0.3, 0.2]).astype(np.int32)   # group 3: no id
    qg = (np.arange(24) % 4).astype(np.int32)
    radius = -1.0
    throws = np.array([heap_empty_closed_form(ref, rows, base, q[i], radius, group_mask(rg, int(qg[i]), n)) for i in range(24)])
    assert throws.any() and not throws.all() and throws[qg == 3].any()   # an EMPTY group's query throws too: it must not be skipped
    with pytest.raises(HeapEmpty):
        grouped_range(ref, rows, base, q, radius, rg, qg, 4)
    ix.reset_stats()
    with pytest.raises(RuntimeError, match="Heap is empty"):
        ix.range_query_grouped(q, radius, rg, qg, 4)
    assert ix.range_grouped_info()["skipped"] == 0 and ix.range_grouped_info()["launched"] == 24
    # the queries the loop completes: equal lists, the empty group's queries launched, not skipped
    keep = np.flatnonzero(~throws)
    want = grouped_range(ref, rows, base, q[keep], radius, rg, qg[keep], 4)
    assert sum(a.size for a in want[0]) > 0
    ix.reset_stats()
    got = ix.range_query_grouped(q[keep], radius, rg, qg[keep], 4)
    assert _same(got, want) and _same(got, _per_group(ix, q[keep], radius, rg, qg[keep], n))
    assert ix.range_grouped_info()["skipped"] == 0 and ix.range_grouped_info()["launched"] == keep.size
    # the C ABI: -1, the message, every array NULL and every count 0
    import ctypes as ct
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    qq = np.ascontiguousarray(q)
    counts = np.full(24, 7, np.int32)
    pp_i, pp_d = (ct.c_void_p * 24)(*[0x1234] * 24), (ct.c_void_p * 24)(*[0x1234] * 24)
    assert lib.hnsw_mi355x_range_query_grouped(ix._h, qq.ctypes.data_as(F), 24, DIM, ct.c_float(radius), 0, rg.ctypes.data_as(I), n, qg.ctypes.data_as(I), 4,
                                               pp_i, pp_d, counts.ctypes.data_as(I)) == -1
    assert "Heap is empty" in hnswindex.net_amd.last_error() and (counts == 0).all() and all(p is None for p in pp_i) and all(p is None for p in pp_d)


def test_removals_leave_vacant_slots_in_no_group(cases):
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
    want = grouped_range(ref, x, "sq_euclid", c.q, radius, c.rg, c.qg, N_GROUPS)
    assert sum(a.size for a in want[0]) > 100 and not np.isin(np.concatenate(want[0]), gone).any()
    got = ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS)
    assert _same(got, want) and _same(got, _per_group(ix, c.q, radius, c.rg, c.qg, N))


def test_one_group_equals_the_unfiltered_call_and_the_results_lie_in_the_grouped_scan(cases):
    c = cases("cosine")
    radius = c.radii[2]
    one = c.ix.range_query_grouped(c.q, radius, np.zeros(N, np.int32), np.zeros(NQ, np.int32), 1)
    assert _same(one, c.ix.range_query(c.q, radius)) and sum(a.size for a in one[0]) > 500
    got = c.ix.range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS)
    scan = c.ix.exact_range_query_grouped(c.q, radius, c.rg, c.qg, N_GROUPS)
    found = 0
    for i in range(NQ):   # every id the traversal returns is in the scan's list, with the same distance bits
        by_id = {int(a): b.tobytes() for a, b in zip(scan[0][i], scan[1][i])}
        assert all(int(a) in by_id and by_id[int(a)] == b.tobytes() for a, b in zip(got[0][i], got[1][i])), i
        found += got[0][i].size
    assert found > 100


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


def test_device_backend_range_search_grouped(cases):
    import hnswindex
    c = cases("sq_euclid", grid=True)
    lv = c.ref.levels()
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=N)
    dev.upload_rows(0, c.x)
    dev.set_graph(lv, _layers(c.ref, lv), M)
    want = c.want(8.0)
    ids, d, flags = dev.range_search_grouped(c.q, c.ref.entry_point, 8.0, c.rg, c.qg, N_GROUPS)
    assert not flags.any() and _same((ids, d), want)
    n_empty = int((c.qg == EMPTY).sum())
    assert dev.range_grouped_info() == {"calls": 1, "launched": NQ - n_empty, "skipped": n_empty, "host_finished": 0}
    with pytest.raises(RuntimeError, match=r"query_group\[0\]"):
        dev.range_search_grouped(c.q, c.ref.entry_point, 8.0, c.rg, np.full(NQ, N_GROUPS, np.int32), N_GROUPS)
    with pytest.raises(RuntimeError, match="65536"):
        dev.range_search_grouped(c.q, c.ref.entry_point, 8.0, c.rg, c.qg, 65537)


def test_jobs_launched_again_for_a_full_arena_keep_their_own_groups():
    """range_batch's second pass: 320 closures of 4 096 entries exceed the arena's floor of 2^20, so the jobs that found it full run
    again as a proper subset of the call's -- and the sort kernel's per-job group table must name THEIR groups.  Expected: the
    per-group filtered calls, 80 queries each (one launch: 80 x 4 096 < 2^20)."""
    import hnswindex
    n, dim, nq, n_groups = 4096, 8, 320, 4
    x, q = uniform(n, dim, 51), uniform(nq, dim, 52)
    ix = hnswindex.Index(dim, "sq_euclid")
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    ix.add(x)
    rg = np.random.default_rng(53).integers(0, n_groups, n).astype(np.int32)
    qg = np.random.default_rng(54).permutation(np.arange(nq) % n_groups).astype(np.int32)
    radius = float(dim) + 1.0            # rows and queries lie in [0, 1)^8: no squared distance exceeds 8
    assert nq * n > 1 << 20 and (nq // n_groups) * n < 1 << 20
    ix.reset_stats()
    got = ix.range_query_grouped(q, radius, rg, qg, n_groups)   # first: the arena is sized by the call before, and there is none
    assert ix.stats()["range_launches"] > 1 and ix.range_grouped_info()["launched"] == nq
    for g in range(n_groups):
        sel = np.flatnonzero(qg == g)
        ix.reset_stats()
        want = ix.range_query(q[sel], radius, allowed=group_mask(rg, g, n))
        assert sel.size == 80 and ix.stats()["range_launches"] == 1, g
        assert all(a.size == int((rg == g).sum()) for a in want[0]), g          # every id of the group: the closure is the graph
        assert _same(([got[0][i] for i in sel], [got[1][i] for i in sel]), want), g
