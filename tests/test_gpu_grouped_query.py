"""GPU tier: knn_query_grouped (hnsw_mi355x_knn_query_grouped / Index.knn_query_grouped) -- a group filter per query, every group in
one device traversal -- against the plain-Python statement of its contract (tests/grouped_query_model.py) on graphs whose hash equals
the CPU oracle's, and against the per-group filtered calls it replaces: ids and distance bits.  The shapes are those of
tests/test_gpu_filtered_query.py; the labels cover what the predicate can meet: groups of about 60 / 30 / 10 % of the ids, a group
of 7 ids (fewer than the beam), a group number no row carries, rows labelled -1 and past n_groups, a row_group shorter than the
graph."""
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from grouped_query_model import group_mask, grouped_knn_batch

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 1200, 16, 8, 20
N_GROUPS, SMALL, EMPTY = 5, 3, 4     # groups 0 .. 2 hold about 60 / 30 / 10 %, group 3 seven ids, group 4 none
N_LABELS = N - 50                    # row_group is shorter than the graph: the last 50 ids have no group
F16 = {"sq_euclid_f16": "sq_euclid"}


def _data(metric, n, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, DIM)).astype(np.float32) if grid else uniform(n, DIM, seed)
    return normalize_f32(x) if metric == "ucosine" else x


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


def _index(dim, metric, m, **knobs):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(N); ix.set_max_edges(m); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    return ix


def _build(metric, x, m=M, **knobs):
    """The index, the oracle it equals, and (base metric, rows) as the models take them (f16: the rows rounded to binary16)."""
    import oracle
    ix = _index(x.shape[1], metric, m, **knobs)
    ix.add(x)
    base = F16.get(metric, metric)
    rows = x.astype(np.float16).astype(np.float32) if metric in F16 else x
    ref = oracle.OracleIndex(x.shape[1], base, max_edges=m, min_nn=MIN_NN, collection_size=N)
    ref.add(rows)
    assert ix.graph_hash() == ref.graph_hash(), metric
    return ix, ref, base, rows


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _per_group(ix, q, k, rg, qg, n_groups=N_GROUPS, layer=0):
    """The loop the call replaces: one filtered call per group, rows scattered back; and the lock-step launches those calls ran."""
    ids = np.full((q.shape[0], k), -1, np.int32)
    d = np.full((q.shape[0], k), np.nan, np.float32)
    lockstep = 0
    for g in np.unique(qg):
        sel = qg == g
        ix.reset_stats()
        ids[sel], d[sel] = ix.knn_query(q[sel], k, allowed=group_mask(rg, int(g), n_groups, N), layer=layer)
        lockstep += ix.stats()["launches"]
    return (ids, d), lockstep


class Case:
    """One metric's data, index, oracle, labels and queries, and the model's answers (computed once, shared by the tests)."""

    def __init__(self, metric):
        self.metric = metric
        self.x = _data(metric, N, 1)
        self.ix, self.ref, self.base, self.rows = _build(metric, self.x)
        self.q = _data(metric, 24, 9)
        self.rg, self.qg = _labels(3), _query_groups(24, 4)
        self._want = {}

    def want(self, k):
        if k not in self._want:
            w = grouped_knn_batch(self.ref, self.rows, self.base, self.q, k, MIN_NN, self.rg, self.qg, N_GROUPS)
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


def test_the_labels_cover_every_case_of_the_predicate():
    rg, qg = _labels(3), _query_groups(24, 4)
    share = np.bincount(rg[(rg >= 0) & (rg < N_GROUPS)], minlength=N_GROUPS) / N
    assert 0.5 < share[0] < 0.65 and 0.2 < share[1] < 0.35 and 0.05 < share[2] < 0.15
    assert (rg == SMALL).sum() == 7 < MIN_NN and (rg == EMPTY).sum() == 0
    assert (rg == -1).sum() == 40 and (rg >= N_GROUPS).sum() == 10 and rg.size < N
    assert all((qg == g).sum() >= 4 for g in range(N_GROUPS))


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_grouped_query_is_the_model_and_the_per_group_filtered_calls(cases, metric):
    c = cases(metric)
    for k in (5, 40):   # below and above MinNN
        c.ix.reset_stats()
        got = c.ix.knn_query_grouped(c.q, k, c.rg, c.qg, N_GROUPS)
        st, info = c.ix.stats(), c.ix.knn_grouped_info()
        assert _same(got, c.want(k)), (metric, k)
        loop, loop_lockstep = _per_group(c.ix, c.q, k, c.rg, c.qg)
        assert _same(got, loop), (metric, k)
        for i in range(24):   # every returned id carries the query's group
            ids = got[0][i][got[0][i] >= 0]
            assert ids.max(initial=-1) < N_LABELS and (c.rg[ids] == c.qg[i]).all(), (metric, k, i)
        empty = c.qg == EMPTY
        assert (got[0][empty] == -1).all() and np.isnan(got[1][empty]).all()
        assert ((got[0][c.qg == SMALL] >= 0).sum(axis=1) <= 7).all()
        assert info["calls"] == 1 and info["skipped"] == int(empty.sum()) and info["launched"] == 24 - int(empty.sum()), info
        assert st["search_launches"] >= 1, st
        if loop_lockstep == 0:   # the device traversal answered the loop: then it answered the grouped call as well
            assert st["launches"] == 0 and info["handbacks"] == 0, (metric, k, st, info)


def test_n_groups_from_the_arrays_and_argument_errors(cases):
    c = cases("sq_euclid")
    assert _same(c.ix.knn_query_grouped(c.q, 5, c.rg, c.qg), c.want(5))            # the largest value plus one covers every group named
    nothing = c.ix.knn_query_grouped(c.q, 5, c.rg, np.full(24, EMPTY), N_GROUPS)    # no query's group holds an id: no launch at all
    assert (nothing[0] == -1).all() and np.isnan(nothing[1]).all()
    for k in (0, -2):
        assert c.ix.knn_query_grouped(c.q, k, c.rg, c.qg, N_GROUPS)[0].shape == (24, 0)
    c.ix.reset_stats()
    with pytest.raises(RuntimeError, match=r"query_group\[3\] = 5 is outside 0 .. n_groups - 1 = 4"):
        c.ix.knn_query_grouped(c.q, 5, c.rg, np.where(np.arange(24) == 3, 5, 0), N_GROUPS)
    with pytest.raises(RuntimeError, match="n_groups = 70000 is outside 1 .. 65536"):
        c.ix.knn_query_grouped(c.q, 5, c.rg, c.qg, 70000)
    assert c.ix.stats()["search_launches"] == 0 and c.ix.knn_grouped_info()["calls"] == 0   # rejected before anything ran


def test_entry_point_in_another_group_and_ties():
    """The grid data of the filtered tests (equal distances abound), and every query's layer-0 entry -- the descent's answer -- in
    a group that is not the query's: the entry is a candidate only."""
    for grid in (False, True):
        x = _data("sq_euclid", N, 2 if grid else 1, grid)
        ix, ref, base, rows = _build("sq_euclid", x)
        q = _data("sq_euclid", 16, 5, grid)
        rg = np.random.default_rng(4).integers(0, 3, N).astype(np.int32)
        entries = [ref.find_entry_point(0, qi) for qi in q]
        qg = np.array([(rg[e] + 1 + i % 2) % 3 for i, e in enumerate(entries)], np.int32)
        assert (rg[entries] != qg).all()
        for k in (10, 30):
            assert _same(ix.knn_query_grouped(q, k, rg, qg, 3), grouped_knn_batch(ref, rows, base, q, k, MIN_NN, rg, qg, 3)), (grid, k)


def test_lists_beyond_64_ids():
    """MaxEdges = 60 at dim 64: layer-0 lists of up to 120 ids, past the overlapped form -- the labels are read after the distances
    there."""
    dim, m = 64, 60
    x, q = uniform(N, dim, 31), uniform(10, dim, 32)
    ix, ref, base, rows = _build("cosine", x, m)
    assert sum(ref.edges(i, 0).size > 64 for i in range(N)) > N // 4
    rg, qg = _labels(12), _query_groups(10, 13)
    for k in (5, 40):
        ix.reset_stats()
        got = ix.knn_query_grouped(q, k, rg, qg, N_GROUPS)
        st = ix.stats()
        assert _same(got, grouped_knn_batch(ref, rows, base, q, k, MIN_NN, rg, qg, N_GROUPS)), k
        loop, loop_lockstep = _per_group(ix, q, k, rg, qg)
        assert _same(got, loop), k
        assert st["search_launches"] >= 1 and (loop_lockstep > 0 or st["launches"] == 0), (k, st)


def test_a_wave_takes_several_jobs_of_different_groups(cases):
    """8 192 queries, more than the waves any kernel form keeps resident: every wave takes several jobs, of different groups, one
    after the other -- a group register kept from the job before, or a visited set not cleared, shows here."""
    c = cases("sq_euclid")
    nq = 8192
    q = _data("sq_euclid", nq, 17)
    rg = np.random.default_rng(18).choice(3, N, p=[0.6, 0.3, 0.1]).astype(np.int32)
    qg = np.random.default_rng(19).integers(0, 3, nq).astype(np.int32)
    c.ix.reset_stats()
    got = c.ix.knn_query_grouped(q, 10, rg, qg, 3)
    info = c.ix.knn_grouped_info()
    assert info["launched"] == nq and info["skipped"] == 0
    loop, _ = _per_group(c.ix, q, 10, rg, qg, 3)
    assert _same(got, loop)
    assert (rg[got[0]] == qg[:, None]).all()


def test_layer_1(cases):
    c = cases("sq_euclid")
    top = c.ix.top_layer()
    assert top >= 1
    for k in (5, 40):
        got = c.ix.knn_query_grouped(c.q, k, c.rg, c.qg, N_GROUPS, layer=1)
        loop, _ = _per_group(c.ix, c.q, k, c.rg, c.qg, layer=1)
        assert _same(got, loop), k
        assert np.isin(got[0][got[0] >= 0], np.flatnonzero(c.ref.levels() >= 1)).all()
        assert not _same(got, c.want(k))
    for layer in (-1, top + 1):
        with pytest.raises(RuntimeError, match=f"layer {layer} is outside 0 .. {top}"):
            c.ix.knn_query_grouped(c.q, 5, c.rg, c.qg, N_GROUPS, layer=layer)
        with pytest.raises(RuntimeError, match=f"layer {layer} is outside 0 .. {top}"):
            c.ix.knn_query(c.q, 5, allowed=c.rg == 0, layer=layer)


def _layers(ref, lv, m):
    """The oracle's graph as (counts, edges) per layer, the layout of DeviceBackend.set_graph."""
    out = []
    for layer in range(int(lv.max()) + 1):
        counts = np.full(lv.size, -1, np.int32)
        edges = np.zeros((lv.size, 2 * m + 2), np.int32)
        for i in np.nonzero(lv >= layer)[0]:
            e = ref.edges(int(i), layer)
            counts[i] = e.size
            edges[i, :e.size] = e
        out.append((counts, edges))
    return out


def test_device_backend_knn_search_grouped(cases):
    """The inner boundary: a host-supplied graph, hnswdev_knn_search_grouped; bad arguments are messages, not launches."""
    import ctypes as ct
    import hnswindex
    c = cases("cosine")
    lv = c.ref.levels()
    dev = hnswindex.DeviceBackend(DIM, "cosine", capacity=N)
    dev.upload_rows(0, c.x)
    dev.set_graph(lv, _layers(c.ref, lv, M), M)
    ep = c.ref.entry_point
    ids, d, flags = dev.knn_search_grouped(c.q, ep, 32, 10, c.rg, c.qg, N_GROUPS)
    assert (flags == 0).all()
    assert _same((ids, d), grouped_knn_batch(c.ref, c.rows, c.base, c.q, 10, 32, c.rg, c.qg, N_GROUPS))
    assert dev.knn_grouped_info() == {"calls": 1, "launched": 24 - int((c.qg == EMPTY).sum()), "skipped": int((c.qg == EMPTY).sum()), "handbacks": 0}
    for g in range(N_GROUPS):   # ... and row by row the filtered call of the same boundary
        sel = c.qg == g
        f_ids, f_d, _ = dev.knn_search(c.q[sel], ep, 32, 10, allowed=group_mask(c.rg, g, N_GROUPS, N))
        assert _same((ids[sel], d[sel]), (f_ids, f_d)), g
    ids, d, flags = dev.knn_search_grouped(c.q, ep, 32, 10, c.rg, np.full(24, EMPTY), N_GROUPS)
    assert (ids == -1).all() and np.isnan(d).all() and (flags == 0).all()
    # (every query skipped: a call and 24 skipped queries more, no launch)
    assert dev.knn_grouped_info() == {"calls": 2, "launched": 24 - int((c.qg == EMPTY).sum()), "skipped": int((c.qg == EMPTY).sum()) + 24, "handbacks": 0}
    launches = dev.stats()["search_launches"]
    with pytest.raises(RuntimeError, match="knn_search_grouped: bad argument"):
        dev.knn_search_grouped(c.q, N + 5, 32, 10, c.rg, c.qg, N_GROUPS)           # entry point outside the graph
    with pytest.raises(RuntimeError, match="knn_search_grouped: bad argument"):
        dev.knn_search_grouped(c.q, ep, 8, 10, c.rg, c.qg, N_GROUPS)               # k_beam < k_out
    with pytest.raises(RuntimeError, match=r"knn_search_grouped: query_group\[0\] = \d+ is outside 0 .. n_groups - 1 = 2"):
        dev.knn_search_grouped(c.q, ep, 32, 10, c.rg, c.qg + 3, 3)
    with pytest.raises(RuntimeError, match="knn_search_grouped: n_groups = 0 is outside 1 .. 65536"):
        dev.knn_search_grouped(c.q, ep, 32, 10, c.rg, c.qg, 0)
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    o_ids, o_d, o_f = np.full((24, 10), 7, np.int32), np.full((24, 10), 7.0, np.float32), np.full(24, 7, np.int32)
    rg = np.ascontiguousarray(c.rg)
    good = dict(q=c.q.ctypes.data_as(F), rg=rg.ctypes.data_as(I), qg=c.qg.ctypes.data_as(I), ids=o_ids.ctypes.data_as(I), d=o_d.ctypes.data_as(F),
                f=o_f.ctypes.data_as(I))
    for null, message in (("rg", "row_group must not be NULL"), ("qg", "query_group must not be NULL"), ("q", "null argument"), ("ids", "null argument"),
                          ("d", "null argument"), ("f", "null argument")):
        a = dict(good, **{null: None})
        assert lib.hnswdev_knn_search_grouped(dev._ctx, a["q"], 24, ep, 32, 10, 0, a["rg"], rg.size, a["qg"], N_GROUPS, a["ids"], a["d"], a["f"]) == -1, null
        assert message in dev.last_error(), (null, dev.last_error())
    assert lib.hnswdev_knn_search_grouped(dev._ctx, good["q"], 24, ep, 32, 10, 0, good["rg"], -1, good["qg"], N_GROUPS, good["ids"], good["d"], good["f"]) == -1
    assert (o_ids == 7).all() and (o_d == 7.0).all() and (o_f == 7).all()
    assert dev.stats()["search_launches"] == launches


def test_forced_handbacks_give_the_same_answers(cases, monkeypatch):
    c = cases("cosine")
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    c.ix.reset_stats()
    for k in (5, 40):
        assert _same(c.ix.knn_query_grouped(c.q, k, c.rg, c.qg, N_GROUPS), c.want(k)), k
    info, st = c.ix.knn_grouped_info(), c.ix.stats()
    assert info["handbacks"] > 0 and st["search_overflows"] == info["handbacks"] and st["launches"] > 0, (info, st)


def test_two_contexts_with_forced_handbacks(cases, monkeypatch):
    """Sharded over two contexts AND jobs handed back: the shards are gathered to the primary, where the host traversal redoes them."""
    c = cases("cosine")
    two = _index(DIM, c.metric, M, set_devices=2)
    two.add(c.x)
    assert two.graph_hash() == c.ref.graph_hash()
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    two.reset_stats()
    for k in (5, 40):
        assert _same(two.knn_query_grouped(c.q, k, c.rg, c.qg, N_GROUPS), c.want(k)), k
    info = two.knn_grouped_info()   # (summed over the contexts)
    assert two.stats()["search_overflows"] + two.stats_at(1)["search_overflows"] > 0 and info["handbacks"] > 0, info
    assert two.stats_at(1)["search_launches"] >= 2 and two.stats()["launches"] > 0


def _other_path(c, **knobs):
    ix = _index(DIM, c.metric, M, **knobs)
    ix.add(c.x)
    assert ix.graph_hash() == c.ref.graph_hash()
    ix.reset_stats()
    for k in (5, 40):
        assert _same(ix.knn_query_grouped(c.q, k, c.rg, c.qg, N_GROUPS), c.want(k)), (knobs, k)
    return ix.stats(), ix.knn_grouped_info()


def test_hashed_visited_sets_host_traversal_and_two_contexts(cases, monkeypatch):
    c = cases("ucosine")
    set_diag(monkeypatch, vis_hash="1")
    st, _ = _other_path(c)
    assert st["visited_hash_launches"] > 0
    monkeypatch.undo()
    st, info = _other_path(c, set_device_traversal=False)
    assert st["search_launches"] == 0 and info["calls"] == 0
    # two contexts: 12 queries each, and the shuffled groups do not line up with the bound between the shards
    assert len(set(c.qg[:12].tolist())) == len(set(c.qg[12:].tolist())) == N_GROUPS
    _, info = _other_path(c, set_devices=2)
    assert info["calls"] == 4 and info["launched"] + info["skipped"] == 48, info


def test_after_removals_the_stale_labels_of_removed_ids_count_for_nothing():
    x = _data("sq_euclid", N, 1)
    ix = _index(DIM, "sq_euclid", M, set_allow_removals=True)
    ix.add(x)
    rg, qg = _labels(3), _query_groups(24, 4)
    q = _data("sq_euclid", 24, 9)
    rng = np.random.default_rng(21)
    gone = np.concatenate([rng.choice(np.flatnonzero(rg == g), n, replace=False) for g, n in ((0, 60), (1, 28), (2, 10), (SMALL, 2))])
    before = ix.knn_query_grouped(q, 5, rg, qg, N_GROUPS)
    ix.remove(gone)
    for k in (5, 40):
        ix.reset_stats()
        got = ix.knn_query_grouped(q, k, rg, qg, N_GROUPS)
        assert ix.knn_grouped_info()["launched"] == 24 - int((qg == EMPTY).sum())
        loop, _ = _per_group(ix, q, k, rg, qg)
        assert _same(got, loop), k
        assert not np.isin(got[0], gone).any()
    assert np.isin(before[0], gone).any()    # (the removed ids were results while they were there)
    # a group all of whose ids are gone is an empty group: padding, and no job
    ix.remove(np.setdiff1d(np.flatnonzero(rg == SMALL), gone))
    ix.reset_stats()
    got = ix.knn_query_grouped(q, 5, rg, qg, N_GROUPS)
    assert (got[0][qg == SMALL] == -1).all() and ix.knn_grouped_info()["skipped"] == int(((qg == SMALL) | (qg == EMPTY)).sum())


def test_threads_mixing_grouped_filtered_and_plain_calls(cases):
    c = cases("sq_euclid")
    masks = [group_mask(c.rg, g, N_GROUPS, N) for g in range(3)]
    want_g = c.want(5)
    want_f = [c.ix.knn_query(c.q, 5, allowed=m) for m in masks]
    want_u = c.ref.knn_query(c.q, 5)
    errors = []

    def work(t):
        try:
            for r in range(6):
                which = (t + r) % 3
                if which == 0:
                    assert _same(c.ix.knn_query_grouped(c.q, 5, c.rg, c.qg, N_GROUPS), want_g)
                elif which == 1:
                    assert _same(c.ix.knn_query(c.q, 5, allowed=masks[r % 3]), want_f[r % 3])
                else:
                    assert _same(c.ix.knn_query(c.q, 5), want_u)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
