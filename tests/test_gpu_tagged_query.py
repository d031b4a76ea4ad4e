"""GPU tier: knn_query_tagged (hnsw_mi355x_knn_query_tagged / Index.knn_query_tagged) -- a tag mask per query, every mask in one
device traversal -- against the plain-Python statement of its contract (tests/tagged_query_model.py) on graphs whose hash equals the
CPU oracle's, and against the per-mask filtered calls it replaces: ids and distance bits, no tolerance.  The shapes are those of
tests/test_gpu_grouped_query.py; the tags meet every branch of the predicate: bits 0 / 1 / 2 on about 60 / 30 / 10 % of the rows,
drawn independently so that they overlap, bit 3 on 7 ids (fewer than the beam), bit 4 on no row, bit 31 on about 5 %, about 40
rows with the word 0, and a row_tags 50 entries shorter than the graph."""
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from tagged_query_model import tag_mask, tagged_knn_batch

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 1200, 16, 8, 20
N_TAGS = N - 50                      # row_tags is shorter than the graph: the last 50 ids carry no tag
B31 = 0x80000000
# single bits 0 .. 4 and 31; 0b101 and 0b11, where "any" and "all" differ; bit 31 with bit 0; every bit; no bit; and 1 | 1 << 4, which
# selects the rows of 1 under "any" and none under "all"
MASKS = np.array([1, 2, 4, 8, 16, B31, 0b101, 0b11, B31 | 1, 0xFFFFFFFF, 0, 1 | 1 << 4], np.uint32)
MODES = ("any", "all")
F16 = {"sq_euclid_f16": "sq_euclid"}


def _data(metric, n, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, DIM)).astype(np.float32) if grid else uniform(n, DIM, seed)
    return normalize_f32(x) if metric == "ucosine" else x


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


def _per_mask(ix, q, k, rt, qt, match, layer=0):
    """The loop the call replaces: one filtered call per distinct mask, rows scattered back; and the lock-step launches those calls
    ran.  A mask without a candidate: padding (knn_query with a set that allows nothing)."""
    ids = np.full((q.shape[0], k), -1, np.int32)
    d = np.full((q.shape[0], k), np.nan, np.float32)
    lockstep = 0
    for m in np.unique(qt):
        sel = qt == m
        ix.reset_stats()
        ids[sel], d[sel] = ix.knn_query(q[sel], k, allowed=tag_mask(rt, int(m), match, N), layer=layer)
        lockstep += ix.stats()["launches"]
    return (ids, d), lockstep


def _no_candidate(rt, qt, match):
    return np.array([not tag_mask(rt, int(m), match, N).any() for m in qt])


class Case:
    """One metric's data, index, oracle, tags and queries, and the model's answers (computed once, shared by the tests)."""

    def __init__(self, metric):
        self.metric = metric
        self.x = _data(metric, N, 1)
        self.ix, self.ref, self.base, self.rows = _build(metric, self.x)
        self.q = _data(metric, 24, 9)
        self.rt, self.qt = _tags(3), _query_tags(24, 4)
        self._want = {}

    def want(self, k, match):
        if (k, match) not in self._want:
            w = tagged_knn_batch(self.ref, self.rows, self.base, self.q, k, MIN_NN, self.rt, self.qt, match)
            w[0].setflags(write=False); w[1].setflags(write=False)
            self._want[k, match] = w
        return self._want[k, match]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


def test_the_tags_cover_every_branch_of_the_predicate():
    rt, qt = _tags(3), _query_tags(24, 4)
    share = [float(((rt >> b) & 1).sum()) / N for b in (0, 1, 2, 31)]
    assert 0.5 < share[0] < 0.65 and 0.2 < share[1] < 0.35 and 0.05 < share[2] < 0.15 and 0.02 < share[3] < 0.08
    assert ((rt & 8) != 0).sum() == 7 < MIN_NN and ((rt & 16) != 0).sum() == 0
    assert 40 <= (rt == 0).sum() and rt.size == N - 50 and rt.dtype == np.uint32
    assert ((rt & 3) == 3).sum() > 50 and ((rt & 5) == 5).sum() > 10 and ((rt & (B31 | 1)) == (B31 | 1)).sum() > 5   # the bits overlap
    assert all((qt == m).sum() == 2 for m in MASKS)
    for m in (0b101, 0b11, B31 | 1, 0xFFFFFFFF, 1 | 1 << 4):      # the modes differ on these
        assert tag_mask(rt, m, "all", N).sum() < tag_mask(rt, m, "any", N).sum(), m
    assert (tag_mask(rt, 1 | 1 << 4, "any", N) == tag_mask(rt, 1, "any", N)).all() and not tag_mask(rt, 1 | 1 << 4, "all", N).any()
    assert not tag_mask(rt, 0xFFFFFFFF, "all", N).any() and tag_mask(rt, 0xFFFFFFFF, "any", N).sum() == (rt != 0).sum()


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_tagged_query_is_the_model_and_the_per_mask_filtered_calls(cases, metric):
    c = cases(metric)
    for match in MODES:
        none = _no_candidate(c.rt, c.qt, match)
        for k in (5, 40):   # below and above MinNN
            c.ix.reset_stats()
            got = c.ix.knn_query_tagged(c.q, k, c.rt, c.qt, match)
            st, info = c.ix.stats(), c.ix.knn_tagged_info()
            assert _same(got, c.want(k, match)), (metric, match, k)
            loop, loop_lockstep = _per_mask(c.ix, c.q, k, c.rt, c.qt, match)
            assert _same(got, loop), (metric, match, k)
            for i in range(24):   # every returned id matches the query's mask
                ids = got[0][i][got[0][i] >= 0]
                assert ids.max(initial=-1) < N_TAGS and tag_mask(c.rt, int(c.qt[i]), match, N)[ids].all(), (metric, match, k, i)
            assert (got[0][none] == -1).all() and np.isnan(got[1][none]).all()
            assert ((got[0][c.qt == 8] >= 0).sum(axis=1) <= 7).all()
            assert info == {"calls": 1, "masks": MASKS.size, "launched": 24 - int(none.sum()), "skipped": int(none.sum()), "handbacks": info["handbacks"]}, info
            assert st["search_launches"] >= 1, st
            if loop_lockstep == 0:   # the device traversal answered the loop: then it answered the tagged call as well
                assert st["launches"] == 0 and info["handbacks"] == 0, (metric, match, k, st, info)
    assert int(_no_candidate(c.rt, c.qt, "any").sum()) == 4 and int(_no_candidate(c.rt, c.qt, "all").sum()) == 8


def test_no_candidate_at_all_k_below_one_and_argument_errors(cases):
    c = cases("sq_euclid")
    for match in MODES:
        c.ix.reset_stats()
        nothing = c.ix.knn_query_tagged(c.q, 5, c.rt, np.where(np.arange(24) % 2, 16, 0), match)   # no query's mask has a candidate: no launch
        assert (nothing[0] == -1).all() and np.isnan(nothing[1]).all()
        assert c.ix.stats()["search_launches"] == 0 and c.ix.knn_tagged_info()["launched"] == 0
        for k in (0, -2):
            assert c.ix.knn_query_tagged(c.q, k, c.rt, c.qt, match)[0].shape == (24, 0)
    # what the bindings stop before the native call, the ABI stops itself
    import ctypes as ct
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    ids, d = np.full((24, 5), 7, np.int32), np.full((24, 5), 7.0, np.float32)
    rt, qt = np.ascontiguousarray(c.rt), np.ascontiguousarray(c.qt)
    c.ix.reset_stats()

    def call(q=c.q.ctypes.data_as(F), nq=24, row=rt.ctypes.data_as(U), n_row=rt.size, qtags=qt.ctypes.data_as(U), match=0, layer=0):
        return lib.hnsw_mi355x_knn_query_tagged(c.ix._h, q, nq, DIM, 5, layer, row, n_row, qtags, match, ids.ctypes.data_as(I), d.ctypes.data_as(F))
    for kwargs, message in ((dict(match=2), "match = 2 is neither 0 (any) nor 1 (all)"), (dict(match=-1), "match = -1 is neither"),
                            (dict(row=None), "row_tags must not be NULL"), (dict(n_row=-1), "n_row_tags must be >= 0"),
                            (dict(qtags=None), "ArgumentNullException"), (dict(q=None), "ArgumentNullException"),
                            (dict(layer=c.ix.top_layer() + 1), "is outside 0 .. ")):
        assert call(**kwargs) == -1, kwargs
        assert message in hnswindex.net_amd.last_error(), (kwargs, hnswindex.net_amd.last_error())
    many = np.arange(65537, dtype=np.uint32)
    qq = np.zeros((65537, DIM), np.float32)
    big_ids, big_d = np.full((65537, 5), 7, np.int32), np.full((65537, 5), 7.0, np.float32)
    assert lib.hnsw_mi355x_knn_query_tagged(c.ix._h, qq.ctypes.data_as(F), 65537, DIM, 5, 0, rt.ctypes.data_as(U), rt.size, many.ctypes.data_as(U), 0,
                                            big_ids.ctypes.data_as(I), big_d.ctypes.data_as(F)) == -1
    assert "more than 65536 distinct masks" in hnswindex.net_amd.last_error()
    assert (ids == 7).all() and (d == 7.0).all() and (big_ids == 7).all()
    assert c.ix.stats()["search_launches"] == 0 and c.ix.knn_tagged_info()["calls"] == 0   # rejected before anything ran


def test_entry_point_without_the_query_s_tags_and_ties():
    """The grid data of the filtered tests (equal distances abound), and every query's layer-0 entry -- the descent's answer --
    carrying none of the query's tags: the entry is a candidate only."""
    for grid in (False, True):
        x = _data("sq_euclid", N, 2 if grid else 1, grid)
        ix, ref, base, rows = _build("sq_euclid", x)
        q = _data("sq_euclid", 16, 5, grid)
        rt = (np.uint32(1) << np.random.default_rng(4).integers(0, 3, N).astype(np.uint32)).astype(np.uint32)   # one of bits 0 .. 2 each
        rt[::5] |= np.uint32(B31)
        entries = [ref.find_entry_point(0, qi) for qi in q]
        bit = [int(rt[e] & 7).bit_length() - 1 for e in entries]              # the entry's one tag among bits 0 .. 2
        qt = np.array([0b111 & ~(1 << b) if i % 2 else 1 << (b + 1) % 3 for i, b in enumerate(bit)], np.uint32)
        assert ((rt[entries] & qt) == 0).all() and (qt != 0).all()
        for match in MODES:
            for k in (10, 30):
                assert _same(ix.knn_query_tagged(q, k, rt, qt, match), tagged_knn_batch(ref, rows, base, q, k, MIN_NN, rt, qt, match)), (grid, match, k)


def test_lists_beyond_64_ids():
    """MaxEdges = 40 at dim 64: layer-0 lists of up to 80 ids.  A list of more than 64 ids is past the overlapped form: the tag words
    are read after the distances there (has(id)).  Few nodes have such a list at this size (10 of 1 200 on these rows), and they are
    the hubs that most traversals expand; MaxEdges = 60 makes every fourth list that long and is tried as well."""
    dim = 64
    x, q = uniform(N, dim, 31), uniform(12, dim, 32)
    for m, at_least in ((40, 5), (60, N // 4)):
        ix, ref, base, rows = _build("cosine", x, m)
        assert sum(ref.edges(i, 0).size > 64 for i in range(N)) > at_least, m
        _lists_beyond_64(ix, ref, base, rows, q)


def _lists_beyond_64(ix, ref, base, rows, q):
    rt, qt = _tags(12), _query_tags(12, 13)
    for match in MODES:
        for k in (5, 40):
            ix.reset_stats()
            got = ix.knn_query_tagged(q, k, rt, qt, match)
            st = ix.stats()
            assert _same(got, tagged_knn_batch(ref, rows, base, q, k, MIN_NN, rt, qt, match)), (match, k)
            loop, loop_lockstep = _per_mask(ix, q, k, rt, qt, match)
            assert _same(got, loop), (match, k)
            assert st["search_launches"] >= 1 and (loop_lockstep > 0 or st["launches"] == 0), (match, k, st)


def test_a_wave_takes_several_jobs_of_different_masks(cases):
    """8 192 queries, more than the waves any kernel form keeps resident: every wave takes several jobs, of different masks, one
    after the other -- a mask register kept from the job before, or a visited set not cleared, shows here."""
    c = cases("sq_euclid")
    nq = 8192
    q = _data("sq_euclid", nq, 17)
    rt = _tags(18, N)
    live = np.array([1, 2, 4, B31, 0b11, 0b101, B31 | 1], np.uint32)
    qt = live[np.random.default_rng(19).integers(0, live.size, nq)]
    for match in MODES:
        c.ix.reset_stats()
        got = c.ix.knn_query_tagged(q, 10, rt, qt, match)
        info = c.ix.knn_tagged_info()
        assert info["launched"] == nq and info["skipped"] == 0 and info["masks"] == live.size, info
        loop, _ = _per_mask(c.ix, q, 10, rt, qt, match)
        assert _same(got, loop), match
        hit = rt[got[0]] & qt[:, None]
        assert (got[0] >= 0).all() and ((hit != 0).all() if match == "any" else (hit == qt[:, None]).all())


def test_layer_1(cases):
    c = cases("sq_euclid")
    top = c.ix.top_layer()
    assert top >= 1
    for match in MODES:
        for k in (5, 40):
            got = c.ix.knn_query_tagged(c.q, k, c.rt, c.qt, match, layer=1)
            loop, _ = _per_mask(c.ix, c.q, k, c.rt, c.qt, match, layer=1)
            assert _same(got, loop), (match, k)
            assert np.isin(got[0][got[0] >= 0], np.flatnonzero(c.ref.levels() >= 1)).all()
            assert not _same(got, c.want(k, match))
    for layer in (-1, top + 1):
        with pytest.raises(RuntimeError, match=f"layer {layer} is outside 0 .. {top}"):
            c.ix.knn_query_tagged(c.q, 5, c.rt, c.qt, layer=layer)


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


def test_device_backend_knn_search_tagged(cases):
    """The inner boundary: a host-supplied graph, hnswdev_knn_search_tagged; bad arguments are messages, not launches."""
    import ctypes as ct
    import hnswindex
    c = cases("cosine")
    lv = c.ref.levels()
    dev = hnswindex.DeviceBackend(DIM, "cosine", capacity=N)
    dev.upload_rows(0, c.x)
    dev.set_graph(lv, _layers(c.ref, lv, M), M)
    ep = c.ref.entry_point
    for match in MODES:
        none = _no_candidate(c.rt, c.qt, match)
        dev.reset_stats()
        ids, d, flags = dev.knn_search_tagged(c.q, ep, 32, 10, c.rt, c.qt, match)
        assert (flags == 0).all()
        assert _same((ids, d), tagged_knn_batch(c.ref, c.rows, c.base, c.q, 10, 32, c.rt, c.qt, match)), match
        assert dev.knn_tagged_info() == {"calls": 1, "masks": MASKS.size, "launched": 24 - int(none.sum()), "skipped": int(none.sum()), "handbacks": 0}
        for m in np.unique(c.qt):   # ... and row by row the filtered call of the same boundary
            sel = c.qt == m
            allowed = tag_mask(c.rt, int(m), match, N)
            if allowed.any():
                f_ids, f_d, _ = dev.knn_search(c.q[sel], ep, 32, 10, allowed=allowed)
                assert _same((ids[sel], d[sel]), (f_ids, f_d)), (match, m)
        ids, d, flags = dev.knn_search_tagged(c.q, ep, 32, 10, c.rt, np.full(24, 16), match)
        assert (ids == -1).all() and np.isnan(d).all() and (flags == 0).all()
        # (every query skipped: a call, a mask and 24 skipped queries more, no launch)
        assert dev.knn_tagged_info() == {"calls": 2, "masks": MASKS.size + 1, "launched": 24 - int(none.sum()), "skipped": int(none.sum()) + 24, "handbacks": 0}
    launches = dev.stats()["search_launches"]
    with pytest.raises(RuntimeError, match="knn_search_tagged: bad argument"):
        dev.knn_search_tagged(c.q, N + 5, 32, 10, c.rt, c.qt)           # entry point outside the graph
    with pytest.raises(RuntimeError, match="knn_search_tagged: bad argument"):
        dev.knn_search_tagged(c.q, ep, 8, 10, c.rt, c.qt)               # k_beam < k_out
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    o_ids, o_d, o_f = np.full((24, 10), 7, np.int32), np.full((24, 10), 7.0, np.float32), np.full(24, 7, np.int32)
    rt, qt = np.ascontiguousarray(c.rt), np.ascontiguousarray(c.qt)
    good = dict(q=c.q.ctypes.data_as(F), rt=rt.ctypes.data_as(U), qt=qt.ctypes.data_as(U), ids=o_ids.ctypes.data_as(I), d=o_d.ctypes.data_as(F),
                f=o_f.ctypes.data_as(I))
    for null, message in (("rt", "row_tags must not be NULL"), ("qt", "query_tags must not be NULL"), ("q", "null argument"), ("ids", "null argument"),
                          ("d", "null argument"), ("f", "null argument")):
        a = dict(good, **{null: None})
        assert lib.hnswdev_knn_search_tagged(dev._ctx, a["q"], 24, ep, 32, 10, 0, a["rt"], rt.size, a["qt"], 0, a["ids"], a["d"], a["f"]) == -1, null
        assert message in dev.last_error(), (null, dev.last_error())
    for n_row, match, message in ((-1, 0, "n_row_tags must be >= 0"), (rt.size, 2, "match = 2 is neither 0 (any) nor 1 (all)")):
        assert lib.hnswdev_knn_search_tagged(dev._ctx, good["q"], 24, ep, 32, 10, 0, good["rt"], n_row, good["qt"], match, good["ids"], good["d"], good["f"]) == -1
        assert message in dev.last_error(), dev.last_error()
    assert (o_ids == 7).all() and (o_d == 7.0).all() and (o_f == 7).all()
    assert dev.stats()["search_launches"] == launches
    dev.reset_stats()   # n_row_tags == 0: no word of a graph id -- nothing goes up, nothing is counted, every row is padded
    assert lib.hnswdev_knn_search_tagged(dev._ctx, good["q"], 24, ep, 32, 10, 0, good["rt"], 0, good["qt"], 0, good["ids"], good["d"], good["f"]) == 0
    assert (o_ids == -1).all() and np.isnan(o_d).all() and (o_f == 0).all()
    assert dev.knn_tagged_info() == {"calls": 1, "masks": MASKS.size, "launched": 0, "skipped": 24, "handbacks": 0}
    assert dev.stats()["search_launches"] == 0


def test_forced_handbacks_give_the_same_answers(cases, monkeypatch):
    c = cases("cosine")
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    c.ix.reset_stats()
    for match in MODES:
        for k in (5, 40):
            assert _same(c.ix.knn_query_tagged(c.q, k, c.rt, c.qt, match), c.want(k, match)), (match, k)
    info, st = c.ix.knn_tagged_info(), c.ix.stats()
    assert info["handbacks"] > 0 and st["search_overflows"] == info["handbacks"] and st["launches"] > 0, (info, st)


def test_two_contexts_with_forced_handbacks(cases, monkeypatch):
    """Sharded over two contexts AND jobs handed back: the shards are gathered to the primary, where the host traversal redoes them."""
    c = cases("cosine")
    two = _index(DIM, c.metric, M, set_devices=2)
    two.add(c.x)
    assert two.graph_hash() == c.ref.graph_hash()
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    two.reset_stats()
    for match in MODES:
        for k in (5, 40):
            assert _same(two.knn_query_tagged(c.q, k, c.rt, c.qt, match), c.want(k, match)), (match, k)
    info = two.knn_tagged_info()   # (summed over the contexts)
    assert two.stats()["search_overflows"] + two.stats_at(1)["search_overflows"] > 0 and info["handbacks"] > 0, info
    assert two.stats_at(1)["search_launches"] >= 2 and two.stats()["launches"] > 0


def _other_path(c, **knobs):
    ix = _index(DIM, c.metric, M, **knobs)
    ix.add(c.x)
    assert ix.graph_hash() == c.ref.graph_hash()
    ix.reset_stats()
    for match in MODES:
        for k in (5, 40):
            assert _same(ix.knn_query_tagged(c.q, k, c.rt, c.qt, match), c.want(k, match)), (knobs, match, k)
    return ix.stats(), ix.knn_tagged_info()


def test_hashed_visited_sets_host_traversal_and_two_contexts(cases, monkeypatch):
    c = cases("ucosine")
    set_diag(monkeypatch, vis_hash="1")
    st, _ = _other_path(c)
    assert st["visited_hash_launches"] > 0
    set_diag(monkeypatch, vis_hash="1", vis_hash_cap="64")   # small tables: a traversal that crowds its table is handed back
    st, _ = _other_path(c)
    assert st["visited_hash_launches"] > 0
    monkeypatch.undo()
    st, info = _other_path(c, set_device_traversal=False)
    assert st["search_launches"] == 0 and info["calls"] == 0
    # two contexts: 12 queries each; the shuffled masks do not line up with the bound between the shards, and each context counts
    # the distinct masks of its own shard
    first, second = len(set(c.qt[:12].tolist())), len(set(c.qt[12:].tolist()))
    assert first > 4 and second > 4 and set(c.qt[:12].tolist()) != set(c.qt[12:].tolist())
    _, info = _other_path(c, set_devices=2)
    assert info["calls"] == 8 and info["launched"] + info["skipped"] == 96 and info["masks"] == 4 * (first + second), info


def test_after_removals_a_vacant_slot_s_tags_count_for_nothing_until_it_is_filled_again():
    x = _data("sq_euclid", N, 1)
    ix = _index(DIM, "sq_euclid", M, set_allow_removals=True)
    ix.add(x)
    rt, qt = _tags(3), _query_tags(24, 4)
    q = _data("sq_euclid", 24, 9)
    rng = np.random.default_rng(21)
    gone = np.concatenate([rng.choice(np.flatnonzero(rt & bit), n, replace=False) for bit, n in ((1, 60), (2, 28), (4, 10), (8, 2), (B31, 6))])
    gone = np.unique(gone)
    assert (rt[gone] != 0).all()                # the removed ids' slots stay tagged in the caller's array
    before = ix.knn_query_tagged(q, 5, rt, qt, "any")
    ix.remove(gone)
    for match in MODES:
        none = _no_candidate(np.where(np.isin(np.arange(N_TAGS), gone), 0, rt), qt, match)
        for k in (5, 40):
            ix.reset_stats()
            got = ix.knn_query_tagged(q, k, rt, qt, match)
            assert ix.knn_tagged_info()["launched"] == 24 - int(none.sum())
            loop, _ = _per_mask(ix, q, k, rt, qt, match)
            assert _same(got, loop), (match, k)
            assert not np.isin(got[0], gone).any()
    assert np.isin(before[0], gone).any()    # (the removed ids were results while they were there)
    # a tag all of whose ids are gone is a tag on no row: padding, and no job
    ix.remove(np.setdiff1d(np.flatnonzero(rt & 8), gone))
    ix.reset_stats()
    got = ix.knn_query_tagged(q, 5, rt, qt, "any")
    assert (got[0][qt == 8] == -1).all() and ix.knn_tagged_info()["skipped"] == int(np.isin(qt, [8, 16, 0]).sum())
    # rows added after the removals (a vacant slot that is filled again answers under the tags the caller's array holds for it)
    new_ids = ix.add(x[:40] + np.float32(0.25))
    assert new_ids.size == 40
    for match in MODES:
        ix.reset_stats()
        got = ix.knn_query_tagged(q, 40, rt, qt, match)
        loop, _ = _per_mask(ix, q, 40, rt, qt, match)
        assert _same(got, loop), match
        for i in range(24):
            ids = got[0][i][got[0][i] >= 0]
            assert tag_mask(rt, int(qt[i]), match, max(N, int(new_ids.max()) + 1))[ids].all(), (match, i)


def test_threads_mixing_tagged_grouped_and_filtered_calls(cases):
    c = cases("sq_euclid")
    masks = [tag_mask(c.rt, m, "any", N) for m in (1, 2, B31)]
    rg = (c.rt & 3).astype(np.int32)
    qg = (np.arange(24) % 4).astype(np.int32)
    want_t = {match: c.want(5, match) for match in MODES}
    want_f = [c.ix.knn_query(c.q, 5, allowed=m) for m in masks]
    want_g = c.ix.knn_query_grouped(c.q, 5, rg, qg, 4)
    errors = []

    def work(t):
        try:
            for r in range(6):
                which = (t + r) % 4
                if which < 2:
                    assert _same(c.ix.knn_query_tagged(c.q, 5, c.rt, c.qt, MODES[which]), want_t[MODES[which]])
                elif which == 2:
                    assert _same(c.ix.knn_query(c.q, 5, allowed=masks[r % 3]), want_f[r % 3])
                else:
                    assert _same(c.ix.knn_query_grouped(c.q, 5, rg, qg, 4), want_g)
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
