"""GPU tier: get_vectors / items and knn_query_by_id.  The rows that come back are those of
DeviceBackend.download_rows on a mirror context, bit for bit, for every row kind; knn_query_by_id is byte for byte the per-id loop
of existing calls it replaces -- knn_query(get_vectors([id]), k, allowed=<every id but id>, layer) -- ids, distance bits, the order
among equal distances and the padding, on 3 000 rows x dim 20 with MaxEdges 8 and 48 query ids, among them the entry point, a row
that is stored under a smaller and a larger id as well, a repeated id and the last id."""
import numpy as np
import pytest

from by_id_model import all_but, knn_by_id_loop
from common import normalize_f32, set_diag, uniform

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN, NQ = 3000, 20, 8, 20, 48
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
A, DUP_LO, DUP_HI = 1500, 100, 2900          # the row of id A is stored under ids DUP_LO < A < DUP_HI as well


def _data(metric, n, dim, seed):
    x = uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _rows(metric, n=N, dim=DIM, seed=1):
    x = _data(metric, n, dim, seed).copy()
    if n > DUP_HI:
        x[DUP_LO] = x[A]
        x[DUP_HI] = x[A]
    return x


def _index(dim, metric, m=M, n=N, **knobs):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(m); ix.set_min_nn(MIN_NN)
    ix.set_insert_batch(0)               # (the knob is the library's, not the index's: every index of this file names its schedule)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    return ix


def _query_ids(ix, n=N, nq=NQ):
    must = [ix.entry_point, A, DUP_LO, 7, 7, n - 1]
    rest = [i for i in np.random.default_rng(5).permutation(n).tolist() if i not in must][:nq - len(must)]
    return np.array(must + rest, np.int32)


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


class Case:
    """One row kind's index and query ids, and the per-id loop's answers (computed once, shared, read-only)."""

    def __init__(self, metric):
        self.metric = metric
        self.x = _rows(metric)
        self.ix = _index(DIM, metric)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        self.qids = _query_ids(self.ix)
        self._want = {}

    def want(self, k, layer=0):
        if (k, layer) not in self._want:
            w = knn_by_id_loop(self.ix, self.qids, k, layer)
            w[0].setflags(write=False); w[1].setflags(write=False)
            self._want[k, layer] = w
        return self._want[k, layer]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


# ---- get_vectors / items ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 7, 33])
@pytest.mark.parametrize("metric", METRICS)
def test_gather_rows_is_download_rows_in_the_order_asked(metric, dim):
    """The inner call on a context: tails (dim 1, 7), the int8 record's padding, f16's odd length (33)."""
    import hnswindex
    n = 130
    x = _data(metric, n, dim, 40 + dim)
    dev = hnswindex.DeviceBackend(dim, metric, capacity=n)
    dev.upload_rows(0, x)
    stored = dev.download_rows(0, n)
    ids = np.concatenate([np.arange(n)[::-1], [3, 3, 129, 0, 64]]).astype(np.int32)     # descending, then repeats
    got = dev.gather_rows(ids)
    assert got.dtype == np.float32 and got.shape == (ids.size, dim) and got.tobytes() == stored[ids].tobytes()
    if metric in ("sq_euclid", "cosine", "ucosine"):
        assert got.tobytes() == x[ids].tobytes()                                          # f32 rows: a copy
    out = dev.gather_rows([5, n, -1, 1 << 30, 6])                                         # outside the uploaded rows: zeros
    assert out[[0, 4]].tobytes() == stored[[5, 6]].tobytes() and (out[1:4] == 0).all()
    assert dev.gather_rows([]).shape == (0, dim)
    assert dev.by_id_info()["rows_gathered"] == ids.size + 5


@pytest.mark.parametrize("dim", [7, 20, 33])
@pytest.mark.parametrize("metric", METRICS)
def test_get_vectors_is_download_rows_of_a_mirror_context(metric, dim):
    import hnswindex
    n = 200
    x = _data(metric, n, dim, 60 + dim)
    ix = _index(dim, metric, n=n)
    ix.add(x)
    dev = hnswindex.DeviceBackend(dim, metric, capacity=n)
    dev.upload_rows(0, x)
    stored = dev.download_rows(0, n)
    ids = np.concatenate([np.arange(n)[::-1], [9, 9, n - 1, 0]]).astype(np.int32)
    assert ix.get_vectors(ids).tobytes() == stored[ids].tobytes()
    assert ix.items().tobytes() == stored[ix.ids()].tobytes()
    assert ix.get_vectors(17).tobytes() == stored[17:18].tobytes()                       # a single id is a list of one
    if metric.endswith("_f16"):
        assert stored.tobytes() == x.astype(np.float16).astype(np.float32).tobytes()     # the rounded row widened
    if metric == "sq_euclid_i8":
        assert not (stored == x).all() and np.abs(stored - x).max() <= np.abs(x).max() / 127   # q * scale, not the caller's copy


def test_items_after_removals_and_slot_reuse_and_ids_that_are_not_live():
    n, dim = 300, DIM
    x = _data("sq_euclid", n + 40, dim, 77)
    ix = _index(dim, "sq_euclid", n=n + 40)
    ix.add(x[:n])
    host = {i: x[i] for i in range(n)}
    gone = np.array([0, 17, 150, 299], np.int32)
    ix.remove(gone)
    for i in gone:
        del host[int(i)]
    with pytest.raises(RuntimeError, match=r"hnsw_mi355x_get_vectors: ids\[2\] = 150 is not a live id"):
        ix.get_vectors([3, 4, 150])
    for bad in (-1, n, 1 << 30):
        with pytest.raises(RuntimeError, match="is not a live id"):
            ix.get_vectors([1, bad])
    new_ids = ix.add(x[n:])                                                              # reuses the vacant slots first
    assert set(gone.tolist()) <= set(new_ids.tolist())
    for i, row in zip(new_ids, x[n:]):
        host[int(i)] = row
    ix.remove([int(new_ids[-1])])
    del host[int(new_ids[-1])]
    items, ids = ix.items(), ix.ids()
    assert items.shape == (ix.count, dim) == (len(host), dim)
    assert items.tobytes() == np.stack([host[int(i)] for i in ids]).tobytes()
    assert ix.get_vectors(gone).tobytes() == np.stack([host[int(i)] for i in gone]).tobytes()   # the slots' new rows


# ---- knn_query_by_id -------------------------------------------------------------------------------------------------------------
def test_the_query_ids_cover_the_cases(cases):
    c = cases("sq_euclid")
    q = c.qids.tolist()
    assert len(q) == NQ and q[0] == c.ix.entry_point and A in q and DUP_LO in q and N - 1 in q and q.count(7) == 2
    assert DUP_LO < A < DUP_HI and (c.x[A] == c.x[DUP_LO]).all() and (c.x[A] == c.x[DUP_HI]).all()
    assert c.ix.top_layer() >= 1


@pytest.mark.parametrize("metric", METRICS)
def test_knn_query_by_id_is_the_per_id_filtered_loop(cases, metric):
    c = cases(metric)
    for k, layer in ((1, 0), (10, 0), (200, 0), (10, 1)):                                # 200: above MinNN, the beam is k
        c.ix.reset_stats()
        got = c.ix.knn_query_by_id(c.qids, k, layer)
        info = c.ix.by_id_info()
        assert got[0].dtype == np.int32 and got[1].dtype == np.float32
        assert _same(got, c.want(k, layer)), (metric, k, layer)
        assert not (got[0] == c.qids[:, None]).any(), (metric, k, layer)                 # never the query's own id
        assert info["calls"] == 1 and info["traversed"] == NQ and info["rows_gathered"] == NQ and info["scanned"] == 0, info
    ids, d = c.ix.knn_query_by_id(c.qids, 10)
    rep = np.flatnonzero(c.qids == 7)
    assert (ids[rep[0]] == ids[rep[1]]).all() and d[rep[0]].tobytes() == d[rep[1]].tobytes()
    assert (ids[:, 0] >= 0).all()


def test_lists_beyond_64_ids():
    """MaxEdges 40 at dim 64 (the rows of tests/test_gpu_tagged_query.py's case): layer-0 lists of up to 80 ids.  A list of more than
    64 ids is past the traversal's overlapped form, which tests the filter after the distances there (has(id)); the few nodes with
    such a list are the hubs most traversals expand.  MaxEdges 60 makes every fourth list that long."""
    n, dim = 1200, 64
    x = uniform(n, dim, 31)
    for m, at_least in ((40, 5), (60, n // 4)):
        ix = _index(dim, "cosine", m=m, n=n, set_insert_batch=1)
        ix.add(x)
        long_lists = [i for i in range(n) if ix.edges(i, 0).size > 64]
        assert len(long_lists) > at_least, (m, len(long_lists))
        qids = np.array([ix.entry_point, 7, 7, n - 1] + long_lists[:4] + list(range(20, 36)), np.int32)
        for k in (10, 60):
            assert _same(ix.knn_query_by_id(qids, k), knn_by_id_loop(ix, qids, k)), (m, k)


def _other_path(c, **knobs):
    ix = _index(DIM, c.metric, **knobs)
    ix.add(c.x)
    ix.reset_stats()
    for k in (10, 200):
        assert _same(ix.knn_query_by_id(c.qids, k), c.want(k)), (knobs, k)
    assert _same(ix.knn_query_by_id(c.qids, 10, 1), c.want(10, 1)), knobs
    return ix


def test_hashed_visited_sets_host_traversal_and_two_contexts(cases, monkeypatch):
    c = cases("cosine")
    for k in (10, 200):
        c.want(k)
    c.want(10, 1)                                                                        # (the reference rows: bitset visited sets, one context)
    set_diag(monkeypatch, vis_hash="1")
    ix = _other_path(c)
    assert ix.stats()["visited_hash_launches"] > 0 and ix.by_id_info()["traversed"] == 3 * NQ
    monkeypatch.undo()
    ix = _other_path(c, set_device_traversal=False)                                      # the host way, the id as the job's exclude
    info = ix.by_id_info()
    assert ix.stats()["search_launches"] == 0 and info["calls"] == 0 and info["traversed"] == 0 and info["rows_gathered"] == 3 * NQ, info
    ix = _other_path(c, set_devices=2)                                                   # every context gathers and answers its half
    info = ix.by_id_info()
    assert info["calls"] == 6 and info["traversed"] == 3 * NQ and ix.stats_at(1)["search_launches"] >= 3, info


def test_a_row_with_a_nan_is_handed_back_and_answered_the_same():
    n = 600
    x = _data("sq_euclid", n, DIM, 11).copy()
    x[300, 4] = np.nan
    ix = _index(DIM, "sq_euclid", n=n)
    ix.add(x)
    qids = np.array([300, 5, n - 1, 300], np.int32)
    ix.reset_stats()
    got = ix.knn_query_by_id(qids, 10)
    info = ix.by_id_info()
    assert info["handbacks"] >= 2 and info["traversed"] == 4 and ix.stats()["search_overflows"] >= 2, info
    assert _same(got, knn_by_id_loop(ix, qids, 10))
    assert np.isnan(ix.get_vectors([300])[0, 4])


def test_an_index_of_one_item_answers_with_padding():
    ix = _index(DIM, "sq_euclid", n=8)
    ix.add(uniform(1, DIM, 2))
    for ids, d in (ix.knn_query_by_id([0, 0], 3), ix.exact_knn_query_by_id([0, 0], 3), ix.exact_knn_graph(3, [0, 0])):
        assert ids.shape == d.shape == (2, 3) and (ids == -1).all() and np.isnan(d).all()


def test_a_removed_id_fails_with_its_name_and_vacant_slots_change_nothing():
    n = 800
    x = _data("ucosine", n, DIM, 13)
    ix = _index(DIM, "ucosine", n=n)
    ix.add(x)
    ix.remove([9, 400])
    ix.reset_stats()
    with pytest.raises(RuntimeError, match=r"hnsw_mi355x_knn_query_by_id: ids\[1\] = 9 is not a live id"):
        ix.knn_query_by_id([3, 9], 5)
    with pytest.raises(RuntimeError, match=r"ids\[0\] = 800 is not a live id"):
        ix.knn_query_by_id([800], 5)
    assert ix.by_id_info()["rows_gathered"] == 0 and ix.stats()["search_launches"] == 0  # nothing was launched
    with pytest.raises(RuntimeError, match="layer 40 is outside"):
        ix.knn_query_by_id([3], 5, 40)
    qids = np.array([ix.entry_point, 8, 10, 399, 401, n - 1], np.int32)
    got = ix.knn_query_by_id(qids, 30)
    assert _same(got, knn_by_id_loop(ix, qids, 30)) and not np.isin(got[0], [9, 400]).any()
    assert ix.knn_query_by_id(qids, 0)[0].shape == (6, 0)


def test_device_backend_knn_search_by_id(cases):
    """The inner boundary: rows and a graph a host uploaded itself; row by row the filtered call of the same boundary."""
    import hnswindex
    c = cases("sq_euclid_i8")
    lv = c.ix.levels()
    dev = hnswindex.DeviceBackend(DIM, c.metric, capacity=N)
    dev.upload_rows(0, c.x)
    dev.set_graph(lv, [c.ix.export_edges(layer, 2 * M + 2) for layer in range(int(lv.max()) + 1)], M)
    ep, qids = c.ix.entry_point, c.qids[:12]
    ids, d, flags = dev.knn_search_by_id(qids, ep, 32, 10)
    assert (flags == 0).all()
    for i, own in enumerate(qids):
        f_ids, f_d, _ = dev.knn_search(dev.gather_rows([own]), ep, 32, 10, allowed=all_but(N, int(own)))
        assert _same((ids[i:i + 1], d[i:i + 1]), (f_ids, f_d)), own
    info = dev.by_id_info()
    assert info["calls"] == 1 and info["traversed"] == 12 and info["handbacks"] == 0, info
    launches = dev.stats()["search_launches"]
    with pytest.raises(RuntimeError, match=r"knn_search_by_id: ids\[1\] = 3000 is no uploaded row"):
        dev.knn_search_by_id([0, N], ep, 32, 10)
    with pytest.raises(RuntimeError, match="knn_search_by_id: bad argument"):
        dev.knn_search_by_id(qids, ep, 8, 10)                                            # k_beam < k_out
    with pytest.raises(RuntimeError, match="knn_search_by_id: layer 9 outside"):
        dev.knn_search_by_id(qids, ep, 32, 10, layer=9)
    assert dev.stats()["search_launches"] == launches
