"""GPU tier: filtered RangeQuery (hnsw_mi355x_range_query_filtered / Index.range_query(..., allowed=...)) against the plain-Python
restatement of SearchLayerRange with a filter (tests/filtered_range_model.py) on graphs whose hash equals the CPU oracle's: ids,
distance bits, order and counts at the four metrics and several selectivities; the order among equal distances on a tie-heavy
grid, where dropping disallowed ids from the unfiltered answer gives another order; the empty-heap exception of negative radii;
and the same answers through every other path (host finishing, hashed visited sets, host traversal, two contexts, DeviceBackend,
concurrent callers)."""
import threading

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from filtered_model import filtered_knn_batch
from filtered_range_model import HeapEmpty, filtered_range, filtered_range_batch

pytestmark = pytest.mark.gpu

N, DIM, M, MIN_NN = 1200, 16, 8, 20


def _data(metric, n, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, DIM)).astype(np.float32) if grid else uniform(n, DIM, seed)
    return normalize_f32(x) if metric == "ucosine" else x


def _build(metric, x, **knobs):
    import hnswindex
    import oracle
    ix = hnswindex.Index(DIM, metric)
    ix.set_collection_size(N); ix.set_max_edges(M); ix.set_min_nn(MIN_NN); ix.set_insert_batch(1)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    ix.add(x)
    ref = oracle.OracleIndex(DIM, metric, max_edges=M, min_nn=MIN_NN, collection_size=N)
    ref.add(x)
    assert ix.graph_hash() == ref.graph_hash(), metric
    return ix, ref


def _masks(x, seed):
    rng = np.random.default_rng(seed)
    out = {f"sel{s}": rng.random(x.shape[0]) < s for s in (1.0, 0.5, 0.1, 0.02)}
    out["empty"] = np.zeros(x.shape[0], dtype=bool)
    out["correlated"] = x[:, 0] < np.quantile(x[:, 0], 0.15)
    out["short"] = rng.random(x.shape[0] // 2) < 0.5                # ids past its end are not allowed
    return out


def _radius(metric, x, q, p):
    import oracle
    d = np.concatenate([oracle.dist_query_rows(metric, x, qq, np.arange(x.shape[0], dtype=np.int32)) for qq in q[:4]])
    return float(np.quantile(d, p))


def _same(got, want):
    return len(got[0]) == len(want[0]) and all(a.tolist() == b.tolist() and c.tobytes() == e.tobytes()
                                               for a, b, c, e in zip(got[0], want[0], got[1], want[1]))


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            x = _data(metric, N, 1 if not grid else 2, grid)
            cache[(metric, grid)] = (x, *_build(metric, x))
        return cache[(metric, grid)]
    return get


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8"])
def test_filtered_range_is_the_reference_on_the_device(built, metric):
    x, ix, ref = built(metric)
    q = _data(metric, 12, 9)
    radius = _radius(metric, x, q, 0.04)
    for name, mask in _masks(x, 3).items():
        ix.reset_stats()
        got = ix.range_query(q, radius, allowed=mask)
        st = ix.stats()
        assert st["range_launches"] >= 1, (metric, name, st)
        assert _same(got, filtered_range_batch(ref, x, metric, q, radius, mask)), (metric, name)
    ids = np.flatnonzero(_masks(x, 3)["sel0.1"])                      # the id-list form
    assert _same(ix.range_query(q, radius, allowed=ids), filtered_range_batch(ref, x, metric, q, radius, _masks(x, 3)["sel0.1"]))


def test_entry_point_disallowed(built):
    x, ix, ref = built("sq_euclid")
    q = _data("sq_euclid", 16, 5)
    radius = _radius("sq_euclid", x, q, 0.05)
    mask = np.random.default_rng(4).random(N) < 0.5
    mask[[ref.find_entry_point(0, qi) for qi in q]] = False
    assert _same(ix.range_query(q, radius, allowed=mask), filtered_range_batch(ref, x, "sq_euclid", q, radius, mask))


def test_all_allowed_equals_range_query(built):
    for metric in ("sq_euclid", "cosine"):
        x, ix, ref = built(metric)
        q = _data(metric, 16, 6)
        radius = _radius(metric, x, q, 0.05)
        assert _same(ix.range_query(q, radius, allowed=np.ones(N, dtype=bool)), ix.range_query(q, radius)), metric


def _grid_case(built):
    x, ix, ref = built("sq_euclid", grid=True)
    q = np.random.default_rng(8).integers(1, 4, (24, DIM)).astype(np.float32)
    masks = {s: np.random.default_rng(int(s * 100)).random(N) < s for s in (0.7, 0.4)}
    return x, ix, ref, q, 8.0, masks


def test_tie_heavy_grid_order_is_completed_on_the_device(built):
    x, ix, ref, q, radius, masks = _grid_case(built)
    full_ids, full_d = ix.range_query(q, radius)
    reordered = 0
    for s, mask in masks.items():
        want = filtered_range_batch(ref, x, "sq_euclid", q, radius, mask)
        for a, d, w in zip(full_ids, full_d, want[0]):
            post = a[mask[a]]                                              # what callers did before: drop disallowed ids
            assert sorted(post.tolist()) == sorted(w.tolist())
            reordered += post.tolist() != w.tolist()
        ix.reset_stats()
        got = ix.range_query(q, radius, allowed=mask)
        st = ix.stats()
        assert _same(got, want), s
        assert st["range_device_ordered"] > 0 and st["range_host_ordered"] == 0, st   # closures here stay below 2 048 entries
    assert reordered > 5                                                     # post-filtering really gives another order


def test_every_other_path_gives_the_same_answers(built, monkeypatch):
    x, ix, ref, q, radius, masks = _grid_case(built)
    want = {s: filtered_range_batch(ref, x, "sq_euclid", q, radius, m) for s, m in masks.items()}
    for finish in ("0", "1"):
        set_diag(monkeypatch, range_finish=finish)
        for s, m in masks.items():
            assert _same(ix.range_query(q, radius, allowed=m), want[s]), (finish, s)
        monkeypatch.undo()
    set_diag(monkeypatch, vis_hash="1")
    iy, _ = _build("sq_euclid", x)
    for s, m in masks.items():
        assert _same(iy.range_query(q, radius, allowed=m), want[s]), ("vis_hash", s)
    monkeypatch.undo()
    for knob in ({"set_device_traversal": False}, {"set_devices": 2}):
        iy, _ = _build("sq_euclid", x, **knob)
        iy.reset_stats()
        for s, m in masks.items():
            assert _same(iy.range_query(q, radius, allowed=m), want[s]), (knob, s)
        if "set_device_traversal" in knob:
            assert iy.stats()["range_launches"] == 0


def _raw_ucosine(n, seed):
    return np.random.default_rng(seed).normal(size=(n, DIM)).astype(np.float32)   # unnormalised: 1 - dot goes negative


def test_empty_heap_rule_of_negative_radii():
    x = _raw_ucosine(N, 21)
    ix, ref = _build("ucosine", x)
    q = _raw_ucosine(40, 22)
    rng = np.random.default_rng(23)
    raised = avoided = 0
    for radius in (-1.0, -3.0):
        mask = rng.random(N) < 0.3
        for qi in q:
            try:
                want = filtered_range(ref, x, "ucosine", qi, radius, mask)
            except HeapEmpty:
                want = None
            if want is None:
                with pytest.raises(RuntimeError, match="Heap is empty"):
                    ix.range_query(qi[None], radius, allowed=mask)
                raised += 1
            else:
                got = ix.range_query(qi[None], radius, allowed=mask)
                assert got[0][0].tolist() == want[0].tolist() and got[1][0].tobytes() == want[1].tobytes()
                avoided += 1
        bad = [i for i, qi in enumerate(q) if _raises(ref, x, qi, radius, mask)]
        if bad:                                                           # one such query fails the whole batch
            with pytest.raises(RuntimeError, match="Heap is empty"):
                ix.range_query(q, radius, allowed=mask)
        # a mask that avoids the rule: everything within range allowed
        allow_all = np.ones(N, dtype=bool)
        assert _same(ix.range_query(q, radius, allowed=allow_all), filtered_range_batch(ref, x, "ucosine", q, radius, allow_all))
    assert raised > 0 and avoided > 0


def _raises(ref, x, qi, radius, mask):
    try:
        filtered_range(ref, x, "ucosine", qi, radius, mask)
        return False
    except HeapEmpty:
        return True


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


def test_device_backend_range_search_filtered(built):
    import hnswindex
    x, _, ref = built("sq_euclid", grid=True)
    lv = ref.levels()
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=N)
    dev.upload_rows(0, x)
    dev.set_graph(lv, _layers(ref, lv), M)
    q = np.random.default_rng(8).integers(1, 4, (16, DIM)).astype(np.float32)
    for s in (1.0, 0.4, 0.05):
        mask = np.random.default_rng(int(s * 100)).random(N) < s
        ids, d, flags = dev.range_search(q, ref.entry_point, 8.0, allowed=mask)
        assert not flags.any()
        for qi in range(q.shape[0]):
            # DeviceBackend starts from the given entry point: descend as the reference does from it
            want = filtered_range(ref, x, "sq_euclid", q[qi], 8.0, mask)
            assert ids[qi].tolist() == want[0].tolist() and d[qi].tobytes() == want[1].tobytes(), (s, qi)


def test_threads_mixing_filtered_range_unfiltered_range_and_filtered_knn(built):
    x, ix, ref = built("cosine")
    q = _data("cosine", 16, 13)
    radius = _radius("cosine", x, q, 0.04)
    masks = [m for k, m in _masks(x, 9).items() if k in ("sel0.5", "sel0.1", "correlated")]
    want_r = [filtered_range_batch(ref, x, "cosine", q, radius, m) for m in masks]
    want_u = ref.range_query(q, radius)
    want_k = [filtered_knn_batch(ref, x, "cosine", q, 10, MIN_NN, m) for m in masks]
    errors = []

    def work(t):
        try:
            for r in range(6):
                i = (t + r) % len(masks)
                kind = (t + r) % 3
                if kind == 0:
                    assert _same(ix.range_query(q, radius, allowed=masks[i]), want_r[i])
                elif kind == 1:
                    assert _same(ix.range_query(q, radius), want_u)
                else:
                    got = ix.knn_query(q, 10, allowed=masks[i])
                    assert (got[0] == want_k[i][0]).all() and got[1].tobytes() == want_k[i][1].tobytes()
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(repr(e))
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
