"""GPU tier: half-precision row storage (sq_euclid_f16, ucosine_f16).  binary16 -> binary32 is exact, so an
X_f16 index fed x IS the X index fed xh = x.astype(float16).astype(float32): the reference of every check here is the oracle (or
the Python models of the filtered / layer queries) on xh with the f32 metric of the same family -- ids and hashes equal,
distances byte-equal.  Queries are never rounded."""
import numpy as np
import pytest

import oracle
from common import default_cap, normalize_f32, set_diag, uniform
from filtered_model import filtered_knn_batch
from filtered_range_model import filtered_range_batch
from layer_query_model import knn_at_layer_batch, multilayer_knn_batch

pytestmark = pytest.mark.gpu

F16 = {"sq_euclid_f16": "sq_euclid", "ucosine_f16": "ucosine"}
DIMS = [1, 4, 7, 8, 33, 96, 120, 128, 136, 264, 768]
SHAPES = [(96, 16, 100), (33, 8, 60), (128, 12, 80)]
N, NQ = 4000, 400


def h(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def _data(metric, n, dim, seed, shifted=False):
    x = uniform(n, dim, seed)
    if F16.get(metric, metric) == "ucosine":
        return normalize_f32(x)
    return x - np.float32(0.5) if shifted else x


@pytest.fixture(scope="module")
def net():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.net_amd


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _same_lists(got, want):
    return len(got[0]) == len(want[0]) and all(a.tolist() == b.tolist() and c.tobytes() == e.tobytes()
                                               for a, b, c, e in zip(got[0], want[0], got[1], want[1]))


# ---- 1. records and distances --------------------------------------------------------------------------------------------
CASES = [(m, d, False) for m in F16 for d in DIMS] + [("sq_euclid_f16", d, True) for d in DIMS if d <= 33]


@pytest.mark.parametrize("metric,dim,shifted", CASES)
def test_records_survive_growth_and_distances_are_the_f32_ones_on_rounded_rows(net, metric, dim, shifted):
    X, n, nq = F16[metric], 3000, 40
    x, q = _data(metric, n, dim, 100 + dim, shifted), _data(metric, nq, dim, 200 + dim, shifted)
    xh = h(x)
    dev = net.DeviceBackend(dim, metric, capacity=100)
    dev.upload_rows(0, x[:100])
    dev.reserve(n)                               # the records must survive the growth
    dev.upload_rows(100, x[100:])
    assert dev.download_rows(0, 200).tobytes() == xh[:200].tobytes()
    assert dev.stats()["row_bytes"] == 2 * dim
    rng = np.random.default_rng(dim)
    counts = rng.integers(0, 70, nq)
    counts[0], counts[1], counts[2] = 0, 65, 69
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    ids = rng.integers(0, n, off[-1]).astype(np.int32)
    got = dev.dist_query_batch(q, off, ids)      # queries stay f32
    want = np.concatenate([oracle.dist_query_rows(X, xh, q[i], ids[off[i]:off[i + 1]]) for i in range(nq)])
    assert got.tobytes() == want.tobytes()
    a, b = rng.integers(0, n, 5000).astype(np.int32), rng.integers(0, n, 5000).astype(np.int32)
    a[:10] = b[:10]
    ab, ba = dev.dist_pair_batch(a, b), dev.dist_pair_batch(b, a)
    assert ab.tobytes() == oracle.dist_pairs(X, xh, a, b).tobytes()
    assert ab.tobytes() == ba.tobytes()
    if X == "sq_euclid":
        assert (ab[:10] == 0).all()


def test_conversion_edges_are_numpys(net):
    dim = 24
    edges = np.array([65504.0, 65519.99, 65520.0, 2.98e-8, 3e-8, 6e-8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -0.0, np.nan], dtype=np.float32)
    x = uniform(8, dim, 3)
    x[0, :10] = edges                            # low halves of the record's words (and two high ones)
    x[1, 10:20] = -edges                         # high halves, the second block
    x[2, 14:24] = edges[::-1]
    dev = net.DeviceBackend(dim, "sq_euclid_f16", capacity=8)
    dev.upload_rows(0, x)
    got = dev.download_rows(0, 8)
    with np.errstate(over="ignore"):
        want = h(x)
    assert np.isinf(want[0, 2]) and want[0, 3] == 0 and want[0, 4] > 0 and np.signbit(want[0, 8]) and want[0, 6] == 1 and want[0, 7] > 1
    nan = np.isnan(want)
    assert nan.sum() == 3 and (np.isnan(got) == nan).all()
    assert got[~nan].tobytes() == want[~nan].tobytes()


# ---- 2. index parity -----------------------------------------------------------------------------------------------------
class Case:
    """Data, rounded data and the oracle indexes of one (metric, shape), built once for the module."""

    def __init__(self, metric, shape):
        self.metric, self.X = metric, F16[metric]
        self.dim, self.M, self.efc = shape
        self.x, self.q = _data(metric, N, self.dim, 21), _data(metric, NQ, self.dim, 22)
        self.xh = h(self.x)
        self._refs, self._built = {}, {}

    def params(self):
        return dict(max_edges=self.M, max_candidates=self.efc)

    def ref(self, kind):
        if kind not in self._refs:
            if kind == "seq":
                r = oracle.OracleIndex(self.dim, self.X, collection_size=1024, **self.params())
                r.add(self.xh[:1500])
            else:
                r = oracle.OracleIndex(self.dim, self.X, collection_size=N, **self.params())
                r.add_batched(self.xh, default_cap() if kind == "default" else 65536)
            self._refs[kind] = r
        return self._refs[kind]

    def index(self, Index, metric=None, collection=N):
        ix = Index(self.dim, metric or self.metric)
        ix.set_collection_size(collection); ix.set_max_edges(self.M); ix.set_max_candidates(self.efc)
        return ix

    def built(self, Index, traversal):
        """The f16 index under the default schedule (shared by the query checks)."""
        if traversal not in self._built:
            ix = self.index(Index)
            ix.set_device_traversal(traversal == "device")
            ix.add(self.x)
            self._built[traversal] = ix
        return self._built[traversal]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric, shape):
        if (metric, shape) not in cache:
            cache[(metric, shape)] = Case(metric, shape)
        return cache[(metric, shape)]
    return get


@pytest.fixture(scope="module")
def Index(net):
    import hnswindex
    return hnswindex.Index


PARITY = pytest.mark.parametrize("traversal", ["device", "host"])
ALL = [pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s))), pytest.mark.parametrize("metric", list(F16))]


def every_case(f):
    for m in ALL:
        f = m(f)
    return PARITY(f)


@every_case
def test_sequential_add_matches_the_oracle_on_rounded_rows(Index, cases, metric, shape, traversal):
    c = cases(metric, shape)
    ix = c.index(Index, collection=1024)
    ix.set_device_traversal(traversal == "device")
    ix.set_insert_batch(1)
    ids = ix.add(c.x[:1500])                     # capacity grows on the way
    ref = c.ref("seq")
    assert ids.tolist() == list(range(1500)) and ix.graph_hash() == ref.graph_hash()
    assert ix.levels().tolist() == ref.levels().tolist() and ix.entry_point == ref.entry_point
    for k in (1, 10, 40):
        assert _same(ix.knn_query(c.q, k), ref.knn_query(c.q, k)), k


@every_case
def test_default_schedule_and_queries_match_the_oracle(Index, cases, metric, shape, traversal):
    c = cases(metric, shape)
    ix, ref = c.built(Index, traversal), c.ref("default")
    assert ix.graph_hash() == ref.graph_hash() and ix.levels().tolist() == ref.levels().tolist()
    for k in (1, 10, 40):
        assert _same(ix.knn_query(c.q, k), ref.knn_query(c.q, k)), k
    assert _same(ix.knn_query(c.q[:1], 10), ref.knn_query(c.q[:1], 10))
    assert ix.stats()["row_bytes"] == 2 * c.dim


@every_case
def test_the_65536_cap_matches_the_oracle(Index, cases, metric, shape, traversal):
    c = cases(metric, shape)
    ix = c.index(Index)
    ix.set_device_traversal(traversal == "device")
    ix.set_insert_batch(65536)
    ix.add(c.x)
    assert ix.graph_hash() == c.ref("cap").graph_hash()


@every_case
def test_range_query_at_the_median_fourth_neighbour(Index, cases, metric, shape, traversal):
    c = cases(metric, shape)
    ix, ref = c.built(Index, traversal), c.ref("default")
    radius = float(np.median(ref.knn_query(c.q, 4)[1][:, 3]))
    got, want = ix.range_query(c.q, radius), ref.range_query(c.q, radius, cap=N)
    assert sum(len(a) for a in got[0]) > NQ and _same_lists(got, want)


@every_case
def test_remove_then_add_matches_the_oracle(Index, cases, metric, shape, traversal):
    c = cases(metric, shape)
    n0 = N - 200
    ix = c.index(Index)
    ix.set_device_traversal(traversal == "device")
    ix.add(c.x[:n0])
    ref = oracle.OracleIndex(c.dim, c.X, collection_size=N, **c.params())
    ref.add_batched(c.xh[:n0], default_cap())
    assert ix.graph_hash() == ref.graph_hash()
    victims = np.random.default_rng(5).permutation(n0)[:200].astype(np.int32)
    ix.remove(victims); ref.remove(victims)
    ix.add(c.x[n0:]); ref.add_batched(c.xh[n0:], default_cap())   # the inserted rows are rounded first; their searches use the rounded rows
    assert ix.graph_hash() == ref.graph_hash() and ix.ids().tolist() == ref.active_ids().tolist()
    assert _same(ix.knn_query(c.q, 10), ref.knn_query(c.q, 10))


@every_case
def test_filtered_layer_and_multilayer_queries_match_the_models(Index, cases, metric, shape, traversal):
    c = cases(metric, shape)
    ix, ref = c.built(Index, traversal), c.ref("default")
    mask = np.random.default_rng(9).random(N) < 0.1
    min_nn = 5                                   # the default MinNN of both
    assert _same(ix.knn_query(c.q, 10, allowed=mask), filtered_knn_batch(ref, c.xh, c.X, c.q, 10, min_nn, mask))
    radius = float(np.median(ref.knn_query(c.q, 4)[1][:, 3]))
    assert _same_lists(ix.range_query(c.q, radius, allowed=mask), filtered_range_batch(ref, c.xh, c.X, c.q, radius, mask))
    assert ix.top_layer() >= 1
    assert _same(ix.knn_query(c.q, 10, layer=1), knn_at_layer_batch(ref, c.xh, c.X, c.q, 10, min_nn, 1))
    assert _same(ix.multilayer_knn_query(c.q, 5), multilayer_knn_batch(ref, c.q, 5))


@pytest.mark.parametrize("metric", list(F16))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_f32_index_of_this_library_on_rounded_rows_is_the_same_graph(Index, cases, metric, shape):
    c = cases(metric, shape)
    iy = c.index(Index, metric=c.X)
    iy.add(c.xh)
    ix = c.built(Index, "device")
    assert iy.graph_hash() == ix.graph_hash()
    assert _same(iy.knn_query(c.q, 10), ix.knn_query(c.q, 10))


# An odd number of 8-blocks (dim 120: the `nblk & 1` step of measure_pass_h / measure_pass2_h / measure_pass_multi_h) and rows beyond
# 256 elements with an odd block count (dim 264: the heuristic stages its candidates on demand, one per step).
ODD = [(120, 12, 80, 4000), (264, 8, 60, 2000)]


@pytest.mark.parametrize("metric", list(F16))
@pytest.mark.parametrize("dim,M,efc,n", ODD, ids=lambda v: str(v))
@pytest.mark.parametrize("way", ["device", "host", "lat2", "novis0"])
def test_odd_block_counts_and_long_rows_match_the_oracle(Index, monkeypatch, metric, dim, M, efc, n, way):
    if way == "lat2":
        set_diag(monkeypatch, lat=2)
    if way == "novis0":
        set_diag(monkeypatch, novis=0)
    x, q = _data(metric, n, dim, 61), _data(metric, 200, dim, 62)
    ix = Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_max_candidates(efc); ix.set_device_traversal(way != "host")
    ix.add(x)
    ref = oracle.OracleIndex(dim, F16[metric], collection_size=n, max_edges=M, max_candidates=efc)
    ref.add_batched(h(x), default_cap())
    assert ix.graph_hash() == ref.graph_hash()
    for k in (1, 10, 40):
        assert _same(ix.knn_query(q, k), ref.knn_query(q, k)), k
    assert _same(ix.knn_query(q[:1], 10), ref.knn_query(q[:1], 10))
    radius = float(np.median(ref.knn_query(q, 4)[1][:, 3]))
    assert _same_lists(ix.range_query(q, radius), ref.range_query(q, radius, cap=n))


@pytest.mark.parametrize("metric,dim", [("sq_euclid_f16", 7), ("ucosine_f16", 24)])
def test_a_large_add_rounds_its_rows_on_the_background_upload_like_the_device(Index, tmp_path, metric, dim):
    # an Add of 262 144 rows or more uploads all but its first 65 536 rows from a host thread, which rounds them itself
    n = 270_000
    x, q = _data(metric, n, dim, 81), _data(metric, 200, dim, 82)
    xh = h(x)
    res = {}
    for m, rows in ((metric, x), (F16[metric], xh)):
        ix = Index(dim, m)
        ix.set_collection_size(n); ix.set_max_edges(6); ix.set_max_candidates(24); ix.set_insert_batch(65536)
        ix.add(rows)
        res[m] = (ix, ix.graph_hash(), ix.knn_query(q, 10))
    assert res[metric][1] == res[F16[metric]][1] and _same(res[metric][2], res[F16[metric]][2])
    # the stored rows, through a snapshot (one tag byte and four bytes per element): h(x), also for rows that went up in the background
    path = tmp_path / "big.bin"
    res[metric][0].serialize(path)
    data = path.read_bytes()
    tag, p = None, data.find(xh[0, :1].tobytes())
    while p > 0 and tag is None:    # the element tag: the byte in front of row 0's first float, where the whole row follows in that form
        t = data[p - 1:p]
        if data[p - 1:p - 1 + 5 * dim] == b"".join(t + v.tobytes() for v in xh[0]):
            tag = t
        p = data.find(xh[0, :1].tobytes(), p + 1)
    assert tag is not None
    for i in [0, 1, 65535, 65536, 65537, 100_000, 200_003, n - 2, n - 1] + np.random.default_rng(1).integers(0, n, 40).tolist():
        assert b"".join(tag + v.tobytes() for v in xh[i]) in data, i


# ---- 3. forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", list(F16))
@pytest.mark.parametrize("diag", [dict(lat=0), dict(lat=2), dict(lean=0), dict(sorted_top=0), dict(vis_hash=1)], ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_every_traversal_form_answers_alike(Index, cases, monkeypatch, metric, diag):
    set_diag(monkeypatch, **diag)
    c = cases(metric, (128, 12, 80))
    ref = c.ref("default")
    ix = c.index(Index)
    ix.add(c.x)
    assert ix.graph_hash() == ref.graph_hash()
    want = ref.knn_query(c.q, 10)
    assert _same(ix.knn_query(c.q, 10), want)                              # a 400-query call
    assert _same(ix.knn_query(c.q[:1], 10), (want[0][:1], want[1][:1]))    # a one-query call


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("metric,dim,kind", [("ucosine_f16", 256, "unit"), ("sq_euclid_f16", 256, "centred")])
def test_the_heuristic_decides_on_exact_distances_with_the_gram_tile_allowed_or_not(Index, monkeypatch, metric, dim, kind, mfma):
    # the shape at which the f32 metrics run the MFMA Gram-block prefilter (beams above 256 candidates, rows of >= 256 elements)
    set_diag(monkeypatch, mfma=mfma)
    n, M, efc = 2500, 24, 300
    x = uniform(n, dim, 71)
    x = normalize_f32(x) if kind == "unit" else x - np.float32(0.5)
    q = x[:100] + np.float32(0.01)
    ix = Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_max_candidates(efc); ix.set_min_nn(64); ix.set_insert_batch(700)
    ix.add(x)
    ref = oracle.OracleIndex(dim, F16[metric], max_edges=M, max_candidates=efc, min_nn=64, collection_size=n)
    ref.add_batched(h(x), 700)
    assert ix.graph_hash() == ref.graph_hash()
    assert _same(ix.knn_query(q, 10), ref.knn_query(q, 10))
    assert _same(ix.knn_query(q[:1], 10), ref.knn_query(q[:1], 10))


# ---- 4. snapshot -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", list(F16))
def test_snapshot_round_trip_and_later_add(Index, cases, tmp_path, metric):
    c = cases(metric, (33, 8, 60))
    n0 = 3000
    ix = c.index(Index)
    ix.add(c.x[:n0])
    want = ix.knn_query(c.q, 10)
    path = tmp_path / "f16.bin"
    ix.serialize(path)
    back = Index.deserialize(path, metric)       # rounding the stored h(x) again changes nothing
    assert back.graph_hash() == ix.graph_hash() and _same(back.knn_query(c.q, 10), want)
    f32 = Index.deserialize(path, c.X)           # the file holds h(x) as floats: an f32 index of the same family reads it
    assert f32.graph_hash() == ix.graph_hash() and _same(f32.knn_query(c.q, 10), want)
    # a later Add: the oracle given the saved graph and the rounded rows (a loaded index draws its levels from a fresh Random(RandomSeed))
    lv = back.levels()
    ref = oracle.OracleIndex(c.dim, c.X, collection_size=N, **c.params())
    ref.import_graph(c.xh[:n0], lv, back.entry_point, [back.export_edges(L, 2 * c.M + 2 if L == 0 else c.M + 2) for L in range(int(lv.max()) + 1)])
    assert ref.graph_hash() == back.graph_hash()
    back.add(c.x[n0:]); ref.add_batched(c.xh[n0:], default_cap())
    assert back.graph_hash() == ref.graph_hash() and _same(back.knn_query(c.q, 10), ref.knn_query(c.q, 10))


# ---- 5. quality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,metric,shifted", [(96, "sq_euclid_f16", False), (33, "sq_euclid_f16", True), (64, "ucosine_f16", False)])
def test_rounding_the_rows_costs_next_to_nothing(Index, dim, metric, shifted):
    """overlap@10 of the f16 index with the f32 index on the unrounded rows > 0.95 (the oracle alone: 0.983, 0.999, 0.988 on these
    inputs), and recall@10 against exact float64 brute force on the unrounded rows within 0.01 of the f32 index's."""
    X = F16[metric]
    x, q = _data(metric, N, dim, 41, shifted), _data(metric, NQ, dim, 42, shifted)
    res = {}
    for m in (metric, X):
        ix = Index(dim, m)
        ix.set_collection_size(N); ix.set_max_edges(12); ix.set_max_candidates(80); ix.set_min_nn(40)
        ix.add(x)
        res[m] = ix.knn_query(q, 10)[0]
    xd, qd = x.astype(np.float64), q.astype(np.float64)
    if X == "sq_euclid":
        D = (qd * qd).sum(1)[:, None] + (xd * xd).sum(1)[None, :] - 2.0 * qd @ xd.T
    else:
        D = 1.0 - qd @ xd.T
    truth = np.argsort(D, axis=1, kind="stable")[:, :10]
    overlap = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(res[metric], res[X])])
    recall = {m: np.mean([len(set(a) & set(t)) / 10 for a, t in zip(res[m], truth)]) for m in res}
    print(f"overlap@10 {overlap:.4f} recall@10 f16 {recall[metric]:.4f} f32 {recall[X]:.4f}")
    assert overlap > 0.95
    assert abs(recall[metric] - recall[X]) <= 0.01


# ---- 6. stats and sharding ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", list(F16))
def test_two_contexts_answer_like_one(Index, cases, metric):
    c = cases(metric, (96, 16, 100))
    one = c.built(Index, "device")
    two = c.index(Index)
    two.set_devices(2)
    two.add(c.x)
    got = two.knn_query(c.q, 10)
    assert _same(got, one.knn_query(c.q, 10)) and _same(got, c.ref("default").knn_query(c.q, 10))
    assert two.stats_at(1)["replica_bytes"] > 0 and two.stats_at(1)["search_launches"] >= 1
    assert two.stats()["row_bytes"] == 2 * c.dim
