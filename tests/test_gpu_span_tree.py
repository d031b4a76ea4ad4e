"""GPU tier: single_linkage_tree and single_linkage_cut -- the minimum spanning forest of the stored rows under
the strict order (distance, a, b), by Boruvka's rounds of span_scan_kernel.  The reference is Kruskal in numpy over all pairs in that
order; the forest is unique, so every comparison is of bytes.  Weights: float64 numpy where every distance is an exact integer, and
otherwise the device's own bits as exact_range_query_by_id reports them at radius +inf (exact_knn_query_by_id, which the contract
names for this, takes k <= 1024 and cannot return the 2 999 distances of a row; the range call returns the same bits)."""
import numpy as np
import pytest

from common import set_diag
from density_rows import CHUNK, DIM, METRICS, N, QTILE, ROUND, links, numpy_dist, radius_between, rows

pytestmark = pytest.mark.gpu


def kruskal(w, members):
    """(a, b, dist float32) of the minimum spanning forest of `members` under w[a, b] (a < b; NaN: no edge), ordered by (w, a, b)."""
    ia, ib = np.triu_indices(len(members), 1)
    a, b = members[ia], members[ib]
    d = w[a, b] + 0.0                                                     # -0 is +0
    order = np.lexsort((b, a, d))[:int((~np.isnan(d)).sum())]             # NaN sorts last: no edge
    parent, out = {int(v): int(v) for v in members}, []
    for e in order:
        ra, rb = int(a[e]), int(b[e])
        while parent[ra] != ra: ra = parent[ra]
        while parent[rb] != rb: rb = parent[rb]
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            for v in (int(a[e]), int(b[e])): parent[v] = min(ra, rb)
            out.append(e)
            if len(out) == len(members) - 1: break
    out = np.array(out, dtype=np.int64)
    return a[out].astype(np.int32), b[out].astype(np.int32), d[out].astype(np.float32)


def _index(dim, metric, n):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(8); ix.set_insert_batch(0)
    return ix


def _same(got, want, what=None):
    assert got[0].dtype == got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want)), what


def _accounted(info, m):
    assert info["members"] == m and info["edges"] + info["components"] == m and info["reserved"] == 0
    assert info["pairs_measured"] + info["pairs_skipped"] == info["rounds"] * (m * (m - 1) // 2), info


def _device_weights(ix, n):
    """w[a, b]: the device's bits for candidate b with the stored row of a as the query (NaN where it reports none)."""
    lists, dists = ix.exact_range_query_by_id(np.arange(n), float("inf"))
    w = np.full((n, n), np.nan, np.float64)
    for a, (ids, d) in enumerate(zip(lists, dists)):
        w[a, ids] = d
    return w


class Case:
    def __init__(self, metric):
        self.x = rows(metric)
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        self.want = kruskal(_device_weights(self.ix, N), np.arange(N))    # computed once per row kind
        self.r = radius_between(metric, self.x, links())[0]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_f16"])
def test_ties_are_broken_by_ids_against_float64(metric):
    """Coordinates 0 / 1 / 2: every distance is an integer below 81, exact in f16, f32 and f64, and thousands of pairs share each;
    one row under three ids and a run of equal rows, so distance 0 occurs under several ids."""
    x = np.random.default_rng(5).integers(0, 3, (N, DIM)).astype(np.float32)
    x[1500] = x[2900] = x[100]
    x[690:710] = x[690]
    ix = _index(DIM, metric, N)
    ix.add(x)
    got = ix.single_linkage_tree()
    _same(got, kruskal(numpy_dist(metric, x), np.arange(N)), metric)
    assert got[3]["edges"] == N - 1 and got[3]["components"] == 1 and (got[0] < got[1]).all()
    _accounted(got[3], N)


@pytest.mark.parametrize("metric", METRICS)
def test_every_row_kind_and_the_cuts(cases, metric):
    c = cases(metric)
    tree = c.ix.single_linkage_tree()
    _same(tree, c.want, metric)
    _accounted(tree[3], N)
    for r in (c.r, c.r / 2, c.r * 2, float("inf")):
        cut = c.ix.single_linkage_cut(tree, r)
        assert cut.dtype == np.int32 and cut.tobytes() == c.ix.duplicate_groups(r)[0].tobytes(), (metric, r)


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8"])
def test_chunks_tiles_and_rounds_keep_the_bytes(cases, monkeypatch, metric):
    c = cases(metric)
    small = dict(exact_chunk=CHUNK, exact_qtile=QTILE)                    # CHUNK is no multiple of 128: segments straddle chunks
    for knobs, pieces in (({}, 1), (small, 1), (dict(small, span_round=ROUND), -(-N // ROUND))):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for _ in range(2):                                                # the offers arrive in another order every time
            c.ix.reset_stats()
            got = c.ix.single_linkage_tree()
            st = c.ix.stats()
            _same(got, c.want, (metric, knobs))
            _accounted(got[3], N)
            assert got[3]["launches"] == got[3]["rounds"] * pieces == st["exact_launches"] and st["search_launches"] == 0
            assert st["exact_evals"] == got[3]["pairs_measured"]


def _ruler(n, scale):
    """n positions on a line whose gaps are scale x (1, 2, 1, 3, 1, 2, 1, 4, ..): Boruvka halves them, log2(n) rounds."""
    gaps = [((i & -i).bit_length()) * scale for i in range(1, n)]
    return np.concatenate(([0], np.cumsum(gaps))).astype(np.float32)


def test_rounds_the_skip_and_the_bridge():
    # two blobs of 256 grid rows on ruler lines, 5 000 apart in another coordinate, interleaved in id: A even, B odd
    n = 512
    x = np.zeros((n, 4), np.float32)
    x[0::2, 0] = x[1::2, 0] = _ruler(n // 2, 1)
    x[1::2, 1] = 5000
    ix = _index(4, "sq_euclid", n)
    ix.add(x)
    a, b, d, info = ix.single_linkage_tree()
    _same((a, b, d), kruskal(numpy_dist("sq_euclid", x), np.arange(n)))
    _accounted(info, n)
    assert info["rounds"] >= 3 and info["pairs_skipped"] > 0 and info["edges"] == n - 1
    assert (a[-1], b[-1], d[-1]) == (0, 1, 25e6) and ((a[:-1] ^ b[:-1]) & 1 == 0).all()   # the last edge is the one bridge
    # one blob under the contiguous ids [0, 384) -- three whole segments of 128 -- that is one component after the first round (unit
    # gaps), beside 128 rows on a ruler line that take seven: from the second round on the blob's pairs are all skipped
    blob = 384
    y = np.zeros((n, 4), np.float32)
    y[:blob, 0] = np.arange(blob)
    y[blob:, 0] = 4000 + _ruler(n - blob, 10)
    ix = _index(4, "sq_euclid", n)
    ix.add(y)
    a, b, d, info = ix.single_linkage_tree()
    _same((a, b, d), kruskal(numpy_dist("sq_euclid", y), np.arange(n)))
    _accounted(info, n)
    assert info["rounds"] >= 3 and info["pairs_skipped"] >= (info["rounds"] - 1) * (blob * (blob - 1) // 2)


def test_allowed_sets_removed_ids_and_few_members(monkeypatch):
    n = 600
    x = np.random.default_rng(8).integers(0, 4, (n, DIM)).astype(np.float32)
    w = numpy_dist("sq_euclid", x)
    ix = _index(DIM, "sq_euclid", n)
    ix.set_allow_removals(True)
    ix.add(x)
    set_diag(monkeypatch, exact_chunk=200, exact_qtile=QTILE, span_round=256)
    allowed = np.ones(n, bool)
    allowed[[0, 5, 6, 7, 8, 9, 203, 599] + list(range(300, 390))] = False     # cuts tiles of 8, a chunk edge and a round edge
    members = np.flatnonzero(allowed)
    for sel in (allowed, members):                                         # the set as a mask and as an id list
        tree = ix.single_linkage_tree(allowed=sel)
        _same(tree, kruskal(w, members))
        _accounted(tree[3], members.size)
        assert ix.single_linkage_cut(tree, 20.0, allowed=sel).tobytes() == ix.duplicate_groups(20.0, allowed=sel)[0].tobytes()
    ix.reset_stats()
    for sel, m in ((np.zeros(n, bool), 0), ([17], 1)):                     # fewer than two members launch nothing
        a, b, d, info = ix.single_linkage_tree(allowed=sel)
        assert a.size == b.size == d.size == 0 and info == {**dict.fromkeys(info, 0), "members": m, "components": m}
    assert ix.stats()["exact_launches"] == 0
    a, b, d, info = ix.single_linkage_tree(allowed=[17, 400])
    assert (a.tolist(), b.tolist(), d.tolist()) == ([17], [400], [w[17, 400]]) and info["rounds"] == info["launches"] == 1
    gone = [1, 2, 203, 204, 511, 598]
    ix.remove(gone)
    live = np.delete(np.arange(n), gone)
    tree = ix.single_linkage_tree()
    _same(tree, kruskal(w, live))
    assert ix.single_linkage_cut(tree, 20.0).tobytes() == ix.duplicate_groups(20.0)[0].tobytes()
    both = np.setdiff1d(members, gone)
    _same(ix.single_linkage_tree(allowed=allowed), kruskal(w, both))


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_device_backend_nan_and_negative_zero(cases, metric):
    import hnswindex
    c = cases(metric)
    dev = hnswindex.DeviceBackend(DIM, metric, capacity=N)
    dev.upload_rows(0, c.x)
    got = dev.exact_span_tree(N)
    _same(got, c.want, metric)
    part = dev.exact_span_tree(1000, allowed=np.arange(1, 1000))           # rows [0, 1000) with an allow-set on top
    assert part[3]["members"] == 999 and part[3]["edges"] == 998 and part[0].min() == 1 and part[1].max() == 999
    if metric != "sq_euclid":
        return
    # a row of NaN has no edge: a forest of two components; -0.0 against +0.0 is distance +0, a tie with the exact duplicates
    y = np.random.default_rng(3).integers(0, 3, (40, DIM)).astype(np.float32)
    y[7] = np.nan
    y[11], y[30], y[35] = 0.0, -0.0, 0.0
    dev = hnswindex.DeviceBackend(DIM, metric, capacity=40)
    dev.upload_rows(0, y)
    a, b, d, info = dev.exact_span_tree(40)
    w = numpy_dist(metric, y)
    _same((a, b, d), kruskal(w, np.arange(40)))
    assert info["components"] == 2 and info["edges"] == 38 and 7 not in a.tolist() + b.tolist()
    assert (a[:2].tolist(), b[:2].tolist()) == ([11, 11], [30, 35]) and d[:2].tobytes() == np.zeros(2, np.float32).tobytes()
    _accounted(info, 40)
