"""GPU tier: knn_query_collapsed (hnsw_mi355x_knn_query_collapsed) -- the traversal's answer at a beam, collapsed to at
most per_group results per label on the device before it is copied out (collapse_rows_kernel), or on the host where the answer
comes from there.  Every run must be byte for byte the numpy walk (tests/collapse_model.py) over the rows that
knn_query(q, beam, allowed=..., layer=...) returns.  2 000 rows x dim 20, M = 8, 48 queries, three row kinds."""
import numpy as np
import pytest

from collapse_model import collapsed_rows
from common import normalize_f32, uniform

pytestmark = pytest.mark.gpu

N, DIM, NQ, M, K = 2000, 20, 48, 8, 10
METRICS = ["sq_euclid", "cosine", "ucosine_f16"]


def _data(metric, n, seed):
    x = uniform(n, DIM, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _index(metric, **knobs):
    import hnswindex
    ix = hnswindex.Index(DIM, metric)
    ix.set_collection_size(N); ix.set_max_edges(M); ix.set_insert_batch(0)
    for name, v in knobs.items():
        getattr(ix, name)(v)
    return ix


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


def _threes():
    return (np.repeat(np.arange(N // 3 + 1), 3)[:N][np.random.default_rng(3).permutation(N)] - 300).astype(np.int32)


def _heavy():
    """Three labels: -1 holds 90 % of the rows."""
    lab = np.full(N, -1, np.int32)
    rest = np.random.default_rng(4).permutation(N)[: N // 10]
    lab[rest[::2]] = 2 ** 31 - 1
    lab[rest[1::2]] = 0
    return lab


def _allowed():
    a = np.zeros(N, bool)
    a[np.random.default_rng(8).choice(N, N // 4, replace=False)] = True
    return a


def _check(ix, q, want_of):
    """Every combination of beam, labels and cap against the walk over the plain call's rows (want_of(beam, allowed, layer), cached)."""
    for labels in (_threes(), _heavy()):
        for beam in (K, 4 * K, 200):
            for m in (1, 2):
                for allowed, layer in ((None, 0), (_allowed(), 0), (None, 1), (_allowed(), 1)):
                    got = ix.knn_query_collapsed(q, K, labels, per_group=m, beam=beam, allowed=allowed, layer=layer)
                    want = collapsed_rows(*want_of(beam, allowed, layer), labels, K, m)
                    assert _same(got, want), (beam, m, allowed is not None, layer)
        # the default beam is 4 * k
        assert _same(ix.knn_query_collapsed(q, K, labels), collapsed_rows(*want_of(4 * K, None, 0), labels, K, 1))


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x, self.q = _data(metric, N, 1), _data(metric, NQ, 2)
        self.ix = _index(metric)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        assert self.ix.top_layer() >= 1
        self._plain = {}

    def plain(self, beam, allowed, layer):
        key = (beam, allowed is not None, layer)
        if key not in self._plain:
            self._plain[key] = self.ix.knn_query(self.q, beam, allowed=allowed, layer=layer)
        return self._plain[key]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


@pytest.mark.parametrize("metric", METRICS)
def test_the_device_way_is_the_walk_over_knn_query(cases, metric):
    c = cases(metric)
    c.ix.reset_stats()
    _check(c.ix, c.q, c.plain)
    assert c.ix.stats()["search_launches"] > 0
    # per_group == k: the cap cannot bind, the row is the plain call's first k entries
    got = c.ix.knn_query_collapsed(c.q, K, _heavy(), per_group=K, beam=200)
    plain = c.plain(200, None, 0)
    assert _same(got, (plain[0][:, :K], plain[1][:, :K]))
    # three labels, one result each: 3 results and 7 paddings whatever the beam finds
    ids, d = c.ix.knn_query_collapsed(c.q, K, _heavy(), beam=200)
    assert ((ids >= 0).sum(axis=1) <= 3).all() and (ids[:, 3:] == -1).all() and np.isnan(d[:, 3:]).all() and (ids[:, 0] >= 0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_the_host_way_gives_the_same_bytes(cases, metric):
    c = cases(metric)
    host = _index(metric, set_device_traversal=False)
    try:
        host.add(c.x)
        host.reset_stats()
        _check(host, c.q, c.plain)                      # against the DEVICE index's plain rows: same graph, same bytes
        assert host.stats()["search_launches"] == 0
    finally:
        host.set_device_traversal(True)


def test_argument_errors(cases):
    c = cases("sq_euclid")
    rg = _threes()
    with pytest.raises(ValueError, match="beam = 9 is below k = 10"):
        c.ix.knn_query_collapsed(c.q, K, rg, beam=9)
    with pytest.raises(ValueError, match=r"per_group = 11 is outside \[1, k = 10\]"):
        c.ix.knn_query_collapsed(c.q, K, rg, per_group=11)
    with pytest.raises(ValueError, match=f"row_group has {N - 1} entries, the index's length is {N}"):
        c.ix.knn_query_collapsed(c.q, K, rg[:-1])
    with pytest.raises(RuntimeError, match="layer 99 is outside"):
        c.ix.knn_query_collapsed(c.q, K, rg, layer=99)
    assert _same(c.ix.knn_query_collapsed(c.q, K, rg), collapsed_rows(*c.plain(4 * K, None, 0), rg, K, 1))
