"""GPU tier: quantize_rows_kernel -- the one int8 quantiser of stored rows and of queries -- on the rows where a quantiser goes
wrong (tests/int8_edges.py): rintf ties, a denormal scale, a scale that rounds to zero, the smallest normal scale, the largest
floats, negative zeros, the row maximum beyond a lane's first 256-element stretch, inf and NaN elements.  The oracle's records
(oracle/hnsw_oracle.c "int8 rows") are the definition: a record that differs in one element changes every distance of its row.

Equality of bytes everywhere; where the definition's value is a NaN (0 x an infinite scale; inf - inf in the distance) the NaN
positions are compared instead of the payloads."""
import numpy as np
import pytest

import oracle
from common import uniform
from exact_knn_model import exact_knn
from int8_edges import EDGE_DIMS, edge_rows

pytestmark = pytest.mark.gpu

METRIC = "sq_euclid_i8"


def _same_numbers(got, want):
    """Byte-equal where `want` is a number, NaN exactly where it is not."""
    got, want = np.asarray(got, np.float32).ravel(), np.asarray(want, np.float32).ravel()
    nan = np.isnan(want)
    return got.shape == want.shape and (np.isnan(got) == nan).all() and got[~nan].tobytes() == want[~nan].tobytes()


@pytest.fixture(scope="module", params=EDGE_DIMS)
def edge(request):
    """(dim, rows, backend): the finite edge rows, the three non-finite ones and four ordinary rows, uploaded in two parts around a
    reserve() that moves the records."""
    import hnswindex
    dim = request.param
    finite, non_finite = edge_rows(dim)
    rows = np.concatenate([finite, non_finite, uniform(4, dim, 5) - np.float32(0.5)])
    rows.setflags(write=False)
    dev = hnswindex.DeviceBackend(dim, METRIC, capacity=4)
    dev.upload_rows(0, rows[:4])
    dev.reserve(64)                                   # the records survive the growth
    dev.upload_rows(4, rows[4:])
    return dim, rows, dev, finite.shape[0]


def test_stored_records_are_the_oracles(edge):
    dim, rows, dev, n_finite = edge
    q, s, n = oracle.i8_quantize(rows)
    assert np.isinf(s[n_finite]) and np.isfinite(s[n_finite + 1]) and np.isinf(s[n_finite + 2])     # the rows are what the module says
    assert s[3] == 0 and 0 < s[2] < np.finfo(np.float32).tiny and s[4] == np.finfo(np.float32).tiny and s[0] == 1
    with np.errstate(invalid="ignore"):
        want = (q.astype(np.float32) * s[:, None]).astype(np.float32)       # 0 x inf: NaN
    got = dev.download_rows(0, rows.shape[0])
    for r in range(rows.shape[0]):
        assert _same_numbers(got[r], want[r]), (dim, r, np.flatnonzero(got[r] != want[r])[:8])
    assert np.isnan(want[n_finite]).sum() == dim - 1 and not np.isnan(want[:n_finite]).any()


def test_pair_distances_are_the_oracles(edge):
    dim, rows, dev, _ = edge
    r = rows.shape[0]
    a, b = [m.ravel().astype(np.int32) for m in np.meshgrid(np.arange(r), np.arange(r), indexing="ij")]    # every ordered pair
    want = oracle.dist_pairs(METRIC, rows, a, b)
    got = dev.dist_pair_batch(a, b)
    bad = np.flatnonzero(~((np.isnan(got) & np.isnan(want)) | (got.view(np.uint32) == want.view(np.uint32))))
    assert bad.size == 0 and _same_numbers(got, want), (dim, [(int(a[i]), int(b[i]), float(got[i]), float(want[i])) for i in bad[:8]])
    assert _same_numbers(got.reshape(r, r).T, got.reshape(r, r))          # symmetric
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any()


def test_query_records_are_the_oracles(edge):
    """The edge rows as the queries: set_queries quantises them with the same kernel into the resident query records."""
    dim, rows, dev, _ = edge
    r = rows.shape[0]
    ids = np.tile(np.arange(r, dtype=np.int32), r)
    off = (np.arange(r + 1) * r).astype(np.int32)
    got = dev.dist_query_batch(rows, off, ids).reshape(r, r)
    for i in range(r):
        want = oracle.dist_query_rows(METRIC, rows, rows[i], np.arange(r, dtype=np.int32))
        assert _same_numbers(got[i], want), (dim, i, got[i].tolist(), want.tolist())


def test_exact_knn_orders_them_as_the_model(edge):
    dim, rows, dev, _ = edge
    r = rows.shape[0]
    dev.reset_stats()
    got_ids, got_d = dev.exact_knn(rows, r)
    w_ids, w_d = exact_knn(METRIC, rows, rows, r)
    assert (got_ids == w_ids).all(), (dim, np.flatnonzero((got_ids != w_ids).any(axis=1)))
    assert _same_numbers(got_d, w_d)
    st = dev.stats()
    assert st["exact_evals"] == r * r and st["exact_launches"] == 1
    nan = np.isnan(w_d)
    assert nan.any()
    for i in range(r):                                # NaN distances last, among themselves by id
        c = int(nan[i].sum())
        assert not nan[i, :r - c].any() and (np.diff(got_ids[i, r - c:]) > 0).all()
