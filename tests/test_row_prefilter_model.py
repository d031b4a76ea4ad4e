"""CPU tier: the bound behind KnnQuery's half-precision row prefilter (tests/row_prefilter.py restates the kernel's
arithmetic).  A row is turned away on its shadow distance D_h only when lb(D_h) > farthest, so everything rests on
lb <= D_x, the f32 distance the oracle computes (AVX lane order, the kernels' order) -- checked here on the rows where the bound is
loose (uniform), where E vanishes (rows that are binary16 values), where halves go subnormal or large (scaled rows) and where it is
tight (every element's rounding pushes the distance the same way).  The tight rows also show that nothing in the bound is slack
that could be dropped: with E halved, or with the rounding allowance g set to 0, rows of that kind break it."""
import numpy as np
import pytest

import oracle
import row_prefilter as rp
from common import uniform

DIMS = [1, 7, 8, 24, 100, 128, 136, 768]
N = 400


def _dists(rows, q):
    """D_x and D_h of every row against ONE query."""
    ids = np.arange(rows.shape[0], dtype=np.int32)
    return (oracle.dist_query_rows("sq_euclid", rows, q, ids, use_avx=True),
            oracle.dist_query_rows("sq_euclid", rp.h(rows), q, ids, use_avx=True))


def _dists_paired(rows, qs):
    """D_x and D_h of row i against query i."""
    one = np.zeros(1, dtype=np.int32)
    hx = rp.h(rows)
    dx = np.array([oracle.dist_query_rows("sq_euclid", rows[i:i + 1], qs[i], one, use_avx=True)[0] for i in range(rows.shape[0])], dtype=np.float32)
    dh = np.array([oracle.dist_query_rows("sq_euclid", hx[i:i + 1], qs[i], one, use_avx=True)[0] for i in range(rows.shape[0])], dtype=np.float32)
    return dx, dh


def _check(dx, dh, rows, dim):
    """lb <= D_x under the index-wide E and under the per-row bound; and the kernel's threshold form decides no more than lb does."""
    per_row, e = rp.row_bounds(rows), rp.e_of(rows)
    assert (rp.lower_bound(dh, per_row, dim) <= dx.astype(np.float64)).all()
    assert (rp.lower_bound(dh, e, dim) <= dx.astype(np.float64)).all()
    for far in (np.float32(0), np.median(dx).astype(np.float32), dx.min(), dx.max(), np.float32(1e-38)):
        away = rp.turned_away(dh, far, e, dim)
        assert (rp.lower_bound(dh[away], e, dim) > float(far)).all()
        assert (dx[away] > far).all()                                # what the search relies on: the f32 key lies above the farthest


@pytest.mark.parametrize("dim", DIMS)
def test_uniform_rows(dim):
    x, q = uniform(N, dim, 500 + dim), uniform(4, dim, 600 + dim)
    for qi in q:
        _check(*_dists(x, qi), x, dim)
    far = np.float32(np.sort(_dists(x, q[0])[0])[10])
    assert rp.turned_away(_dists(x, q[0])[1], far, rp.e_of(x), dim).sum() > (N // 2 if dim >= 24 else 0)   # and it does turn rows away


@pytest.mark.parametrize("dim", DIMS)
def test_rows_that_are_half_values(dim):
    x, q = rp.representable_rows(N, dim, 700 + dim), uniform(2, dim, 800 + dim)
    assert rp.e_of(x) <= np.float32(2e-37)
    for qi in q:
        dx, dh = _dists(x, qi)
        assert dx.tobytes() == dh.tobytes()
        _check(dx, dh, x, dim)


@pytest.mark.parametrize("scale", [1e3, 1e-3, 1e-6])
@pytest.mark.parametrize("dim", DIMS)
def test_scaled_rows(dim, scale):
    """1e3: halves near the top of their range; 1e-3 / 1e-6: elements below 6.1e-5 round to SUBNORMAL halves (absolute, not relative error)."""
    x = (uniform(N, dim, 900 + dim) * np.float32(scale)).astype(np.float32)
    q = (uniform(2, dim, 1000 + dim) * np.float32(scale)).astype(np.float32)
    for qi in q:
        _check(*_dists(x, qi), x, dim)


@pytest.mark.parametrize("stretch", [1.5, 5.0, 200.0, 5000.0])
@pytest.mark.parametrize("dim", DIMS)
def test_worst_case_rows(dim, stretch):
    x, qs = rp.worst_case(N, dim, 1100 + dim, stretch)
    dx, dh = _dists_paired(x, qs)
    per_row = rp.row_bounds(x)
    assert (rp.lower_bound(dh, per_row, dim) <= dx.astype(np.float64)).all()
    assert (rp.lower_bound(dh, rp.e_of(x), dim) <= dx.astype(np.float64)).all()


def test_the_bound_has_no_slack_to_drop():
    """On the tight rows: half of E breaks the bound (near the segment's end, where E matters), and so does g = 0 (far out, where the
    roundings of the two sums are larger than E's own 2^-20)."""
    dim = 128
    x, qs = rp.worst_case(N, dim, 1100 + dim, 5.0)
    dx, dh = _dists_paired(x, qs)
    assert (rp.lower_bound(dh, rp.row_bounds(x) * np.float32(0.5), dim) > dx.astype(np.float64)).any()
    broken = 0
    for d in (128, 768):
        x, qs = rp.worst_case(N, d, 1100 + d, 5000.0)
        dx, dh = _dists_paired(x, qs)
        broken += int((rp.lower_bound(dh, rp.row_bounds(x), d, g=0.0) > dx.astype(np.float64)).sum())
        assert (rp.lower_bound(dh, rp.row_bounds(x), d) <= dx.astype(np.float64)).all()
    assert broken > 0


@pytest.mark.parametrize("bad", [1e5, np.nan, -np.inf])
def test_a_row_that_does_not_fit_a_half_is_never_turned_away(bad):
    dim = 24
    x, q = uniform(50, dim, 5), uniform(1, dim, 6)[0]
    x[7, 3] = bad
    assert np.isinf(rp.e_of(x))
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dh = _dists(x, q)
    for far in (np.float32(0), np.float32(1e-3), np.float32(3e38)):
        assert not rp.turned_away(dh, far, rp.e_of(x), dim).any()
    assert (rp.lower_bound(dh, rp.e_of(x), dim) == 0).all()
    # ... and a NaN shadow distance is kept under any finite E
    assert not rp.turned_away(np.float32(np.nan), np.float32(1.0), np.float32(0.01), dim)
