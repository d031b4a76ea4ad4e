"""GPU tier: the flat scan behind its f16 MFMA tile (exact_scan_pf_kernel, csrc/dk_exact_mfma.h), forced with
exact_prefilter=2: ids and distance BYTES are the model's (tests/exact_knn_model.py) and the plain kernel's (exact_prefilter=0), the
pairs are counted once, and the tile's own counters say what it judged and what it sent on to be measured."""
import numpy as np
import pytest

from common import set_diag, uniform
from exact_knn_model import boundary_tie, exact_knn

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "sq_euclid_f16"]
NQ = 33                                   # one past an MFMA tile of 32 queries
ROWS = {64: 3000, 96: 300, 160: 1411}     # two chunks with a ragged last step; one short chunk; 11 steps and 3 rows


def _same(got, want):
    return (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()


def _backend(metric, x):
    import hnswindex
    db = hnswindex.DeviceBackend(x.shape[1], metric, capacity=x.shape[0])
    db.upload_rows(0, x)
    return db


def _check(monkeypatch, call, stats, pf_stats, want, pairs, what, chunk=0):
    """One call under exact_prefilter=2 and the same call under 0: the model's bytes both times, pairs counted once, all on the tile."""
    set_diag(monkeypatch, exact_prefilter=2, exact_chunk=chunk)
    st0, pf0 = stats(), pf_stats()
    got = call()
    st1, pf1 = stats(), pf_stats()
    set_diag(monkeypatch, exact_prefilter=0, exact_chunk=chunk)
    plain = call()
    assert pf_stats() == pf1, what                                      # 0: the form is never taken
    assert _same(got, want) and _same(got, plain), what
    evals = st1["exact_evals"] - st0["exact_evals"]
    assert evals == pairs and pf1["launches"] - pf0["launches"] >= 1 and pf1["pairs_on_tile"] - pf0["pairs_on_tile"] == evals, (what, st1, pf1)
    return pf1["pairs_remeasured"] - pf0["pairs_remeasured"], evals


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("dim", sorted(ROWS))
@pytest.mark.parametrize("metric", METRICS)
def test_small_shapes_give_the_models_bytes(monkeypatch, metric, dim, grid):
    n = ROWS[dim]
    if grid:   # rows that are exact halves, equal distances everywhere
        rng = np.random.default_rng(dim)
        x, q = rng.integers(1, 4, (n, dim)).astype(np.float32), rng.integers(1, 4, (NQ, dim)).astype(np.float32)
        assert any(boundary_tie(metric, x, q[:9], k) for k in (1, 10, 65)), (metric, dim)
    else:
        x, q = uniform(n, dim, dim + 1), uniform(NQ, dim, dim + 2)
    db = _backend(metric, x)
    for k in (1, 10, 65):
        _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, k), NQ * n, (metric, dim, grid, k))
    # k above the rows of a chunk: no list ever fills, every pair survives every step
    rem, evals = _check(monkeypatch, lambda: db.exact_knn(q, 65), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, 65), NQ * n,
                        (metric, dim, grid, "chunk 48"), chunk=48)
    assert rem == evals


@pytest.mark.parametrize("metric", METRICS)
def test_allow_sets_and_removals_through_the_index(monkeypatch, metric):
    import hnswindex
    n, dim = 1500, 64
    x, q = uniform(n, dim, 31), uniform(NQ, dim, 32)
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(2048); ix.set_min_nn(20)
    ix.add(x)
    rng = np.random.default_rng(33)
    ix.remove(np.unique(np.concatenate([[ix.entry_point], rng.choice(n, 99, replace=False)])).astype(np.int32))
    live = np.sort(ix.ids())
    for sel in (None, 0.5, 0.01):
        mask = None if sel is None else rng.random(n) < sel
        m = live.size if mask is None else int(mask[live].sum())
        assert m > 0
        _check(monkeypatch, lambda: ix.exact_knn_query(q, 10, allowed=mask), ix.stats, ix.exact_prefilter_stats,
               exact_knn(metric, x, q, 10, mask=mask, live=live), NQ * m, (metric, sel))


@pytest.mark.parametrize("metric", METRICS)
def test_values_that_do_not_fit_a_half(monkeypatch, metric):
    n = 80
    x, q = uniform(n, 64, 41).copy(), uniform(NQ, 64, 42).copy()
    x[5, 3] = q[2, 7] = 70000.0
    x[7, 60] = np.inf
    x[9, 0] = np.nan
    db = _backend(metric, x)
    for k in (10, n):   # k = n: the inf row and the NaN row are in every answer
        with np.errstate(over="ignore", invalid="ignore"):
            want = exact_knn(metric, x, q, k)
        _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, want, NQ * n, (metric, k))


@pytest.mark.parametrize("metric", METRICS)
def test_cancellation_measures_every_pair(monkeypatch, metric):
    """Rows 100 + 0.1 noise: eps N~ (17) exceeds every distance (1.3), and the half-precision grid at 100 (1/16) is as coarse as the
    noise -- a tile without e or without eps answers wrongly, this one turns nothing away."""
    rng = np.random.default_rng(51)
    x = (100.0 + 0.1 * rng.standard_normal((2000, 64))).astype(np.float32)
    q = (100.0 + 0.1 * rng.standard_normal((NQ, 64))).astype(np.float32)
    db = _backend(metric, x)
    rem, evals = _check(monkeypatch, lambda: db.exact_knn(q, 10), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, 10), NQ * 2000, metric)
    assert rem == evals


@pytest.mark.parametrize("metric", METRICS)
def test_the_tile_turns_pairs_away_and_the_picker_has_floors(monkeypatch, metric):
    x, q = uniform(4096, 64, 61), uniform(32, 64, 62)
    db = _backend(metric, x)
    rem, evals = _check(monkeypatch, lambda: db.exact_knn(q, 10), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, 10), 32 * 4096, metric)
    assert 0 < rem < evals, (rem, evals)
    set_diag(monkeypatch, exact_prefilter=1)      # the default: 32 queries and 4 096 rows are below the picker's floors (256, 65 536)
    before = db.exact_prefilter_stats()
    db.exact_knn(q, 10)
    assert db.exact_prefilter_stats() == before
