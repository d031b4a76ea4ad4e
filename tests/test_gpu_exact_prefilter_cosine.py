"""GPU tier: the cosine family's flat scan behind its f16 MFMA tile (exact_scan_ip_pf_kernel, csrc/dk_exact_mfma_ip.h),
forced with exact_prefilter=2: ids and distance BYTES are the model's (tests/exact_knn_model.py) and the plain kernel's
(exact_prefilter=0), the pairs are counted once, and the tile's own counters say what it judged and what it sent on to be measured."""
import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_knn_model import boundary_tie, exact_knn, stored

pytestmark = pytest.mark.gpu

METRICS = ["cosine", "ucosine", "ucosine_f16"]
NQ = 33                                   # one past an MFMA tile of 32 queries
# two chunks and a ragged last step; the first dim past 256, one short chunk; the 8-wave form, 5 steps of 256 and 131 rows; the LDS ceiling
ROWS = {64: 3000, 288: 300, 768: 1411, 1024: 520}


def max_k(dim, lds=160 * 1024, waves=8):
    """exact_ip_pf_max_k (csrc/dk_exact_mfma_ip.h) at the 8 waves the largest k of a row length runs with, 160 KB of LDS."""
    fixed = 128 * (dim + 8) + 64 * 8 + 3 * 64 * 4 + 64 * 8 + 2 * 32 * waves * 4 + 32 * waves * 8 + 2 * 64 * waves * 4 + waves * 32 * 8 + waves * 4 + 16
    return (lds - fixed) // 512


def _same(got, want):
    return (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()


def _same_as_model(got, want):
    """_same, but a NaN is a NaN: cosine's inf / inf has the host's sign bit in the model and the device's in both kernels."""
    nan = np.isnan(want[1])
    return (got[0] == want[0]).all() and (np.isnan(got[1]) == nan).all() and got[1][~nan].tobytes() == want[1][~nan].tobytes()


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
    assert _same_as_model(got, want) and _same(got, plain), what
    evals = st1["exact_evals"] - st0["exact_evals"]
    assert evals == pairs and pf1["launches"] - pf0["launches"] >= 1 and pf1["pairs_on_tile"] - pf0["pairs_on_tile"] == evals, (what, st1, pf1)
    return pf1["pairs_remeasured"] - pf0["pairs_remeasured"], evals, got


def _unit_for(metric, v):
    return v if metric == "cosine" else normalize_f32(v)


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("dim", sorted(ROWS))
@pytest.mark.parametrize("metric", METRICS)
def test_small_shapes_give_the_models_bytes(monkeypatch, metric, dim, grid):
    n, kmax = ROWS[dim], max_k(dim)
    if grid:   # rows that are exact halves, every row twice: equal distances at every odd rank
        rng = np.random.default_rng(dim)
        x, q = rng.integers(1, 4, (n, dim)).astype(np.float32), rng.integers(1, 4, (NQ, dim)).astype(np.float32)
        x[n // 2:] = x[:n - n // 2]
        assert any(boundary_tie(metric, x, q[:9], k) for k in (1, 10, kmax)), (metric, dim)
    else:
        x, q = _unit_for(metric, uniform(n, dim, dim + 1)), _unit_for(metric, uniform(NQ, dim, dim + 2))
    db = _backend(metric, x)
    for k in (1, 10, kmax):
        got = _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, k), NQ * n, (metric, dim, grid, k))[2]
        if not grid:   # against 1 - cos in float64 from the stored rows, within BASELINE.md's 1e-5
            rows, ids = stored(metric, x)[1].astype(np.float64), got[0]
            ok = ids >= 0
            r, qq = rows[np.where(ok, ids, 0)], q.astype(np.float64)[:, None, :]
            s = (r * qq).sum(-1)
            if metric == "cosine":
                s = s / (np.linalg.norm(r, axis=-1) * np.linalg.norm(qq, axis=-1))
            assert np.abs(got[1].astype(np.float64) - (1.0 - s))[ok].max() <= 1e-5, (metric, dim, k)
    # no list ever fills in chunks of 48 rows: every pair survives every step
    k = min(kmax, 65)
    rem, evals, _ = _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, k), NQ * n,
                           (metric, dim, grid, "chunk 48"), chunk=48)
    assert rem == evals


@pytest.mark.parametrize("metric", METRICS)
def test_values_off_the_tile(monkeypatch, metric):
    n = 80
    x, q = _unit_for(metric, uniform(n, 64, 41)).copy(), _unit_for(metric, uniform(NQ, 64, 42)).copy()
    x[5, 3] = q[2, 7] = 70000.0
    x[7, 60] = np.inf
    x[9, 0] = np.nan
    if metric == "cosine":
        x[11] = 0.0                       # denom = 0
        x[13] *= np.float32(1e-20)        # denom < 1e-30: distance 1 exactly
    if metric == "ucosine":
        x[15:18] *= np.float32(3.0)       # negative distances in the answer
    db = _backend(metric, x)
    for k in (10, n):   # k = n: the inf row and the NaN row are in every answer
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            want = exact_knn(metric, x, q, k)
        _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, want, NQ * n, (metric, k))
    if metric == "ucosine":
        assert (want[1][:, 0] < 0).all()


@pytest.mark.parametrize("metric", METRICS)
def test_nearly_parallel_rows_measure_every_pair(monkeypatch, metric):
    """Rows and queries unit(v + 1e-4 noise) for one v: every distance (about 1e-8 dim) is far below what rounding the operands to
    halves moves the dot product by (about 2^-11) -- a tile without e_x or e_q answers wrongly, this one turns nothing away.
    (On f16 records the premise does not hold -- storing the rows has rounded them, the stored rows' distances are spread by that
    rounding (a sigma of 3.5e-5) and e_x is 0, so the margin, |a| e_q = 2.8e-4, is a few sigma and a few pairs in 66 000 lie
    beyond it: there the answer's bytes are the check, and that nearly every pair is measured.)"""
    rng = np.random.default_rng(51)
    v = rng.random(64, dtype=np.float32)
    x = normalize_f32(v + np.float32(1e-4) * rng.standard_normal((2000, 64)).astype(np.float32))
    q = normalize_f32(v + np.float32(1e-4) * rng.standard_normal((NQ, 64)).astype(np.float32))
    db = _backend(metric, x)
    rem, evals, _ = _check(monkeypatch, lambda: db.exact_knn(q, 10), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, 10), NQ * 2000, metric)
    assert rem == evals if metric != "ucosine_f16" else rem > 0.99 * evals, (rem, evals)


@pytest.mark.parametrize("metric", METRICS)
def test_the_tile_turns_pairs_away_and_the_default_has_floors(monkeypatch, metric):
    x, q = normalize_f32(uniform(4096, 64, 61)), normalize_f32(uniform(32, 64, 62))
    db = _backend(metric, x)
    rem, evals, _ = _check(monkeypatch, lambda: db.exact_knn(q, 10), db.stats, db.exact_prefilter_stats, exact_knn(metric, x, q, 10), 32 * 4096, metric)
    assert 0 < rem < evals, (rem, evals)
    set_diag(monkeypatch, exact_prefilter=1)      # the default: 32 queries and 4 096 rows are below its floors (256, 65 536)
    before = db.exact_prefilter_stats()
    db.exact_knn(q, 10)
    assert db.exact_prefilter_stats() == before


def test_allow_sets_and_removals_through_the_index(monkeypatch):
    import hnswindex
    metric, n, dim = "ucosine", 1500, 64
    x, q = normalize_f32(uniform(n, dim, 31)), normalize_f32(uniform(NQ, dim, 32))
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
