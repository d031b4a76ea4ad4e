"""GPU tier: the flat scan of the int8 rows with its dot product on the i8 MFMA tile (exact_scan_i8_mfma_kernel, csrc/dk_exact_mfma_i8.h;
DESIGN.md 3.39), forced with exact_prefilter=2: ids and distance BYTES are the model's (tests/exact_knn_model.py) and the plain
kernel's (exact_prefilter=0), the pairs are counted once, and the form's counters say what was on the tile and what went to the drain."""
import numpy as np
import pytest

from common import set_diag, uniform
from exact_knn_model import boundary_tie, exact_knn

pytestmark = pytest.mark.gpu

METRIC = "sq_euclid_i8"
# dim -> (rows, queries, ks): record pitches 16, 32, 48 and 144 words.  3 000 rows: several chunks with a ragged last step; 300: one
# short chunk; 1 411: 11 steps and 3 rows; 33 queries: one past an MFMA half-tile; 65: a second tile.  At pitch 144 64 KB hold k <= 40.
SHAPES = {5: (3000, 33, (1, 10, 65)), 96: (300, 33, (1, 10, 65)), 128: (1411, 65, (1, 10, 65)), 520: (300, 33, (1, 10))}


def _same(got, want, nan_is_nan=False):
    if nan_is_nan:   # every NaN is one value
        return (got[0] == want[0]).all() and np.array_equal(got[1], want[1], equal_nan=True)
    return (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()


def _backend(x):
    import hnswindex
    db = hnswindex.DeviceBackend(x.shape[1], METRIC, capacity=x.shape[0])
    db.upload_rows(0, x)
    return db


def _check(monkeypatch, call, stats, pf_stats, want, pairs, what, chunk=0, nan_is_nan=False):
    """One call under exact_prefilter=2 and the same call under 0: the model's bytes both times, pairs counted once, all on the tile."""
    set_diag(monkeypatch, exact_prefilter=2, exact_chunk=chunk)
    st0, pf0 = stats(), pf_stats()
    got = call()
    st1, pf1 = stats(), pf_stats()
    set_diag(monkeypatch, exact_prefilter=0, exact_chunk=chunk)
    plain = call()
    assert pf_stats() == pf1, what                                      # 0: the form is never taken
    assert _same(got, want, nan_is_nan) and _same(got, plain), what
    evals = st1["exact_evals"] - st0["exact_evals"]
    assert evals == pairs and pf1["launches"] - pf0["launches"] >= 1 and pf1["pairs_on_tile"] - pf0["pairs_on_tile"] == evals, (what, st1, pf1)
    assert pf1["reserved"] == 0
    return pf1["pairs_remeasured"] - pf0["pairs_remeasured"], evals


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_small_shapes_give_the_models_bytes(monkeypatch, dim, grid):
    n, nq, ks = SHAPES[dim]
    if grid:   # elements -1, 0, 1: every quantised element is -127, 0 or 127, equal distances everywhere
        rng = np.random.default_rng(dim)
        x, q = rng.integers(-1, 2, (n, dim)).astype(np.float32), rng.integers(-1, 2, (nq, dim)).astype(np.float32)
        assert any(boundary_tie(METRIC, x, q[:9], k) for k in ks), dim
    else:
        x, q = uniform(n, dim, dim + 1), uniform(nq, dim, dim + 2)
    db = _backend(x)
    for k in ks:
        _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, exact_knn(METRIC, x, q, k), nq * n, (dim, grid, k))
    if 65 in ks:   # k above the rows of a chunk: no list ever fills, every pair goes to the drain
        rem, evals = _check(monkeypatch, lambda: db.exact_knn(q, 65), db.stats, db.exact_prefilter_stats, exact_knn(METRIC, x, q, 65), nq * n,
                            (dim, grid, "chunk 48"), chunk=48)
        assert rem == evals


@pytest.mark.parametrize("distinct", [1, 4])
def test_few_distinct_rows_do_not_survive_wholesale(monkeypatch, distinct):
    """Equal distances everywhere: a bound alone turns nothing away, the key compare in the lane does."""
    n, dim = 4096, 96
    x, q = uniform(distinct, dim, 71)[np.arange(n) % distinct], uniform(33, dim, 72)
    db = _backend(x)
    rem, evals = _check(monkeypatch, lambda: db.exact_knn(q, 10), db.stats, db.exact_prefilter_stats, exact_knn(METRIC, x, q, 10), 33 * n, distinct)
    assert 0 < rem < evals, (rem, evals)


def test_rows_that_break_the_quantiser(monkeypatch):
    n = 80
    x, q = uniform(n, 96, 41).copy(), uniform(33, 96, 42).copy()
    x[7, 60] = np.inf
    x[9, 0] = np.nan
    x[11] = 0.0      # scale 0
    q[3] = 0.0
    db = _backend(x)
    for k in (10, n):   # k = n: the inf row and the NaN row are in every answer
        with np.errstate(all="ignore"):
            want = exact_knn(METRIC, x, q, k)
        _check(monkeypatch, lambda: db.exact_knn(q, k), db.stats, db.exact_prefilter_stats, want, 33 * n, k, nan_is_nan=True)


def test_allow_sets_and_removals_through_the_index(monkeypatch):
    import hnswindex
    n, dim = 1500, 96
    x, q = uniform(n, dim, 31), uniform(33, dim, 32)
    ix = hnswindex.Index(dim, METRIC)
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
               exact_knn(METRIC, x, q, 10, mask=mask, live=live), 33 * m, sel)


def test_the_tile_turns_pairs_away_and_the_picker_has_floors(monkeypatch):
    x, q = uniform(4096, 96, 61), uniform(32, 96, 62)
    db = _backend(x)
    rem, evals = _check(monkeypatch, lambda: db.exact_knn(q, 10), db.stats, db.exact_prefilter_stats, exact_knn(METRIC, x, q, 10), 32 * 4096, "uniform")
    assert 0 < rem < evals, (rem, evals)
    set_diag(monkeypatch, exact_prefilter=1)      # the default: 32 queries and 4 096 rows are below the picker's floors (256, 65 536)
    before = db.exact_prefilter_stats()
    db.exact_knn(q, 10)
    assert db.exact_prefilter_stats() == before
