"""GPU tier: the fixed-radius triangle scans behind the f16 MFMA tile (exact_tri_pf_kernel, csrc/dk_exact_tri.h),
forced with exact_prefilter=2: labels, counts and info are byte for byte the plain kernel's (exact_prefilter=0) and the contract
models' (tests/near_dup_model.py, tests/density_model.py) on float64 distances of the stored values, the pairs are counted once, and the
tile's own counters say what it judged and what it sent on to be measured.  exact_chunk=192 and exact_union_round=150 put blocks above,
on and below the diagonal, partial query tiles (64 + 64 + 22), ragged row steps and several launches into every call."""
import numpy as np
import pytest

from common import set_diag, uniform
from density_model import counts_only_info, density_clusters
from near_dup_model import duplicate_groups

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "sq_euclid_f16"]
DIMS = [64, 96, 256]
N = 1200
KNOBS = dict(exact_chunk=192, exact_union_round=150)
_cache = {}


def _members(seed=7):
    mask = np.random.default_rng(seed).random(N) < 0.84
    mask[[5, 7, 9]] = True                                 # the rows of _odd that do not fit a half
    m = int(mask.sum())
    assert m % 64 and m % 128 and m < N                    # no whole tiles or steps, and the ids are not the identity
    return mask


def _planted(dim):
    """Uniform rows; 120 of them are near copies of the first 30, so that groups and clusters have several members."""
    rng = np.random.default_rng(dim)
    x = uniform(N, dim, dim + 3).copy()
    dst = 30 + rng.choice(N - 30, 120, replace=False)
    x[dst] = x[rng.integers(0, 30, 120)] + rng.uniform(-0.01, 0.01, (120, dim)).astype(np.float32)
    return x


def _grid(dim):
    return np.random.default_rng(dim + 1).integers(1, 4, (N, dim)).astype(np.float32)


def _odd(dim):
    x = _planted(dim)
    x[5, 3] = 70000.0
    x[7, dim - 4] = np.inf
    x[9, 0] = np.nan
    return x


def _cancel(dim):
    return (100.0 + 0.1 * np.random.default_rng(dim + 2).standard_normal((N, dim))).astype(np.float32)


def _case(make, metric, dim):
    """(backend, float64 distances [a, b] of the stored values with a's row as the query), made once per data set and shared."""
    key = (make.__name__, metric, dim)
    if key not in _cache:
        import hnswindex
        x = make(dim)
        db = hnswindex.DeviceBackend(dim, metric, capacity=N)
        db.upload_rows(0, x)
        with np.errstate(all="ignore"):
            s = (x.astype(np.float16) if metric.endswith("_f16") else x).astype(np.float64)
            _cache[key] = db, np.stack([((s - r) ** 2).sum(1) for r in s])
    return _cache[key]


def _dist_to(d64):
    def dist_to(own, cand):
        with np.errstate(over="ignore"):
            return d64[own, cand].astype(np.float32)
    return dist_to


def _same(got, want):
    return len(got) == len(want) and all(a == b if a is None or isinstance(a, dict) else a.tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))


def _check(monkeypatch, stats, call, want, what):
    """One call under exact_prefilter=2 and the same call under 0: the model's bytes both times, every counted pair on the tile."""
    set_diag(monkeypatch, exact_prefilter=2, **KNOBS)
    s0 = stats()
    got = call()
    s1 = stats()
    set_diag(monkeypatch, exact_prefilter=0, **KNOBS)
    plain = call()
    assert stats() == s1, what                                          # 0: the form is never taken
    assert _same(got, plain), (what, got[-1], plain[-1])
    assert want is None or _same(got, want), (what, got[-1], want[-1])
    on_tile = s1["pairs_on_tile"] - s0["pairs_on_tile"]
    assert s1["launches"] - s0["launches"] >= 1 and on_tile == got[-1]["pairs_measured"] and s1["reserved"] == 0, (what, s0, s1, got[-1])
    return s1["pairs_remeasured"] - s0["pairs_remeasured"], on_tile


def _groups(monkeypatch, make, metric, dim, radius, model=True):
    db, d64 = _case(make, metric, dim)
    mask = _members()
    want = duplicate_groups(_dist_to(d64), N, np.arange(N), radius, allowed=mask) if model else None
    rem, on_tile = _check(monkeypatch, db.triangle_prefilter_stats, lambda: db.exact_range_groups(radius, N, allowed=mask), want, (metric, dim, radius))
    m = int(mask.sum())
    assert on_tile == m * (m - 1) // 2
    return rem, on_tile, want


def _gap(d64, radius):
    """No pair within a relative 1e-4 of the radius: far above the f32 summation error, so float64 decides every pair."""
    with np.errstate(invalid="ignore"):
        return not (np.abs(d64 - radius) <= 1e-4 * radius).any()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_planted_near_duplicates(monkeypatch, metric, dim):
    assert _gap(_case(_planted, metric, dim)[1], 0.5)
    rem, on_tile, want = _groups(monkeypatch, _planted, metric, dim, 0.5)
    assert 0 < want[1]["pairs_within"] <= rem < on_tile, (rem, on_tile, want[1])


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_ties_at_the_radius_are_within(monkeypatch, metric, dim):
    """Entries in {1, 2, 3}: every distance is an exact integer in every precision, and the radius is one that pairs attain."""
    d64 = _case(_grid, metric, dim)[1]
    radius = float(np.sort(d64[np.triu_indices(N, 1)])[200])
    assert radius == int(radius) and (d64 == radius).sum() >= 2
    _, _, want = _groups(monkeypatch, _grid, metric, dim, radius)
    assert want[1]["pairs_within"] > 0


@pytest.mark.parametrize("metric", METRICS)
def test_values_that_do_not_fit_a_half(monkeypatch, metric):
    """70 000, inf and NaN in three rows: their pairs are never turned away, a NaN distance admits nothing."""
    d64 = _case(_odd, metric, 64)[1]
    assert _gap(d64, 0.5)
    rem, _, _ = _groups(monkeypatch, _odd, metric, 64, 0.5)
    m = int(_members().sum())
    assert rem >= 3 * (m - 3)


@pytest.mark.parametrize("metric", METRICS)
def test_cancellation_measures_every_pair(monkeypatch, metric):
    """Rows 100 + 0.1 noise: eps N~ exceeds every distance -- nothing can be turned away, and nothing is.  (The plain kernel is the
    reference here: the distances crowd around the radius.)"""
    rem, on_tile, _ = _groups(monkeypatch, _cancel, metric, 64, 1.3, model=False)
    assert rem == on_tile


@pytest.mark.parametrize("radius", [np.inf, np.nan, -1.0])
@pytest.mark.parametrize("metric", METRICS)
def test_radii_that_are_no_positive_number(monkeypatch, metric, radius):
    _, _, want = _groups(monkeypatch, _planted, metric, 64, radius)
    m = int(_members().sum())
    assert want[1]["pairs_within"] == (m * (m - 1) // 2 if radius == np.inf else 0)


@pytest.mark.parametrize("form", ["counts", "arena", "join"])
@pytest.mark.parametrize("min_samples", [1, 3])
@pytest.mark.parametrize("metric", METRICS)
def test_density(monkeypatch, metric, min_samples, form):
    """The three ways through exact_range_density: counts alone, phase B from the arena, phase B as a second scan (density_pair_cap=1)."""
    db, d64 = _case(_planted, metric, 96)
    mask = _members()
    scans = 2 if form == "join" else 1
    labels, counts, info = density_clusters(_dist_to(d64), N, np.arange(N), 0.5, min_samples, allowed=mask, scans=scans)
    want = (None, counts, counts_only_info(info)) if form == "counts" else (labels, counts, info)
    set_diag(monkeypatch, density_pair_cap=1 if form == "join" else 0)
    _check(monkeypatch, db.triangle_prefilter_stats, lambda: db.exact_range_density(0.5, min_samples, N, allowed=mask, labels=form != "counts"), want,
           (metric, min_samples, form))
    assert info["scans"] == scans and info["pairs_within"] > 1


@pytest.mark.parametrize("metric", METRICS)
def test_the_picker_leaves_small_calls_alone(monkeypatch, metric):
    db, _ = _case(_planted, metric, 64)
    set_diag(monkeypatch, exact_prefilter=1)      # the default: a thousand members are below the picker's floors
    before = db.triangle_prefilter_stats()
    db.exact_range_groups(0.5, N)
    db.exact_range_density(0.5, 3, N)
    assert db.triangle_prefilter_stats() == before


@pytest.mark.parametrize("metric", METRICS)
def test_removals_and_an_allow_set_through_the_index(monkeypatch, metric):
    import hnswindex
    x = _planted(64)
    ix = hnswindex.Index(64, metric)
    ix.set_collection_size(2048); ix.set_min_nn(20)
    ix.add(x)
    rng = np.random.default_rng(33)
    ix.remove(np.unique(np.concatenate([[ix.entry_point], rng.choice(N, 99, replace=False)])).astype(np.int32))
    mask = rng.random(N) < 0.9
    _check(monkeypatch, ix.triangle_prefilter_stats, lambda: ix.duplicate_groups(0.5, allowed=mask), None, metric)
