"""GPU tier: the Boruvka scans of the two spanning trees behind the f16 MFMA tile (span_pf_kernel, csrc/dk_span_tree_pf.h; DESIGN.md
3.37), forced with exact_prefilter=2: edges, weights, core and info are byte for byte the plain kernels' (exact_prefilter=0) and, where
every distance is an exact integer, the float64 reference's (core, max, Kruskal in (w, a, b) order).  exact_chunk=192 and
span_round=150 put blocks above, on and below the diagonal, partial query tiles (64 + 64 + 22), ragged row steps and several launches
into every round."""
import numpy as np
import pytest

from common import set_diag, uniform
from density_rows import numpy_dist
from test_gpu_mreach_tree import want
from test_gpu_span_tree import _ruler, kruskal

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "sq_euclid_f16"]
DIMS = [64, 96, 256]
TREES = [("span", 0), ("mreach", 1), ("mreach", 2), ("mreach", 6)]
N = 1200
KNOBS = dict(exact_chunk=192, span_round=150)
_cache = {}


def _members():
    mask = np.random.default_rng(7).random(N) < 0.84
    mask[[5, 7, 9, 100, 500, 900]] = True                  # the rows of _odd that do not fit a half; the row under three ids
    mask[690:710] = True                                   # the block of equal rows
    m = int(mask.sum())
    assert m % 64 and m % 128 and m < N                    # no whole tiles or steps, and the ids are not the identity
    return mask


def _grid(dim):
    """Coordinates 0 / 1 / 2: every distance is an integer, exact in f16, f32 and f64, and thousands of pairs share each."""
    x = np.random.default_rng(dim + 1).integers(0, 3, (N, dim)).astype(np.float32)
    x[500] = x[900] = x[100]
    x[690:710] = x[690]
    return x


def _planted(dim):
    """Uniform rows; 120 of them are near copies of the first 30."""
    rng = np.random.default_rng(dim)
    x = uniform(N, dim, dim + 3).copy()
    dst = 30 + rng.choice(N - 30, 120, replace=False)
    x[dst] = x[rng.integers(0, 30, 120)] + rng.uniform(-0.01, 0.01, (120, dim)).astype(np.float32)
    return x


def _odd(dim):
    x = _planted(dim)
    x[5, 3] = 70000.0
    x[7, dim - 4] = np.inf
    x[9, 0] = np.nan
    return x


def _cancel(dim):
    return (100.0 + 0.1 * np.random.default_rng(dim + 2).standard_normal((N, dim))).astype(np.float32)


def _backend(make, metric, dim):
    key = (make.__name__, metric, dim)
    if key not in _cache:
        import hnswindex
        x = make(dim)
        db = hnswindex.DeviceBackend(dim, metric, capacity=N)
        db.upload_rows(0, x)
        _cache[key] = db, x
    return _cache[key]


def _tree(obj, tree, s, allowed, n=None):
    if hasattr(obj, "exact_span_tree"):
        return obj.exact_span_tree(n or N, allowed=allowed) if tree == "span" else obj.exact_mreach_tree(n or N, s, allowed=allowed)
    return obj.single_linkage_tree(allowed=allowed) if tree == "span" else obj.mutual_reachability_tree(s, allowed=allowed)


def _both(monkeypatch, obj, call, what, knobs=KNOBS):
    """One call under exact_prefilter=2 and the same call under 0: equal bytes and info; (result, the getter's movement under 2)."""
    set_diag(monkeypatch, exact_prefilter=2, **knobs)
    s0 = obj.span_prefilter_stats()
    got = call()
    s1 = obj.span_prefilter_stats()
    set_diag(monkeypatch, exact_prefilter=0, **knobs)
    plain = call()
    assert obj.span_prefilter_stats() == s1, what                       # 0: the form is never taken
    assert all(g.tobytes() == p.tobytes() for g, p in zip(got[:-1], plain[:-1])) and got[-1] == plain[-1], (what, got[-1], plain[-1])
    return got, {k: s1[k] - s0[k] for k in s1}


@pytest.mark.parametrize("tree,s", TREES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_integer_rows_against_float64(monkeypatch, metric, dim, tree, s):
    """The tie cases: weights equal to the bound must be measured, and the (a, b) order decides."""
    db, x = _backend(_grid, metric, dim)
    mask = _members()
    members, w = np.flatnonzero(mask), numpy_dist(metric, x)
    got, moved = _both(monkeypatch, db, lambda: _tree(db, tree, s, mask), (metric, dim, tree, s))
    ref = kruskal(w, members) if tree == "span" else want(w, members, s)
    assert all(g.tobytes() == r.tobytes() for g, r in zip(got[:-1], ref)), (metric, dim, tree, s)
    info = got[-1]
    assert info["edges"] == members.size - 1 and moved["launches"] == info["launches"] and moved["pairs_on_tile"] == info["pairs_measured"], (info, moved)
    assert info["pairs_measured"] + info["pairs_skipped"] == info["rounds"] * (members.size * (members.size - 1) // 2), info


@pytest.mark.parametrize("tree,s", TREES)
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_planted_near_duplicates_turn_pairs_away(monkeypatch, metric, dim, tree, s):
    db, _ = _backend(_planted, metric, dim)
    mask = _members()
    got, moved = _both(monkeypatch, db, lambda: _tree(db, tree, s, mask), (metric, dim, tree, s))
    assert moved["launches"] > 0 and 0 < moved["pairs_remeasured"] < moved["pairs_on_tile"] == got[-1]["pairs_measured"] and moved["reserved"] == 0, moved


@pytest.mark.parametrize("tree,s", TREES)
@pytest.mark.parametrize("metric", METRICS)
def test_values_that_do_not_fit_a_half(monkeypatch, metric, tree, s):
    """70 000, +inf and NaN in three rows: e = +inf keeps their pairs, a NaN distance is no edge."""
    db, _ = _backend(_odd, metric, 64)
    got, _ = _both(monkeypatch, db, lambda: _tree(db, tree, s, _members()), (metric, tree, s))
    assert 9 not in got[0].tolist() + got[1].tolist() and got[-1]["components"] >= 2


@pytest.mark.parametrize("tree,s", TREES)
@pytest.mark.parametrize("metric", METRICS)
def test_cancellation_keeps_the_bytes(monkeypatch, metric, tree, s):
    """Rows 100 + 0.1 noise: eps N~ exceeds every distance, so the tile may turn nothing away -- that is legal; the share it sent on
    is reported, not pinned."""
    db, _ = _backend(_cancel, metric, 64)
    got, moved = _both(monkeypatch, db, lambda: _tree(db, tree, s, _members()), (metric, tree, s))
    assert moved["pairs_remeasured"] <= moved["pairs_on_tile"] == got[-1]["pairs_measured"], \
        f"remeasured / on_tile = {moved['pairs_remeasured']} / {moved['pairs_on_tile']}"


@pytest.mark.parametrize("tree,s", [("span", 0), ("mreach", 3)])
def test_one_component_after_the_first_round_and_the_segment_skip(monkeypatch, tree, s):
    """Ids [0, 384) on a line with unit gaps -- one component after round 1, three whole segments the later rounds do not read --
    beside 128 rows on a ruler line that take seven rounds; then 20 equal rows alone: one round."""
    import hnswindex
    n, blob = 512, 384
    y = np.zeros((n, 64), np.float32)
    y[:blob, 0] = np.arange(blob)
    y[blob:, 0] = 1000 + _ruler(n - blob, 2)                               # integers below 2048: exact as halves, squares exact in f32
    db = hnswindex.DeviceBackend(64, "sq_euclid", capacity=n)
    db.upload_rows(0, y)
    got, moved = _both(monkeypatch, db, lambda: _tree(db, tree, s, None, n), (tree, s))
    ref = kruskal(numpy_dist("sq_euclid", y), np.arange(n)) if tree == "span" else want(numpy_dist("sq_euclid", y), np.arange(n), s)
    assert all(g.tobytes() == r.tobytes() for g, r in zip(got[:-1], ref))
    info = got[-1]
    assert info["rounds"] >= 3 and info["pairs_skipped"] >= (info["rounds"] - 1) * (blob * (blob - 1) // 2) and moved["launches"] == info["launches"], info
    db, _ = _backend(_grid, "sq_euclid", 64)
    got, _ = _both(monkeypatch, db, lambda: _tree(db, tree, s, np.arange(690, 710)), (tree, s, "equal rows"))
    assert got[-1]["rounds"] == 1 and got[-1]["edges"] == 19 and not got[2].any()


@pytest.mark.parametrize("tree,s", [("span", 0), ("mreach", 4)])
@pytest.mark.parametrize("metric", METRICS)
def test_removed_ids_and_two_members_through_the_index(monkeypatch, metric, tree, s):
    import hnswindex
    x = _grid(64)
    ix = hnswindex.Index(64, metric)
    ix.set_collection_size(2048); ix.set_min_nn(20); ix.set_allow_removals(True)
    ix.add(x)
    rng = np.random.default_rng(33)
    gone = np.unique(np.concatenate([[ix.entry_point], rng.choice(N, 99, replace=False)])).astype(np.int32)
    ix.remove(gone)
    mask = rng.random(N) < 0.9
    members, w = np.setdiff1d(np.flatnonzero(mask), gone), numpy_dist(metric, x)
    got, moved = _both(monkeypatch, ix, lambda: _tree(ix, tree, s, mask), (metric, tree, s))
    ref = kruskal(w, members) if tree == "span" else want(w, members, s)
    assert all(g.tobytes() == r.tobytes() for g, r in zip(got[:-1], ref)) and moved["launches"] == got[-1]["launches"] > 0
    two = np.setdiff1d(np.arange(N), gone)[[3, 700]]
    got, moved = _both(monkeypatch, ix, lambda: _tree(ix, tree, s, two), (metric, tree, s, "two members"))
    assert (got[0].tolist(), got[1].tolist()) == ([two[0]], [two[1]]) and moved["launches"] == got[-1]["launches"] == 1


@pytest.mark.parametrize("tree,s", [("span", 0), ("mreach", 5)])
def test_the_picker(monkeypatch, tree, s):
    db, _ = _backend(_planted, "sq_euclid", 64)
    set_diag(monkeypatch, exact_prefilter=1)              # the default: a thousand members are below the picker's floor
    before = db.span_prefilter_stats()
    _tree(db, tree, s, None)
    assert db.span_prefilter_stats() == before
    import hnswindex
    cos = hnswindex.DeviceBackend(64, "cosine", capacity=N)   # no kernel of this form is built for the metric: the plain one runs
    cos.upload_rows(0, _planted(64))
    got, moved = _both(monkeypatch, cos, lambda: _tree(cos, tree, s, _members()), ("cosine", tree, s))
    assert not any(moved.values()) and got[-1]["edges"] == int(_members().sum()) - 1
