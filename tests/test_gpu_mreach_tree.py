"""GPU tier: mutual_reachability_tree -- HDBSCAN*'s tree, the minimum spanning forest of the stored rows under
max(d(a, b), core[a], core[b]) in the strict order (weight, a, b), by Boruvka's rounds of mreach_scan_kernel.  The reference is numpy:
core[v] the (min_samples - 1)-th smallest off-diagonal entry of row v (+inf where there is none or it is NaN, -inf at min_samples 1),
the weights by max, Kruskal in that order (test_gpu_span_tree's); the forest is unique, so every comparison is of bytes.  Distances:
float64 numpy where every one is an exact integer, otherwise the device's own bits from exact_range_query_by_id at +inf, where row v
is what v measures as the query -- what its core distance is defined on."""
import numpy as np
import pytest

from common import set_diag
from density_rows import DIM, METRICS, MIN_SAMPLES, QTILE, links, numpy_dist, radius_between, rows
from test_gpu_span_tree import _device_weights, _index, kruskal

pytestmark = pytest.mark.gpu
N = 600
SMALL = dict(exact_chunk=200, exact_qtile=QTILE, span_round=256)          # three chunks, tiles of 8 members, three launches a round


def want(w, members, s):
    """(a, b, dist, core float32[len(w)]) of the reference; w[v] is row v as the query, the weight of a < b is built on w[a, b]."""
    core = np.full(len(w), np.nan)
    for v in members:
        near = np.sort(w[v, members[members != v]])                        # NaN sorts last
        core[v] = -np.inf if s == 1 else near[s - 2] if s - 2 < near.size and not np.isnan(near[s - 2]) else np.inf
    return kruskal(np.maximum(w, np.maximum.outer(core, core)), members) + (core.astype(np.float32),)


def same(got, ref, what=None):
    assert got[0].dtype == got[1].dtype == np.int32 and got[2].dtype == got[3].dtype == np.float32
    assert all(g.tobytes() == r.tobytes() for g, r in zip(got[:4], ref)), what


def accounted(info, m, s, pieces=None):
    assert info["members"] == m and info["edges"] + info["components"] == m and (info["core_launches"] == 0) == (s == 1 or m < 2), info
    assert info["pairs_measured"] + info["pairs_skipped"] == info["rounds"] * (m * (m - 1) // 2), info
    if pieces:
        assert info["launches"] == info["rounds"] * pieces and info["core_launches"] == (0 if s == 1 else pieces), info


@pytest.fixture(scope="module")
def ties():
    """Coordinates 0 / 1 / 2: every distance is an integer below 81, exact in f16, f32 and f64, and thousands of pairs share each; one
    row under three ids and a run of 20 equal rows, so distance 0 -- and core distance 0 -- occurs under several ids."""
    x = np.random.default_rng(5).integers(0, 3, (N, DIM)).astype(np.float32)
    x[300] = x[580] = x[100]
    x[190:210] = x[190]
    out = {}
    for metric in ("sq_euclid", "sq_euclid_f16"):
        ix = _index(DIM, metric, N)
        ix.add(x)
        out[metric] = ix, numpy_dist(metric, x)
    return out


@pytest.mark.parametrize("knobs", [{}, SMALL], ids=["default", "small"])
@pytest.mark.parametrize("s", [1, 2, 5, 40])
@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_f16"])
def test_ties_against_float64(ties, monkeypatch, metric, s, knobs):
    ix, w = ties[metric]
    if knobs:
        set_diag(monkeypatch, **knobs)
    got = ix.mutual_reachability_tree(s)
    same(got, want(w, np.arange(N), s), (metric, s))
    accounted(got[4], N, s, 3 if knobs else 1)
    assert got[4]["edges"] == N - 1 and (got[0] < got[1]).all()
    if s == 1:
        assert all(g.tobytes() == t.tobytes() for g, t in zip(got[:3], ix.single_linkage_tree()))


@pytest.mark.parametrize("metric", METRICS)
def test_every_row_kind_and_the_density_cuts(metric):
    x = rows(metric)[:N]
    ix = _index(DIM, metric, N)
    ix.add(x)
    a, b, d, core, info = got = ix.mutual_reachability_tree(MIN_SAMPLES)
    same(got, want(_device_weights(ix, N), np.arange(N), MIN_SAMPLES), metric)
    accounted(info, N, MIN_SAMPLES, 1)
    if metric == "sq_euclid_i8":
        return
    r = radius_between(metric, x, {p for p in links() if p[1] < N})[0]
    for radius in (r, 2 * r):                                              # DBSCAN at any radius is a cut of the one tree
        at = core <= np.float32(radius)
        labels = ix.density_clusters(radius, MIN_SAMPLES)[0]
        assert at.any() and ix.single_linkage_cut((a, b, d, info), radius)[at].tobytes() == labels[at].tobytes(), (metric, radius)


def test_allowed_sets_removed_ids_and_few_members(monkeypatch):
    x = np.random.default_rng(8).integers(0, 4, (N, DIM)).astype(np.float32)
    w = numpy_dist("sq_euclid", x)
    ix = _index(DIM, "sq_euclid", N)
    ix.set_allow_removals(True)
    ix.add(x)
    set_diag(monkeypatch, **SMALL)
    allowed = np.ones(N, bool)
    allowed[[0, 5, 6, 7, 8, 9, 203, 599] + list(range(300, 390))] = False     # cuts tiles of 8, a chunk edge and a round edge
    members = np.flatnonzero(allowed)
    for sel in (allowed, members):                                         # the set as a mask and as an id list
        got = ix.mutual_reachability_tree(5, allowed=sel)
        same(got, want(w, members, 5))
        accounted(got[4], members.size, 5, 2)
        at = got[3] <= 20.0
        assert ix.single_linkage_cut(got[:3] + got[4:], 20.0, allowed=sel)[at].tobytes() == ix.density_clusters(20.0, 5, allowed=sel)[0][at].tobytes()
    ix.reset_stats()
    for sel, s, lone in (([], 3, None), ([17], 1, -np.inf), ([17], 3, np.inf)):   # fewer than two members launch nothing
        a, b, d, core, info = ix.mutual_reachability_tree(s, allowed=np.isin(np.arange(N), sel))
        assert a.size == b.size == d.size == 0 and info == {**dict.fromkeys(info, 0), "members": len(sel), "components": len(sel)}
        assert np.isnan(np.delete(core, sel)).all() and (core[sel] == lone).all()
    assert ix.stats()["exact_launches"] == 0
    a, b, d, core, info = ix.mutual_reachability_tree(2, allowed=[17, 400])
    assert (a.tolist(), b.tolist(), d.tolist(), core[[17, 400]].tolist()) == ([17], [400], [w[17, 400]], [w[17, 400]] * 2) and info["rounds"] == 1
    few = np.array([3, 17, 400, 555])                                      # fewer other members than min_samples - 1: every core is +inf
    got = ix.mutual_reachability_tree(6, allowed=few)
    same(got, want(w, few, 6))
    assert np.isinf(got[2]).all() and (got[0].tolist(), got[1].tolist()) == ([3, 3, 3], [17, 400, 555]) and (got[3][few] == np.inf).all()
    gone = [1, 2, 203, 204, 511, 598]
    ix.remove(gone)
    same(ix.mutual_reachability_tree(5), want(w, np.delete(np.arange(N), gone), 5))
    same(ix.mutual_reachability_tree(5, allowed=allowed), want(w, np.setdiff1d(members, gone), 5))
    for s in (0, 1026):
        with pytest.raises(RuntimeError, match=f"hnsw_mi355x_mutual_reachability_tree: min_samples = {s}"):
            ix.mutual_reachability_tree(s)


def test_device_backend_nan_row():
    import hnswindex
    y = np.random.default_rng(3).integers(0, 3, (40, DIM)).astype(np.float32)
    y[7] = np.nan                                                          # no edge, a core of +inf, and no neighbour's core moves
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=40)
    dev.upload_rows(0, y)
    got = dev.exact_mreach_tree(40, 3)
    same(got, want(numpy_dist("sq_euclid", y), np.arange(40), 3))
    assert got[4]["components"] == 2 and got[4]["edges"] == 38 and 7 not in got[0].tolist() + got[1].tolist() and got[3][7] == np.inf
    accounted(got[4], 40, 3)
    part = dev.exact_mreach_tree(30, 3, allowed=np.arange(8, 30))          # rows [0, 30) with an allow-set on top
    same(part, want(numpy_dist("sq_euclid", y[:30]), np.arange(8, 30), 3))
    for s in (0, 1026):
        with pytest.raises(RuntimeError, match=f"exact_mreach_tree: min_samples = {s}"):
            dev.exact_mreach_tree(40, s)
