"""GPU tier: KnnQuery's half-precision row prefilter (kFormLeanPF) where its bound is TIGHT, and the shadow read back.
tests/test_gpu_row_prefilter.py holds the answers on uniform rows, where a kernel whose E were half its value would still pass;
here the kernel is tied to the numpy model (tests/row_prefilter.py), which has no slack:

* gadgets (tests/test_row_prefilter_inputs.py checks them on the CPU): hand-made graphs on which the answer IS one decision of the
  prefilter at the edge of its bound -- a kernel with half of E, with E short of an element set, or with E of the last pack alone
  answers with another id;
* the shadow rows and E read back through row_prefilter_peek and held to h(x) bit for bit and to e_of(x) within one float;
* the counters when a wave serves more than one job, and on the second query lane.

Every test runs with lat=0 (these small calls take the lean family), row_prefilter=2 (on regardless) and shadow=0 (no idle wave
starts the exact traversal beside the prefilter's), and the gadget tests require search_repeats == 0: the PF traversal itself answered."""
import math
import threading

import numpy as np
import pytest

import oracle
import row_prefilter as rp
from common import default_cap, set_diag, uniform

pytestmark = pytest.mark.gpu

NAMES = [f"a_{d}" for d in rp.A_DIMS] + list(rp.B_SETS) + [f"c_m{m}" for m in rp.C_LISTS] + ["d_100"]
PEEK_DIMS = [1, 7, 8, 9, 15, 16, 17, 24, 100, 128, 129, 136, 200, 255, 256]
INF_BITS = 0x7f800000


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


def _diag(monkeypatch, **kw):
    set_diag(monkeypatch, lat=0, row_prefilter=2, shadow=0, **kw)


# ---------------------------------------------------------------- gadgets
def _gadget_index(Index, gi, extra=0):
    ix = Index(gi.dim, "sq_euclid")
    ix.set_collection_size(gi.rows.shape[0] + extra); ix.set_max_edges(gi.m); ix.set_min_nn(1); ix.set_allow_removals(False)
    ix.set_insert_batch(1)                                               # (d)'s Add: one item after the other, the oracle's add()
    ix.import_graph(gi.rows, gi.levels, gi.entry, gi.layers)
    return ix


def _ask(ix, ref, gi, j, model):
    """Gadget j's query: the oracle's answer from the PF traversal itself, and the model's counters."""
    gd = gi.gadgets[j]
    st0, pf0 = ix.stats(), ix.row_prefilter_stats()
    got, want = ix.knn_query(gd.q, gd.k), ref.knn_query(gd.q, gd.k)
    st1, pf1 = ix.stats(), ix.row_prefilter_stats()
    on_shadow, reread = pf1["rows_on_shadow"] - pf0["rows_on_shadow"], pf1["rows_reread"] - pf0["rows_reread"]
    print(f"{gd.name}: ids {'equal' if (got[0] == want[0]).all() else 'DIFFER'}, probe {'kept' if gi.probe_id(j) in got[0] else 'TURNED AWAY'}, "
          f"on shadow {on_shadow} (model {model['rows_on_shadow']}), re-read {reread} (model {model['rows_reread']}, sure {model['rows_reread_sure']})")
    assert want[0][0].tolist() == model["ids"], gd.name
    assert _same(got, want), (gd.name, got[0].tolist(), want[0].tolist())
    assert st1["search_repeats"] == st0["search_repeats"] and st1["search_overflows"] == st0["search_overflows"], gd.name
    assert st1["lean_launches"] == st0["lean_launches"] + 1 and st1["lat_launches"] == 0 and pf1["launches"] == pf0["launches"] + 1, gd.name
    assert on_shadow == model["rows_on_shadow"], gd.name
    assert model["rows_reread_sure"] <= reread <= on_shadow, gd.name
    return got


@pytest.mark.parametrize("vis_hash", [0, 1])
@pytest.mark.parametrize("name", [n for n in NAMES if n != "d_100"])
def test_the_decision_at_the_edge_of_the_bound(Index, monkeypatch, name, vis_hash):
    _diag(monkeypatch, vis_hash=vis_hash)
    gi = rp.catalogue()[name]
    assert gi is not None, "no gadget: tests/test_row_prefilter_inputs.py says which"
    ix, ref = _gadget_index(Index, gi), rp.oracle_of(gi)
    for j in range(len(gi.gadgets)):
        _ask(ix, ref, gi, j, gi.model(j))
    peek = ix.row_prefilter_peek()
    assert peek["packed"] == gi.rows.shape[0] and ix.row_prefilter_stats()["rows_packed"] == gi.rows.shape[0]
    assert float(gi.e) <= float(peek["e"]) <= float(np.nextafter(gi.e, np.float32(np.inf))), (name, peek["e"], gi.e)


@pytest.mark.parametrize("vis_hash", [0, 1])
def test_rows_packed_later_do_not_lower_the_bound(Index, monkeypatch, vis_hash):
    """(d): the first query packs the gadget's rows; an Add of binary16-valued rows far away is packed by the next query, whose E
    must still be that of ALL rows -- E of the last pack alone is E of binary16 rows, and turns the probe away."""
    _diag(monkeypatch, vis_hash=vis_hash)
    gi = rp.catalogue()["d_100"]
    more = rp.added_rows(gi.dim)
    n = gi.rows.shape[0]
    ix, ref = _gadget_index(Index, gi, extra=more.shape[0]), rp.oracle_of(gi, extra=more.shape[0])
    for j in range(len(gi.gadgets)):
        _ask(ix, ref, gi, j, gi.model(j))
    before = ix.row_prefilter_peek()
    assert before["packed"] == n
    assert (ix.add(more) == ref.add(more)).all() and ix.graph_hash() == ref.graph_hash()
    assert ix.row_prefilter_peek()["packed"] == n                        # nothing is packed before a launch needs it
    levels, layers = rp.graph_of(ref, gi.m)
    rows = np.concatenate([gi.rows, more])
    for j in range(len(gi.gadgets)):
        _ask(ix, ref, gi, j, gi.model(j, rows=rows, layers=layers, levels=levels))
    after = ix.row_prefilter_peek()
    assert after["packed"] == n + more.shape[0] and ix.row_prefilter_stats()["rows_packed"] == n + more.shape[0]
    assert after["e_bits"] == before["e_bits"]                           # binary16 rows add nothing to it


# ---------------------------------------------------------------- the shadow and E, read back
def _edge_rows(dim, seed, n=40):
    """Uniform rows, and rows of the values where the conversion changes its rule: halves that go subnormal (below 6.1e-5), to zero
    (2^-25 ties to even; just above it rounds up), -0, the largest half and the f32 values around it that still round to it."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, dim), dtype=np.float32)
    x[1] *= np.float32(1e-4)                                             # normal and subnormal halves mixed
    x[2] *= np.float32(1e-6)                                             # subnormal halves, some to zero
    x[3] = -x[3]
    edge = np.array([-0.0, 0.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), -2.0 ** -24 * 1.5, 2.0 ** -24 * 2.5, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12),
                     6.1e-5, 65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 0.333], dtype=np.float32)
    x[4] = np.resize(edge, dim)
    x[5] = np.resize(edge[::-1], dim)
    return x


def _exact_norm(x):
    """max over rows of sqrt(sum (x - h(x))^2): every difference and every square is exact in double, fsum adds them exactly."""
    d = x.astype(np.float64) - rp.h(x).astype(np.float64)
    return max(math.sqrt(math.fsum((r * r).tolist())) for r in d)


def _check_shadow(ix, x, where):
    peek = ix.row_prefilter_peek(0, x.shape[0])
    assert peek["packed"] == x.shape[0], where
    with np.errstate(invalid="ignore"):
        assert peek["rows"].view(np.uint32).tolist() == rp.h(x).view(np.uint32).tolist(), where      # bit for bit: -0, NaN payloads, subnormals
    want = rp.e_of(x)
    print(f"{where}: E {peek['e']!r} (bits {peek['e_bits']:#x}), e_of {want!r}")
    if np.isinf(want):
        assert peek["e_bits"] == INF_BITS, where
    else:
        assert _exact_norm(x) <= float(peek["e"]) <= float(np.nextafter(want, np.float32(np.inf))), (where, peek["e"], want)
        assert float(peek["e"]) >= float(np.nextafter(want, np.float32(0))), (where, peek["e"], want)   # the lane-order sum: one place, no more
    return peek


def _small_index(Index, dim, x, capacity):
    ix = Index(dim, "sq_euclid")
    ix.set_collection_size(capacity); ix.set_max_edges(16); ix.set_min_nn(8)
    ix.add(x)
    return ix


@pytest.mark.parametrize("dim", PEEK_DIMS)
def test_the_shadow_rows_and_e_are_the_models(Index, monkeypatch, dim):
    _diag(monkeypatch)
    x = _edge_rows(dim, 4000 + dim)
    ix = _small_index(Index, dim, x, 64)
    assert ix.row_prefilter_peek()["packed"] == 0                        # no lean launch yet: no shadow, and the peek makes none
    q = uniform(3, dim, 4100 + dim)
    ix.knn_query(q, 5)
    assert ix.stats()["lean_launches"] == 1 and ix.row_prefilter_stats()["launches"] == 1
    _check_shadow(ix, x, f"dim {dim}")
    with pytest.raises(RuntimeError):
        ix.row_prefilter_peek(x.shape[0] - 1, 2)                         # past the watermark


@pytest.mark.parametrize("bad", [65520.0, np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dim", PEEK_DIMS)
def test_a_row_that_does_not_fit_a_half_makes_e_infinite(Index, monkeypatch, dim, bad):
    """65520 is the first value that rounds to +inf in binary16.  The row is alone in its index, at the last element (the second step
    of the pack kernel's lane loop where dim > 128, the partial 16-block where there is one)."""
    _diag(monkeypatch)
    x = uniform(1, dim, 4200 + dim)
    x[0, dim - 1] = bad
    assert np.isinf(rp.row_bounds(x)[0])
    ix = _small_index(Index, dim, x, 8)
    ix.knn_query(uniform(2, dim, 4300 + dim), 1)
    assert ix.row_prefilter_stats()["launches"] == 1
    _check_shadow(ix, x, f"dim {dim}, {bad}")


@pytest.mark.parametrize("dim", [100, 200])
def test_e_grows_with_a_partial_repack_and_starts_over_with_a_full_one(Index, monkeypatch, dim):
    _diag(monkeypatch)
    n0, cap = 30, 48
    x = _edge_rows(dim, 4400 + dim, n0)
    q = uniform(3, dim, 4500 + dim)
    ix = _small_index(Index, dim, x, cap)
    ix.knn_query(q, 5)
    first = _check_shadow(ix, x, "first pack")
    worse = uniform(4, dim, 4600 + dim)
    worse[2, dim - 1] = np.float32(65519.0)                              # rounds to 65504: this row's bound is 15 and more
    ids = ix.add(worse)
    ix.knn_query(q, 5)
    x1 = np.concatenate([x, worse])
    second = _check_shadow(ix, x1, "partial repack")
    assert second["e"] >= first["e"] and second["e"] > 14 and ix.row_prefilter_stats()["rows_packed"] == n0 + 4
    # the worst row leaves, a binary16-valued row takes its slot: a partial repack from that slot on, and E stays (it only grows)
    ix.remove(ids[2:3])
    mild = rp.h(uniform(1, dim, 4700 + dim))
    assert ix.add(mild).tolist() == [int(ids[2])]
    ix.knn_query(q, 5)
    x2 = x1.copy()
    x2[int(ids[2])] = mild[0]
    third = ix.row_prefilter_peek(0, x2.shape[0])
    assert third["e_bits"] == second["e_bits"] and third["rows"].tobytes() == rp.h(x2).tobytes()
    assert ix.row_prefilter_stats()["rows_packed"] == n0 + 4 + (n0 + 4 - int(ids[2]))
    # growing past the collection size moves the row matrix: everything is packed again and E starts over
    grow = uniform(cap, dim, 4800 + dim)
    ix.add(grow)
    ix.knn_query(q, 5)
    x3 = np.concatenate([x2, grow])
    fourth = _check_shadow(ix, x3, "full repack")
    assert fourth["e"] < 1 and ix.row_prefilter_stats()["rows_packed"] == n0 + 4 + (n0 + 4 - int(ids[2])) + x3.shape[0]


# ---------------------------------------------------------------- more jobs than waves; the second lane
@pytest.fixture(scope="module")
def uniform_graph(Index):
    """tests/test_gpu_row_prefilter.py's 6000 x 100 uniform graph (M 16), built once with the prefilter off."""
    import os
    from test_gpu_row_prefilter import Graph
    old = os.environ.get("HNSW_MI355X_DIAG")
    os.environ["HNSW_MI355X_DIAG"] = ((old + ",") if old else "") + "row_prefilter=0"
    try:
        return Graph(Index, "uniform", 100)
    finally:
        if old is None:
            del os.environ["HNSW_MI355X_DIAG"]
        else:
            os.environ["HNSW_MI355X_DIAG"] = old


def test_the_counters_add_up_when_a_wave_serves_many_jobs(uniform_graph, monkeypatch):
    """8192 queries are more jobs than the chip has resident waves: one call (a wave takes job after job) and 32 calls of 256 (a wave
    takes at most one) must measure and re-read the same rows."""
    _diag(monkeypatch)
    g, ef, k = uniform_graph, 64, 10
    q = uniform(8192, g.dim, 5100)
    ref = oracle.OracleIndex(g.dim, "sq_euclid", max_edges=16, min_nn=ef, collection_size=g.x.shape[0], allow_removals=False)
    ref.import_graph(g.x, g.lv, g.entry, g.layers)
    want = ref.knn_query(q, k, threads=8)
    one, many = g.at(ef), g.at(ef)
    assert _same(one.knn_query(q, k), want)
    parts = [many.knn_query(q[i:i + 256], k) for i in range(0, q.shape[0], 256)]
    assert _same((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want)
    a, b = one.row_prefilter_stats(), many.row_prefilter_stats()
    print(f"one call {a}, 32 calls {b}")
    assert a["launches"] == 1 and b["launches"] == 32 and one.stats()["search_repeats"] == many.stats()["search_repeats"] == 0
    assert a["rows_on_shadow"] == b["rows_on_shadow"] > 0 and a["rows_reread"] == b["rows_reread"] > 0
    assert a["rows_reread"] < a["rows_on_shadow"] and a["rows_packed"] == b["rows_packed"] == g.x.shape[0]


def test_the_second_query_lane_shares_the_shadow(Index, monkeypatch):
    """Two threads, each with half of the queries, after an Add that follows the first pack: the call that finds lane 0 busy runs on
    a view that borrows the primary's shadow.  Answers, counter totals and rows packed are the single-thread run's."""
    _diag(monkeypatch)
    dim, n0, rounds = 100, 3000, 4
    x, more, q = uniform(n0, dim, 5200), uniform(200, dim, 5201), uniform(600, dim, 5202)
    halves = [q[:300], q[300:]]

    def make():
        ix = Index(dim, "sq_euclid")
        ix.set_collection_size(n0 + 200); ix.set_max_edges(16); ix.set_min_nn(64)
        ix.add(x)
        ix.knn_query(q[:8], 10)                                          # the first pack
        ix.add(more)
        return ix

    single, pair = make(), make()
    assert single.graph_hash() == pair.graph_hash()
    want = [single.knn_query(hq, 10) for hq in halves]
    for _ in range(rounds - 1):
        for hq in halves:
            single.knn_query(hq, 10)
    ref = oracle.OracleIndex(dim, "sq_euclid", max_edges=16, min_nn=64, collection_size=n0 + 200)
    ref.add_batched(x, default_cap(), threads=8); ref.add_batched(more, default_cap(), threads=8)
    assert ref.graph_hash() == single.graph_hash() and all(_same(w, ref.knn_query(hq, 10, threads=8)) for w, hq in zip(want, halves))
    got, errs, gate = [[], []], [], threading.Barrier(2)

    def worker(t):
        try:
            for _ in range(rounds):
                gate.wait()
                got[t].append(pair.knn_query(halves[t], 10))
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    assert all(_same(r, want[t]) for t in range(2) for r in got[t])
    a, b = single.row_prefilter_stats(), pair.row_prefilter_stats()
    print(f"single {a}, two threads {b}")
    assert a == b and a["rows_packed"] == n0 + 200 and a["launches"] == 1 + 2 * rounds
    assert single.stats()["lean_launches"] == pair.stats()["lean_launches"] == 1 + 2 * rounds
    peek = pair.row_prefilter_peek(0, n0 + 200)
    assert peek["rows"].tobytes() == rp.h(np.concatenate([x, more])).tobytes()
