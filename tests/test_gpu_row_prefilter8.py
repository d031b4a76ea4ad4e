"""GPU tier: the 8-bit row prefilter of KnnQuery (kFormLeanPF8Fixed; the bound restated in tests/row_prefilter8.py).
Dim 128, M 16, lat=0 (these small calls take the lean family).  Answers must be the oracle's -- ids equal, distance bytes equal --
with the 8-bit form forced (diag row_prefilter=3), with the prefilter off (0) and by default; the counters must be the model's; every
write to the stored rows must reach the code bytes (a stale shadow row answers wrongly without any other sign); and the shadow read
back through row_prefilter8_peek must bound what the pack kernel says it bounds.

Where counters are compared with the model, shadow=0 as well: an idle wave that starts the exact traversal of a job beside its owner
may answer it first, and whether it does is a race that search_repeats would show."""
import os

import numpy as np
import pytest

import oracle
import row_prefilter8 as r8
from common import default_cap, set_diag, uniform

pytestmark = pytest.mark.gpu

DIM, M, N = 128, 16, 3000
BEAMS = [(64, 10), (128, 10), (200, 130)]                                # (efSearch = MinNN, k); the last one: four register sets
ZERO8 = dict.fromkeys(("launches", "rows_packed", "rows_on_shadow", "rows_reread", "full_packs", "fallbacks_to_f16"), 0)


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _same(a, b):
    return a[0].shape == b[0].shape and (a[0] == b[0]).all() and a[1].tobytes() == np.ascontiguousarray(b[1]).tobytes()


class Graph:
    """One graph over rows x (M = 16), built on the device with the prefilter off; at(ef) is that graph in a fresh index whose MinNN
    is ef, want(q, ef, k) the oracle's answer on the same graph."""

    def __init__(self, Index, x):
        self.Index, self.x = Index, x
        old = os.environ.get("HNSW_MI355X_DIAG")
        os.environ["HNSW_MI355X_DIAG"] = ((old + ",") if old else "") + "row_prefilter=0"
        try:
            ix = self._index(5)
            ix.add(x)
        finally:
            if old is None:
                del os.environ["HNSW_MI355X_DIAG"]
            else:
                os.environ["HNSW_MI355X_DIAG"] = old
        self.hash, self.lv, self.entry = ix.graph_hash(), ix.levels(), ix.entry_point
        self.layers = [ix.export_edges(L, 2 * M + 2 if L == 0 else M + 2) for L in range(int(self.lv.max()) + 1)]
        self._refs = {}

    def _index(self, min_nn):
        ix = self.Index(DIM, "sq_euclid")
        ix.set_collection_size(self.x.shape[0]); ix.set_max_edges(M); ix.set_min_nn(min_nn)
        return ix

    def at(self, ef):
        ix = self._index(ef)
        ix.import_graph(self.x, self.lv, self.entry, self.layers)
        assert ix.graph_hash() == self.hash
        return ix

    def want(self, q, ef, k):
        if ef not in self._refs:
            r = oracle.OracleIndex(DIM, "sq_euclid", max_edges=M, min_nn=ef, collection_size=self.x.shape[0], allow_removals=False)
            r.import_graph(self.x, self.lv, self.entry, self.layers)
            assert r.graph_hash() == self.hash
            self._refs[ef] = r
        return self._refs[ef].knn_query(q, k, threads=8)


@pytest.fixture(scope="module")
def g(Index):
    return Graph(Index, uniform(N, DIM, 9100))


@pytest.fixture(scope="module")
def q():
    return uniform(256, DIM, 9101)


def _peeked(ix, rows):
    """The whole shadow read back: (peek, decoded shadow rows, the exact ||x - h8(x)||_2 per row in float64)."""
    peek = ix.row_prefilter8_peek(0, rows.shape[0])
    shadow = r8.decode(peek["codes"], peek["lo"], peek["step"])
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.sqrt(((rows.astype(np.float64) - shadow.astype(np.float64)) ** 2).sum(axis=1))
    return peek, shadow, err


def _bound_holds(peek, err):
    """E8 >= max ||x - decode(codes)||_2, and no more than that maximum (1 + 2^-19) + 1e-36."""
    top = float(err.max())
    assert float(peek["e"]) >= top and float(peek["e"]) <= top * (1 + 2.0 ** -19) + 1e-36, (peek["e"], top)


# ---- answers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vis_hash", [0, 1], ids=["bitset", "hashed"])
@pytest.mark.parametrize("ef,k", BEAMS)
def test_answers_are_the_oracles_forced_off_and_by_default(g, q, monkeypatch, ef, k, vis_hash):
    want = g.want(q, ef, k)
    for mode in (3, 0, 1):                                               # (1: the default)
        set_diag(monkeypatch, lat=0, vis_hash=vis_hash, row_prefilter=mode)
        ix = g.at(ef)
        got = ix.knn_query(q, k)
        st, pf, pf8, form = ix.stats(), ix.row_prefilter_stats(), ix.row_prefilter8_stats(), ix.row_prefilter_form_stats()
        print(f"row_prefilter {mode} ef {ef} k {k} hashed {vis_hash}: {pf8}, totals {pf}, f16 forms {form}, repeats {st['search_repeats']}")
        assert _same(got, want), (mode, ef, k)
        assert st["lean_launches"] > 0 and st["lat_launches"] == 0 and st["search_overflows"] == 0
        assert (st["visited_hash_launches"] > 0) == bool(vis_hash)
        if mode == 3:
            assert pf8["launches"] > 0 and pf8["rows_packed"] == N and pf8["full_packs"] == 1 and pf8["fallbacks_to_f16"] == 0
            assert 0 < pf8["rows_reread"] < pf8["rows_on_shadow"]        # rows were turned away on the 8-bit value
            assert form == {"runtime_dim": 0, "fixed_dim": 0}            # neither f16 slot
            assert pf == {"launches": pf8["launches"], "rows_on_shadow": pf8["rows_on_shadow"], "rows_reread": pf8["rows_reread"], "rows_packed": N}
        elif mode == 0:
            assert pf8 == ZERO8 and pf["launches"] == 0 and ix.row_prefilter8_peek()["packed"] == 0
        else:
            assert pf["launches"] > 0 and pf["rows_packed"] == N         # one shadow, whichever width the library chose
            assert pf8["launches"] + form["fixed_dim"] == pf["launches"] and form["runtime_dim"] == 0


def test_mode_2_is_the_f16_prefilter_and_allocates_no_code_bytes(g, q, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=2)
    ix = g.at(64)
    assert _same(ix.knn_query(q, 10), g.want(q, 64, 10))
    pf = ix.row_prefilter_stats()
    assert ix.row_prefilter8_stats() == ZERO8 and ix.row_prefilter8_peek()["packed"] == 0
    assert ix.row_prefilter_form_stats() == {"runtime_dim": 0, "fixed_dim": pf["launches"]} and pf["launches"] > 0
    assert ix.row_prefilter_peek()["packed"] == N


def test_other_row_lengths_take_the_f16_forms_under_mode_3(Index, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=3)
    x, qq = uniform(1200, 120, 9200), uniform(64, 120, 9201)
    ix = Index(120, "sq_euclid"); ix.set_collection_size(1200); ix.set_max_edges(M); ix.set_min_nn(64)
    ref = oracle.OracleIndex(120, "sq_euclid", max_edges=M, min_nn=64, collection_size=1200)
    assert (ix.add(x) == ref.add_batched(x, default_cap(), threads=8)).all()
    assert _same(ix.knn_query(qq, 10), ref.knn_query(qq, 10, threads=8))
    pf = ix.row_prefilter_stats()
    assert ix.row_prefilter8_stats() == ZERO8 and ix.row_prefilter_form_stats() == {"runtime_dim": pf["launches"], "fixed_dim": 0} and pf["launches"] > 0


# ---- the counters are the model's -----------------------------------------------------------------------------------------------------
def test_the_counters_are_the_models_on_uniform_rows(g, monkeypatch):
    set_diag(monkeypatch, lat=0, row_prefilter=3, shadow=0)
    ef, k = 64, 10
    qq = uniform(24, DIM, 9102)
    ix = g.at(ef)
    got = ix.knn_query(qq, k)
    assert _same(got, g.want(qq, ef, k)) and ix.stats()["search_repeats"] == 0   # (the sorted traversal answered every job itself)
    peek, shadow, err = _peeked(ix, g.x)
    _bound_holds(peek, err)
    models = [r8.search_model8(g.x, shadow, g.layers, g.lv, g.entry, qi, ef, peek["e"]) for qi in qq]
    assert all(m["ids"][:k] == row.tolist() for m, row in zip(models, got[0]))
    pf8 = ix.row_prefilter8_stats()
    on, lo, hi = (sum(m[name] for m in models) for name in ("rows_on_shadow", "rows_reread_lo", "rows_reread_hi"))
    print(f"device {pf8}; model: on the shadow {on}, re-read {sum(m['rows_reread'] for m in models)} in [{lo}, {hi}]")
    assert pf8["rows_on_shadow"] == on and lo <= pf8["rows_reread"] <= hi
    assert 0.05 < pf8["rows_reread"] / pf8["rows_on_shadow"] < 0.6


# ---- one decision at the edge of the bound, through every pass width ------------------------------------------------------------------
@pytest.mark.parametrize("vis_hash", [0, 1], ids=["bitset", "hashed"])
@pytest.mark.parametrize("m", sorted(r8.C_LISTS8))
def test_the_decision_at_the_edge_of_the_bound(Index, monkeypatch, m, vis_hash):
    """Lists of 3, 12, 20, 31, 40 and 64 ids put the probe's code bytes through each pass width and tail of measure_shadow8, k = 130
    through four register sets.  The model with half of E8 answers with the decoy f (tests/test_row_prefilter8_model.py): the kernel
    must keep the probe, like the oracle."""
    set_diag(monkeypatch, lat=0, row_prefilter=3, shadow=0, vis_hash=vis_hash)
    gi = r8.catalogue8(m)
    assert gi is not None, "no gadgets: tests/test_row_prefilter8_model.py says which"
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(gi.rows.shape[0]); ix.set_max_edges(m); ix.set_min_nn(1); ix.set_allow_removals(False)
    ix.import_graph(gi.rows, gi.levels, gi.entry, gi.layers)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=m, min_nn=1, collection_size=gi.rows.shape[0], allow_removals=False)
    ref.import_graph(gi.rows, gi.levels, gi.entry, gi.layers)
    for j, gd in enumerate(gi.gadgets):
        st0, p0 = ix.stats(), ix.row_prefilter8_stats()
        got, want = ix.knn_query(gd.q, gd.k), ref.knn_query(gd.q, gd.k)
        st1, p1 = ix.stats(), ix.row_prefilter8_stats()
        if j == 0:                                                       # the model runs on the device's own codes and E8
            peek, shadow, err = _peeked(ix, gi.rows)
            _bound_holds(peek, err)
            assert (peek["lo"], peek["step"]) == gi.grid and float(peek["e"]) >= float(np.max(err))
        model = r8.search_model8(gi.rows, shadow, gi.layers, gi.levels, gi.entry, gd.q, gd.k, peek["e"])
        on, reread = p1["rows_on_shadow"] - p0["rows_on_shadow"], p1["rows_reread"] - p0["rows_reread"]
        print(f"{gd.name}: probe {'kept' if gi.probe_id(j) in got[0] else 'TURNED AWAY'}, on the shadow {on} (model {model['rows_on_shadow']}), "
              f"re-read {reread} (model {model['rows_reread_lo']} .. {model['rows_reread_hi']})")
        assert _same(got, want) and want[0][0].tolist() == model["ids"], gd.name
        assert gi.probe_id(j) in got[0] and gi.far_id(j) not in got[0], gd.name
        assert st1["search_repeats"] == st0["search_repeats"] and p1["launches"] == p0["launches"] + 1, gd.name
        assert on == model["rows_on_shadow"] and model["rows_reread_lo"] <= reread <= model["rows_reread_hi"], gd.name


def test_the_worst_case_family_on_a_real_graph(g, monkeypatch):
    """q = h8 + stretch (x - h8) for rows of the index, from the codes the device packed: the rounding of every element moves the
    distance the same way.  Answers like the oracle's."""
    set_diag(monkeypatch, lat=0, row_prefilter=3)
    ix = g.at(64)
    ix.knn_query(g.x[:1], 1)                                             # (packs)
    peek, shadow, err = _peeked(ix, g.x)
    rows = np.random.default_rng(9103).choice(N, 96, replace=False)
    for stretch in (2.0, 40.0):
        qq = r8.worst_case8(g.x[rows], shadow[rows], stretch)
        assert _same(ix.knn_query(qq, 10), g.want(qq, 64, 10)), stretch


# ---- writes reach the shadow --------------------------------------------------------------------------------------------------------
def test_every_write_to_the_stored_rows_reaches_the_code_bytes(Index, monkeypatch, tmp_path):
    """query; Add within the capacity (rows outside the grid among them: clamped, E8 grows); Add past it (a full pack, a fresh grid);
    Serialize / Deserialize; Remove + Add into the freed slots -- each step against the oracle, the 8-bit form forced.  Every Add makes
    rows nearer to the queries than anything before: a query answered from a stale shadow would turn them away."""
    set_diag(monkeypatch, lat=0, row_prefilter=3)
    n0 = 3000
    x, qq = uniform(n0, DIM, 71), uniform(200, DIM, 72)
    near = lambda seed: (qq + np.float32(1e-2) * uniform(200, DIM, seed)).astype(np.float32)
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(n0 + 300); ix.set_max_edges(M)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=M, collection_size=n0 + 300)

    def step(what, packed, full_packs):
        got, want = ix.knn_query(qq, 10), ref.knn_query(qq, 10, threads=8)
        assert ix.graph_hash() == ref.graph_hash(), what
        assert _same(got, want), what
        pf8 = ix.row_prefilter8_stats()
        assert pf8["rows_packed"] == packed and pf8["full_packs"] == full_packs, (what, pf8)
        assert ix.row_prefilter_stats()["rows_packed"] == packed and ix.row_prefilter_form_stats() == {"runtime_dim": 0, "fixed_dim": 0}, what
        return pf8

    assert (ix.add(x) == ref.add_batched(x, default_cap(), threads=8)).all()
    step("built", n0, 1)
    step("again: nothing to pack", n0, 1)
    first = ix.row_prefilter8_peek()
    a = near(73)
    a[5, 7], a[6, 8] = 1.5, -0.5                                         # outside the grid of a [0, 1) index
    assert (ix.add(a) == ref.add_batched(a, default_cap(), threads=8)).all()
    step("added within the capacity", n0 + 200, 1)                       # only the new rows, on the same grid
    second = ix.row_prefilter8_peek(n0, 200)
    assert (second["lo"], second["step"]) == (first["lo"], first["step"]) and second["e"] > first["e"] and second["e"] > 0.45
    assert second["codes"][5, 7] == 255 and second["codes"][6, 8] == 0   # clamped
    b = np.concatenate([near(74), uniform(300, DIM, 75)])
    assert (ix.add(b) == ref.add_batched(b, default_cap(), threads=8)).all()
    step("grown past the collection size", n0 + 200 + (n0 + 700), 2)     # the matrix moved: all of it again, a fresh grid
    third = ix.row_prefilter8_peek()
    assert third["lo"] == np.float32(-0.5) and third["step"] > first["step"] and third["e"] < second["e"]   # E8 started over
    path = tmp_path / "index.bin"
    ix.serialize(path)
    ix2 = Index.deserialize(path)
    got, want = ix2.knn_query(qq, 10), ref.knn_query(qq, 10, threads=8)
    assert _same(got, want) and ix2.row_prefilter8_stats()["launches"] > 0 and ix2.row_prefilter8_stats()["rows_packed"] == n0 + 700
    gone = np.arange(n0, n0 + 200, dtype=np.int32)                       # the first batch of near rows leaves ...
    ix.remove(gone); ref.remove(gone)
    c = near(76)                                                         # ... and other near rows take their slots
    ids_c, want_c = ix.add(c), ref.add_batched(c, default_cap(), threads=8)
    assert (ids_c == want_c).all() and set(ids_c.tolist()) == set(gone.tolist())
    before = ix.row_prefilter8_stats()
    step("slots re-used", before["rows_packed"] + (n0 + 700 - int(ids_c.min())), 2)
    peek, shadow, err = _peeked(ix, ix.get_vectors(np.arange(n0 + 700, dtype=np.int32)))
    _bound_holds(peek, err)
    assert peek["e"] >= third["e"]                                       # never lower after a partial repack


def test_an_infinite_element_re_reads_everything_and_falls_back_to_f16_once(g, Index, monkeypatch):
    """The graph of the uniform rows with one element of one row set to +inf (imported: no insert measures that row from itself).
    E8 = +inf turns nothing away; by default the next call runs the f16 form, and the call after a write tries the 8-bit form again."""
    set_diag(monkeypatch, lat=0)                                         # row_prefilter at its default
    ef, qq = 64, uniform(200, DIM, 82)
    x = g.x.copy()
    x[1234, 5] = np.inf
    more = uniform(5, DIM, 83)
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(N + 5); ix.set_max_edges(M); ix.set_min_nn(ef); ix.set_allow_removals(False); ix.set_insert_batch(1)
    ix.import_graph(x, g.lv, g.entry, g.layers)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=M, min_nn=ef, collection_size=N + 5, allow_removals=False)
    ref.import_graph(x, g.lv, g.entry, g.layers)
    ref.rng_skip(N)
    want = ref.knn_query(qq, 10, threads=8)
    assert _same(ix.knn_query(qq, 10), want)
    pf8, peek = ix.row_prefilter8_stats(), ix.row_prefilter8_peek()
    assert pf8["launches"] == 1, "the default took no 8-bit launch at dim 128"
    assert pf8["rows_reread"] == pf8["rows_on_shadow"] > 0 and pf8["fallbacks_to_f16"] == 1 and pf8["full_packs"] == 1
    assert peek["packed"] == 0 and peek["e_bits"] == 0x7f800000          # the watermark is 0: the next try derives a fresh grid
    assert (peek["lo"], peek["step"]) == r8.grid_of(x)                   # ... this one came from the finite elements
    assert _same(ix.knn_query(qq, 10), want)                             # the f16 form (its E is +inf as well: it re-reads everything, once)
    assert ix.row_prefilter8_stats()["launches"] == 1 and ix.row_prefilter_form_stats() == {"runtime_dim": 0, "fixed_dim": 1}
    assert (ix.add(more) == ref.add(more)).all() and ix.graph_hash() == ref.graph_hash()
    assert _same(ix.knn_query(qq, 10), ref.knn_query(qq, 10, threads=8))  # after a write: the 8-bit form again, on a fresh grid
    pf8 = ix.row_prefilter8_stats()
    assert pf8["launches"] == 2 and pf8["full_packs"] == 2 and pf8["fallbacks_to_f16"] == 2 and pf8["rows_packed"] == N + (N + 5)


def test_a_tight_cluster_costs_one_8_bit_launch_then_one_f16_launch_then_runs_lean(Index, monkeypatch):
    set_diag(monkeypatch, lat=0)
    n = 3000
    rng = np.random.default_rng(41)
    c = rng.random(DIM, dtype=np.float32)
    x = (c + np.float32(1e-4) * rng.standard_normal((n, DIM), dtype=np.float32)).astype(np.float32)
    qq = (c + np.float32(1e-4) * rng.standard_normal((200, DIM), dtype=np.float32)).astype(np.float32)
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_min_nn(64)
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=M, min_nn=64, collection_size=n)
    assert (ix.add(x) == ref.add_batched(x, default_cap(), threads=8)).all()
    want = ref.knn_query(qq, 10, threads=8)
    seen = []
    for _ in range(4):
        assert _same(ix.knn_query(qq, 10), want)
        seen.append((ix.row_prefilter8_stats()["launches"], ix.row_prefilter_form_stats()["fixed_dim"], ix.stats()["lean_launches"]))
    print(f"(8-bit launches, f16 launches, lean-family launches) after each call: {seen}")
    assert seen == [(1, 0, 1), (1, 1, 2), (1, 1, 3), (1, 1, 4)]
    pf8 = ix.row_prefilter8_stats()
    assert pf8["fallbacks_to_f16"] == 1 and 4 * pf8["rows_reread"] > pf8["rows_on_shadow"]


# ---- peek -----------------------------------------------------------------------------------------------------------------------------
def test_the_shadow_read_back_bounds_what_it_says(Index, monkeypatch):
    """E8 against the exact ||x - decode(codes)||_2 of every packed row; the grid against the rows' smallest and largest element
    (negative elements: the ordered keys); E8 never lower after a partial repack."""
    set_diag(monkeypatch, lat=0, row_prefilter=3)
    n = 3000
    x = (uniform(n, DIM, 91) * np.float32(3.0) - np.float32(2.0)).astype(np.float32)
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(n + 64); ix.set_max_edges(M)
    assert ix.row_prefilter8_peek()["packed"] == 0
    ix.add(x)
    assert ix.row_prefilter8_peek()["packed"] == 0                       # no lean launch yet: no shadow, and the peek makes none
    ix.knn_query(x[:4], 3)
    peek, shadow, err = _peeked(ix, x)
    assert peek["packed"] == n and (peek["lo"], peek["step"]) == r8.grid_of(x)
    _bound_holds(peek, err)
    print(f"largest |x - h8| {np.abs(x.astype(np.float64) - shadow).max()!r} of step / 2 = {float(peek['step']) / 2!r}")
    with pytest.raises(RuntimeError, match="range outside the packed shadow rows"):
        ix.row_prefilter8_peek(n - 1, 2)
    more = uniform(8, DIM, 92)                                           # inside the grid: a partial repack cannot lower E8
    ix.add(more)
    assert ix.row_prefilter8_peek()["packed"] == n                       # nothing is packed before a launch needs it
    ix.knn_query(x[:4], 3)
    after = ix.row_prefilter8_peek()
    assert after["packed"] == n + 8 and after["e"] >= peek["e"] and (after["lo"], after["step"]) == (peek["lo"], peek["step"])


def test_elements_inside_the_grid_are_within_half_a_step_of_their_shadow_value(Index, monkeypatch):
    """|x_i - h8_i| <= step / 2 (1 + 2^-20) for elements inside the grid.  The rows hold 0 and 255 / 256, so step = 2^-8 and every
    shadow value c / 256 is exact: the figure then is the encoder's alone.  On a grid whose values are not representable the shadow
    value is ONE f32 rounding of step c + lo, and an element next to the midpoint of two grid values can be off by half an ulp of h8
    more than step / 2 whatever the encoder does -- measured on uniform rows in [-2, 1): 0.0058823824 against
    step / 2 = 0.0058823037 (1.3e-5 of it, with the quotient in f32; 2e-5 of it is half an ulp of 2) -- which E8 covers: it is
    taken from the decoded values (test_the_shadow_read_back_bounds_what_it_says)."""
    set_diag(monkeypatch, lat=0, row_prefilter=3)
    n = 3000
    x = (uniform(n, DIM, 93) * np.float32(255.0 / 256.0)).astype(np.float32)
    x[0, 0], x[0, 1] = 0.0, 255.0 / 256.0
    x[1, :] = (np.arange(DIM, dtype=np.float32) + np.float32(0.5)) / np.float32(256.0)      # midpoints: either neighbour is half a step away
    x[2, :64] = np.nextafter(x[1, :64], np.float32(1.0)); x[2, 64:] = np.nextafter(x[1, 64:], np.float32(0.0))
    ix = Index(DIM, "sq_euclid")
    ix.set_collection_size(n); ix.set_max_edges(M)
    ix.add(x)
    ix.knn_query(x[:4], 3)
    peek, shadow, err = _peeked(ix, x)
    assert peek["lo"] == 0 and peek["step"] == np.float32(2.0 ** -8)
    _bound_holds(peek, err)
    dev = np.abs(x.astype(np.float64) - shadow)
    assert dev.max() <= float(peek["step"]) / 2 * (1 + 2.0 ** -20) and dev[1].max() == 2.0 ** -9
    assert (peek["codes"][2, :64] == np.arange(64) + 1).all() and (peek["codes"][2, 64:] == np.arange(64, DIM)).all()   # the nearer side
