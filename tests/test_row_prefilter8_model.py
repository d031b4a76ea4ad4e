"""CPU tier: the bound of the 8-bit row prefilter (tests/row_prefilter8.py).  lb(D_8) must not exceed the oracle's f32
distance of the real row -- on uniform rows, on rows that ARE grid values (E8 at its floor), on rows clamped after a partial repack,
and on the worst-case family q = h8 + stretch (x - h8), where the triangle bound holds with equality.  On gadgets built from that
family (row_prefilter8.catalogue8) the model with E8 halved turns a true neighbour away and answers wrongly: the inputs of the GPU
test can tell a wrong bound."""
import numpy as np
import pytest

import oracle
import row_prefilter8 as r8

DIM = r8.DIM


def _dists(rows, q):
    ids = np.arange(rows.shape[0], dtype=np.int32)
    return np.stack([oracle.dist_query_rows("sq_euclid", np.ascontiguousarray(rows, dtype=np.float32), qi, ids, use_avx=True) for qi in q])


def _check(x, shadow, e8, q):
    """lb(D_8, E8) <= D_x for every (query, row) pair; -> the largest lb / D_x seen."""
    d_x, d_8 = _dists(x, q), _dists(shadow, q)
    lb = r8.lower_bound(d_8, e8, DIM)
    assert (lb <= d_x.astype(np.float64)).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(d_x > 0, lb / d_x, 0.0)))


def test_the_decoded_value_is_one_rounding_of_step_c_plus_lo():
    lo, step = np.float32(-0.37), np.float32(0.0123456)
    tab = r8.table(lo, step)
    exact = np.float64(step) * np.arange(256) + np.float64(lo)          # (24 + 8 bits: the double product is exact; the sum nearly always)
    assert np.abs(tab.astype(np.float64) - exact).max() <= np.spacing(np.abs(tab).max()) / 2 + 1e-12
    assert (np.diff(tab) > 0).all() and tab[0] == lo


def test_the_grid_covers_the_rows_and_handles_negative_elements():
    x = (np.random.default_rng(1).random((500, DIM), dtype=np.float32) * np.float32(3.0) - np.float32(2.0))
    lo, step, codes, shadow, e8 = r8.pack(x)
    assert lo == x.min() and np.float64(step) * 255 >= np.float64(x.max()) - np.float64(lo)
    assert np.abs(x.astype(np.float64) - shadow).max() <= float(step) / 2 * (1 + 2.0 ** -20)
    assert r8.grid_of(np.full((3, DIM), 0.25, np.float32)) == (np.float32(0.25), np.float32(1.0))      # hi == lo: any positive step
    bad = x.copy(); bad[7, 3] = np.inf; bad[8, 4] = np.nan
    assert r8.grid_of(bad) == (lo, step) and r8.pack(bad)[4] == np.inf   # the grid from the finite elements; E8 = +inf


def test_uniform_rows():
    x = np.random.default_rng(2).random((1500, DIM), dtype=np.float32)
    q = np.random.default_rng(3).random((24, DIM), dtype=np.float32)
    lo, step, codes, shadow, e8 = r8.pack(x)
    print(f"uniform: step {step}, E8 {e8}, largest lb / D_x {_check(x, shadow, e8, q):.4f}")
    assert 0.010 < e8 < 0.020                                            # step sqrt(128 / 12) = 0.0128 on average


def test_rows_that_are_grid_values():
    x = np.random.default_rng(4).random((800, DIM), dtype=np.float32)
    x[0, 0], x[0, 1] = 0.0, 1.0
    lo, step, codes, _, _ = r8.pack(x)
    y = r8.decode(codes, lo, step)                                       # grid values of the same grid (its ends are elements of row 0)
    lo2, step2, codes2, shadow2, e8 = r8.pack(y)
    assert (lo2, step2) == (lo, step) and (codes2 == codes).all() and shadow2.tobytes() == y.tobytes()
    assert e8 <= 1e-36                                                   # the floor: 0 raised by 1e-37
    q = np.random.default_rng(5).random((16, DIM), dtype=np.float32)
    _check(y, shadow2, e8, q)


def test_rows_clamped_after_a_partial_repack():
    x = np.random.default_rng(6).random((1000, DIM), dtype=np.float32)
    lo, step, _, shadow, e0 = r8.pack(x)
    more = np.random.default_rng(7).random((50, DIM), dtype=np.float32)
    more[3, 10], more[4, 20] = 1.5, -0.5                                 # outside the grid of the first pack
    _, _, codes, shadow_more, e_more = r8.pack(more, (lo, step))
    assert codes[3, 10] == 255 and codes[4, 20] == 0 and e_more > 0.45   # clamped: the bound grows to the overshoot
    e8 = max(e0, e_more)                                                 # E8 only grows until a full repack
    q = np.concatenate([np.random.default_rng(8).random((12, DIM), dtype=np.float32), more[3:5]])
    _check(np.concatenate([x, more]), np.concatenate([shadow, shadow_more]), e8, q)


@pytest.mark.parametrize("stretch", [2.0, 4.0, 50.0, 5000.0])
def test_the_worst_case_family_meets_the_bound_and_half_of_e8_breaks_it(stretch):
    x = np.random.default_rng(9).random((300, DIM), dtype=np.float32)
    _, _, _, shadow, e8 = r8.pack(x)
    q = r8.worst_case8(x, shadow, stretch)
    ids = np.arange(x.shape[0], dtype=np.int32)
    d_x = np.array([oracle.dist_query_rows("sq_euclid", x, q[i], ids[i:i + 1], use_avx=True)[0] for i in range(x.shape[0])])
    d_8 = np.array([oracle.dist_query_rows("sq_euclid", shadow, q[i], ids[i:i + 1], use_avx=True)[0] for i in range(x.shape[0])])
    per_row = r8.row_bounds8(x, shadow)
    assert (r8.lower_bound(d_8, per_row, DIM) <= d_x).all() and (r8.lower_bound(d_8, e8, DIM) <= d_x).all()
    tight = r8.lower_bound(d_8, per_row, DIM) / d_x
    print(f"stretch {stretch}: lb / D_x with the row's own bound in [{tight.min():.6f}, {tight.max():.6f}]")
    assert tight.min() > 0.99                                            # equality up to the roundings
    assert (r8.lower_bound(d_8, 0.5 * per_row.astype(np.float64), DIM) > d_x).all()   # half the bound is wrong for every row


@pytest.mark.parametrize("m", sorted(r8.C_LISTS8))
def test_gadgets_the_model_is_the_oracle_and_with_half_of_e8_it_is_not(m):
    gi = r8.catalogue8(m)
    assert gi is not None, "the seeded search found no gadgets"
    ref = oracle.OracleIndex(DIM, "sq_euclid", max_edges=m, min_nn=1, collection_size=gi.rows.shape[0], allow_removals=False)
    ref.import_graph(gi.rows, gi.levels, gi.entry, gi.layers)
    for j, gd in enumerate(gi.gadgets):
        want_ids, want_d = ref.knn_query(gd.q.reshape(1, -1), gd.k)
        good, bad = gi.model8(j), gi.model8(j, e=np.float32(0.5) * gi.e8)
        assert good["ids"] == want_ids[0].tolist() and good["dists"].tobytes() == want_d[0].tobytes(), gd.name
        assert gi.probe_id(j) in good["ids"] and gi.far_id(j) not in good["ids"], gd.name
        assert gi.probe_id(j) not in bad["ids"] and gi.far_id(j) in bad["ids"], gd.name        # a true neighbour turned away
        assert len(set(good["dists"].tolist())) == gd.k, gd.name        # no equal distances: the sorted traversal answers
        assert len(gd.lists[0]) == dict(r8.C_LISTS8[m])[gd.k], gd.name  # d1's list: the pass width under test
