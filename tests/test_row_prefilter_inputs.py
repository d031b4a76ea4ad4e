"""CPU tier: the inputs of tests/test_gpu_row_prefilter_tight.py (tests/row_prefilter.py: search_model and the gadget catalogue) are
what they are meant to be.  A gadget is a hand-made graph on which ONE decision of the row prefilter is the answer: the list is full,
its farthest entry f lies just above the probe row's f32 distance, and the probe's shadow distance is as far above its f32 distance
as the bound allows.  For every gadget: the model with the true bound answers as the oracle does; the model with the gadget's
mutation (half of E; E without the chosen element set; E of the last pack alone) answers with another id set; the probe is first
met on a full list; no two distances in play are equal; and E is the largest probe bound, nothing else."""
import numpy as np
import pytest

import row_prefilter as rp

NAMES = ([f"a_{d}" for d in rp.A_DIMS] + list(rp.B_SETS) + [f"c_m{m}" for m in rp.C_LISTS] + ["d_100"])


def test_every_gadget_of_the_catalogue_was_found():
    """No kind, dim, element set or list length may drop out silently: a seeded search that finds nothing is a finding."""
    cat = rp.catalogue()
    assert sorted(cat) == sorted(NAMES)
    assert [n for n in NAMES if cat[n] is None] == []
    assert [len(cat[f"c_m{m}"].gadgets) for m in rp.C_LISTS] == [len(v) for v in rp.C_LISTS.values()]
    assert all(len(cat[n].gadgets) == len(rp.A_STRETCHES) for n in NAMES if not n.startswith("c_"))
    lengths = sorted(len(gd.lists[0]) for m in rp.C_LISTS for gd in cat[f"c_m{m}"].gadgets)
    assert lengths == [3, 12, 20, 31, 40, 64, 64] and max(gd.k for gd in cat["c_m32"].gadgets) == 130


def _check_gadget(gi, j, ref, rows, levels, layers):
    gd = gi.gadgets[j]
    true = rp.search_model(rows, layers, levels, gi.entry, gd.q, gd.k, gi.e)
    mutated = rp.search_model(rows, layers, levels, gi.entry, gd.q, gd.k, gi.e_mut, gi.g_mut)
    ids, d = ref.knn_query(gd.q, gd.k)
    assert ids[0].tolist() == true["ids"] and d[0].tobytes() == true["dists"].tobytes(), gd.name
    p, f = gi.probe_id(j), gi.far_id(j)
    assert p in true["ids"] and f not in true["ids"], gd.name
    assert set(mutated["ids"]) != set(true["ids"]) and f in mutated["ids"] and p not in mutated["ids"], gd.name
    first = next(l for l in true["log"] if l["id"] == p)
    assert first["full"] and not first["away"] and first["far"] == true["d_x"][f], gd.name     # decided on a full list, against f
    assert next(l for l in mutated["log"] if l["id"] == p)["away"], gd.name
    # f lies in the middle half of (D_x(p), lb_mut) -- and so the true bound keeps p with room, the mutated one turns it away with room
    lo, hi = float(true["d_x"][p]), float(rp.lower_bound(true["d_h"][p], gi.e_mut, gi.dim, gi.g_mut))
    assert lo + 0.25 * (hi - lo) <= float(true["d_x"][f]) <= hi - 0.25 * (hi - lo), gd.name
    near = [gi.base[j] + i for i in range(gd.k - 1)]
    assert (true["d_x"][near] < true["d_x"][p]).all() and sorted(true["ids"]) == sorted(near + [p]), gd.name   # every other decoy is nearer than p
    met = sorted(set([l["id"] for l in true["log"]] + true["popped"]))
    assert len(set(true["d_x"][met].tolist())) == len(met), gd.name                           # no two distances in play are equal
    assert true["rows_reread"] < true["rows_on_shadow"] and mutated["rows_reread"] < true["rows_reread"], gd.name
    assert true["rows_reread_sure"] <= true["rows_reread"]
    return true


@pytest.mark.parametrize("name", [n for n in NAMES if n != "d_100"])
def test_the_model_answers_as_the_oracle_and_the_mutation_does_not(name):
    gi = rp.catalogue()[name]
    assert gi is not None, "no gadget found: see test_every_gadget_of_the_catalogue_was_found"
    ref = rp.oracle_of(gi)
    for j in range(len(gi.gadgets)):
        _check_gadget(gi, j, ref, gi.rows, gi.levels, gi.layers)


def test_e_is_the_largest_probe_bound_and_nothing_else():
    for name, gi in rp.catalogue().items():
        probes = np.stack([gd.p for gd in gi.gadgets])
        assert gi.e == rp.row_bounds(probes).max() and np.isfinite(gi.e) and gi.e > 1e-6, name
        others = np.ones(gi.rows.shape[0], dtype=bool)
        others[[gi.probe_id(j) for j in range(len(gi.gadgets))]] = False
        assert (rp.row_bounds(gi.rows[others]) <= np.float32(2e-37)).all(), name               # hub and decoys ARE binary16 values
        assert (rp.h(gi.rows[others]) == gi.rows[others]).all(), name
        if name.startswith("b_"):                                                             # the error sits on the chosen elements alone
            dim, elements = rp.B_SETS[name]
            off = np.setdiff1d(np.arange(dim), np.fromiter(elements, dtype=np.int64))
            assert (rp.h(probes)[:, off] == probes[:, off]).all() and (rp.h(probes) != probes).any(), name


def test_the_gadget_survives_an_add_of_binary16_rows_and_catches_e_of_the_last_pack():
    """(d): rows added after the first pack leave the lists of the gadget's decoys longer, not different in what they decide; E of
    those rows alone is E of binary16 values, with which the model answers with f."""
    gi = rp.catalogue()["d_100"]
    more = rp.added_rows(gi.dim)
    assert rp.e_of(more) == gi.e_mut <= np.float32(2e-37)
    ref = rp.oracle_of(gi, extra=more.shape[0])
    for j in range(len(gi.gadgets)):
        _check_gadget(gi, j, ref, gi.rows, gi.levels, gi.layers)
    ids = ref.add(more)
    assert ids.tolist() == list(range(gi.rows.shape[0], gi.rows.shape[0] + more.shape[0]))
    levels, layers = rp.graph_of(ref, gi.m)
    rows = np.concatenate([gi.rows, more])
    assert rp.e_of(rows) == gi.e and ref.entry_point == gi.entry
    for j in range(len(gi.gadgets)):
        _check_gadget(gi, j, ref, rows, levels, layers)


def test_no_input_can_tell_g_from_zero_in_the_kernels_form():
    """The g leg.  lb with g = 0 does exceed D_x on tight rows far out (stretch 5000; test_row_prefilter_model.py), by at most
    2e-7 of D_x -- but the kernel tests D_h > T, and T is raised by 2^-18 = 3.8e-6 for its own f32 roundings.  A gadget needs a
    farthest key above D_x(p) at which the mutated threshold turns p away; T grows with that key, so the smallest such key, the
    float after D_x(p), decides: with g = 0 no candidate probe is turned away there, so no gadget for g exists among them."""
    for dim in (128, 256):
        x, q = rp.worst_case(400, dim, 1100 + dim, 5000.0)
        d_x = np.array([rp._d32(x[i], q[i]) for i in range(x.shape[0])], dtype=np.float32)
        d_h = np.array([rp._d32(rp.h(x[i]), q[i]) for i in range(x.shape[0])], dtype=np.float32)
        e = rp.row_bounds(x)
        assert (rp.lower_bound(d_h, e, dim, g=0.0) > d_x.astype(np.float64)).any()            # the model's form: g matters
        assert not (d_h > rp.threshold(np.nextafter(d_x, np.float32(np.inf)), e, dim, g=0.0)).any()
