"""GPU tier: the MFMA Gram-tile prefilter of the neighbour heuristic (relative_neighbor_pruning<METRIC, MFMA = true>, csrc/dk_heuristic.h,
DESIGN.md 3.4) where its rounding bound is tight and at the edges of its block loop.

The tiles settle `dist(s, c) < c.Dist` only when the approximate margin exceeds E; everything else goes back to the exact kernels.
On i.i.d. uniform rows the two sums agree 25 to 50 times better than E, so a margin of zero would pass there.  The rows of
tests/gram_prefilter.py do not forgive that: unit rows that round in one direction (a fifth to nine tenths of their comparisons are
inside the margin), a cluster far from the origin, norms that overflow, bit-copies and one-ulp neighbours of accepted rows, integer
grids, accepted lists of up to 126 ids (four tiles), candidate lists of every length, and long rows scattered among unit rows.
tests/test_gram_prefilter_inputs.py checks on the CPU that the rows do what is said here.

Every case builds with the prefilter allowed (mfma=1) and forbidden (mfma=0); both legs must end in the oracle's graph hash, levels
and entry point and answer a 100-query knn_query with its ids and distance bytes.  And the form must have been taken when the
rule says so: the tile form counts rows streamed per tile, the exact forms count pairs, so insert_evals of an eligible case
differs between its legs, and that of an ineligible case does not."""
import numpy as np
import pytest

import gram_prefilter as gp
import oracle
import wide_beams as wb
from common import set_diag

pytestmark = pytest.mark.gpu

NQ = 100


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


_REFS = {}


def _oracle(case, schedule):
    """The oracle's graph of a case under a schedule and its answer to the case's queries, once per module."""
    key = (case.id, schedule)
    if key not in _REFS:
        x = wb.oracle_rows(case.metric, case.rows())
        ref = oracle.OracleIndex(case.dim, wb.base_metric(case.metric), max_edges=case.M, max_candidates=case.efc, collection_size=case.n)
        gp.add_by_schedule(ref, x, schedule, threads=8)
        q = gp.queries(case.rows(), NQ)
        _REFS[key] = (ref, q, ref.knn_query(q, 10, threads=8))
    return _REFS[key]


def _leg(Index, monkeypatch, case, schedule, mfma):
    """One build on the device under mfma=<mfma>, held against the oracle; returns insert_evals of the whole build."""
    ref, q, want = _oracle(case, schedule)
    x = case.rows()
    set_diag(monkeypatch, mfma=mfma)
    ix = Index(case.dim, case.metric)
    ix.set_collection_size(case.n); ix.set_max_edges(case.M); ix.set_max_candidates(case.efc)
    ix.set_insert_batch(1 if schedule == "seq" else gp.BATCH)
    if schedule == "calls":
        ix.add(x[:case.n - 400])
        with monkeypatch.context() as small:            # the latency insert form for the small calls (and for them alone)
            set_diag(small, lat=2)
            for i in range(case.n - 400, case.n, 40):
                ix.add(x[i:i + 40])
    else:
        ix.add(x)
    st = ix.stats()
    assert ix.graph_hash() == ref.graph_hash(), (case.id, schedule, mfma)
    assert ix.levels().tolist() == ref.levels().tolist() and ix.entry_point == ref.entry_point
    ids, d = ix.knn_query(q, 10)
    assert (ids == want[0]).all(), (case.id, schedule, mfma)
    if case.group == "nan":
        # Known difference, outside the heuristic: knn_query reports a distance to a NaN row as 0xFFC00000 where the oracle has
        # 0x7FC00000 (the sign of a NaN).  The places of the NaNs and every other distance byte must still be the oracle's.
        isn = np.isnan(want[1])
        assert (np.isnan(d) == isn).all() and d[~isn].tobytes() == want[1][~isn].tobytes(), (case.id, schedule, mfma)
    else:
        assert d.tobytes() == np.ascontiguousarray(want[1]).tobytes(), (case.id, schedule, mfma)
    if schedule == "calls":
        assert st["lat_launches"] > 0
    return st["insert_evals"]


def _both_legs(Index, monkeypatch, case, schedule):
    on = _leg(Index, monkeypatch, case, schedule, 1)
    off = _leg(Index, monkeypatch, case, schedule, 0)
    print(f"{case.id} {schedule}: insert_evals {on} with the tiles allowed, {off} without")
    if case.eligible():
        assert gp.prefilter_applies(case.metric, case.dim, case.efc)
        assert on != off, (case.id, on)                 # equal counters: not one tile ran
    else:
        assert not gp.prefilter_applies(case.metric, case.dim, case.efc)
        assert on == off, (case.id, on, off)


def _params(cases):
    return [pytest.param(c, s, id=f"{c.id}-{s}") for c in cases for s in c.schedules]


@pytest.mark.parametrize("case,schedule", _params([c for c in gp.CASES if c.group == "tight"]))
def test_rows_that_round_one_way_far_from_the_origin_or_past_the_range(Index, monkeypatch, case, schedule):
    """biased: a fifth (dim 256) to nine tenths (dim 768) of the comparisons inside E, and a margin of E / 8 wrong on hundreds of them
    under the chain model.  offset_cluster: Esq (n_i + n_j) swamps every distance.  overflow: norms of 8e37 and of inf (d is NaN)."""
    _both_legs(Index, monkeypatch, case, schedule)


@pytest.mark.parametrize("case,schedule", _params([c for c in gp.CASES if c.group == "ties"]))
def test_exact_ties_in_front_of_the_tiles(Index, monkeypatch, case, schedule):
    """dist(s, c) == c.Dist bit for bit (the exact test says "not closer", the tile's number lands on either side), and equal pairs in
    the candidate lists: the insert goes to the exact traversal, which hands the heuristic an unsorted list of 300."""
    _both_legs(Index, monkeypatch, case, schedule)


@pytest.mark.parametrize("case,schedule", _params([c for c in gp.CASES if c.group == "accepted"]))
def test_accepted_lists_of_two_three_and_four_tiles(Index, monkeypatch, case, schedule):
    """M 40 and M 63 (layer 0 keeps 80 and 126 ids) at efc 512 and 257: a0 = 32, 64, 96, partial tiles, nacc / snacc positions past 64."""
    _both_legs(Index, monkeypatch, case, schedule)


@pytest.mark.parametrize("case,schedule", _params([c for c in gp.CASES if c.group == "ragged"]))
def test_every_candidate_count_of_a_sequential_build(Index, monkeypatch, case, schedule):
    """400 rows one at a time at efc 300: the candidate count takes every value from 1 to 300 -- the `n < max_edges` return, every
    bsz of the last block."""
    _both_legs(Index, monkeypatch, case, schedule)


@pytest.mark.parametrize("case,schedule", _params([c for c in gp.CASES if c.group == "mixed"]))
def test_long_rows_scattered_among_unit_rows(Index, monkeypatch, case, schedule):
    """5 % of the rows longer than 1: their blocks take the exact-only loop, the others the tiles, and at M = 8 the list fills inside
    such a block."""
    _both_legs(Index, monkeypatch, case, schedule)


@pytest.mark.parametrize("case,schedule", _params([c for c in gp.CASES if c.group == "nan"]))
def test_rows_with_a_nan_element(Index, monkeypatch, case, schedule):
    """Three rows with one NaN element each, which the oracle's build accepts: every distance to them is NaN, on the tiles too."""
    _both_legs(Index, monkeypatch, case, schedule)


@pytest.mark.parametrize("case,schedule", _params(gp.EDGE_CASES))
def test_the_rules_edges_take_no_tile(Index, monkeypatch, case, schedule):
    """dim 248 (below 256), dim 260 (no multiple of 8), efc 256 (four register sets), half-precision rows: same counters on both legs."""
    _both_legs(Index, monkeypatch, case, schedule)
