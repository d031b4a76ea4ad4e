"""CPU tier: the inputs of tests/test_gpu_wide_beams.py do what that file relies on, checked against the oracle alone -- so the GPU
tests cannot pass vacuously.  The tie case must put an equal pair of distances across the edge of two register sets (positions
64t - 1 and 64t of the result list, and nowhere else in it) for enough queries at every beam the GPU tests run; the plain case
must meet equal distances rarely enough for the cap on search_repeats to mean that the wide form answered."""
import numpy as np
import pytest

import wide_beams as wb


@pytest.mark.parametrize("beam,sets", [(1, 2), (64, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 0)])
def test_sets_for_restates_sorted_top_sets(beam, sets):
    assert wb.sets_for(beam) == sets


def test_every_beam_of_the_gpu_tests_names_its_set_count():
    assert [wb.sets_for(b) for b in wb.EDGE_BEAMS] == [2, 4, 4, 8, 8, 0]
    assert [wb.sets_for(b) for b in wb.FORM_BEAMS] == [4, 8]
    assert [wb.sets_for(b) for b in wb.TIE_BEAMS] == [4, 8, 8]
    assert wb.sets_for(wb.PREFIX_BEAM) == 8 and 64 < wb.PREFIX_K <= 128      # the prefix ends inside set 1: only the edge 63|64 lies in it


def test_straddling_only_counts_one_pair_at_a_set_edge():
    d = np.arange(4 * 200, dtype=np.float32).reshape(4, 200)
    d[0, 64] = d[0, 63]                          # across 63|64
    d[1, 128] = d[1, 127]; d[1, 10] = d[1, 9]    # a second pair elsewhere: not "only"
    d[2, 65] = d[2, 64]                          # inside a set
    d[3, 128] = d[3, 127]                        # across 127|128
    assert wb.straddling_only(d).tolist() == [True, False, False, True]
    assert wb.straddling_only(d, 100).tolist() == [True, False, False, False]
    assert wb.straddling_only(d, 64).tolist() == [False, False, False, False]   # position 64 is outside a prefix of 64


@pytest.mark.parametrize("metric", wb.ROW_KINDS)
def test_builders_are_fixed_and_the_tie_case_differs_in_six_rows(metric):
    x, q = wb.plain_case(metric)
    t, tq = wb.tie_case(metric)
    assert x.shape == (wb.N, wb.DIM) and q.shape == (wb.NQ, wb.DIM) and x.dtype == np.float32
    assert q.tobytes() == tq.tobytes()
    a, b = wb.duplicate_pairs()
    assert len(set(a.tolist()) | set(b.tolist())) == 2 * wb.N_PAIRS
    changed = np.flatnonzero((x != t).any(axis=1))
    assert sorted(changed.tolist()) == sorted(a.tolist())
    assert t[a].tobytes() == t[b].tobytes()
    # rounding to binary16 keeps the copies equal
    assert wb.oracle_rows(metric, t)[a].tobytes() == wb.oracle_rows(metric, t)[b].tobytes()
    if wb.base_metric(metric) == "ucosine":
        assert np.allclose((x.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)
    for dim in (wb.DIM_TAIL, wb.DIM_F16_ODD):
        assert wb.plain_case(metric, dim=dim, nq=8)[0].shape == (wb.N, dim)


@pytest.fixture(scope="module")
def tie_lists():
    """The oracle's result lists of the tie case, k = the widest beam of each graph search, per metric: {(metric, beam): dists}."""
    out = {}
    for metric in ("sq_euclid", "ucosine"):
        x, q = wb.tie_case(metric)
        ref = wb.query_oracle(metric, x)
        for beam in wb.TIE_BEAMS:
            out[(metric, beam)] = ref.knn_query(q, beam, threads=8)[1]
    return out


@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_tie_case_puts_ties_across_set_edges_at_every_beam(tie_lists, metric):
    counts = {beam: int(wb.straddling_only(tie_lists[(metric, beam)]).sum()) for beam in wb.TIE_BEAMS}
    print(f"straddling-only queries, {metric}: {counts}")
    assert all(c >= wb.MIN_STRADDLING for c in counts.values()), counts


@pytest.mark.parametrize("metric", ["sq_euclid", "ucosine"])
def test_tie_case_puts_ties_across_the_first_edge_of_the_prefix(tie_lists, metric):
    # k_out = 100 under beam 300: OrderBy + Take(100) of the beam-300 list
    c = int(wb.straddling_only(tie_lists[(metric, wb.PREFIX_BEAM)], wb.PREFIX_K).sum())
    print(f"straddling-only queries in the first {wb.PREFIX_K} of beam {wb.PREFIX_BEAM}, {metric}: {c}")
    assert c >= wb.MIN_STRADDLING_PREFIX


@pytest.mark.parametrize("metric", wb.ROW_KINDS)
def test_plain_case_meets_equal_distances_rarely(metric):
    # by brute force over all rows: the 600 nearest cover every beam of the GPU tests (the widest is 513).  A query can hand its
    # search to the exact traversal only if it meets a tie, so this share bounds search_repeats / jobs from above.
    x, q = wb.plain_case(metric, nq=1000 if metric == "sq_euclid_i8" else wb.NQ)   # (the int8 metric quantises the rows per call)
    lists = wb.brute_force_lists(metric, wb.oracle_rows(metric, x), q, wb.TIE_WINDOW)
    share = wb.any_tie_share(lists)
    print(f"share of queries with an equal pair among their {wb.TIE_WINDOW} nearest rows, {metric}: {share:.3f}")
    assert share <= wb.REPEAT_CAP_SHARE
