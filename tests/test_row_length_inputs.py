"""CPU tier: the inputs of the row-length tests are what the GPU tests assume (tests/row_lengths.py holds them and the rules).

* every chosen length hits the class its table names: chunk sequence, pitch, 1 KB rule, prefetch limit;
* the restated record sizes agree with the oracle's and with the library's own restatement of the int8 pitch;
* the LDS boundaries: where Add, the link launches and the queries stop fitting 64 KB -- and that no length admits Add while its
  link launch would exceed the budget (with the rule as it stood before, the gap is there: the last test shows it);
* the hand-made graphs have the list lengths they are made for, and no query of a pass case has two equal distances."""
import numpy as np
import pytest

import graph_reach_model as rm
import oracle
import row_lengths as rl
import wide_beams as wb


def test_f32_lengths_hit_their_chunk_sequences():
    for dim, (p8, p2) in rl.F32_LENGTHS.items():
        assert rl.pass8_chunks(dim) == p8, dim
        assert (rl.pass2_chunks(dim) if dim & 7 == 0 else None) == p2, dim
    seq2 = {d: c for d, (_, c) in rl.F32_LENGTHS.items() if c}
    assert seq2[192] == (1, 1, 0) and seq2[200] == (1, 1, 1) and seq2[248] == (1, 1, 7)        # a 16-chunk, the 8-chunk, 0 / 1 / 7 blocks
    assert seq2[136] == (1, 0, 1) and seq2[2056] == (16, 0, 1)                                  # no 8-chunk: singles right behind the 16s
    # a scalar tail behind a full chunk, and the 8-lane form under lat=2 for it
    assert [d for d, (p8, _) in rl.F32_LENGTHS.items() if p8[0] >= 1 and p8[2]] == [250, 257]
    assert not rl.two_lane_form("sq_euclid", 250) and not rl.two_lane_form("cosine", 257) and rl.two_lane_form("ucosine", 248)
    # either side of the 1 KB rule and of the prefetch limit (both at 256 words), and lengths far beyond
    for kind in rl.F32_KINDS:
        assert rl.novis_rule(kind, 256) and not rl.novis_rule(kind, 257)
        assert rl.prefetch_rule(kind, 256) and not rl.prefetch_rule(kind, 257)
        assert [rl.novis_rule(kind, d) for d in rl.F32_LENGTHS] == [True] * 6 + [False] * 3
    assert max(rl.F32_LENGTHS) > 768


def test_f16_lengths_hit_their_chunk_sequences():
    for dim, want in rl.F16_LENGTHS.items():
        assert rl.passh_chunks(dim) == want, dim
        assert rl.f16_row_words(dim) * 2 >= dim and rl.f16_row_words(dim) % 8 == 0
    got = set(rl.F16_LENGTHS.values())
    assert any(c[0] and c[1] for c in got)                       # an 8-pair chunk followed by the 4-pair chunk
    assert any(c[0] and c[1] and c[2] == 3 and c[3] and c[4] for c in got)     # ... by single pairs, the odd block and a tail
    assert any(c[0] == 3 and not c[1] and c[3] for c in got)     # 8-pair chunks and the odd block alone
    assert rl.two_lane_form("sq_euclid_f16", 232) and not rl.two_lane_form("ucosine_f16", 250)
    assert rl.novis_rule("sq_euclid_f16", 250) and not rl.novis_rule("sq_euclid_f16", 392)      # the QUERY's words decide (pitch_: f32)


def test_int8_lengths_sit_on_both_sides_of_each_pitch_step():
    for dim, pitch in rl.I8_LENGTHS.items():
        assert rl.i8_pitch(dim) == pitch == oracle.lib().orc_i8_pitch(dim), dim
        assert pitch % 16 == 0 and (pitch - 2) * 4 >= dim
    compiled = {d: rl.i8_blocks(d) for d in rl.I8_LENGTHS}
    assert compiled[120] == (4, True) and compiled[121] == (6, True) and compiled[184] == (6, True)
    assert compiled[185] == (8, False) and min(d for d, (_, c) in compiled.items() if not c) == 185
    assert rl.i8_pitch(184) != rl.i8_pitch(185) and rl.i8_pitch(248) != rl.i8_pitch(249) and rl.i8_pitch(120) != rl.i8_pitch(121)
    assert rl.novis_rule(rl.I8_KIND, 1016) and not rl.novis_rule(rl.I8_KIND, 1017)
    assert rl.prefetch_rule(rl.I8_KIND, 1016) and not rl.prefetch_rule(rl.I8_KIND, 1017)
    assert rl.I8_SHIFTED in rl.I8_LENGTHS and not rl.i8_blocks(rl.I8_SHIFTED)[1]
    assert all(not rl.i8_blocks(d)[1] for d in rl.INDEX_LENGTHS["i8"])           # every index build runs the run-time-length pass
    assert len(rl.pass_cases()) == 3 * 9 + 2 * 6 + 10 + 1


def test_index_lengths_are_lengths_of_the_tables_and_fit_the_device():
    for kind in rl.ROW_KINDS:
        assert set(rl.index_lengths(kind)) <= set(rl.lengths_of(kind)), kind
        for dim in rl.index_lengths(kind):
            assert rl.add_fits(kind, dim, rl.INDEX_M, rl.INDEX_EFC) and rl.query_fits(kind, dim, rl.INDEX_M, 40), (kind, dim)
            assert rl.remove_fits(kind, dim, rl.INDEX_M) == (dim <= 2048), (kind, dim)
    assert 2 * rl.INDEX_M + 1 > 24                                # layer-0 lists pass 24 ids
    for dim in rl.WIDE_LENGTHS:                                   # the 8-set insert kernel, below the MFMA threshold, no 128-multiple
        assert wb.sets_for(rl.WIDE_EFC) == 8 and dim < 256 and dim % 128 and rl.add_fits("sq_euclid", dim, rl.INDEX_M, rl.WIDE_EFC)
    for dim in rl.REMOVE_DIMS:
        for kind in ("sq_euclid", rl.I8_KIND):
            assert rl.remove_fits(kind, dim, 16) == (dim == 2048) and rl.add_fits(kind, dim, 16, 100) and rl.query_fits(kind, dim, 16, 10)


def test_plan_of_the_pass_graphs():
    """The forms the pass tests assert from stats(): a beam over the full graph runs on eight register sets (no lean form), a beam
    over a lean graph on four; the latency form may always run there (12 jobs, lists of up to 64 ids)."""
    n_full = rl.hub_graph(rl.HUB_LISTS)[0]
    assert n_full == 327 and wb.sets_for(n_full) == 8
    for lists in rl.LEAN_LISTS:
        n = rl.hub_graph(lists)[0]
        assert 128 < n <= 256 and wb.sets_for(n) == 4
    assert set(rl.HUB_LISTS) == set(rl.LEAN_LISTS[0]) | set(rl.LEAN_LISTS[1])
    for kind, dim, _ in rl.pass_cases():
        novis = rl.novis_rule(kind, dim)
        for n in (n_full, rl.hub_graph(rl.LEAN_LISTS[0])[0]):
            lean_able = wb.sets_for(n) <= 4
            p = rl.search_plan(kind, dim, n, rl.GRAPH_M)
            assert p["lat_ok"] and p["form"] == "lat" and p["lds"] + rl.TEAM_LDS <= rl.LDS_BUDGET, (kind, dim, n)
            assert rl.search_plan(kind, dim, n, rl.GRAPH_M, {"lat": 0})["form"] == ("lean" if novis and lean_able else "plain")
            assert rl.search_plan(kind, dim, n, rl.GRAPH_M, {"lat": 0, "lean": 0})["form"] == "plain"
            assert rl.search_plan(kind, dim, n, rl.GRAPH_M, {"lat": 0, "lean": 0})["novis"] == novis
            p = rl.search_plan(kind, dim, n, rl.GRAPH_M, {"sorted_top": 0})
            assert p["exact_only"] and not p["lat_ok"] and p["form"] == "plain"
            p = rl.search_plan(kind, dim, n, rl.GRAPH_M, {"novis": 0, "lat": 0})
            assert not p["novis"] and p["form"] == "plain"


@pytest.mark.parametrize("lists", [rl.HUB_LISTS, *rl.LEAN_LISTS], ids=["full", "lean0", "lean1"])
def test_hub_graph_has_the_lists_it_is_made_for(lists):
    n, lv, layers = rl.hub_graph(lists)
    counts, edges = layers[0]
    h = len(lists)
    assert counts[:h].tolist() == list(lists) and (counts[h:] == 1).all() and (lv == 0).all()
    assert edges.shape == (n, 2 * rl.GRAPH_M + 2) and max(lists) <= 2 * rl.GRAPH_M
    seen = {0}
    for i in range(n):
        lst = edges[i, :counts[i]].tolist()
        assert len(set(lst)) == len(lst) and i not in lst and all(0 <= v < n for v in lst)
        if i < h:
            seen.update(lst)
    assert seen == set(range(n))                                  # every node is in a hub's list: the walk from id 0 reaches all


def test_no_query_of_a_pass_case_has_two_equal_distances():
    """... over the nodes of the full graph, of which the lean graphs use a prefix: every list of the tests is strictly ascending,
    so that the order of the answers is decided by the distances alone."""
    n = rl.hub_graph(rl.HUB_LISTS)[0]
    ids = np.arange(n, dtype=np.int32)
    for kind, dim, shifted in rl.pass_cases():
        x, q = rl.pass_rows(kind, dim, shifted)                   # (raises where none of its seeds is free of ties)
        assert x.shape == (n, dim) and q.shape == (rl.NQ, dim)
        rows = wb.oracle_rows(kind, x)
        for qi in q:
            d = oracle.dist_query_rows(wb.base_metric(kind), rows, qi, ids)
            assert np.isfinite(d).all() and np.unique(d).size == n, (kind, dim, shifted)
    x, _ = rl.pass_rows(rl.I8_KIND, rl.I8_SHIFTED, True)
    assert (oracle.i8_quantize(x)[0] < 0).any()


# ---- LDS boundaries ----------------------------------------------------------------------------------------------------------------
PARENT = {(8, 40): (5324, 5340), (8, 4): (5348, 5340), (63, 1): (5204, 4992)}    # (Add fits up to, link LDS <= 64 KB up to) before the link term


def test_lds_boundaries_before_the_link_term():
    """The rule as it stood (link_term=False): Add admitted past the link launches' budget for (8, 4) and (63, 1), not for (8, 40)."""
    for (m, efc), (add_to, link_to) in PARENT.items():
        got = rl.lds_boundaries(m, efc, 10, link_term=False)
        assert got[:2] == (add_to, link_to), ((m, efc), got)
    gap = {me: [d for d in range(4, 6001) if rl.add_fits("sq_euclid", d, *me, link_term=False) and not rl.link_fits("sq_euclid", d, me[0])]
           for me in PARENT}
    assert gap[8, 40] == [] and gap[8, 4] == list(range(5341, 5349)) and gap[63, 1] == list(range(4993, 5205))
    assert [d for d in gap[8, 4] if d % 4 == 0] == [5344, 5348] and min(d for d in gap[63, 1] if d % 4 == 0) == 4996


@pytest.mark.parametrize("m,efc", [(8, 40), (8, 4), (63, 1), (16, 100)])
def test_no_length_admits_add_past_the_link_budget(m, efc):
    """With the link launches' LDS in traversal_fits, no length in 4 .. 6000 admits Add while a link launch would exceed 64 KB --
    for the float rows, the f16 rows (same LDS: the query is f32) and the int8 records of the same pitch."""
    for kind in ("sq_euclid", "ucosine_f16"):
        assert [d for d in range(4, 6001) if rl.add_fits(kind, d, m, efc) and not rl.link_fits(kind, d, m)] == []
    assert [d for d in range(4, 24001, 3) if rl.add_fits(rl.I8_KIND, d, m, efc) and not rl.link_fits(rl.I8_KIND, d, m)] == []
    add_to, link_to, _ = rl.lds_boundaries(m, efc, 10)
    assert add_to <= link_to
    if (m, efc) in PARENT:
        assert add_to == min(PARENT[m, efc])


def test_lengths_at_the_lds_budget_sit_on_the_edges():
    """The lengths of test_gpu_row_length_lds.py are the last / first lengths of each side, in steps of 4 elements."""
    k = rl.LDS_K
    add_to, link_to, query_to = rl.lds_boundaries(8, 40, k)
    assert (add_to, query_to) == (5324, 5380) and rl.LDS_CASES[8, 40] == (add_to, add_to + 4, query_to, query_to + 4)
    for kind in rl.LDS_KINDS:
        fits = [(rl.add_fits(kind, d, 8, 40), rl.query_fits(kind, d, 8, k), rl.query_fits(kind, d, 8, 1)) for d in rl.LDS_CASES[8, 40]]
        assert fits == [(True, True, True), (False, True, True), (False, True, True), (False, False, False)], kind
    add_to, link_to, query_to = rl.lds_boundaries(8, 4, k)
    assert add_to == link_to == 5340 and rl.LDS_CASES[8, 4] == (5340, 5344, 5348, 5352)
    assert [rl.add_fits("sq_euclid", d, 8, 4) for d in rl.LDS_CASES[8, 4]] == [True, False, False, False]
    assert [rl.add_fits("sq_euclid", d, 8, 4, link_term=False) for d in rl.LDS_CASES[8, 4]] == [True, True, True, False]
    assert all(rl.query_fits("sq_euclid", d, 8, k) for d in rl.LDS_CASES[8, 4])
    add_to, link_to, query_to = rl.lds_boundaries(63, 1, k)
    assert add_to == link_to == 4992 and rl.LDS_CASES[63, 1] == (4992, 4996)
    assert rl.add_fits("sq_euclid", 4996, 63, 1, link_term=False) and all(rl.query_fits("sq_euclid", d, 63, k) for d in rl.LDS_CASES[63, 1])
    # int8: pitch 5376 is the last record with device queries at M 8 (and far past Add's), four words more is the first without
    a, b = rl.LDS_I8_DIMS
    assert rl.i8_pitch(a) == 5376 and rl.i8_pitch(b) == 5392 and b == a + 16
    assert rl.query_fits(rl.I8_KIND, a, 8, k) and not rl.query_fits(rl.I8_KIND, b, 8, k) and not rl.query_fits(rl.I8_KIND, b, 8, 1)
    assert not rl.add_fits(rl.I8_KIND, a, 8, 40)
    assert rl.LDS_N * max(rl.LDS_I8_DIMS) * 4 < 32 << 20          # the largest upload of the suite's new tests: 300 rows of 21 506 floats


def test_which_host_only_graphs_have_a_node_to_repair():
    """The cases of test_gpu_row_length_lds.py in which everything runs on the host are exactly LDS_HOST_ONLY's, and the oracle's
    graph of each (batches of LDS_CAP items, so the same on every host) leaves that many nodes of layer 0 unreached from the entry
    point, none above: the GPU test holds the repair of the one and the untouched hash of the others to it."""
    cases = [(kind, m, efc, dim) for (m, efc), dims in rl.LDS_CASES.items() for dim in dims for kind in rl.LDS_KINDS]
    cases += [(rl.I8_KIND, 8, 40, dim) for dim in rl.LDS_I8_DIMS]
    assert {c for c in cases if not rl.query_fits(c[0], c[3], c[1], rl.LDS_K)} == set(rl.LDS_HOST_ONLY)
    assert sorted(rl.LDS_HOST_ONLY.values()) == [0, 0, 1]
    for (kind, m, efc, dim), lost in rl.LDS_HOST_ONLY.items():
        x, _ = rl.lds_rows(kind, dim)
        ref = oracle.OracleIndex(dim, wb.base_metric(kind), max_edges=m, max_candidates=efc, min_nn=5, collection_size=rl.LDS_N)
        ref.add_batched(wb.oracle_rows(kind, x), rl.LDS_CAP, threads=8)
        lv = ref.levels()
        hops = rm.reach_chain(lv, np.ones(lv.size, bool), wb.oracle_layers(ref, lv, m), ref.entry_point)[2]
        assert [rm.unreachable_ids(hops[layer]).size for layer in sorted(hops)] == [lost] + [0] * (len(hops) - 1), (kind, dim)
