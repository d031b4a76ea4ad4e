"""CPU tier: the inputs of tests/test_gpu_gram_prefilter.py do what that file relies on, checked against the oracle and the chain model
alone (tests/gram_prefilter.py) -- so that the GPU tests cannot pass vacuously.

Per case the oracle is built at the case's own M and efc; its last 200 rows are added one by one, and before each Add the heuristic
calls of that Add are restated (insert_traces -> prune_trace) and, after it, compared with the edges the oracle gave the row: that
pins prune_trace.  What the traces must then show: on the rounding-biased families the kernel's margin decides nothing wrongly
under the chain model while an eighth of it, and none, do (20 is a floor against vacuity, not a measurement); on the tie families
dist(s, c) == c.Dist bit for bit, and equal pairs in the candidate lists (the route through the exact traversal into an unsorted
list); accepted lists past 32, 64 and 96 ids; blocks of 32 candidates that mix long and unit rows.  The share of comparisons
inside the margin is printed per case (DESIGN.md 3.4 holds the table)."""
import numpy as np
import pytest

import gram_prefilter as gp
import oracle
import wide_beams as wb

FLOOR = 20
# offset_cluster: 100 + 0.01 noise puts EVERY comparison inside Esq (n_i + n_j) / 8 (about 23 against distances of 0.05 and a chain
# error of a few units), so an eighth of the margin decides nothing at all there, rightly or wrongly; what that family holds is the
# other end: a margin that forgets the norms (0, or the bare E) is wrong about every second comparison.  DESIGN.md 3.4 says so.
EIGHTH_FLOOR = {"offset_cluster": 0}
CHAIN_EVERY = {"tight": 1, "ragged": 1}       # the other groups print a share only: every fifth sampled row is enough for it

_SUMMARY = {}


def summary(case):
    if case.id in _SUMMARY:
        return _SUMMARY[case.id]
    x, n, metric = case.rows(), case.n, case.metric
    ref = oracle.OracleIndex(case.dim, metric, max_edges=case.M, max_candidates=case.efc, collection_size=n)
    if case.schedules == ("seq",):
        ref.add(x[:n - gp.SAMPLE])
    else:
        ref.add_batched(x[:n - gp.SAMPLE], gp.BATCH, threads=8)
    every = CHAIN_EVERY.get(case.group, 5)
    long = gp.long_rows(x)
    s = dict(comparisons=0, modelled=0, wrong=0, wrong8=0, wrong0=0, inside=0, ties=0, tie_rows=0, accepted=[], mixed_blocks=0, calls=0,
             short_calls=0, sizes=set(), full_in_mixed=0, nan=0)
    for i in range(n - gp.SAMPLE, n):
        traces = gp.insert_traces(ref, metric, x, i, case.M, case.efc, chain=i % every == 0)
        assert ref.add(x[i:i + 1]).tolist() == [i]
        for layer, t in traces.items():
            assert ref.edges(i, layer).tolist() == t.accepted.tolist(), (case.id, i, layer)   # prune_trace IS the oracle's heuristic
            s["sizes"].add(t.n)
            if t.n < t.max_edges:
                s["short_calls"] += 1
                continue
            s["calls"] += 1
            s["comparisons"] += t.d_exact.size
            s["nan"] += int((np.isnan(t.d_exact) | np.isnan(t.thr)).sum())
            s["ties"] += int((t.d_exact.view(np.uint32) == t.thr.view(np.uint32)).sum())
            d = np.sort(t.sorted_d)
            s["tie_rows"] += int((d[1:].view(np.uint32) == d[:-1].view(np.uint32)).any())
            s["accepted"].append(t.accepted.size)
            for b0 in range(0, t.decided, 32):
                blk = long[t.sorted_ids[b0:min(b0 + 32, t.n)]]
                s["mixed_blocks"] += int(blk.any() and not blk.all())
                # MaxEdges reached inside a block that holds a long row (the exact-only loop's own `rc < max_edges`)
                s["full_in_mixed"] += int(blk.any() and not blk.all() and t.accepted.size == t.max_edges and b0 + 32 > t.decided - 1 and t.decided < t.n)
            if t.d_chain.size:
                s["modelled"] += t.d_chain.size
                w, ins = gp.wrong_and_inside(metric, case.dim, t)
                s["wrong"] += w; s["inside"] += ins
                s["wrong8"] += gp.wrong_and_inside(metric, case.dim, t, 8)[0]
                s["wrong0"] += gp.wrong_and_inside(metric, case.dim, t, 0)[0]
    s["accepted"] = np.asarray(s["accepted"])
    s["share"] = s["inside"] / max(1, s["modelled"])
    print(f"{case.id}: {s['calls']} heuristic calls, {s['comparisons']} comparisons, {s['modelled']} modelled; inside the margin {s['share']:.4f}; "
          f"decided wrongly with E {s['wrong']}, E/8 {s['wrong8']}, no margin {s['wrong0']}; d == thr {s['ties']}, lists with an equal pair {s['tie_rows']}; "
          f"accepted > 32 / 64 / 96: {(s['accepted'] > 32).sum()} / {(s['accepted'] > 64).sum()} / {(s['accepted'] > 96).sum()}; "
          f"mixed blocks {s['mixed_blocks']}, lists filled inside one {s['full_in_mixed']}; NaN comparisons {s['nan']}")
    _SUMMARY[case.id] = s
    return s


def by_group(*groups):
    return [pytest.param(c, id=c.id) for c in gp.CASES if c.group in groups]


def test_prefilter_applies_restates_the_rule():
    assert gp.prefilter_applies("ucosine", 256, 257) and gp.prefilter_applies("cosine", 264, 512) and gp.prefilter_applies("sq_euclid", 768, 300)
    assert not gp.prefilter_applies("ucosine", 248, 300) and not gp.prefilter_applies("ucosine", 260, 300)
    assert not gp.prefilter_applies("ucosine", 256, 256) and not gp.prefilter_applies("ucosine", 256, 513)
    assert not gp.prefilter_applies("ucosine_f16", 256, 300) and not gp.prefilter_applies("sq_euclid_i8", 256, 300)
    assert all(c.eligible() for c in gp.CASES) and not any(c.eligible() for c in gp.EDGE_CASES)
    assert len({c.id for c in gp.CASES + gp.EDGE_CASES}) == len(gp.CASES) + len(gp.EDGE_CASES)
    assert all(c.n <= (1200 if c.dim == 768 else 2000) for c in gp.CASES + gp.EDGE_CASES)


def test_margins_are_the_kernels():
    assert abs(float(gp.margin_E(768)) - (1.125 * 768 + 32) * 2.0 ** -24) < 1e-11 and abs(float(gp.margin_E(768)) - 5.3e-5) < 1e-6
    assert abs(float(gp.margin_Esq(256)) - (2.25 * 256 + 32) * 2.0 ** -24 * 1.01) < 1e-11


def test_chain_dot_is_a_sequential_fp32_chain():
    rng = np.random.default_rng(3)
    a, b = rng.random((3, 40), dtype=np.float32), rng.random((2, 40), dtype=np.float32)
    want = np.zeros((3, 2), dtype=np.float32)
    for i in range(3):
        for j in range(2):
            acc = np.float32(0)
            for k in range(40):
                acc = np.float32(np.float64(acc) + np.float64(a[i, k]) * np.float64(b[j, k]))
            want[i, j] = acc
    assert gp.chain_dot(a, b).tobytes() == want.tobytes()
    assert gp.chain_norm(a).tobytes() == np.diag(gp.chain_dot(a, a)).tobytes()
    g = gp.grid(256)[:8]                                   # integer rows: exact in any order
    assert (gp.chain_dot(g, g) == g.astype(np.float64) @ g.astype(np.float64).T).all()
    # lane_norm is the kernels' order: 1 - ucosine(a, a) can only be compared on exact sums
    assert (gp.lane_norm(g) == (g.astype(np.float64) ** 2).sum(1)).all()


def test_families_are_fixed_and_shaped_as_described():
    for c in gp.CASES + gp.EDGE_CASES:
        x = c.rows()
        assert x.dtype == np.float32 and x.tobytes() == np.ascontiguousarray(c.make()[:c.n]).tobytes(), c.id
    x = gp.biased(256, 0.7)
    assert np.allclose((x.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6) and np.allclose(x[:, 0], 0.7, atol=0.01)
    moved = (np.abs(x[:, 1:] - np.median(x[:, 1:], axis=1, keepdims=True)) > 1e-6).sum(1)
    assert moved.min() >= 3 and moved.max() <= 16
    xc = gp.biased(264, 0.7, "cosine")
    norms = np.sqrt((xc.astype(np.float64) ** 2).sum(1))
    assert (norms == 0).sum() >= 10 and norms[norms > 0].min() < 2e-14 and norms.max() > 5e14
    assert 1e-30 < norms[norms > 0].min() ** 2 < 1e-27                   # products of two small rows: just above the 1e-30 guard
    xo = gp.overflow(256)
    with np.errstate(over="ignore"):
        n32 = (xo * xo).sum(1, dtype=np.float32)
    assert np.isinf(n32).sum() == gp.OVERFLOW_ROWS and ((n32 > 1e37) & np.isfinite(n32)).sum() == gp.OVERFLOW_ROWS
    xoff = gp.offset_cluster(256)
    assert 2.5e6 < (xoff.astype(np.float64) ** 2).sum(1).mean() < 2.7e6
    xd = gp.near_duplicates(256, "sq_euclid")
    _, inv, cnt = np.unique(xd, axis=0, return_inverse=True, return_counts=True)
    assert (cnt[inv.ravel()] > 1).sum() >= 2 * (2000 // 10)              # the copies and their sources
    xm = gp.mixed_length(256)
    assert gp.long_rows(xm).sum() == 100 and not gp.long_rows(gp.biased(256, 0.7)).any()
    lengths = np.sqrt((xm[gp.long_rows(xm)].astype(np.float64) ** 2).sum(1))
    assert all((np.abs(lengths - v) < 1e-4).any() for v in gp.LONG_LENGTHS)
    xg = gp.grid(256)
    assert xg.min() == 0 and xg.max() == 3 and (xg == np.round(xg)).all()


@pytest.mark.parametrize("case", by_group("tight"))
def test_kernel_margin_decides_nothing_wrongly_and_smaller_ones_do(case):
    s = summary(case)
    assert s["modelled"] == s["comparisons"] > 10000
    assert s["wrong"] == 0, s["wrong"]
    if case.family == "overflow":
        return                                            # uniform rows: the family is there for inf and NaN, not for the margin
    assert s["wrong0"] >= FLOOR, s["wrong0"]
    assert s["wrong8"] >= EIGHTH_FLOOR.get(case.family, FLOOR), s["wrong8"]
    if case.family == "offset_cluster":
        assert s["share"] == 1.0                          # the norms swamp every distance: every comparison goes to the exact kernels


def test_overflow_rows_reach_the_candidate_lists():
    case = next(c for c in gp.CASES if c.family == "overflow")
    s = summary(case)
    x = case.rows()
    with np.errstate(over="ignore"):
        big = np.isinf((x * x).sum(1, dtype=np.float32))
    ref = oracle.OracleIndex(case.dim, case.metric, max_edges=case.M, max_candidates=case.efc, collection_size=case.n)
    ref.add_batched(x, gp.BATCH, threads=8)
    linked = sum(int(np.isin(ref.edges(i, 0), np.flatnonzero(big)).any()) for i in range(case.n))
    print(f"{case.id}: rows with an edge to a row of infinite norm: {linked}")
    assert linked >= 1 and s["wrong"] == 0


@pytest.mark.parametrize("case", by_group("ties"))
def test_tie_families_put_exact_ties_in_front_of_the_tiles(case):
    s = summary(case)
    assert s["ties"] >= FLOOR, s["ties"]
    assert s["tie_rows"] >= FLOOR, s["tie_rows"]
    assert s["wrong"] == 0


@pytest.mark.parametrize("case", by_group("accepted"))
def test_accepted_lists_pass_one_two_and_three_tiles(case):
    s = summary(case)
    a = s["accepted"]
    assert (a > 32).sum() >= 5
    if case.efc == 512:
        assert (a > 64).sum() >= 5
        if case.M == 63:
            assert (a > 96).sum() >= 5
    assert len(set(a.tolist())) > 10                      # ... and not always the full list: partial tiles of accepted ids
    assert s["wrong"] == 0


@pytest.mark.parametrize("case", by_group("mixed"))
def test_mixed_length_blocks_hold_long_and_unit_rows(case):
    s = summary(case)
    assert s["mixed_blocks"] >= FLOOR
    assert s["full_in_mixed"] >= FLOOR                    # MaxEdges (16 ids) reached inside such a block
    assert s["wrong"] == 0


@pytest.mark.parametrize("case", by_group("ragged"))
def test_sequential_case_meets_every_candidate_count(case):
    s = summary(case)                                     # rows 200 .. 399 of a sequential build at efc 300: lists of 200 .. 300 candidates
    assert len(s["sizes"]) >= 90 and s["wrong"] == 0
    assert wb.sets_for(case.efc) == 8


@pytest.mark.parametrize("case", by_group("nan"))
def test_the_oracle_takes_rows_with_a_nan_element_and_they_reach_the_lists(case):
    s = summary(case)                                     # (the build itself is the first claim: it ends, and prune_trace follows it)
    assert s["nan"] >= FLOOR and s["wrong"] == 0
