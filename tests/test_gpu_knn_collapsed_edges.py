"""GPU tier: knn_query_collapsed past the one shape of tests/test_gpu_knn_collapsed.py -- more than 64 kept entries
and the row edges of collapse_rows_kernel, all six row kinds, queries the device hands back (all of a call, and a part of one: host-
collapsed rows between device-collapsed ones), two contexts, the other kernel forms in front of the collapse, the traversal against
the flat scan, and the C ABI's argument errors.

The reference of every assertion but section 6's: the rows knn_query(q, beam, allowed=..., layer=...) returns with nothing forced, on
one context, walked by collapse_model.collapsed_rows; ids equal and distances byte-equal.  Each case asserts through a counter that
the path it is named for ran.  2 000 rows x dim 20, M = 8, 48 queries (the existing file's helpers); one dim-128 index of 3 000 rows
for the row prefilter; one of 300 rows for section 6."""
import ctypes as ct
import importlib
import os

import numpy as np
import pytest

import collapse_model as cm
from collapse_model import collapsed_rows, same
from common import novis_active, set_diag, uniform
from test_gpu_knn_collapsed import DIM, K, M, N, NQ, Case, _allowed, _check, _data, _heavy, _index, _threes

pytestmark = pytest.mark.gpu

LAYOUTS = {"threes": _threes, "heavy": _heavy}
WAYS = ["device", "host"]
NAN_QUERIES = [0, 9, 23, 38, 47]            # the queries that get one NaN element: scattered, the first and the last among them


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


@pytest.fixture(scope="module")
def hosts(cases):
    """Per row kind an index of the same rows (and so the same graph) that answers on the host."""
    cache = {}

    def get(metric):
        if metric not in cache:
            ix = _index(metric, set_device_traversal=False)
            try:
                ix.add(cases(metric).x)
            finally:
                ix.set_device_traversal(True)      # (the pending value, for an index made after a failed add)
            assert ix.graph_hash() == cases(metric).ix.graph_hash()
            cache[metric] = ix
        return cache[metric]
    return get


def _on(way, cases, hosts, metric="sq_euclid"):
    """The index that answers `way`, its counters reset."""
    ix = cases(metric).ix if way == "device" else hosts(metric)
    ix.reset_stats()
    return ix


def _ran(way, ix):
    """The counter that says the way was the one asked for."""
    launches = ix.stats()["search_launches"]
    assert launches > 0 if way == "device" else launches == 0, (way, launches)


def _padded_from(ids, d, kept):
    """Row i holds kept[i] results, then -1 / NaN."""
    cols = np.arange(ids.shape[1])[None, :]
    return ((ids >= 0) == (cols < kept[:, None])).all() and (np.isnan(d) == (cols >= kept[:, None])).all()


# ---- 1. more than 64 kept entries, and the row edges of the collapse kernel ---------------------------------------------------------
@pytest.mark.parametrize("way", WAYS)
def test_two_labels_capped_at_60_fill_both_pieces_of_the_kept_list(cases, hosts, way):
    """k = 120 of a beam of 400, labels id % 2, 60 of each: the count of kept entries of a label takes a second ballot from the 65th
    kept entry on, and both labels have kept members in entries 0 .. 63 and in entries 64 .. 119."""
    c, lab = cases("sq_euclid"), (np.arange(N) % 2).astype(np.int32)
    ix = _on(way, cases, hosts)
    ids, d = ix.knn_query_collapsed(c.q, 120, lab, per_group=60, beam=400)
    _ran(way, ix)
    plain = c.plain(400, None, 0)
    assert same((ids, d), collapsed_rows(*plain, lab, 120, 60))
    assert (ids >= 0).all()
    for g in (0, 1):
        mine = lab[ids] == g
        assert (mine.sum(axis=1) == 60).all() and mine[:, :64].any(axis=1).all() and mine[:, 64:].any(axis=1).all()
        assert ((lab[plain[0]] == g).sum(axis=1) > 60).all()                     # both caps bind


@pytest.mark.parametrize("way", WAYS)
def test_a_row_of_more_than_64_survivors_that_ends_in_padding(cases, hosts, way):
    """k = 130 of a beam of 400 under three labels capped at 50: 50 of the heavy label and what the beam holds of the two light ones."""
    c, lab = cases("sq_euclid"), _heavy()
    ix = _on(way, cases, hosts)
    ids, d = ix.knn_query_collapsed(c.q, 130, lab, per_group=50, beam=400)
    _ran(way, ix)
    assert same((ids, d), collapsed_rows(*c.plain(400, None, 0), lab, 130, 50))
    kept = (ids >= 0).sum(axis=1)
    assert (kept < 130).all() and (kept > 64).all() and _padded_from(ids, d, kept)
    assert ((lab[np.maximum(ids, 0)] == -1) & (ids >= 0)).sum(axis=1).tolist() == [50] * NQ


@pytest.mark.parametrize("way", WAYS)
def test_k_equal_to_the_beam_at_65(cases, hosts, way):
    """k == beam: the collapse can only shorten the row."""
    c, lab = cases("sq_euclid"), _threes()
    ix = _on(way, cases, hosts)
    ids, d = ix.knn_query_collapsed(c.q, 65, lab, per_group=1, beam=65)
    _ran(way, ix)
    plain = c.plain(65, None, 0)
    assert same((ids, d), collapsed_rows(*plain, lab, 65, 1))
    kept = (ids >= 0).sum(axis=1)
    assert (kept <= (plain[0] >= 0).sum(axis=1)).all() and _padded_from(ids, d, kept)
    # per_group == k == beam: the plain row itself
    assert same(ix.knn_query_collapsed(c.q, 65, lab, per_group=65, beam=65), plain)


@pytest.mark.parametrize("way", WAYS)
def test_k_1_at_a_beam_of_1(cases, hosts, way):
    c = cases("sq_euclid")
    ix = _on(way, cases, hosts)
    plain = c.plain(1, None, 0)
    for lab in (_threes(), _heavy()):
        assert same(ix.knn_query_collapsed(c.q, 1, lab, per_group=1, beam=1), plain)
    assert (plain[0] >= 0).all()
    _ran(way, ix)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("k", [64, 65])
def test_k_64_and_65_at_the_first_beam_of_four_register_sets(cases, hosts, way, k):
    c = cases("sq_euclid")
    ix = _on(way, cases, hosts)
    plain = c.plain(129, None, 0)
    for lab, m in ((_threes(), 1), (_threes(), 2), (_heavy(), 30), (_heavy(), k)):
        got = ix.knn_query_collapsed(c.q, k, lab, per_group=m, beam=129)
        assert same(got, collapsed_rows(*plain, lab, k, m)), m
    assert ((got[0] >= 0).sum(axis=1) == k).all()                                # (per_group == k: nothing is capped)
    _ran(way, ix)


@pytest.mark.parametrize("way", WAYS)
@pytest.mark.parametrize("beam", [257, 513])
def test_the_first_beams_of_eight_sets_and_of_the_exact_traversal(cases, hosts, way, beam):
    c = cases("sq_euclid")
    ix = _on(way, cases, hosts)
    plain = c.plain(beam, None, 0)
    for name, lab in LAYOUTS.items():
        for m in (1, 2):
            assert same(ix.knn_query_collapsed(c.q, K, lab(), per_group=m, beam=beam), collapsed_rows(*plain, lab(), K, m)), (name, m)
    _ran(way, ix)


@pytest.mark.parametrize("way", WAYS)
def test_padding_inside_the_input_rows(cases, hosts, way):
    c = cases("sq_euclid")
    ix = _on(way, cases, hosts)
    # an allow-set of 7 ids (seven of the rows query 0's traversal finds): the row is 7 entries and 33 paddings
    seven = c.plain(200, None, 0)[0][0, [0, 20, 50, 90, 130, 170, 199]]
    assert (seven >= 0).all() and np.unique(seven).size == 7
    allowed = np.zeros(N, bool)
    allowed[seven] = True
    plain = c.ix.knn_query(c.q, 40, allowed=allowed)
    assert ((plain[0] >= 0).sum(axis=1) == 7).all() and (plain[0][:, 7:] == -1).all()
    lab = np.arange(N, dtype=np.int32)
    lab[seven[3]] = lab[seven[5]]                                                # two of the seven share a label
    ids, d = ix.knn_query_collapsed(c.q, K, lab, per_group=1, beam=40, allowed=allowed)
    assert same((ids, d), collapsed_rows(*plain, lab, K, 1))
    assert _padded_from(ids, d, np.full(NQ, 6))
    ids, d = ix.knn_query_collapsed(c.q, K, lab, per_group=2, beam=40, allowed=allowed)
    assert same((ids, d), collapsed_rows(*plain, lab, K, 2)) and _padded_from(ids, d, np.full(NQ, 7))
    # an allow-set of one id
    one = np.array([int(seven[2])])
    plain = c.ix.knn_query(c.q, 40, allowed=one)
    assert (plain[0][:, 0] == one[0]).all() and (plain[0][:, 1:] == -1).all()
    for name, lab in LAYOUTS.items():
        ids, d = ix.knn_query_collapsed(c.q, K, lab(), per_group=1, beam=40, allowed=one)
        assert same((ids, d), collapsed_rows(*plain, lab(), K, 1)) and _padded_from(ids, d, np.full(NQ, 1)), name
    # layer 1 under a beam larger than the layer: the plain row itself ends in padding
    on_1 = int((c.ix.levels() >= 1).sum())
    beam = on_1 + 20
    plain = c.plain(beam, None, 1)
    assert 0 < on_1 and (plain[0][:, on_1:] == -1).all() and (plain[0][:, 0] >= 0).all()
    for name, lab in LAYOUTS.items():
        for m in (1, 2):
            got = ix.knn_query_collapsed(c.q, K, lab(), per_group=m, beam=beam, layer=1)
            assert same(got, collapsed_rows(*plain, lab(), K, m)), (name, m)
    _ran(way, ix)


@pytest.mark.parametrize("way", WAYS)
def test_a_label_array_longer_than_the_index(cases, hosts, way):
    c = cases("sq_euclid")
    ix = _on(way, cases, hosts)
    for name, lab in LAYOUTS.items():
        longer = np.concatenate([lab(), np.arange(100, dtype=np.int32) - 50])
        assert longer.size == c.ix.length + 100
        for allowed in (None, _allowed()):
            got = ix.knn_query_collapsed(c.q, K, longer, per_group=2, beam=40, allowed=allowed)
            assert same(got, ix.knn_query_collapsed(c.q, K, lab(), per_group=2, beam=40, allowed=allowed)), name
            assert same(got, collapsed_rows(*c.plain(40, allowed, 0), lab(), K, 2)), name
    _ran(way, ix)


@pytest.mark.parametrize("way", WAYS)
def test_removed_ids_never_come_back(cases, way):
    c = cases("sq_euclid")
    q = c.q[:24]
    ix = _index("sq_euclid", set_device_traversal=way == "device")
    try:
        ix.add(c.x)
    finally:
        ix.set_device_traversal(True)
    assert ix.graph_hash() == c.ix.graph_hash()
    lab = _threes()
    first = ix.knn_query_collapsed(q, K, lab)
    assert same(first, collapsed_rows(c.plain(4 * K, None, 0)[0][:24], c.plain(4 * K, None, 0)[1][:24], lab, K, 1))
    gone = np.unique(first[0][:, 0])
    assert (gone >= 0).all()
    ix.remove(gone)
    assert ix.length == N and ix.count == N - gone.size
    ix.reset_stats()
    for name, lab in LAYOUTS.items():
        for m in (1, 2):
            for allowed in (None, _allowed()):
                got = ix.knn_query_collapsed(q, K, lab(), per_group=m, beam=4 * K, allowed=allowed)
                plain = ix.knn_query(q, 4 * K, allowed=allowed)
                assert same(got, collapsed_rows(*plain, lab(), K, m)), (name, m, allowed is not None)
                assert not np.isin(got[0], gone).any() and not np.isin(plain[0], gone).any()
    _ran(way, ix)


# ---- 2. all six row kinds -------------------------------------------------------------------------------------------------------------
OTHER_KINDS = ["ucosine", "sq_euclid_i8", "sq_euclid_f16"]


@pytest.mark.parametrize("metric", OTHER_KINDS)
def test_the_device_way_on_the_other_three_row_kinds(cases, metric):
    c = cases(metric)
    c.ix.reset_stats()
    _check(c.ix, c.q, c.plain)
    assert c.ix.stats()["search_launches"] > 0
    got = c.ix.knn_query_collapsed(c.q, K, _heavy(), per_group=K, beam=200)    # per_group == k: the plain call's first k entries
    plain = c.plain(200, None, 0)
    assert same(got, (plain[0][:, :K], plain[1][:, :K]))


@pytest.mark.parametrize("metric", OTHER_KINDS)
def test_the_host_way_on_the_other_three_row_kinds(cases, hosts, metric):
    c, host = cases(metric), hosts(metric)
    host.reset_stats()
    _check(host, c.q, c.plain)                                                   # against the DEVICE index's plain rows
    assert host.stats()["search_launches"] == 0


# ---- 3. hand-backs --------------------------------------------------------------------------------------------------------------------
FILTERS = [(False, 0), (True, 0), (False, 1), (True, 1)]


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_every_query_handed_back(cases, monkeypatch, metric):
    """Candidate heaps of 24 entries and a spill of 8: a traversal that keeps a candidate heap gives up at a beam of 40 and the host
    answers, into rows of 40 that it collapses itself.  With an allow-set that is every call.  Without one the beam is a sorted list
    and there is no heap to outgrow (0 hand-backs observed under these two hooks alone), so those calls run once more with
    sorted_top=0, the two-heap traversal, which has one.
    Observed on an MI355X, of the 192 queries in the four calls of a filter and layer: 192 with an allow-set (layer 0 and 1, both
    metrics); without one 0 (cosine at layer 0: 4), and 192 under sorted_top=0."""
    c = cases(metric)
    want = {f: c.plain(4 * K, _allowed() if f[0] else None, f[1]) for f in FILTERS}      # nothing forced yet

    def run(filt, layer):
        c.ix.reset_stats()
        for name, lab in LAYOUTS.items():
            for m in (1, 2):
                got = c.ix.knn_query_collapsed(c.q, K, lab(), per_group=m, beam=4 * K, allowed=_allowed() if filt else None, layer=layer)
                assert same(got, collapsed_rows(*want[filt, layer], lab(), K, m)), (name, m, filt, layer)
        st = c.ix.stats()
        print(f"forced hand-backs {metric} {os.environ['HNSW_MI355X_DIAG']} filter {filt} layer {layer}: {st['search_overflows']} of {4 * NQ} queries in 4 calls")
        assert st["search_launches"] > 0
        return st["search_overflows"]
    set_diag(monkeypatch, cand_cap="24", spill_cap="8")
    total = 0
    for filt, layer in FILTERS:
        over = run(filt, layer)
        assert over > 0 or not filt, (filt, layer)
        total += over
    assert total > 0
    set_diag(monkeypatch, sorted_top=0)
    for layer in (0, 1):
        assert run(False, layer) > 0, layer


def _nan_queries(q):
    out = q.copy()
    out[NAN_QUERIES, np.arange(len(NAN_QUERIES)) * 3 % DIM] = np.nan
    return out


def _overflows(ix, contexts=1):
    return ix.stats()["search_overflows"] + sum(ix.stats_at(g)["search_overflows"] for g in range(1, contexts))


def _part_handed_back(ix, q, want_of, contexts=1):
    """Every layout, cap and filter with the NaN queries among the 48: each call must hand back a strict part, and all 48 rows are
    the walk over `want_of(allowed)`.  Returns the hand-back counts seen."""
    seen = set()
    for filt in (False, True):
        allowed = _allowed() if filt else None
        want = want_of(allowed)
        for name, lab in LAYOUTS.items():
            for m in (1, 2):
                ix.reset_stats()
                got = ix.knn_query_collapsed(q, K, lab(), per_group=m, beam=4 * K, allowed=allowed)
                over = _overflows(ix, contexts)
                seen.add(over)
                assert 0 < over < NQ, (over, filt, name, m)
                assert same(got, collapsed_rows(*want, lab(), K, m)), (name, m, filt)
    return sorted(seen)


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_a_part_of_the_queries_handed_back(cases, metric):
    """5 of the 48 queries hold a NaN: every distance of theirs is NaN, the device gives them back, and the host writes their
    collapsed rows between the 43 the device collapsed.  The plain call answers those five through the same host traversal, so its
    rows, NaN distances included, are the reference of all 48.
    Observed on an MI355X: 5 of 48 handed back in every call, with and without an allow-set, both metrics."""
    c = cases(metric)
    q = _nan_queries(c.q)
    plain = {}

    def want_of(allowed):
        key = allowed is not None
        if key not in plain:
            plain[key] = c.ix.knn_query(q, 4 * K, allowed=allowed)
        return plain[key]
    nan_rows = np.isnan(want_of(None)[1]).any(axis=1)
    assert nan_rows[NAN_QUERIES].all() and nan_rows.sum() == len(NAN_QUERIES)
    counts = _part_handed_back(c.ix, q, want_of)
    print(f"part handed back, {metric}: {counts} of {NQ}")
    assert counts[0] >= len(NAN_QUERIES)


# ---- 4. two contexts ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two(cases):
    c = cases("sq_euclid")
    ix = _index("sq_euclid", set_devices=2)
    try:
        ix.add(c.x)
    finally:
        ix.set_devices(1)
    assert ix.graph_hash() == c.ix.graph_hash()
    return ix


def test_two_contexts_give_the_one_context_rows(cases, two):
    c = cases("sq_euclid")
    two.reset_stats()
    _check(two, c.q, c.plain)
    assert two.stats_at(1)["search_launches"] > 0 and two.stats()["search_launches"] > 0
    assert _overflows(two, 2) == 0


def test_two_contexts_with_a_part_handed_back(cases, two):
    """The shards are gathered to the primary, the host redoes the NaN queries -- they fall into both shards -- and nothing changes.
    Observed on an MI355X: 5 of 48 handed back, summed over the two contexts, in every call."""
    c = cases("sq_euclid")
    q = _nan_queries(c.q)
    plain = {}

    def want_of(allowed):                                                        # the ONE-context index's plain rows
        key = allowed is not None
        if key not in plain:
            plain[key] = c.ix.knn_query(q, 4 * K, allowed=allowed)
        return plain[key]
    counts = _part_handed_back(two, q, want_of, contexts=2)
    print(f"part handed back over two contexts: {counts} of {NQ}")
    assert two.stats_at(1)["search_launches"] > 0
    # ... and a call without hand-backs right after: the set stays sharded and the rows stay right
    two.reset_stats()
    assert same(two.knn_query_collapsed(c.q, K, _threes()), collapsed_rows(*c.plain(4 * K, None, 0), _threes(), K, 1))
    assert two.stats_at(1)["search_launches"] > 0 and _overflows(two, 2) == 0


# ---- 5. other kernel forms in front of the collapse -------------------------------------------------------------------------------
FORMS = [dict(lat=2), dict(lat=0), dict(lat=0, lean=0), dict(lat=0, vis_hash=1)]


@pytest.mark.parametrize("hooks", FORMS, ids=lambda hk: ",".join(f"{k}={v}" for k, v in hk.items()))
def test_every_traversal_form_in_front_of_the_collapse(cases, monkeypatch, hooks):
    c = cases("sq_euclid")
    want = {beam: c.plain(beam, None, 0) for beam in (4 * K, 200)}               # the default run, nothing forced
    set_diag(monkeypatch, **hooks)
    for beam in (4 * K, 200):
        c.ix.reset_stats()
        for name, lab in LAYOUTS.items():
            for m in (1, 2):
                got = c.ix.knn_query_collapsed(c.q, K, lab(), per_group=m, beam=beam)
                assert same(got, collapsed_rows(*want[beam], lab(), K, m)), (beam, name, m)
        st = c.ix.stats()
        assert st["search_launches"] > 0 and st["search_overflows"] == 0
        assert (st["lat_launches"] > 0) == (hooks.get("lat") == 2), beam
        if hooks == dict(lat=0) and novis_active(st):
            assert st["lean_launches"] > 0, beam
        if hooks.get("lean") == 0:
            assert st["lean_launches"] == 0, beam
        if hooks.get("vis_hash") == 1:
            assert st["visited_hash_launches"] > 0, beam


@pytest.fixture(scope="module")
def wide():
    """3 000 rows x dim 128, M = 16, built with the row prefilter off; its queries and the plain rows of that setting."""
    import hnswindex
    x, q = uniform(3000, 128, 9100), uniform(NQ, 128, 9101)
    with pytest.MonkeyPatch.context() as mp:
        set_diag(mp, row_prefilter=0)
        ix = hnswindex.Index(128, "sq_euclid")
        ix.set_collection_size(3000); ix.set_max_edges(16)
        assert (ix.add(x) == np.arange(3000)).all()
        plain = {beam: ix.knn_query(q, beam) for beam in (64, 200)}
        assert ix.row_prefilter_stats()["launches"] == 0
    lab = (np.repeat(np.arange(1000), 3)[np.random.default_rng(5).permutation(3000)] - 300).astype(np.int32)
    return ix, q, plain, lab


@pytest.mark.parametrize("fixed", [1, 0], ids=["fixed_dim", "runtime_dim"])
def test_the_row_prefilter_forms_in_front_of_the_collapse(wide, monkeypatch, fixed):
    ix, q, plain, lab = wide
    set_diag(monkeypatch, lat=0, row_prefilter=2, pf_fixed_dim=fixed)
    pf0, form0 = ix.row_prefilter_stats(), ix.row_prefilter_form_stats()
    ix.reset_stats()
    for beam in (64, 200):
        for m in (1, 2):
            assert same(ix.knn_query_collapsed(q, K, lab, per_group=m, beam=beam), collapsed_rows(*plain[beam], lab, K, m)), (beam, m)
    pf1, form1, st = ix.row_prefilter_stats(), ix.row_prefilter_form_stats(), ix.stats()
    launches = pf1["launches"] - pf0["launches"]
    assert launches > 0 and pf1["rows_on_shadow"] > pf0["rows_on_shadow"]
    ran = {name: form1[name] - form0[name] for name in form1}
    assert ran == ({"runtime_dim": 0, "fixed_dim": launches} if fixed else {"runtime_dim": launches, "fixed_dim": 0})
    assert st["lean_launches"] > 0 and st["lat_launches"] == 0 and st["search_overflows"] == 0


# ---- 6. the two forms against each other ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", cm.FULL_METRICS)
def test_the_traversal_at_a_beam_of_the_whole_index_is_the_flat_scan(metric):
    """300 uniform rows, one at a time (so the graph is the one tests/test_collapse_model.py walked on the oracle): at a beam of 300
    the traversal returns every row, and the flat scan measures each with the traversal's own arithmetic."""
    import hnswindex
    import oracle
    n = cm.FULL_N
    x, q = cm.full_case()
    ix = hnswindex.Index(cm.FULL_DIM, metric)
    ix.set_collection_size(n); ix.set_max_edges(cm.FULL_M); ix.set_insert_batch(1)
    assert (ix.add(x) == np.arange(n)).all()
    ref = oracle.OracleIndex(cm.FULL_DIM, metric, max_edges=cm.FULL_M, collection_size=n)
    ref.add(x)
    assert ix.graph_hash() == ref.graph_hash()
    ids, d = ix.knn_query(q, n)
    assert (ids >= 0).all() and (np.sort(ids, axis=1) == np.arange(n)).all() and (d[:, 1:] > d[:, :-1]).all()
    rng = np.random.default_rng(3)
    threes = (np.repeat(np.arange(n // 3), 3)[rng.permutation(n)] - 30).astype(np.int32)
    heavy = np.full(n, -1, np.int32)
    rest = rng.permutation(n)[: n // 10]
    heavy[rest[::2]], heavy[rest[1::2]] = 2 ** 31 - 1, 0
    ix.reset_stats()
    for name, lab in (("threes", threes), ("heavy", heavy)):
        for m in (1, 3):
            got = ix.knn_query_collapsed(q, K, lab, per_group=m, beam=n)
            assert same(got, ix.exact_knn_query_collapsed(q, K, lab, per_group=m)), (name, m)
            assert same(got, collapsed_rows(ids, d, lab, K, m)), (name, m)
    st = ix.stats()
    assert st["search_launches"] > 0 and st["exact_launches"] > 0 and st["search_overflows"] == 0


# ---- 7. the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_c_abi_turns_bad_arguments_away_before_anything_runs(cases):
    import hnswindex
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)
    lib = net.lib
    c = cases("sq_euclid")
    rg = _threes()
    want = collapsed_rows(*c.plain(4 * K, None, 0), rg, K, 1)
    words, nbits = net.allow_bits(_allowed())
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    ids, d = np.full((NQ, K), 7, np.int32), np.full((NQ, K), 7.0, np.float32)

    def call(beam=4 * K, row_group=rg.ctypes.data_as(I), n_rg=N, m=1, allow=None, bits=0):
        return lib.hnsw_mi355x_knn_query_collapsed(c.ix._h, c.q.ctypes.data_as(F), NQ, DIM, K, beam, row_group, n_rg, m, 0, allow, bits,
                                                   ids.ctypes.data_as(I), d.ctypes.data_as(F))
    c.ix.reset_stats()
    for args, msg in ((dict(row_group=None), "row_group must not be NULL and n_row_group must be >= 0"),
                      (dict(n_rg=-1), "row_group must not be NULL and n_row_group must be >= 0"),
                      (dict(allow=words.ctypes.data_as(U), bits=-1), "nbits must be >= 0"),
                      (dict(m=0), "per_group = 0 is outside [1, k = 10]"),
                      (dict(beam=K - 1), "beam = 9 is below k = 10")):
        assert call(**args) == -1, args
        assert "hnsw_mi355x_knn_query_collapsed: " + msg in net.last_error(), (args, net.last_error())
        assert (ids == 7).all() and (d == 7.0).all(), args
        assert c.ix.stats()["search_launches"] == 0, args
    assert call() == 0 and same((ids, d), want)
    assert c.ix.stats()["search_launches"] > 0
    assert call(allow=words.ctypes.data_as(U), bits=nbits) == 0 and same((ids, d), collapsed_rows(*c.plain(4 * K, _allowed(), 0), rg, K, 1))
    # an allow-set with no bit set: all padding, nothing launched
    c.ix.reset_stats()
    none = np.zeros(len(words), np.uint32)
    assert call(allow=none.ctypes.data_as(U), bits=nbits) == 0
    assert (ids == -1).all() and np.isnan(d).all() and c.ix.stats()["search_launches"] == 0
    got = c.ix.knn_query_collapsed(c.q, K, rg, allowed=np.zeros(N, bool), layer=1)
    assert (got[0] == -1).all() and np.isnan(got[1]).all() and c.ix.stats()["search_launches"] == 0
    assert same(c.ix.knn_query_collapsed(c.q, K, rg), want)
