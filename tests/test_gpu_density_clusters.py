"""GPU tier: density_clusters and neighbor_counts -- DBSCAN over the stored rows from the flat scan: a counting scan
whose within pairs go to an arena, a second phase that joins cores and attaches borders, labels.  3 000 rows x dim 20, six row kinds,
the structure of tests/density_rows.py planted on top of uniform rows; the radius lies between the largest planted-link distance and
the smallest distance of any other pair with a factor of 2 to spare on either side, both worked out there in float64 numpy.  Labels,
counts and info must equal the model (tests/density_model.py) over the lists exact_range_query_by_id returns, on float32 rows over
the oracle's distances as well, and the sets read off the plant; and their bytes must not depend on chunks, tiles, rounds, the
arena's capacity or the order the device finds the pairs in."""
import ctypes as ct

import numpy as np
import pytest

from common import set_diag, uniform
from density_model import (INFO, clusters_from_pairs, counts_only_info, density_clusters, neighbor_counts, pairs_from_range_lists,
                           pairs_within_d)
from density_rows import (BIG, CHAIN, CHUNK, DIM, HIGH, LOW, METRICS, MIN_SAMPLES, N, QTILE, ROUND, STRADDLE, TRIPLE, links, radius_between,
                          rows)

pytestmark = pytest.mark.gpu

ALL_PAIRS = N * (N - 1) // 2
SMALL = dict(exact_chunk=CHUNK, exact_qtile=QTILE, exact_union_round=ROUND)


def _index(dim, metric, n):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(8); ix.set_insert_batch(0)
    return ix


def _oracle_dist(metric, x):
    import oracle
    return lambda own, cand: oracle.dist_query_rows(metric, x, x[own], cand) if cand.size else np.zeros(0, np.float32)


def _same(got, want, what=None):
    assert got[0].dtype == got[1].dtype == np.int32
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2], (what, got[2], want[2])


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x = rows(metric)
        self.r, self.d64 = radius_between(metric, self.x, links())       # asserts the factor-2 margin for this row kind
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        lists, dists = self.ix.exact_range_query_by_id(np.arange(N), self.r)
        self.pairs = pairs_from_range_lists(np.arange(N), lists, dists)  # the within pairs as the device's own range lists have them, computed once
        self._want = {}

    def want(self, min_samples, scans=1):
        """The model over the range lists."""
        if (min_samples, scans) not in self._want:
            self._want[min_samples, scans] = clusters_from_pairs(N, np.arange(N), self.pairs, min_samples, scans)
        return self._want[min_samples, scans]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


def test_the_plant_straddles_the_edges():
    assert STRADDLE[0] < 696 < CHUNK < 704 < STRADDLE[-1] and CHAIN[4] == 2 * CHUNK and len(BIG) == 200 and -(-N // ROUND) == 6
    planted = TRIPLE + CHAIN + STRADDLE + BIG + LOW.ids() + HIGH.ids()
    assert len(set(planted)) == len(planted) == 3 + 10 + 12 + 200 + 2 * 17
    assert {b // CHUNK for b in BIG} == {0, 1, 2, 3, 4} and {b // ROUND for b in BIG} == set(range(6))
    assert {v // ROUND for v in CHAIN} >= {2, 3, 4, 5}
    # X lies below every core it is within, X' above; B holds the smaller ids, and A and B are cut by chunks and rounds
    assert LOW.x < min(LOW.a1 + LOW.b1) and HIGH.x > max(HIGH.a1 + HIGH.b1)
    for ab in (LOW, HIGH):
        assert max(ab.b) < min(ab.a) and len({v // CHUNK for v in ab.a + ab.b}) >= 3 and len({v // ROUND for v in ab.a + ab.b}) >= 3


@pytest.mark.parametrize("metric", METRICS)
def test_the_plant_comes_out_as_planted(cases, metric):
    """The model over the device's range lists sees the planted graph and nothing else, and the sets are the ones the plant means."""
    c = cases(metric)
    assert {(a, b) for a, b, _ in c.pairs} == links()
    planted = [(a, b, np.float32(c.d64[a, b])) for a, b in sorted(links())]          # the same graph with numpy's distances
    for ms in (3, 4, MIN_SAMPLES):
        labels, counts, info = c.want(ms)
        by_plant = clusters_from_pairs(N, np.arange(N), planted, ms)
        assert labels.tolist() == by_plant[0].tolist() and counts.tolist() == by_plant[1].tolist() and info == by_plant[2], (metric, ms)
    labels, counts, info = c.want(3)
    # min_samples 3: the chain's inner rows are core (two neighbours), its ends borders of their cluster; the triple is a cluster
    assert counts[CHAIN].tolist() == [1, 2, 2, 2, 2, 2, 2, 2, 2, 1] and (labels[CHAIN] == min(CHAIN[1:-1])).all()
    assert (labels[TRIPLE] == TRIPLE[0]).all() and (counts[TRIPLE] == 2).all()
    # ... and X, with four neighbours, is core: it joins A and B, here and only here
    assert labels[LOW.x] == labels[LOW.a[0]] == labels[LOW.b[0]] == LOW.x and labels[HIGH.x] == labels[HIGH.a[0]] == HIGH.b[0]
    assert (info["clusters"], info["border"]) == (6, 2) and info["core"] == 8 + 3 + 12 + 200 + 2 * 17
    labels, counts, info = c.want(4)
    assert (labels[CHAIN] == -1).all() and (labels[TRIPLE] == -1).all()              # all ten rows of the chain are noise
    labels, counts, info = c.want(MIN_SAMPLES)
    for ab in (LOW, HIGH):
        assert counts[ab.x] == 4 and (counts[ab.a1 + ab.b1] == 8).all() and (counts[ab.a2 + ab.b2] == 7).all()
        assert (labels[ab.a] == min(ab.a)).all() and (labels[ab.b] == min(ab.b)).all()
        assert labels[ab.x] == min(ab.a) > min(ab.b)                                  # the nearer core's cluster, not the smaller label
    assert (labels[BIG] == BIG[0]).all() and (counts[BIG] == 199).all() and (labels[STRADDLE] == STRADDLE[0]).all() and (counts[STRADDLE] == 11).all()
    assert info == {"members": N, "clusters": 6, "core": 200 + 12 + 2 * 16, "border": 2, "noise": N - 200 - 12 - 2 * 17, "pairs_within": len(links()),
                    "pairs_measured": ALL_PAIRS, "scans": 1}
    assert tuple(info) == INFO


@pytest.mark.parametrize("metric", METRICS)
def test_clusters_are_the_model_whatever_the_chunks_rounds_and_arena(cases, monkeypatch, metric):
    c = cases(metric)
    pw = len(c.pairs)
    knob_sets = (({}, 1, 1), (dict(exact_chunk=CHUNK, exact_qtile=QTILE), 1, 1), (SMALL, 6, 1), (dict(SMALL, density_pair_cap=pw), 6, 1),
                 (dict(SMALL, density_pair_cap=pw - 1), 6, 2), (dict(SMALL, density_pair_cap=1), 6, 2),
                 (dict(exact_chunk=0, exact_qtile=0, exact_union_round=0, density_pair_cap=1), 1, 2))
    for knobs, rounds, scans in knob_sets:
        if knobs:
            set_diag(monkeypatch, **knobs)
        for ms in (3, MIN_SAMPLES):
            first = None
            for _ in range(2):                                           # the pairs arrive in another order every time
                c.ix.reset_stats()
                got = c.ix.density_clusters(c.r, ms)
                st = c.ix.stats()
                want = c.want(ms, scans)
                _same(got, want, (metric, knobs, ms))
                assert got[2]["scans"] == scans and got[2]["pairs_measured"] == scans * ALL_PAIRS and got[2]["pairs_within"] == pw
                assert st["exact_launches"] == rounds * scans and st["exact_evals"] == scans * ALL_PAIRS and st["search_launches"] == 0, (metric, knobs, st)
                first = first or (got[0].tobytes(), got[1].tobytes())
                assert (got[0].tobytes(), got[1].tobytes()) == first


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine"])
def test_clusters_are_the_model_over_the_oracles_distances(cases, metric):
    c = cases(metric)
    pairs = pairs_within_d(_oracle_dist(metric, c.x), np.arange(N), c.r)
    for ms in (3, MIN_SAMPLES):
        _same(c.ix.density_clusters(c.r, ms), clusters_from_pairs(N, np.arange(N), pairs, ms), (metric, ms))


@pytest.mark.parametrize("metric", METRICS)
def test_min_samples_at_its_ends_and_the_counts_alone(cases, monkeypatch, metric):
    c = cases(metric)
    for knobs in ({}, SMALL, dict(SMALL, density_pair_cap=1)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        groups, groups_info = c.ix.duplicate_groups(c.r)
        labels, counts, info = c.ix.density_clusters(c.r, 1)
        assert labels.tobytes() == groups.tobytes() and info["pairs_within"] == groups_info["pairs_within"] and info["clusters"] == groups_info["groups"]
        assert info["core"] == N and info["border"] == info["noise"] == 0
        labels2, counts2, info2 = c.ix.density_clusters(c.r, 2)                       # the same, except that singletons are noise
        assert labels2.tobytes() == np.where(counts == 0, -1, groups).astype(np.int32).tobytes() and counts2.tobytes() == counts.tobytes()
        assert info2["noise"] == int((counts == 0).sum()) and info2["border"] == 0
        # min_samples above the member count: nobody is core
        labels, counts_n, info = c.ix.density_clusters(c.r, N + 1)
        assert (labels == -1).all() and counts_n.tobytes() == counts.tobytes()
        assert (info["clusters"], info["core"], info["border"], info["noise"]) == (0, 0, 0, N)
        # the counts alone: one scan whatever the arena's capacity, the slots that need labels 0
        c.ix.reset_stats()
        alone = c.ix.neighbor_counts(c.r)
        st = c.ix.stats()
        assert alone.dtype == np.int32 and alone.tobytes() == counts.tobytes() == c.want(1)[1].tobytes()
        assert st["exact_evals"] == ALL_PAIRS and st["exact_launches"] == (6 if knobs else 1)
    import hnswindex
    info = (ct.c_uint64 * 8)()
    out = np.full(N, 7, np.int32)
    assert hnswindex.net_amd.lib.hnsw_mi355x_density_clusters(c.ix._h, c.r, 5, None, 0, None, out.ctypes.data_as(ct.POINTER(ct.c_int)), N, info) == 0
    assert out.tobytes() == counts.tobytes() and dict(zip(INFO, info)) == counts_only_info(c.want(5)[2])


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8", "ucosine_f16"])
def test_allowed_sets_nan_and_infinity(cases, monkeypatch, metric):
    c = cases(metric)
    set_diag(monkeypatch, **SMALL)
    # the two rows of A1 of the first copy are not allowed, so its X has only B's cores left; half of BIG, part of the straddling cluster,
    # a chain row and a run of ids are not allowed either
    allowed = np.ones(N, bool)
    out = LOW.a1 + [CHAIN[3]] + STRADDLE[:4] + BIG[::2] + list(range(2100, 2200))
    allowed[out] = False
    members = np.flatnonzero(allowed)
    lists, dists = c.ix.exact_range_query_by_id(members, c.r, allowed=allowed)
    pairs = pairs_from_range_lists(members, lists, dists)
    for ms in (3, 5):
        want = clusters_from_pairs(N, members, pairs, ms)
        got = c.ix.density_clusters(c.r, ms, allowed=allowed)
        _same(got, want, (metric, ms))
        assert (got[0][out] == -1).all() and (got[1][out] == -1).all() and (got[1][members] >= 0).all()
        _same(c.ix.density_clusters(c.r, ms, allowed=members), want)                  # the set as an id list
    labels, counts, info = c.ix.density_clusters(c.r, 5, allowed=allowed)
    assert counts[LOW.x] == 2 and labels[LOW.x] == min(LOW.b) and (labels[LOW.a2] == min(LOW.a2)).all()   # X turned over to B; A goes on without A1
    labels, counts, info = c.ix.density_clusters(c.r, 3, allowed=allowed)
    assert labels[CHAIN[2]] == CHAIN[1] and labels[CHAIN[4]] == CHAIN[5]                # the chain fell in two: each end of the gap is a border now
    assert info["pairs_measured"] == members.size * (members.size - 1) // 2
    assert c.ix.neighbor_counts(c.r, allowed=allowed).tobytes() == counts.tobytes()
    # NaN: nothing is within; +inf: everything; a negative radius is ordinary: nothing is within it here
    m = members.size
    for ms, label in ((1, None), (2, -1)):
        labels, counts, info = c.ix.density_clusters(float("nan"), ms)
        assert labels.tolist() == (list(range(N)) if label is None else [-1] * N) and (counts == 0).all() and info["pairs_within"] == 0
        assert (info["clusters"], info["core"], info["noise"], info["scans"]) == ((N, N, 0, 1) if label is None else (0, 0, N, 1))
    for cap in (0, 1):                                                                  # every pair is within: the default arena holds them, an arena of one does not
        set_diag(monkeypatch, density_pair_cap=cap)
        labels, counts, info = c.ix.density_clusters(float("inf"), m, allowed=allowed)
        assert (labels[members] == members[0]).all() and (labels[out] == -1).all() and (counts[members] == m - 1).all() and (counts[out] == -1).all()
        assert info == {"members": m, "clusters": 1, "core": m, "border": 0, "noise": 0, "pairs_within": m * (m - 1) // 2,
                        "pairs_measured": (cap + 1) * (m * (m - 1) // 2), "scans": cap + 1}
    labels, counts, info = c.ix.density_clusters(float("inf"), m + 1, allowed=allowed)
    assert (labels == -1).all() and (counts[members] == m - 1).all() and info["noise"] == m and info["clusters"] == 0
    labels, counts, info = c.ix.density_clusters(-1.0, 1)
    assert labels.tolist() == list(range(N)) and info["pairs_within"] == 0 and (counts == 0).all()


def test_removed_ids_are_no_members(monkeypatch):
    """An index of its own (removal changes it): the two cores of A that X is within are removed, and so is a row of the chain."""
    metric = "sq_euclid"
    x = rows(metric)
    r, _ = radius_between(metric, x, links())
    ix = _index(DIM, metric, N)
    ix.add(x)
    before = ix.density_clusters(r, MIN_SAMPLES)
    assert before[0][LOW.x] == min(LOW.a) and before[0][HIGH.x] == min(HIGH.a)
    gone = LOW.a1 + [CHAIN[5], BIG[0], TRIPLE[0]]
    ix.remove(gone)
    live = np.delete(np.arange(N), gone)
    pairs = pairs_within_d(_oracle_dist(metric, x), live, r)
    for knobs in ({}, dict(SMALL, density_pair_cap=1)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for ms in (2, 3, MIN_SAMPLES):
            got = ix.density_clusters(r, ms)
            _same(got, clusters_from_pairs(N, live, pairs, ms, scans=2 if knobs else 1), (knobs, ms))
            assert (got[0][gone] == -1).all() and (got[1][gone] == -1).all()
    labels, counts, info = ix.density_clusters(r, MIN_SAMPLES)
    assert counts[LOW.x] == 2 and labels[LOW.x] == min(LOW.b) and labels[HIGH.x] == min(HIGH.a)   # its nearer cores are gone: X is a border of B now
    labels, counts, info = ix.density_clusters(r, 3)
    assert labels[HIGH.x] == HIGH.b[0] and labels[BIG[1]] == BIG[1] and counts[BIG[1]] == 198 and labels[TRIPLE[1]] == -1 and counts[TRIPLE[1]] == 1
    assert info["members"] == N - len(gone) and info["pairs_measured"] == 2 * ((N - len(gone)) * (N - len(gone) - 1) // 2)


def test_fewer_than_two_members_launch_nothing():
    import hnswindex
    zeros = dict.fromkeys(INFO, 0)
    empty = hnswindex.Index(DIM, "sq_euclid")
    labels, counts, info = empty.density_clusters(1.0, 2)
    assert labels.size == 0 and counts.size == 0 and info == zeros and empty.neighbor_counts(1.0).size == 0
    one = _index(DIM, "sq_euclid", 16)
    one.add(uniform(1, DIM, 3))
    one.reset_stats()
    labels, counts, info = one.density_clusters(float("inf"), 1)
    assert labels.tolist() == [0] and counts.tolist() == [0] and info == {**zeros, "members": 1, "clusters": 1, "core": 1}
    labels, counts, info = one.density_clusters(float("inf"), 2)
    assert labels.tolist() == [-1] and counts.tolist() == [0] and info == {**zeros, "members": 1, "noise": 1}
    assert one.neighbor_counts(1.0).tolist() == [0]
    two = _index(DIM, "sq_euclid", 16)
    two.add(uniform(2, DIM, 3))
    two.reset_stats()
    labels, counts, info = two.density_clusters(float("inf"), 1, allowed=[1])           # one member of two items: nothing to measure either
    assert labels.tolist() == [-1, 1] and counts.tolist() == [-1, 0] and info["members"] == 1 and info["clusters"] == 1 and info["scans"] == 0
    labels, counts, info = two.density_clusters(float("inf"), 1, allowed=np.zeros(2, bool))
    assert labels.tolist() == [-1, -1] and counts.tolist() == [-1, -1] and info == zeros
    assert one.stats()["exact_launches"] == 0 and two.stats()["exact_launches"] == 0
    labels, counts, info = two.density_clusters(float("inf"), 2)
    assert labels.tolist() == [0, 0] and counts.tolist() == [1, 1]
    assert info == {"members": 2, "clusters": 1, "core": 2, "border": 0, "noise": 0, "pairs_within": 1, "pairs_measured": 1, "scans": 1}
    assert two.stats()["exact_launches"] == 1
    labels, counts, info = two.density_clusters(float("inf"), 3)
    assert labels.tolist() == [-1, -1] and counts.tolist() == [1, 1] and info["noise"] == 2 and info["clusters"] == 0
    assert two.neighbor_counts(float("inf")).tolist() == [1, 1] and two.stats()["exact_launches"] == 3


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_device_backend_matches_the_index_and_leaves_the_resident_set(cases, monkeypatch, metric):
    import hnswindex
    c = cases(metric)
    dev = hnswindex.DeviceBackend(DIM, metric, capacity=N)
    dev.upload_rows(0, c.x)
    q = uniform(6, DIM, 43)
    dev.set_queries(q)
    before = dev.exact_range_grouped(None, 3.5, np.zeros(N, np.int32), np.zeros(6, np.int32), 1)   # answered from the resident set
    for knobs in ({}, dict(SMALL, density_pair_cap=1)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for ms in (3, MIN_SAMPLES):
            _same(dev.exact_range_density(c.r, ms, N), c.want(ms, 2 if knobs else 1), (metric, knobs, ms))
        labels, counts, info = dev.exact_range_density(c.r, MIN_SAMPLES, N, labels=False)
        assert labels is None and counts.tobytes() == c.want(1)[1].tobytes() and info == counts_only_info(c.want(MIN_SAMPLES)[2])
    after = dev.exact_range_grouped(None, 3.5, np.zeros(N, np.int32), np.zeros(6, np.int32), 1)
    assert all(a.tolist() == b.tolist() and u.tobytes() == v.tobytes() for a, b, u, v in zip(before[0], after[0], before[1], after[1]))
    # rows [0, 1000) with an allow-set on top: the other ids are no members, and the arrays end at n_rows
    allowed = np.arange(1, 1000)
    labels, counts, info = dev.exact_range_density(c.r, 3, 1000, allowed=allowed)
    pairs = [p for p in c.pairs if 1 <= p[0] < 1000 and p[1] < 1000]
    _same((labels, counts, info), clusters_from_pairs(1000, allowed, pairs, 3, scans=2))
    assert labels.shape == counts.shape == (1000,) and labels[0] == counts[0] == -1 and info["members"] == 999
