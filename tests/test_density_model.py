"""CPU tier: the numpy statement of the density clusters' contract (tests/density_model.py) on inputs small enough to check by hand --
counts, core / border / noise, the label of a cluster, where a border goes, and the two settings at which the call is
duplicate_groups again."""
import numpy as np
import pytest

from density_model import (INFO, clusters_from_pairs, counts_only_info, density_clusters, neighbor_counts, pairs_from_range_lists,
                           pairs_within_d)
from near_dup_model import duplicate_groups, exact_range_by_id

FAR = np.float32(100.0)


def table(n, near):
    """dist_to over an n x n table: FAR everywhere but the pairs of `near` ((a, b) -> d, a < b: the row of a is the query)."""
    t = np.full((n, n), FAR, np.float32)
    for (a, b), d in near.items():
        assert a < b
        t[a, b] = d
        t[b, a] = np.float32(99.0)                               # never read: a pair is measured from its smaller id
    return lambda own, cand: t[own, np.asarray(cand, np.int64)]


def mutual(ids, d=0.1):
    return {(a, b): np.float32(d) for i, a in enumerate(ids) for b in ids[i + 1:]}


# points on a line, squared distance, radius 1: 0 1 2 are mutually within; 3 reaches 2 alone; 4 is alone; 5 6 7 are mutually within;
# 8 and 9 are within each other and nobody else
LINE = np.array([0.0, 0.5, 1.0, 1.9, 10.0, 20.0, 20.5, 21.0, 30.0, 30.5], np.float32)


def line_dist(own, cand):
    d = LINE[np.asarray(cand, np.int64)] - LINE[own]
    return (d * d).astype(np.float32)


def test_hand_written_example():
    labels, counts, info = density_clusters(line_dist, 10, np.arange(10), 1.0, 3)
    assert counts.tolist() == [2, 2, 3, 1, 0, 2, 2, 2, 1, 1] and counts.dtype == np.int32
    # 3 is a border of the cluster of 0 (its one neighbour, 2, is core); 4 is noise; 8 and 9 have each other and no core: noise both
    assert labels.tolist() == [0, 0, 0, 0, -1, 5, 5, 5, -1, -1] and labels.dtype == np.int32
    assert info == {"members": 10, "clusters": 2, "core": 6, "border": 1, "noise": 3, "pairs_within": 8, "pairs_measured": 45, "scans": 1}
    assert tuple(info) == INFO
    # min_samples 4: only 2 is core (3 + 1), and its three neighbours are its borders
    labels, counts4, info = density_clusters(line_dist, 10, np.arange(10), 1.0, 4)
    assert counts4.tolist() == counts.tolist() and labels.tolist() == [2, 2, 2, 2, -1, -1, -1, -1, -1, -1]
    assert (info["clusters"], info["core"], info["border"], info["noise"]) == (1, 1, 3, 6)
    # nobody is core: noise only, the counts as before
    labels, counts5, info = density_clusters(line_dist, 10, np.arange(10), 1.0, 5)
    assert (labels == -1).all() and counts5.tolist() == counts.tolist() and (info["clusters"], info["core"], info["border"], info["noise"]) == (0, 0, 0, 10)
    with pytest.raises(ValueError, match="min_samples = 0 is below 1"):
        density_clusters(line_dist, 10, np.arange(10), 1.0, 0)
    assert counts_only_info(info) == {**info, "noise": 0}


def test_a_border_between_two_clusters_goes_to_the_nearer_core():
    # B = {0, 1, 2, 3} holds the smaller ids; A = {4, 5, 6, 7}; 8 is within core 1 of B at 0.5 and within core 5 of A at 0.3
    near = {**mutual([0, 1, 2, 3]), **mutual([4, 5, 6, 7]), (1, 8): np.float32(0.5), (5, 8): np.float32(0.3)}
    labels, counts, info = density_clusters(table(9, near), 9, np.arange(9), 1.0, 4)
    assert counts.tolist() == [3, 4, 3, 3, 3, 4, 3, 3, 2]
    assert labels.tolist() == [0, 0, 0, 0, 4, 4, 4, 4, 4]       # not 0, the smaller label and the smaller core id: the nearer core decides
    assert (info["clusters"], info["core"], info["border"], info["noise"]) == (2, 8, 1, 0)
    # the border does not join the two clusters, whatever it is within
    assert labels[0] != labels[4]


def test_a_border_at_equal_distances_goes_to_the_smaller_core_id_not_the_smaller_label():
    # A = {0, 5, 6, 7} has the smaller label, 0; B = {1, 2, 3, 4}; 8 is within core 3 of B and core 5 of A at the same distance
    for d3, d5 in ((0.3, 0.3), (0.0, -0.0), (-0.0, 0.0)):
        near = {**mutual([0, 5, 6, 7]), **mutual([1, 2, 3, 4]), (3, 8): np.float32(d3), (5, 8): np.float32(d5)}
        labels, _, info = density_clusters(table(9, near), 9, np.arange(9), 1.0, 4)
        assert labels.tolist() == [0, 1, 1, 1, 1, 0, 0, 0, 1], (d3, d5)   # core 3 < core 5: the label of 3's cluster, 1, although 0 is smaller
        assert info["border"] == 1
    # the border under an id BELOW its cores (the pair is then measured from the border's row): the same rule
    near = {**mutual([1, 6, 7, 8]), **mutual([2, 3, 4, 5]), (0, 4): np.float32(0.3), (0, 6): np.float32(0.3)}
    labels, _, _ = density_clusters(table(9, near), 9, np.arange(9), 1.0, 4)
    assert labels.tolist() == [2, 1, 2, 2, 2, 2, 1, 1, 1]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 14))
    x = rng.random((n, 2)).astype(np.float32)

    def dist_to(own, cand):
        d = x[np.asarray(cand, np.int64)] - x[own]
        return (d * d).sum(1).astype(np.float32)
    live = np.flatnonzero(rng.random(n) < 0.85)
    return n, dist_to, live, float(rng.choice([0.02, 0.08, 0.2]))


@pytest.mark.parametrize("seed", range(30))
def test_min_samples_1_and_2_are_duplicate_groups(seed):
    n, dist_to, live, r = _random_case(seed)
    want, want_info = duplicate_groups(dist_to, n, live, r)
    labels, counts, info = density_clusters(dist_to, n, live, r, 1)
    assert labels.tobytes() == want.tobytes() and info["pairs_within"] == want_info["pairs_within"] and info["clusters"] == want_info["groups"]
    assert info["core"] == info["members"] == want_info["members"] and info["border"] == info["noise"] == 0
    labels2, counts2, info2 = density_clusters(dist_to, n, live, r, 2)
    singles = np.zeros(n, bool)
    singles[live] = counts[live] == 0
    assert labels2.tobytes() == np.where(singles, -1, want).astype(np.int32).tobytes() and counts2.tolist() == counts.tolist()
    assert info2["noise"] == int(singles.sum()) and info2["border"] == 0 and info2["clusters"] == want_info["groups"] - int(singles.sum())


def test_nan_infinite_and_negative_radius():
    labels, counts, info = density_clusters(line_dist, 10, np.arange(10), np.nan, 1)
    assert labels.tolist() == list(range(10)) and (counts == 0).all() and info["pairs_within"] == 0 and info["clusters"] == 10
    labels, counts, info = density_clusters(line_dist, 10, np.arange(10), np.nan, 2)
    assert (labels == -1).all() and (counts == 0).all() and info["noise"] == 10
    labels, counts, info = density_clusters(line_dist, 10, np.arange(10), np.inf, 10)
    assert (labels == 0).all() and (counts == 9).all() and (info["clusters"], info["core"], info["pairs_within"]) == (1, 10, 45)
    assert (density_clusters(line_dist, 10, np.arange(10), np.inf, 11)[0] == -1).all()
    labels, counts, info = density_clusters(line_dist, 10, np.arange(10), -1.0, 1)
    assert labels.tolist() == list(range(10)) and info["pairs_within"] == 0
    # a NaN distance is never within, whatever the radius
    nan_to = lambda own, cand: np.full(len(cand), np.nan, np.float32)
    assert density_clusters(nan_to, 4, np.arange(4), np.inf, 1)[2]["pairs_within"] == 0


def test_allowed_subsets_and_removed_ids():
    # without 2 nobody of the first cluster is core at min_samples 3, and 3 has no neighbour at all
    labels, counts, info = density_clusters(line_dist, 10, np.arange(10), 1.0, 3, allowed=[0, 1, 3, 4, 5, 6, 7, 8, 9])
    assert counts.tolist() == [1, 1, -1, 0, 0, 2, 2, 2, 1, 1] and labels.tolist() == [-1, -1, -1, -1, -1, 5, 5, 5, -1, -1]
    assert (info["members"], info["clusters"], info["core"], info["border"], info["noise"], info["pairs_measured"]) == (9, 1, 3, 0, 6, 36)
    mask = np.ones(10, bool)
    mask[2] = False
    as_mask = density_clusters(line_dist, 10, np.arange(10), 1.0, 3, allowed=mask)
    assert as_mask[0].tolist() == labels.tolist() and as_mask[1].tolist() == counts.tolist() and as_mask[2] == info
    # a removed id is no member: 5 gone, 6 and 7 have one neighbour each
    labels, counts, info = density_clusters(line_dist, 10, np.array([0, 1, 2, 3, 4, 6, 7, 8, 9]), 1.0, 3)
    assert counts.tolist() == [2, 2, 3, 1, 0, -1, 1, 1, 1, 1] and labels.tolist() == [0, 0, 0, 0, -1, -1, -1, -1, -1, -1]
    # no member, one member: nothing is measured; a lone member is core when it alone is enough
    labels, counts, info = density_clusters(line_dist, 3, [], 1.0, 1)
    assert labels.tolist() == counts.tolist() == [-1, -1, -1] and info == dict.fromkeys(INFO, 0)
    labels, counts, info = density_clusters(line_dist, 3, [1], 1.0, 1)
    assert labels.tolist() == [-1, 1, -1] and counts.tolist() == [-1, 0, -1] and info == {**dict.fromkeys(INFO, 0), "members": 1, "clusters": 1, "core": 1}
    labels, _, info = density_clusters(line_dist, 3, [1], 1.0, 2)
    assert labels.tolist() == [-1, -1, -1] and info["noise"] == 1 and info["scans"] == 0


def test_the_model_over_range_lists_equals_the_model_over_distances():
    members = np.arange(10)
    lists, dists = exact_range_by_id(line_dist, members, members, 1.0)
    pairs = pairs_from_range_lists(members, lists, dists)
    assert sorted(pairs) == sorted(pairs_within_d(line_dist, members, 1.0))
    assert neighbor_counts(10, members, pairs).tolist() == [2, 2, 3, 1, 0, 2, 2, 2, 1, 1]
    for ms in (1, 2, 3, 4):
        got, want = clusters_from_pairs(10, members, pairs, ms, scans=2), density_clusters(line_dist, 10, members, 1.0, ms, scans=2)
        assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and got[2] == want[2] and got[2]["pairs_measured"] == 90
