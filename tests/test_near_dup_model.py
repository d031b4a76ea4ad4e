"""CPU tier: the numpy statement of the near-duplicate contracts (tests/near_dup_model.py) on rows small enough to check by hand --
the range list of a stored item (order, own id dropped, allow-sets, vacant slots) and the single-linkage groups (a duplicate under a
smaller id, a chain whose ends are farther apart than the radius, labels that are the smallest ids, -1 off the members)."""
import numpy as np

from near_dup_model import duplicate_groups, exact_range_by_id, groups_from_pairs, groups_from_range_lists, within_by_distance_and_id

# points on a line: 0 and 5 are the same point (5 is the duplicate under the LARGER id, 0 under the smaller); 1 - 2 - 3 is a chain
# with steps of 1 and ends 2 apart; 4 is far from everything
X = np.array([[0.0], [10.0], [11.0], [12.0], [50.0], [0.0], [10.5]], np.float32)


def dist_to(own, cand):
    d = X[np.asarray(cand, np.int64), 0] - X[own, 0]
    return (d * d).astype(np.float32)


def test_range_list_order_and_own_id():
    ids, d = exact_range_by_id(dist_to, np.arange(7), [5, 0, 2, 2, 4], 1.0)
    assert ids[0].tolist() == [0] and d[0].tolist() == [0.0]            # the duplicate under the smaller id: an ordinary result
    assert ids[1].tolist() == [5]                                       # ... and under the larger; neither list holds its own id
    assert ids[2].tolist() == [6, 1, 3] and d[2].tolist() == [0.25, 1.0, 1.0]   # ascending (distance, id): 1 before 3 at one distance
    assert ids[3].tolist() == ids[2].tolist() and ids[4].size == 0      # an id twice; a singleton
    assert all(a.dtype == np.int32 and b.dtype == np.float32 for a, b in zip(ids, d))


def test_range_list_radius_edge_cases():
    every = exact_range_by_id(dist_to, np.arange(7), [2], np.inf)[0][0]
    assert sorted(every.tolist()) == [0, 1, 3, 4, 5, 6]
    assert exact_range_by_id(dist_to, np.arange(7), [2], np.nan)[0][0].size == 0
    assert exact_range_by_id(dist_to, np.arange(7), [2], -1.0)[0][0].size == 0
    ids, d = within_by_distance_and_id(np.array([np.nan, -0.0, 0.0, 1.0], np.float32), np.array([9, 8, 7, 6]), np.inf)
    assert ids.tolist() == [7, 8, 6] and np.signbit(d[1]) and not np.signbit(d[0])   # a NaN distance is never within; -0 == +0: the id decides


def test_range_list_allow_sets_and_vacant_slots():
    allowed = np.array([1, 1, 0, 1, 1, 1, 1], bool)
    ids, _ = exact_range_by_id(dist_to, np.arange(7), [2, 1], 1.0, allowed)
    assert ids[0].tolist() == [6, 1, 3]                                 # a set that lacks the own id changes nothing for that query
    assert ids[1].tolist() == [6]                                       # ... and 2 is no candidate of 1
    assert exact_range_by_id(dist_to, np.arange(7), [2], 1.0, [2])[0][0].size == 0          # only the own id: empty
    live = np.array([0, 1, 2, 3, 4, 6])                                 # slot 5 is vacant
    assert exact_range_by_id(dist_to, live, [0], 1.0)[0][0].size == 0


def test_groups_chain_duplicate_labels_and_non_members():
    labels, info = duplicate_groups(dist_to, 7, np.arange(7), 1.0)
    assert labels.tolist() == [0, 1, 1, 1, 4, 0, 1] and labels.dtype == np.int32     # 1 - 2 - 3 one group although d(1, 3) = 4 > 1
    assert info == {"members": 7, "groups": 3, "pairs_within": 5, "pairs_measured": 21}   # (0,5) (1,2) (1,6) (2,3) (2,6)
    # without 2 the chain falls apart, but 6 still joins 1; 2 is -1 and joins nobody although it lies between two members
    labels, info = duplicate_groups(dist_to, 7, np.arange(7), 1.0, allowed=[0, 1, 3, 4, 5, 6])
    assert labels.tolist() == [0, 1, -1, 3, 4, 0, 1] and info["members"] == 6 and info["groups"] == 4 and info["pairs_measured"] == 15
    # a vacant slot under the smallest id of a group: the label is the smallest MEMBER
    labels, _ = duplicate_groups(dist_to, 7, np.array([2, 3, 4, 5, 6]), 1.0)
    assert labels.tolist() == [-1, -1, 2, 2, 4, 5, 2]
    assert duplicate_groups(dist_to, 7, np.arange(7), np.nan)[0].tolist() == list(range(7))
    assert duplicate_groups(dist_to, 7, np.arange(7), np.inf)[0].tolist() == [0] * 7
    labels, info = duplicate_groups(dist_to, 3, [], 1.0)
    assert labels.tolist() == [-1, -1, -1] and info == {"members": 0, "groups": 0, "pairs_within": 0, "pairs_measured": 0}


def test_groups_do_not_depend_on_the_order_of_the_pairs():
    pairs = [(0, 5), (1, 2), (1, 6), (2, 3), (2, 6)]
    want = groups_from_pairs(7, np.arange(7), pairs).tolist()
    rng = np.random.default_rng(0)
    for _ in range(20):
        p = [pairs[i] for i in rng.permutation(len(pairs))]
        assert groups_from_pairs(7, np.arange(7), [(b, a) if rng.random() < 0.5 else (a, b) for a, b in p]).tolist() == want


def test_groups_from_range_lists_equal_groups_from_distances():
    members = np.arange(7)
    lists, _ = exact_range_by_id(dist_to, members, members, 1.0)
    labels, info = groups_from_range_lists(7, members, lists)
    want = duplicate_groups(dist_to, 7, members, 1.0)
    assert labels.tolist() == want[0].tolist() and info == want[1]
