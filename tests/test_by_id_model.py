"""CPU tier: the numpy statement of the by-id contracts (tests/by_id_model.py) -- top-k by (distance, id) over every candidate but
the query's own id -- and the properties the device code is built on: why the exclusion sits in the scan's sink and is not "ask for
k + 1, drop the first", and where padding begins."""
import numpy as np

from by_id_model import all_but, candidates, drop_first_of_k_plus_1, exact_knn_by_id, top_k_by_distance_and_id


def _sq(rows):
    """Squared Euclidean distances of stored rows on an integer grid: exact in float32 whatever the order of the sum."""
    rows = np.asarray(rows, np.float32)
    return lambda own, cand: ((rows[cand] - rows[own]) ** 2).sum(axis=1, dtype=np.float32)


def _grid(n, dim, seed):
    return np.random.default_rng(seed).integers(0, 5, (n, dim)).astype(np.float32)


def test_top_k_orders_by_distance_then_id_and_pads():
    ids, d = top_k_by_distance_and_id([2.0, 0.0, 2.0, -0.0, np.nan], [9, 7, 3, 5, 1], 7)
    assert ids.tolist() == [5, 7, 3, 9, 1, -1, -1]                     # -0 == +0: id 5 before id 7; the tie at 2.0 by id; NaN last
    assert d[:4].tolist() == [0.0, 0.0, 2.0, 2.0] and np.signbit(d[0]) and np.isnan(d[4:]).all()
    assert top_k_by_distance_and_id([], [], 2)[0].tolist() == [-1, -1]


def test_dropping_the_first_of_k_plus_1_is_wrong_when_a_duplicate_has_a_smaller_id():
    rows = _grid(40, 6, 1)
    rows[31] = rows[4]                                                  # id 31's row is stored under the smaller id 4 as well
    live = np.arange(40)
    want = exact_knn_by_id(_sq(rows), live, [31, 4, 10], 5)
    short = drop_first_of_k_plus_1(_sq(rows), live, [31, 4, 10], 5)
    # the contract: the duplicate comes first, at distance 0, and the query's own id never appears
    assert want[0][0, 0] == 4 and want[1][0, 0] == 0.0 and 31 not in want[0][0]
    assert want[0][1, 0] == 31 and want[1][1, 0] == 0.0 and 4 not in want[0][1]
    # the shortcut drops id 4 -- the first of (0, 4), (0, 31) -- and returns the query itself
    assert short[0][0, 0] == 31 and 4 not in short[0][0]
    assert not (short[0][0] == want[0][0]).all()
    # where the row has no duplicate under a smaller id the two agree: the shortcut's fault shows only on such inputs
    assert (short[0][1:] == want[0][1:]).all() and short[1][1:].tobytes() == want[1][1:].tobytes()


def test_rows_are_unique_and_ascending_by_distance_then_id():
    rows = _grid(60, 3, 2)                                              # a coarse grid: many equal distances
    ids, d = exact_knn_by_id(_sq(rows), np.arange(60), np.arange(60), 12)
    for i in range(60):
        assert i not in ids[i] and np.unique(ids[i]).size == 12
        assert all((d[i, j], ids[i, j]) < (d[i, j + 1], ids[i, j + 1]) for j in range(11))


def test_padding_begins_where_k_reaches_the_other_items():
    rows = _grid(9, 4, 3)
    live = np.arange(9)
    for k in (7, 8, 9, 20):                                             # n - 2, n - 1, n, beyond
        ids, d = exact_knn_by_id(_sq(rows), live, live, k)
        valid = min(k, 8)                                               # an index of n items gives at most n - 1 results
        assert (ids[:, :valid] >= 0).all() and (ids[:, valid:] == -1).all() and np.isnan(d[:, valid:]).all()
        assert all(sorted(ids[i, :8].tolist()) == [j for j in range(9) if j != i] for i in range(9)) or k < 8
    one = exact_knn_by_id(_sq(rows[:1]), [0], [0, 0], 3)                # one item: nothing but itself
    assert (one[0] == -1).all() and np.isnan(one[1]).all()


def test_allowed_sets_and_vacant_slots():
    rows = _grid(30, 4, 4)
    live = np.delete(np.arange(30), [3, 17])                            # ids 3 and 17 are vacant
    allowed = np.zeros(30, bool)
    allowed[[3, 5, 6, 8, 20]] = True                                    # (3 is allowed but not live)
    assert candidates(live, allowed).tolist() == [5, 6, 8, 20] == candidates(live, [20, 8, 3, 6, 5]).tolist()
    ids, _ = exact_knn_by_id(_sq(rows), live, [5, 9], 6, allowed)
    assert sorted(ids[0][ids[0] >= 0].tolist()) == [6, 8, 20]           # the query's own id leaves the set
    assert sorted(ids[1][ids[1] >= 0].tolist()) == [5, 6, 8, 20]        # a set that does not hold the id answers normally
    only_self = exact_knn_by_id(_sq(rows), live, [5], 2, [5])
    assert (only_self[0] == -1).all() and np.isnan(only_self[1]).all()   # a set that holds only the id itself: padding
    assert all_but(5, 2).tolist() == [True, True, False, True, True]
