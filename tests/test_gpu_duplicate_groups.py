"""GPU tier: duplicate_groups -- single-linkage groups of near-duplicates from one flat scan whose sink is a
union-find on the device.  3 000 rows x dim 20, six row kinds, planted structure on top of uniform rows: an exact triple of duplicates;
a chain whose ends are farther apart than the radius; a cluster that straddles a chunk edge and two tile edges; one cluster of 200
tight rows, which puts many unions on one root; everything else singletons.  The radius lies between the largest planted-link
distance and the smallest distance of any other pair, both worked out here in numpy.  The labels must equal the plain union-find
(tests/near_dup_model.py) over the lists exact_range_query_by_id returns, and on float32 rows over the oracle's distances; and they
must not depend on chunks, tiles, rounds or the order the device finds the pairs in."""
import ctypes as ct

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from near_dup_model import duplicate_groups, groups_from_range_lists

pytestmark = pytest.mark.gpu

N, DIM = 3000, 20
CHUNK, QTILE, ROUND = 700, 8, 512              # five chunks; tiles of 8 members; six rounds of 512 members
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
TRIPLE = [100, 1500, 2900]                     # one row under three ids
CHAIN = [1399, 1400, 2000]                     # a - b - c in steps of STEP: the ends are 2 STEP apart; 1399 | 1400 is a chunk edge
STRADDLE = list(range(694, 706))               # around the chunk edge 700 and the tile edges 696 and 704
STEP, NOISE = np.float32(0.1414), 0.01         # the chain's step along a unit direction; the clusters' half-width per element


def _big():
    taken = set(TRIPLE + CHAIN + STRADDLE)
    ids = [i for i in np.random.default_rng(9).permutation(N).tolist() if i not in taken][:200]
    return sorted(ids)


BIG = _big()


def _rows(metric):
    rng = np.random.default_rng(77)
    x = uniform(N, DIM, 1).copy()
    x[TRIPLE[1]] = x[TRIPLE[0]]
    x[TRIPLE[2]] = x[TRIPLE[0]]
    u = rng.standard_normal(DIM).astype(np.float32)
    u /= np.linalg.norm(u)
    x[CHAIN[1]] = x[CHAIN[0]] + STEP * u
    x[CHAIN[2]] = x[CHAIN[0]] + 2 * STEP * u
    for ids in (STRADDLE, BIG):
        x[ids] = x[ids[0]] + rng.uniform(-NOISE, NOISE, (len(ids), DIM)).astype(np.float32)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _links():
    """The planted pairs that are to be within the radius."""
    out = {(TRIPLE[0], TRIPLE[1]), (TRIPLE[0], TRIPLE[2]), (TRIPLE[1], TRIPLE[2]), (CHAIN[0], CHAIN[1]), (CHAIN[1], CHAIN[2])}
    for ids in (STRADDLE, BIG):
        out |= {(a, b) for i, a in enumerate(ids) for b in ids[i + 1:]}
    return out


def _numpy_dist(metric, x):
    """float64 distances of every pair of rows by the metric's formula (half-precision kinds: on the rounded rows)."""
    x = (x.astype(np.float16) if metric.endswith("_f16") else x).astype(np.float64)
    g = x @ x.T
    n2 = np.diag(g)
    if metric.startswith("sq_euclid"):
        return n2[:, None] + n2[None, :] - 2 * g
    return 1.0 - g if metric.startswith("ucosine") else 1.0 - g / np.sqrt(n2[:, None] * n2[None, :])


def _radius(metric, x):
    """Between the largest planted-link distance and the smallest distance of any other pair a < b (the chain's ends among them)."""
    d = _numpy_dist(metric, x)
    link = np.zeros((N, N), bool)
    a, b = np.array(sorted(_links())).T
    link[a, b] = True
    upper = np.triu(np.ones((N, N), bool), 1)
    largest_link, smallest_other = d[link].max(), d[upper & ~link].min()
    assert 0 < largest_link * 2 < smallest_other <= d[CHAIN[0], CHAIN[2]] * 1.001, (metric, largest_link, smallest_other)
    return float(np.float32(np.sqrt(largest_link * smallest_other)))


def _index(dim, metric, n):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(8); ix.set_insert_batch(0)
    return ix


def _planted_labels():
    want = np.arange(N, dtype=np.int32)
    for ids in (TRIPLE, CHAIN, STRADDLE, BIG):
        want[ids] = min(ids)
    return want


def _oracle_dist(metric, rows):
    import oracle
    return lambda own, cand: oracle.dist_query_rows(metric, rows, rows[own], cand) if cand.size else np.zeros(0, np.float32)


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x = _rows(metric)
        self.r = _radius(metric, self.x)
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        lists, _ = self.ix.exact_range_query_by_id(np.arange(N), self.r)
        self.want = groups_from_range_lists(N, np.arange(N), lists)      # the model over the range lists, computed once
        self.want[0].setflags(write=False)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


def test_the_plant_straddles_the_edges():
    assert STRADDLE[0] < 696 < CHUNK < 704 < STRADDLE[-1] and CHAIN[1] == 2 * CHUNK and len(BIG) == 200 and -(-N // ROUND) == 6
    assert len(set(TRIPLE + CHAIN + STRADDLE + BIG)) == 3 + 3 + 12 + 200
    assert {b // CHUNK for b in BIG} == {0, 1, 2, 3, 4} and {b // ROUND for b in BIG} == set(range(6))


@pytest.mark.parametrize("metric", METRICS)
def test_groups_are_the_model_over_the_range_lists(cases, monkeypatch, metric):
    c = cases(metric)
    want_labels, want_info = c.want
    m = N
    assert want_info["pairs_measured"] == m * (m - 1) // 2 and want_info["members"] == m
    # the plant came out as planted: the chain is one group although its ends are apart, the clusters have one root each
    assert want_labels.tolist() == _planted_labels().tolist(), metric
    assert want_info["groups"] == N - 2 - 2 - 11 - 199 and want_info["pairs_within"] == len(_links())
    first = None
    for knobs, launches in (({}, 1), (dict(exact_chunk=CHUNK, exact_qtile=QTILE), 1), (dict(exact_chunk=CHUNK, exact_qtile=QTILE, exact_union_round=ROUND), 6),
                            (dict(exact_chunk=0, exact_qtile=0, exact_union_round=ROUND), 6)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for _ in range(3):                                               # the unions arrive in another order every time
            c.ix.reset_stats()
            labels, info = c.ix.duplicate_groups(c.r)
            st = c.ix.stats()
            assert labels.dtype == np.int32 and labels.tobytes() == want_labels.tobytes(), (metric, knobs)
            assert info == want_info, (metric, knobs, info)
            assert st["exact_launches"] == launches and st["exact_evals"] == m * (m - 1) // 2 and st["search_launches"] == 0, (metric, knobs, st)
            first = first or (labels.tobytes(), info)
            assert (labels.tobytes(), info) == first


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine"])
def test_groups_are_the_model_over_the_oracles_distances(cases, metric):
    c = cases(metric)
    want_labels, want_info = duplicate_groups(_oracle_dist(metric, c.x), N, np.arange(N), c.r)
    labels, info = c.ix.duplicate_groups(c.r)
    assert labels.tobytes() == want_labels.tobytes() and info == want_info, metric


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_allowed_sets_nan_and_infinity(cases, monkeypatch, metric):
    c = cases(metric)
    set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE, exact_union_round=ROUND)
    # the chain's middle, the triple's smallest id and part of the straddling cluster are not allowed: -1, and they join nobody
    allowed = np.ones(N, bool)
    out = [CHAIN[1], TRIPLE[0]] + STRADDLE[:4] + BIG[::2] + list(range(2100, 2400))
    allowed[out] = False
    members = np.flatnonzero(allowed)
    lists, _ = c.ix.exact_range_query_by_id(members, c.r, allowed=allowed)
    want_labels, want_info = groups_from_range_lists(N, members, lists)
    labels, info = c.ix.duplicate_groups(c.r, allowed=allowed)
    assert labels.tobytes() == want_labels.tobytes() and info == want_info and info["pairs_measured"] == members.size * (members.size - 1) // 2
    assert (labels[out] == -1).all() and (labels[members] >= 0).all()
    assert labels[CHAIN[0]] == CHAIN[0] and labels[CHAIN[2]] == CHAIN[2]                 # the chain fell apart: its middle is no member
    assert labels[TRIPLE[1]] == labels[TRIPLE[2]] == TRIPLE[1] and labels[STRADDLE[-1]] == STRADDLE[4]
    as_ids = c.ix.duplicate_groups(c.r, allowed=members)                                  # the set as an id list
    assert as_ids[0].tobytes() == labels.tobytes() and as_ids[1] == info
    # NaN: every member its own group; +inf: one group
    labels, info = c.ix.duplicate_groups(float("nan"))
    assert labels.tolist() == list(range(N)) and info == {"members": N, "groups": N, "pairs_within": 0, "pairs_measured": N * (N - 1) // 2}
    labels, info = c.ix.duplicate_groups(float("inf"), allowed=allowed)
    assert (labels[members] == members[0]).all() and (labels[out] == -1).all()
    assert info == {"members": members.size, "groups": 1, "pairs_within": members.size * (members.size - 1) // 2, "pairs_measured": members.size * (members.size - 1) // 2}
    labels, info = c.ix.duplicate_groups(-1.0)                                            # a negative radius is ordinary: nothing is within it here
    assert labels.tolist() == list(range(N)) and info["pairs_within"] == 0


def test_removed_ids_are_no_members():
    n = 300
    x = uniform(n, DIM, 23).copy()
    x[[10, 150, 290]] = x[10]                                             # a triple whose smallest id is removed below
    x[201] = x[200] + np.float32(0.05)
    x[202] = x[200] + np.float32(0.10)                                    # a chain 200 - 201 - 202 whose middle is removed below
    ix = _index(DIM, "sq_euclid", n)
    ix.add(x)
    r = 0.06                                                              # 20 * 0.05^2 = 0.05 < r < 20 * 0.1^2 = 0.2; the background is far above
    labels, info = ix.duplicate_groups(r)
    assert labels[[10, 150, 290]].tolist() == [10, 10, 10] and labels[[200, 201, 202]].tolist() == [200, 200, 200] and info["groups"] == n - 4
    ix.remove([10, 201])
    live = np.delete(np.arange(n), [10, 201])
    labels, info = ix.duplicate_groups(r)
    want = duplicate_groups(_oracle_dist("sq_euclid", x), n, live, r)
    assert labels.tobytes() == want[0].tobytes() and info == want[1]
    assert labels[[10, 201]].tolist() == [-1, -1] and labels[[150, 290]].tolist() == [150, 150] and labels[[200, 202]].tolist() == [200, 202]
    assert info == {"members": n - 2, "groups": n - 3, "pairs_within": 1, "pairs_measured": (n - 2) * (n - 3) // 2}


def test_the_default_chunks_past_one_chunk():
    """Nothing forced on 4 500 rows: the call cuts its members into chunks of about 2 048 rows -- two here -- so that blocks below the
    diagonal leave early.  Grid rows (elements 1 .. 3, dim 6: 729 distinct rows): the groups are the distinct rows, each labelled with
    the id it occurs under first; every group spans both chunks."""
    n, dim = 4500, 6
    x = np.random.default_rng(2).integers(1, 4, (n, dim)).astype(np.float32)
    ix = _index(dim, "sq_euclid", n)
    ix.add(x)
    _, first, inverse = np.unique(x, axis=0, return_index=True, return_inverse=True)
    want = first[inverse.ravel()].astype(np.int32)
    for r in (0.0, 0.5):                                                  # the nearest distinct row is 1.0 away
        ix.reset_stats()
        labels, info = ix.duplicate_groups(r)
        assert labels.tobytes() == want.tobytes() and info["groups"] == first.size and info["pairs_measured"] == n * (n - 1) // 2
        assert info["pairs_within"] == int(sum(c * (c - 1) // 2 for c in np.bincount(inverse.ravel())))
        assert ix.stats()["exact_launches"] == 1 and ix.stats()["exact_evals"] == n * (n - 1) // 2
    allowed = np.random.default_rng(3).random(n) < 0.7                    # members that are no run of ids
    members = np.flatnonzero(allowed)
    _, first, inverse = np.unique(x[members], axis=0, return_index=True, return_inverse=True)
    want = np.full(n, -1, np.int32)
    want[members] = members[first[inverse.ravel()]]
    labels, info = ix.duplicate_groups(0.5, allowed=allowed)
    assert labels.tobytes() == want.tobytes() and info["members"] == members.size and info["groups"] == first.size


def test_fewer_than_two_members_launch_nothing():
    import hnswindex
    empty = hnswindex.Index(DIM, "sq_euclid")
    labels, info = empty.duplicate_groups(1.0)
    assert labels.size == 0 and info == {"members": 0, "groups": 0, "pairs_within": 0, "pairs_measured": 0}
    one = _index(DIM, "sq_euclid", 16)
    one.add(uniform(1, DIM, 3))
    one.reset_stats()
    labels, info = one.duplicate_groups(float("inf"))
    assert labels.tolist() == [0] and info == {"members": 1, "groups": 1, "pairs_within": 0, "pairs_measured": 0}
    two = _index(DIM, "sq_euclid", 16)
    two.add(uniform(2, DIM, 3))
    two.reset_stats()
    labels, info = two.duplicate_groups(float("inf"), allowed=[1])        # one member of two items: nothing to measure either
    assert labels.tolist() == [-1, 1] and info["members"] == 1 and info["groups"] == 1
    labels, info = two.duplicate_groups(float("inf"), allowed=np.zeros(2, bool))
    assert labels.tolist() == [-1, -1] and info["members"] == 0
    assert one.stats()["exact_launches"] == 0 and two.stats()["exact_launches"] == 0
    labels, info = two.duplicate_groups(float("inf"))
    assert labels.tolist() == [0, 0] and info == {"members": 2, "groups": 1, "pairs_within": 1, "pairs_measured": 1} and two.stats()["exact_launches"] == 1
    # cap below the length: -1 and a message
    import importlib
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)
    out, inf = np.full(2, 7, np.int32), (ct.c_uint64 * 4)()
    assert net.lib.hnsw_mi355x_duplicate_groups(two._h, 1.0, None, 0, out.ctypes.data_as(ct.POINTER(ct.c_int)), 1, inf) == -1
    assert "cap = 1 is below the index's length of 2" in net.last_error() and (out == 7).all() and two.stats()["exact_launches"] == 1


def test_device_backend_groups_leave_the_resident_set_and_pending_results():
    import hnswindex
    n = 900
    x = uniform(n, 33, 41).copy()
    x[[5, 450, 899]] = x[5]
    dev = hnswindex.DeviceBackend(33, "sq_euclid", capacity=n)
    dev.upload_rows(0, x)
    q = uniform(6, 33, 43)
    dev.set_queries(q)
    before = dev.exact_range_grouped(None, 3.5, np.zeros(n, np.int32), np.zeros(6, np.int32), 1)   # answered from the resident set
    pending = dev.exact_range(q[:3], 3.2)                                                          # ... and these results stay pending
    total = sum(l.size for l in pending[0])
    assert total > 0
    labels, info = dev.exact_range_groups(1e-6, n)
    assert labels.tolist() == [5 if v in (450, 899) else v for v in range(n)] and info == {"members": n, "groups": n - 2, "pairs_within": 3, "pairs_measured": n * (n - 1) // 2}
    ids, d = np.empty(total, np.int32), np.empty(total, np.float32)
    assert hnswindex.net_amd.lib.hnswdev_exact_range_results(dev._ctx, ids.ctypes.data_as(ct.POINTER(ct.c_int)), d.ctypes.data_as(ct.POINTER(ct.c_float))) == 0
    assert ids.tolist() == np.concatenate(pending[0]).tolist() and d.tobytes() == np.concatenate(pending[1]).tobytes()
    after = dev.exact_range_grouped(None, 3.5, np.zeros(n, np.int32), np.zeros(6, np.int32), 1)
    assert all(a.tolist() == b.tolist() and u.tobytes() == v.tobytes() for a, b, u, v in zip(before[0], after[0], before[1], after[1]))
    assert sum(l.size for l in after[0]) > 0
    # rows [0, 500): 899 is no member; an allow-set on top
    labels, info = dev.exact_range_groups(1e-6, 500, allowed=np.arange(1, 500))
    assert labels.shape == (500,) and labels[0] == -1 and labels[450] == 5 and info["members"] == 499 and info["groups"] == 498
