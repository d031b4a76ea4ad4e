"""GPU tier: exact_range_query_by_id and exact_radius_graph -- the range scan whose queries are stored rows and whose
sink drops the pair (query, its own row).  Byte for byte the per-id loop of existing calls it replaces --
exact_range_query(get_vectors([id]), r, allowed=<allowed, or every live id, minus id>) -- for every row kind, and on float32 rows the
numpy statement of the contract (tests/near_dup_model.py) over the oracle's distances.  The shapes of test_gpu_exact_by_id.py: 3 000
rows x dim 20, 48 query ids; exact_chunk / exact_qtile cut the rows into five chunks and the queries into six tiles, and the query ids
sit in the first chunk, in the last one and on both sides of a chunk's edge; one row is stored under three ids.  The radii are
quantiles of distances worked out here in numpy: about 0, about 10 and about 300 results per query."""
import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from near_dup_model import all_but, exact_range_by_id, range_by_id_loop

pytestmark = pytest.mark.gpu

N, DIM, NQ = 3000, 20, 48
CHUNK, QTILE = 700, 8                          # chunks [0, 700) .. [2800, 3000): five; 48 queries: six tiles
METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
A, DUP_LO, DUP_HI = 1500, 100, 2900            # the row of id A is stored under ids DUP_LO < A < DUP_HI as well
MUST = [0, 1, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, A, DUP_LO, DUP_HI, 7, 7, 2800, N - 1]
PER_QUERY = (0.2, 10, 300)                     # results per query the three radii aim at


def _data(metric, n, dim, seed):
    x = uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _rows(metric):
    x = _data(metric, N, DIM, 1).copy()
    x[DUP_LO] = x[A]
    x[DUP_HI] = x[A]
    return x


def _index(dim, metric, n):
    import hnswindex
    ix = hnswindex.Index(dim, metric)
    ix.set_collection_size(n); ix.set_max_edges(8); ix.set_insert_batch(0)
    return ix


def _query_ids():
    rest = [i for i in np.random.default_rng(5).permutation(N).tolist() if i not in MUST][:NQ - len(MUST)]
    return np.array(MUST + rest, np.int32)


def _numpy_dist(metric, x, q):
    """float64 distances of the rows q to the rows x by the metric's formula: what the radii are picked from, nothing else."""
    x, q = x.astype(np.float64), q.astype(np.float64)
    if metric.startswith("sq_euclid"):
        return ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    dot = q @ x.T
    return 1.0 - dot if metric.startswith("ucosine") else 1.0 - dot / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :])


def _radii(metric, x, qids):
    d = _numpy_dist(metric, x, x[qids])
    d[np.arange(qids.size), qids] = np.inf     # the own row is no result
    return [float(np.float32(np.quantile(d, per / N))) for per in PER_QUERY]


def _same(a, b):
    return len(a[0]) == len(b[0]) and all(x.tolist() == y.tolist() and u.tobytes() == v.tobytes() for x, y, u, v in zip(a[0], b[0], a[1], b[1]))


def _oracle_dist(metric, rows):
    """dist_to of tests/near_dup_model.py from the oracle: the distances of the stored row `own` to the candidates (float32 rows)."""
    import oracle
    return lambda own, cand: oracle.dist_query_rows(metric, rows, rows[own], cand) if cand.size else np.zeros(0, np.float32)


class Case:
    def __init__(self, metric):
        self.metric = metric
        self.x = _rows(metric)
        self.ix = _index(DIM, metric, N)
        assert (self.ix.add(self.x) == np.arange(N)).all()
        self.qids = _query_ids()
        self.radii = _radii(metric, self.x, self.qids)
        self._want = {}

    def want(self, r):
        if r not in self._want:
            self._want[r] = range_by_id_loop(self.ix, self.qids, r)
        return self._want[r]


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(metric):
        if metric not in cache:
            cache[metric] = Case(metric)
        return cache[metric]
    return get


def test_the_query_ids_sit_where_the_chunks_begin_and_end():
    q = _query_ids()
    assert q.size == NQ > QTILE and -(-N // CHUNK) == 5
    assert {0, 4} <= set((q // CHUNK).tolist()) and {CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, 2800, N - 1} <= set(q.tolist())
    assert (q == 7).sum() == 2 and {A, DUP_LO, DUP_HI} <= set(q.tolist())


@pytest.mark.parametrize("metric", METRICS)
def test_range_by_id_is_the_per_id_loop(cases, monkeypatch, metric):
    c = cases(metric)
    at = {int(q): i for i, q in enumerate(c.qids)}
    sizes = []
    for knobs in ({}, dict(exact_chunk=CHUNK, exact_qtile=QTILE)):
        if knobs:
            set_diag(monkeypatch, **knobs)
        for r in c.radii:
            c.ix.reset_stats()
            got = c.ix.exact_range_query_by_id(c.qids, r)
            st, info, rinfo = c.ix.stats(), c.ix.by_id_info(), c.ix.exact_range_info()
            assert _same(got, c.want(r)), (metric, knobs, r)
            assert not any((l == q).any() for l, q in zip(got[0], c.qids))
            total = sum(l.size for l in got[0])
            print(metric, knobs, r, "results per query", total / NQ)
            # every pair but the 48 (query, own row) pairs was measured, in one launch: nothing exceeded pass A's capacity
            assert st["exact_evals"] == NQ * N - NQ and st["exact_launches"] == 1 and st["search_launches"] == 0, (metric, knobs, r, st)
            assert info == {"calls": 1, "traversed": 0, "handbacks": 0, "scanned": NQ, "rows_gathered": NQ, "self_skipped": NQ}, info
            assert rinfo == {"device_sorted": sum(l.size >= 2 for l in got[0]), "host_sorted": 0, "repeated_rounds": 0, "results": total}, rinfo
            if not knobs:
                sizes.append(total / NQ)
            for own, others in ((A, [DUP_LO, DUP_HI]), (DUP_LO, [A, DUP_HI]), (DUP_HI, [DUP_LO, A])):
                ids, d = got[0][at[own]], got[1][at[own]]                    # the duplicates first, by id, at one distance
                assert ids[:2].tolist() == others and d[0].tobytes() == d[1].tobytes() and (ids.size == 2 or d[1] <= d[2]), (metric, own)
            rep = np.flatnonzero(c.qids == 7)
            assert got[0][rep[0]].tolist() == got[0][rep[1]].tolist() and got[1][rep[0]].tobytes() == got[1][rep[1]].tobytes()
    assert sizes[0] < 2 and 3 < sizes[1] < 30 and 100 < sizes[2] < 900, sizes    # about 0 (the duplicates apart), about 10, about 300


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine"])
def test_range_by_id_is_the_numpy_model_on_float32_rows(cases, monkeypatch, metric):
    c = cases(metric)
    for r in c.radii:
        want = exact_range_by_id(_oracle_dist(metric, c.x), np.arange(N), c.qids, r)
        assert _same(c.ix.exact_range_query_by_id(c.qids, r), want), (metric, r)
        set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE)
        assert _same(c.ix.exact_range_query_by_id(c.qids, r), want), (metric, r)
        set_diag(monkeypatch, exact_chunk=0, exact_qtile=0)


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8", "ucosine_f16"])
def test_repeated_pass_and_rounds_keep_the_bytes(cases, monkeypatch, metric):
    """exact_range_cap below the longest list: the round is cut into pieces that are scanned again with their own ids (self + q0);
    a small arena: several rounds.  The duplicates' lists are among those scanned again."""
    c = cases(metric)
    r = c.radii[2]
    want = c.want(r)
    at = {int(q): i for i, q in enumerate(c.qids)}
    longest = max(l.size for l in want[0])
    cap = 64
    assert all(want[0][at[o]].size > cap for o in (A, DUP_LO, DUP_HI)) and longest > cap
    arena = max(1600, longest + 1)
    set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE, exact_range_cap=cap, exact_range_arena=arena)
    c.ix.reset_stats()
    got = c.ix.exact_range_query_by_id(c.qids, r)
    rinfo, st = c.ix.exact_range_info(), c.ix.stats()
    assert _same(got, want), metric
    # rounds of arena / cap queries (1600 / 64 = 25: two) in pass A; every piece of pass B is one more launch, and the second
    # round's pieces read their ids from the middle of the call's
    rounds = -(-NQ // (arena // cap))
    assert rounds >= 2 and rinfo["repeated_rounds"] >= rounds and st["exact_launches"] == rounds + rinfo["repeated_rounds"], (rinfo, st)
    assert rinfo["results"] == sum(l.size for l in want[0])
    assert c.ix.by_id_info()["self_skipped"] == NQ
    # lists split between the device's order and the host's
    set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE, exact_range_sort=100)
    c.ix.reset_stats()
    got = c.ix.exact_range_query_by_id(c.qids, r)
    rinfo = c.ix.exact_range_info()
    assert _same(got, want), metric
    assert rinfo["host_sorted"] == sum(l.size > 100 for l in want[0]) > 0 and rinfo["device_sorted"] == sum(2 <= l.size <= 100 for l in want[0]) > 0, rinfo


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine"])
def test_negative_nan_and_infinite_radius(cases, metric):
    c = cases(metric)
    q = c.qids[:12]
    launches = c.ix.stats()["exact_launches"]
    ids, d = c.ix.exact_range_query_by_id(q, float("nan"))
    assert all(l.size == 0 for l in ids) and c.ix.stats()["exact_launches"] == launches + 1
    assert _same(c.ix.exact_range_query_by_id(q, -1.0), range_by_id_loop(c.ix, q, -1.0))
    got = c.ix.exact_range_query_by_id(q, float("inf"))
    assert _same(got, range_by_id_loop(c.ix, q, float("inf")))
    assert all(l.size == N - 1 and sorted(l.tolist()) == [j for j in range(N) if j != o] for l, o in zip(got[0], q))


def test_allowed_sets(cases, monkeypatch):
    c = cases("sq_euclid_i8")
    r = c.radii[2]
    set_diag(monkeypatch, exact_chunk=CHUNK, exact_qtile=QTILE)
    allowed = np.zeros(N, bool)
    allowed[np.random.default_rng(8).choice(N, 900, replace=False)] = True
    allowed[[0, A, DUP_LO, N - 1]] = True                                                 # some query ids are in the set ...
    allowed[[1, CHUNK, DUP_HI]] = False                                                   # ... and some are not: they answer normally
    inside = int(allowed[c.qids].sum())
    assert 4 <= inside < NQ
    c.ix.reset_stats()
    got = c.ix.exact_range_query_by_id(c.qids, r, allowed=allowed)
    assert c.ix.stats()["exact_evals"] == NQ * int(allowed.sum()) - inside and c.ix.by_id_info()["self_skipped"] == inside
    assert _same(got, range_by_id_loop(c.ix, c.qids, r, allowed)) and sum(l.size for l in got[0]) > NQ
    assert _same(c.ix.exact_range_query_by_id(c.qids, r, allowed=np.flatnonzero(allowed)), got)   # the set as an id list
    # a set that holds only the id itself: an empty list; beside a query whose id is not in it
    ids, d = c.ix.exact_range_query_by_id([A, 5, A], float("inf"), allowed=[A])
    assert ids[0].size == ids[2].size == 0 and ids[1].tolist() == [A]
    launches = c.ix.stats()["exact_launches"]
    ids, d = c.ix.exact_range_query_by_id([A], float("inf"), allowed=np.zeros(N, bool))   # a set that allows nothing: no launch
    assert ids[0].size == 0 and c.ix.stats()["exact_launches"] == launches


def test_a_removed_id_fails_with_its_name_and_is_no_result():
    n = 300
    x = _data("sq_euclid", n, DIM, 23)
    ix = _index(DIM, "sq_euclid", n)
    ix.add(x)
    ix.remove([5, 250])
    launches = ix.stats()["exact_launches"]
    with pytest.raises(RuntimeError, match=r"hnsw_mi355x_exact_range_query_by_id: ids\[1\] = 250 is not a live id"):
        ix.exact_range_query_by_id([3, 250], 1.0)
    assert ix.stats()["exact_launches"] == launches
    live = np.delete(np.arange(n), [5, 250])
    got = ix.exact_range_query_by_id([3, 299, 0], float("inf"))
    assert _same(got, exact_range_by_id(_oracle_dist("sq_euclid", x), live, [3, 299, 0], float("inf")))
    assert all(l.size == n - 3 for l in got[0])


@pytest.mark.parametrize("dim", [7, 136])
@pytest.mark.parametrize("metric", ["cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_other_row_lengths(metric, dim):
    n = 300
    x = _data(metric, n, dim, 40 + dim).copy()
    x[290] = x[10]
    ix = _index(dim, metric, n)
    ix.add(x)
    qids = np.array([0, 10, 290, 299, 150, 150], np.int32)
    d = _numpy_dist(metric, x, x[qids])
    d[np.arange(qids.size), qids] = np.inf
    for r in (float(np.quantile(d, 10 / n)), float(np.quantile(d, 0.5))):
        got = ix.exact_range_query_by_id(qids, r)
        assert _same(got, range_by_id_loop(ix, qids, r)), (metric, dim, r)
        assert got[0][1][0] == 290 and got[0][2][0] == 10
        if metric == "cosine":
            assert _same(got, exact_range_by_id(_oracle_dist(metric, x), np.arange(n), qids, r))


def test_device_backend_exact_range_by_id():
    """The inner boundary: rows a host uploaded itself; list by list hnswdev_exact_range for the gathered row with the id taken out."""
    import hnswindex
    n = 900
    x = _data("ucosine_f16", n, 33, 41)
    dev = hnswindex.DeviceBackend(33, "ucosine_f16", capacity=n)
    dev.upload_rows(0, x)
    qids = np.array([0, 899, 450, 450, 17], np.int32)
    d = _numpy_dist("ucosine_f16", x, x[qids])
    d[np.arange(qids.size), qids] = np.inf
    r = float(np.quantile(d, 20 / n))
    dev.reset_stats()
    ids, dist = dev.exact_range_by_id(qids, r)
    assert dev.stats()["exact_evals"] == 5 * n - 5 and sum(l.size for l in ids) > 20
    for i, own in enumerate(qids):
        want = dev.exact_range(dev.gather_rows([own]), r, allowed=all_but(n, int(own)))
        assert _same(([ids[i]], [dist[i]]), want), own
    half = dev.exact_range_by_id(qids, r, n_rows=400)                                     # rows [0, 400): ids 899 and 450 are outside, and answer
    for i, own in enumerate(qids):
        m = all_but(n, int(own))
        m[400:] = False
        assert _same(([half[0][i]], [half[1][i]]), dev.exact_range(dev.gather_rows([own]), r, allowed=m)), own
    launches = dev.stats()["exact_launches"]
    with pytest.raises(RuntimeError, match=r"exact_range_by_id: ids\[1\] = 900 is no uploaded row"):
        dev.exact_range_by_id([0, n], r)
    assert dev.stats()["exact_launches"] == launches


def test_exact_radius_graph_on_700_rows():
    n = 700
    x = _data("sq_euclid", n, DIM, 31).copy()
    x[650] = x[30]
    x[40] = x[660]
    ix = _index(DIM, "sq_euclid", n)
    ix.add(x)
    d = _numpy_dist("sq_euclid", x, x)
    np.fill_diagonal(d, np.inf)
    r = float(np.quantile(d, 12 / n))
    ids, dist = ix.exact_radius_graph(r)
    assert len(ids) == len(dist) == n and all(a.dtype == np.int32 and b.dtype == np.float32 for a, b in zip(ids, dist))
    assert _same((ids, dist), ix.exact_range_query_by_id(np.arange(n), r))
    assert _same((ids, dist), exact_range_by_id(_oracle_dist("sq_euclid", x), np.arange(n), np.arange(n), r))
    assert not any((l == i).any() for i, l in enumerate(ids)) and 5 * n < sum(l.size for l in ids) < 30 * n
    assert ids[30][0] == 650 and ids[650][0] == 30 and ids[40][0] == 660 and ids[660][0] == 40 and dist[30][0] == dist[650][0] == 0.0
    some = np.array([699, 30, 30, 0], np.int32)
    assert _same(ix.exact_radius_graph(r, some), ([ids[i] for i in some], [dist[i] for i in some]))
    ix.remove([5, 650])                                                                   # the default: every live id, ascending
    live = np.delete(np.arange(n), [5, 650])
    g = ix.exact_radius_graph(r)
    assert _same(g, exact_range_by_id(_oracle_dist("sq_euclid", x), live, live, r))
    assert not any(np.isin(l, [5, 650]).any() for l in g[0])
