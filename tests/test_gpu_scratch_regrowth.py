"""GPU tier: the context's scratch memory as it is regrown, kept and let go (csrc/dev_buf.h).  One handle answers
a ladder of calls -- small, large, small again -- through every query kind, so that each buffer is allocated, outgrown, replaced
and then reused with room to spare; every answer must equal, byte for byte, that of a fresh handle built the same way that made
only that one call.  The metrics: sq_euclid, cosine (the norm arrays beside rows and queries) and sq_euclid_f16 (the float staging
area of the row uploads).  The index is built by three add calls (500, 2000, 500 rows) from a collection size of 600, so the row
store and the graph mirror are extended between them.  Beside that: the distance boundary's own buffers (dist_pair_batch, the step
buffers) up and down in size against the oracle, bit for bit as test_gpu_distance.py holds them; handles created, queried and
dropped in a row; and query lanes (views that borrow the primary's rows and graph) across an add that moves both."""
import threading

import numpy as np
import pytest

import oracle
from common import normalize_f32, uniform

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "sq_euclid_f16"]
N, DIM = 3000, 24
ADDS = (500, 2000, 500)
RUNGS = ((3, 5), (1500, 200), (7, 5))   # (nq, k): small, large, small again
ALLOWED = np.arange(0, N, 3, dtype=np.int32)
CALLS = ("knn", "knn_allowed", "range", "range_allowed", "multilayer", "exact")


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def rows_of(metric):
    return uniform(N + 500, DIM, 40 + METRICS.index(metric))


def queries_of(metric, rung):
    return uniform(RUNGS[rung][0], DIM, 70 + 10 * METRICS.index(metric) + rung)


def radius_of(metric):
    """About 20 hits per query: the median over 64 queries of the 20th smallest distance, worked out from the data in float64."""
    x, q = rows_of(metric)[:N].astype(np.float64), uniform(64, DIM, 99).astype(np.float64)
    if metric == "cosine":
        d = 1.0 - (q @ x.T) / np.outer(np.linalg.norm(q, axis=1), np.linalg.norm(x, axis=1))
    else:
        d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return float(np.median(np.sort(d, axis=1)[:, 19]))


def built(Index, metric):
    x = rows_of(metric)
    ix = Index(DIM, metric)
    ix.set_collection_size(600)
    at = 0
    for n in ADDS:
        ix.add(x[at:at + n])
        at += n
    assert ix.count == N
    return ix


def answer(ix, call, metric, rung):
    """One call's results as bytes: ids first, then the distances' bit patterns."""
    q, k = queries_of(metric, rung), RUNGS[rung][1]
    if call.startswith("range"):
        ids, d = ix.range_query(q, radius_of(metric), allowed=ALLOWED if call.endswith("allowed") else None)
        return [a.tobytes() for a in ids] + [a.tobytes() for a in d]
    if call == "knn":
        ids, d = ix.knn_query(q, k)
    elif call == "knn_allowed":
        ids, d = ix.knn_query(q, k, allowed=ALLOWED)
    elif call == "multilayer":
        ids, d = ix.multilayer_knn_query(q, k)
    else:
        ids, d = ix.exact_knn_query(q, k)
    return [ids.tobytes(), d.tobytes()]


_fresh = {}


def fresh_answer(Index, call, metric, rung):
    """The answer of a handle built the same way that made only this call (worked out once per case)."""
    key = (call, metric, rung)
    if key not in _fresh:
        _fresh[key] = answer(built(Index, metric), call, metric, rung)
    return _fresh[key]


@pytest.mark.parametrize("metric", METRICS)
def test_one_handle_up_and_down_the_ladder_answers_like_fresh_handles(Index, metric):
    ix = built(Index, metric)
    hits = []
    for rung in range(len(RUNGS)):
        for call in CALLS:
            got = answer(ix, call, metric, rung)
            assert got == fresh_answer(Index, call, metric, rung), (metric, call, rung)
            if call == "range":
                hits.append(sum(len(b) for b in got[:len(got) // 2]) / 4 / RUNGS[rung][0])
    assert 5 <= hits[1] <= 60, hits   # the radius does what it was chosen for (the large rung: 1500 queries)


@pytest.mark.parametrize("metric", METRICS)
def test_ten_handles_in_a_row(Index, metric):
    first = fresh_answer(Index, "knn", metric, 0)
    for _ in range(9):
        ix = built(Index, metric)
        last = answer(ix, "knn", metric, 0)
        del ix
    assert last == first


@pytest.mark.parametrize("metric", METRICS)
def test_query_lanes_follow_the_primary_across_an_add(Index, metric):
    T = 4
    x = rows_of(metric)
    ix = built(Index, metric)
    sets = [uniform(40 + 30 * t, DIM, 300 + t) for t in range(T)]

    def from_threads():
        got, errs = [None] * T, []

        def worker(t):
            try:
                got[t] = ix.knn_query(sets[t], 10)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        return got

    for grown in (False, True):
        if grown:
            ix.add(x[N:N + 500])   # past the collection size the views were bound to: rows and graph mirror move
        got = from_threads()
        for t in range(T):
            ids, d = ix.knn_query(sets[t], 10)
            assert (got[t][0] == ids).all() and got[t][1].tobytes() == d.tobytes(), (metric, grown, t)
    assert ix.count == N + 500


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine"])
def test_distance_boundary_buffers_up_and_down(metric):
    """dist_pair_batch with 10, 5000 and 10 pairs; step buffers of 8, 512 and 8 slots: each result against the oracle, bit for
    bit -- test_gpu_distance.py's own reference and tolerance (0 ulp) for these metrics."""
    import hnswindex
    n, dim, stride = 2000, 24, 40
    rows, q = uniform(n, dim, 11), uniform(16, dim, 12)
    if metric == "ucosine":
        rows, q = normalize_f32(rows), normalize_f32(q)
    dev = hnswindex.net_amd.DeviceBackend(dim, metric, capacity=n)
    dev.upload_rows(0, rows)
    dev.set_queries(q)
    rng = np.random.default_rng(13)
    for pairs in (10, 5000, 10):
        a, b = rng.integers(0, n, pairs).astype(np.int32), rng.integers(0, n, pairs).astype(np.int32)
        assert dev.dist_pair_batch(a, b).tobytes() == oracle.dist_pairs(metric, rows, a, b).tobytes(), pairs
    for nslots in (8, 512, 8):
        rec, dist = dev.step_buffers(0, nslots, stride)
        cnt = rng.integers(1, stride + 1, nslots).astype(np.int32)
        qidx = rng.integers(0, q.shape[0], nslots).astype(np.int32)
        ids = rng.integers(0, n, (nslots, stride)).astype(np.int32)
        rec[:, 0], rec[:, 1], rec[:, 2:] = cnt, qidx, ids
        dev.step_submit(0, nslots)
        dev.step_wait(0)
        for s in range(nslots):
            want = oracle.dist_query_rows(metric, rows, q[qidx[s]], ids[s, :cnt[s]])
            assert dist[s, :cnt[s]].tobytes() == want.tobytes(), (nslots, s)
