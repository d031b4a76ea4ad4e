"""GPU tier: the exact k-NN call where the host-side plan (exact_plan, Device::exact_knn) leaves its simplest
route -- tests/test_gpu_exact_knn.py scans 1500 rows, where the compaction is one block, the default picker gives one chunk and a
call is one round.  Here: 20000 rows (three blocks of exact_compact_kernel, 18 chunks of the default picker), the 4096-chunk cap,
two rounds by the list budget and by the output budget, more than 65 536 queries in a query set above the 4 MB staging switch,
rows longer than the 16 KB staging area under the default tile, k on both sides of exact_list_insert's 64-entry steps.

The reference is tests/exact_knn_model.py (the oracle's distances, np.lexsort((ids, dist))): ids equal, distance bytes equal.
Every test asserts through exact_knn_model.plan -- the picker restated -- that the route it is about is the one taken, and ties the
restatement to the product: exact_launches == ceil(nq / round), exact_evals == nq x candidates."""
import ctypes as ct
import gc

import numpy as np
import pytest

from common import normalize_f32, set_diag, uniform
from exact_knn_model import boundary_tie, candidates, distances, exact_knn, plan, select_rows

pytestmark = pytest.mark.gpu

METRICS = ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16", "ucosine_f16"]
N, DIM, NQ = 20000, 8, 67
BLOCK = 8192                  # ids per block of exact_compact_kernel: 256 words
KS = (1, 10, 63, 64, 65, 128, 129, 1024)   # exact_list_insert moves 64 entries per step
GRID_SEED = 2                 # data seed of the grid sets: the reference meets a tie across rank k-1 / k at every metric (asserted)


def _pitch(metric, dim):
    """32-bit words per resident query: what exact_plan gets (the int8 record; dim otherwise -- _f16 queries stay f32)."""
    return ((dim + 3) // 4 + 2 + 15) & ~15 if metric == "sq_euclid_i8" else dim


def _data(metric, n, dim, seed, grid=False):
    x = np.random.default_rng(seed).integers(1, 4, (n, dim)).astype(np.float32) if grid else uniform(n, dim, seed)
    return normalize_f32(x) if metric.startswith("ucosine") else x


def _backend(metric, x):
    import hnswindex
    db = hnswindex.DeviceBackend(x.shape[1], metric, capacity=max(x.shape[0], 1))
    db.upload_rows(0, x)
    return db


def _same(got, want):
    return (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes()


def _rounds(nq, p):
    return -(-nq // p["round"])


def _call(db, q, k, m, p, **kw):
    """One call with its counters checked against the plan p of (len(q), m candidates, k)."""
    db.reset_stats()
    got = db.exact_knn(q, k, **kw)
    st = db.stats()
    assert st["exact_launches"] == _rounds(q.shape[0], p) and st["exact_evals"] == q.shape[0] * m and st["search_launches"] == 0, (st, p)
    return got


@pytest.fixture(scope="module")
def sets():
    """(x, q, backend, the model's distance matrix, the model's first 1024 per query) per (metric, grid): computed once, shared,
    never written.  N > 1024: the model's answer at any k is the first k columns."""
    cache = {}

    def get(metric, grid=False):
        if (metric, grid) not in cache:
            x = _data(metric, N, DIM, GRID_SEED if grid else 1, grid)
            q = _data(metric, NQ, DIM, (GRID_SEED if grid else 1) + 100, grid)
            d = distances(metric, x, q, np.arange(N, dtype=np.int32))
            full = select_rows(d, np.arange(N, dtype=np.int32), 1024)
            for a in (x, q, d) + full:
                a.setflags(write=False)
            cache[(metric, grid)] = (x, q, _backend(metric, x), d, full)
        return cache[(metric, grid)]
    return get


# ---- a. the default plan: 18 chunks, merged ----------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("metric", METRICS)
def test_default_plan_merges_many_chunks(sets, metric, grid):
    x, q, db, d, full = sets(metric, grid)
    for nq in (1, 9, NQ):
        for k in KS:
            p = plan(nq, N, k, _pitch(metric, DIM))
            assert p["n_chunks"] >= 2 and p["chunk"] % 128 == 0 and N % p["chunk"] != 0 and p["round"] == nq, p   # ragged last chunk, one round
            got = _call(db, q[:nq], k, N, p)
            assert _same(got, (full[0][:nq, :k], full[1][:nq, :k])), (metric, grid, nq, k)
    # the merge is exercised only when some query's answer comes from more than one chunk
    chunk = plan(NQ, N, 10, _pitch(metric, DIM))["chunk"]
    assert any(np.unique(full[0][i, :10] // chunk).size >= 2 for i in range(NQ)), metric
    if grid:   # the condition: the reference itself meets a tie across the boundary, or the id order is never exercised
        assert boundary_tie(metric, x, q[:9], 10), metric
        # ... and somewhere the two sides of such a tie lie in different chunks: the merge, not a scan block, orders them
        k = 10
        assert any(full[1][i, k - 1] == full[1][i, k] and full[0][i, k - 1] // chunk != full[0][i, k] // chunk for i in range(NQ)), metric


# ---- b. compaction beyond one block ------------------------------------------------------------------------------------
def _block_masks():
    rng = np.random.default_rng(3)
    out = {"sel0.5": rng.random(N) < 0.5, "sel0.01": rng.random(N) < 0.01}
    empty = rng.random(N) < 0.5
    empty[BLOCK:2 * BLOCK] = False
    out["block1_empty"] = empty
    full = rng.random(N) < 0.02
    full[BLOCK:2 * BLOCK] = True
    out["block1_full"] = full
    edges = np.zeros(N, bool)
    edges[[2047, 2048, 8191, 8192, 16383, 16384, 19999]] = True       # wave and block edges; fewer than k
    out["edges"] = edges
    half = rng.random(N + 5000) < 0.5
    half[[8191, 8192, 19998, 19999]] = True
    out["nbits8192"], out["nbits8193"], out["nbits19999"] = half[:8192], half[:8193], half[:19999]
    out["wide"] = half                                                # longer than the uploaded rows: clamped
    return out


def _raw_call(db, q, k, words, nbits):
    """hnswdev_exact_knn with the caller's own words: bits at and beyond nbits may be set (the host masks them)."""
    import hnswindex
    q = np.ascontiguousarray(q, np.float32)
    ids = np.empty((q.shape[0], k), np.int32)
    d = np.empty((q.shape[0], k), np.float32)
    rc = hnswindex.net_amd.lib.hnswdev_exact_knn(db._ctx, q.ctypes.data_as(ct.POINTER(ct.c_float)), q.shape[0], 1 << 62, k,
                                                 words.ctypes.data_as(ct.POINTER(ct.c_uint32)), nbits, ids.ctypes.data_as(ct.POINTER(ct.c_int)),
                                                 d.ctypes.data_as(ct.POINTER(ct.c_float)))
    assert rc == 0, db.last_error()
    return ids, d


@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_compaction_over_three_blocks(sets, metric):
    x, q, db, d, _ = sets(metric, False)
    nq, k = 9, 10
    assert -(-((N + 31) // 32) // 256) == 3        # the grid of exact_compact_kernel at N ids
    for name, mask in _block_masks().items():
        ids = candidates(N, mask)
        assert ids.size > 0, name
        p = plan(nq, ids.size, k, _pitch(metric, DIM))
        assert _rounds(nq, p) == 1
        got = _call(db, q[:nq], k, ids.size, p, allowed=mask)
        assert _same(got, select_rows(d[:nq][:, ids], ids, k)), (metric, name)
        assert np.isin(got[0][got[0] >= 0], ids).all(), (metric, name)
    # every bit set, also at and beyond nbits: the last word is masked on the host, in block 1 (8193), in block 2 (19999), and
    # the words beyond the uploaded rows are never read
    ones = np.full((N + 5000 + 31) // 32, 0xFFFFFFFF, np.uint32)
    for nbits in (8192, 8193, 19999, N, N + 5000):
        ids = np.arange(min(nbits, N), dtype=np.int32)
        db.reset_stats()
        got = _raw_call(db, q[:nq], k, ones, nbits)
        assert _same(got, select_rows(d[:nq][:, ids], ids, k)), (metric, nbits)
        st = db.stats()
        assert st["exact_launches"] == 1 and st["exact_evals"] == nq * ids.size, (nbits, st)


def test_compaction_of_the_live_set_through_the_index(sets):
    import hnswindex
    x, q, _, d, _ = sets("sq_euclid", False)
    ix = hnswindex.Index(DIM, "sq_euclid")
    ix.set_collection_size(N); ix.set_min_nn(20)
    assert (ix.add(x) == np.arange(N)).all()
    rng = np.random.default_rng(53)
    named = np.unique([ix.entry_point, 0, 8191, 8192, 16383, 16384, N - 1])      # the block edges and the entry point
    rest = rng.choice(np.setdiff1d(np.arange(N), named), 300 - named.size, replace=False)
    gone = np.sort(np.concatenate([named, rest])).astype(np.int32)
    assert gone.size == 300 and all(((gone >= b * BLOCK) & (gone < (b + 1) * BLOCK)).sum() > 20 for b in range(3))
    ix.remove(gone)
    live = np.sort(ix.ids())
    assert live.size == N - gone.size and not np.isin(gone, live).any()
    mask = rng.random(N) < 0.5
    nq, k = 9, 10
    for allowed in (None, mask):
        ids = candidates(N, allowed, live)
        ix.reset_stats()
        got = ix.exact_knn_query(q[:nq], k, allowed=allowed)
        assert _same(got, select_rows(d[:nq][:, ids], ids, k))
        assert _same(got, exact_knn("sq_euclid", x, q[:nq], k, mask=allowed, live=live))
        st = ix.stats()
        assert st["exact_launches"] == 1 and st["exact_evals"] == nq * ids.size, st
        assert not np.isin(got[0], gone).any()


# ---- c. the 4096-chunk cap ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,chunk,n_chunks", [(4096, 1, 4096), (5000, 2, 2500)])
def test_the_chunk_cap(monkeypatch, sets, m, chunk, n_chunks):
    """exact_chunk=1: 4096 rows are 4096 chunks of one row; 5000 rows would be 5000, are capped and divided again: 2500 of 2."""
    x, q, db, d, _ = sets("sq_euclid", True)
    set_diag(monkeypatch, exact_chunk=1)
    ids = np.arange(m, dtype=np.int32)
    for k in (1, 10):
        p = plan(9, m, k, DIM, forced_chunk=1)
        assert (p["chunk"], p["n_chunks"]) == (chunk, n_chunks)
        got = _call(db, q[:9], k, m, p, n_rows=m)
        assert _same(got, select_rows(d[:9, :m], ids, k)), (m, k)
    assert boundary_tie("sq_euclid", x[:m], q[:9], 10)     # equal distances in different chunks: every chunk holds one or two rows


# ---- d. two rounds by the list budget ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["cosine", "sq_euclid_i8"])
def test_rounds_by_the_list_budget(monkeypatch, metric):
    """2049 chunks x 128 keys x 8 B = 2 MB of lists per query: 1 GiB holds 511 queries, 600 take two rounds.  The second round reads
    its queries at d_q + 511 * pitch (int8: records) and its query norms at d_qsn + 511 (cosine), and writes at out + 511 * k."""
    n, nq, k = 4097, 600, 128
    x, q = _data(metric, n, DIM, GRID_SEED, grid=True), _data(metric, nq, DIM, GRID_SEED + 100, grid=True)
    set_diag(monkeypatch, exact_chunk=1)
    p = plan(nq, n, k, _pitch(metric, DIM), forced_chunk=1)
    assert (p["n_chunks"], p["round"]) == (2049, 511) and _rounds(nq, p) == 2
    want = exact_knn(metric, x, q, k)
    db = _backend(metric, x)       # the call allocates the full list workspace: a backend of the test's own, dropped below
    try:
        got = _call(db, q, k, n, p)
        assert db.stats()["exact_launches"] == 2
        assert _same((got[0][:511], got[1][:511]), (want[0][:511], want[1][:511])), metric
        assert _same((got[0][511:], got[1][511:]), (want[0][511:], want[1][511:])), metric
    finally:
        del db
        gc.collect()


# ---- e. two rounds by the output budget --------------------------------------------------------------------------------
def test_rounds_by_the_output_budget():
    """2^24 output entries at k = 1024 are 16384 queries: 16400 take rounds of 16384 and 16.  300 rows: every row is padded."""
    n, nq, k = 300, 16400, 1024
    x, q = _data("cosine", n, DIM, 11), _data("cosine", nq, DIM, 12)
    p = plan(nq, n, k, DIM)
    assert p["round"] == 16384 and p["n_chunks"] == 1 and _rounds(nq, p) == 2
    db = _backend("cosine", x)
    got = _call(db, q, k, n, p)
    assert db.stats()["exact_launches"] == 2
    ids = np.arange(n, dtype=np.int32)
    want = select_rows(distances("cosine", x, q, ids), ids, k)
    for lo, hi in ((0, 16384), (16384, nq)):
        assert _same((got[0][lo:hi], got[1][lo:hi]), (want[0][lo:hi], want[1][lo:hi])), lo
        assert (got[0][lo:hi, :n] >= 0).all() and (got[0][lo:hi, n:] == -1).all() and np.isnan(got[1][lo:hi, n:]).all()
        assert not np.isnan(got[1][lo:hi, :n]).any()
    del db
    gc.collect()


# ---- f. beyond 65 536 queries, a query set above the 4 MB staging switch -----------------------------------------------
@pytest.mark.parametrize("metric", ["sq_euclid", "sq_euclid_i8"])
def test_more_than_65536_queries_through_the_staged_upload(metric):
    n, dim, nq, k = 64, 16, 65600, 10
    assert nq > 65536 and nq * dim * 4 >= 4 << 20      # set_queries takes staged_upload; int8 quantises from the staging area
    x, q = _data(metric, n, dim, 21), _data(metric, nq, dim, 22)
    p = plan(nq, n, k, _pitch(metric, dim))
    assert p["round"] == nq and p["qtile"] == 32 and -(-nq // p["qtile"]) > 2048
    db = _backend(metric, x)
    got = _call(db, q, k, n, p)
    ids = np.arange(n, dtype=np.int32)
    want = select_rows(distances(metric, x, q, ids), ids, k)
    assert _same(got, want), (metric, np.flatnonzero((got[0] != want[0]).any(axis=1))[:8])     # every row


# ---- g. rows longer than the staging area, default tile ----------------------------------------------------------------
LONG = [("sq_euclid", 1100), ("cosine", 1100), ("ucosine", 1100), ("ucosine_f16", 2200), ("sq_euclid_f16", 2200), ("sq_euclid_i8", 4200)]


@pytest.mark.parametrize("metric,dim", LONG)
def test_long_rows_are_walked_in_pieces_under_the_default_tile(metric, dim):
    """1100 words: a piece of 1024 and one of 76, whose last 4 elements are the scalar tail.  2200: three pieces over 1104 record
    words of halves.  int8 4200: a 1056-word record, the scale / sumsq words in the second piece."""
    n, nq, k = 300, 5, 10
    pitch = _pitch(metric, dim)
    p = plan(nq, n, k, pitch)
    assert p["piece"] < pitch and p["piece"] % 16 == 0 and p["qtile"] == 4, p
    if metric == "sq_euclid_i8":
        assert pitch == 1056 and pitch - 2 >= p["piece"]
    x, q = _data(metric, n, dim, 13), _data(metric, nq, dim, 14)
    db = _backend(metric, x)
    assert _same(_call(db, q, k, n, p), exact_knn(metric, x, q, k)), (metric, dim)


# ---- h. byte identity across plans at size -----------------------------------------------------------------------------
def test_plans_give_identical_bytes_at_size(monkeypatch, sets):
    x, q, db, d, full = sets("sq_euclid_f16", True)
    k = 10
    want = (full[0][:, :k], full[1][:, :k])
    seen = set()
    for chunk in (0, 128, 1153):
        for qtile in (0, 1, 3):
            set_diag(monkeypatch, exact_chunk=chunk, exact_qtile=qtile)
            p = plan(NQ, N, k, DIM, forced_qtile=qtile, forced_chunk=chunk)
            seen.add((p["qtile"], p["chunk"]))
            assert p["n_chunks"] >= 2
            assert _same(_call(db, q, k, N, p), want), (chunk, qtile)
    assert len(seen) == 9      # nine different shapes of the launch, one answer
