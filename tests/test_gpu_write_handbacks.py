"""GPU tier: Add and Remove where the device hands work back to the host, and the two query junctions of the same kind.

A device traversal gives a job back on a NaN or -0 distance, on a full candidate heap and spill area, on a full visited table; the
host redoes it on the lock-step engine and joins the result with what the device finished.  On the write side a wrong join is a
wrong graph for good.  Forced here (tests/handbacks.py has the shapes, triggers and rows; tests/test_handback_inputs.py checks them
on the CPU):

  * the host-grouped form of link_half_device alone (link_plan=0), in one sub-batch and in four on two staging sets;
  * batches of which PART was handed back (search_overflows strictly between 0 and the items of the call): selections from the
    device and from the lock-step path joined in one link, refresh_host_lists after batches linked on the device, and the planned
    path again afterwards on the same mirror;
  * the exact window, where a handed-back item goes alone and voids every speculative result;
  * sequential and batched Remove with flagged search steps;
  * a query lane that meets a hand-back, and a streamed upload with hand-backs among its jobs.

The reference everywhere is the oracle under the same schedule.  Equal bit for bit: graph hash, levels, entry point, Ids() order
and the answers (ids, distance bytes) to 300 queries -- a hand-back must never change a result.

Which link path ran is read off link_launches (hnswdev_stats has no counter of its own for it): the planned path counts one launch
per batch, the host-grouped path one per sub-batch -- four for a batch of 2 048 items or more (handbacks.host_link_launches).  Below
2 048 items both count one, and there the graph hash is the check."""
import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

import handbacks as hb
import oracle
from common import default_cap, diag_values, set_diag, uniform

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _index(Index, metric, shape):
    ix = Index(shape.dim, metric)
    ix.set_collection_size(shape.n); ix.set_max_edges(shape.M); ix.set_max_candidates(shape.efc); ix.set_insert_batch(shape.cap)
    return ix


def _holds(ix, want, q, tag):
    """The index is the oracle's at that stage: hash, levels, entry point, Ids() order, answers."""
    assert ix.graph_hash() == want["hash"], tag
    assert ix.levels().tolist() == want["levels"].tolist() and ix.entry_point == want["entry"], tag
    assert ix.ids().tolist() == want["ids"].tolist(), tag
    assert hb.same_answers(ix.knn_query(q, 10), want["knn"]), tag


def _three_calls(Index, monkeypatch, metric, shape, rows_kind, trigger, always=None):
    """first call | second call under `trigger` | tail of 500 clean rows with the trigger cleared; `always` holds for all three.
    Every stage is held to the oracle.  -> (stats of the second call, stats of the tail, batch sizes of the three calls)"""
    want = hb.reference(metric, shape, rows_kind)
    x, q = want["x"], want["q"]
    lv = want["tail"]["levels"]
    a, b = shape.first, shape.first + shape.second
    sizes = [hb.batch_sizes(lv, 0, a, shape.cap), hb.batch_sizes(lv, a, shape.second, shape.cap), hb.batch_sizes(lv, b, shape.tail, shape.cap)]
    tag = (metric, str(shape), rows_kind, trigger)
    if always:
        set_diag(monkeypatch, **always)
    ix = _index(Index, metric, shape)
    assert (ix.add(x[:a]) == np.arange(a)).all()
    first = ix.stats()
    _holds(ix, want["first"], q, tag + ("first",))
    ix.reset_stats()
    with monkeypatch.context() as m:
        set_diag(m, **trigger)
        assert (ix.add(x[a:b]) == np.arange(a, b)).all()
    second = ix.stats()
    _holds(ix, want["second"], q, tag + ("second",))
    ix.reset_stats()
    assert (ix.add(x[b:]) == np.arange(b, shape.n)).all()
    tail = ix.stats()
    _holds(ix, want["tail"], q, tag + ("tail",))
    print(f"{tag}: second call {shape.second} items in batches {sizes[1]}: search_overflows {second['search_overflows']}, link_launches {second['link_launches']}, "
          f"lock-step launches {second['launches']}; tail: search_overflows {tail['search_overflows']}, link_launches {tail['link_launches']}; "
          f"first call: link_launches {first['link_launches']} in {len(sizes[0])} batches")
    return first, second, tail, sizes


# ---- 1. the host-grouped link half alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [hb.SMALL, hb.LARGE], ids=repr)
@pytest.mark.parametrize("metric", hb.ROW_KINDS)
def test_host_grouped_link_half_alone(Index, monkeypatch, metric, shape):
    """link_plan=0 in all three calls: nothing is handed back, every batch is searched on the device and linked by the host-grouped
    form -- in four sub-batches where it holds 2 048 items or more (the large shape: the late batches of its first call and the
    first two of its second)."""
    first, second, tail, sizes = _three_calls(Index, monkeypatch, metric, shape, "clean", {}, always=hb.PLAN0)
    for st, s in zip((first, second, tail), sizes):
        assert st["search_overflows"] == 0 and st["link_launches"] == hb.host_link_launches(s), (metric, shape)
    if shape is hb.LARGE:
        assert hb.host_link_launches(sizes[1]) >= len(sizes[1]) + 6      # two batches in four sub-batches each


@pytest.mark.parametrize("shape,always", [(hb.SMALL_M32, hb.PLAN0), (hb.SMALL, dict(hb.PLAN0, lat=2))], ids=["m32", "lat2"])
def test_host_grouped_link_half_with_lists_of_64_and_behind_the_latency_form(Index, monkeypatch, shape, always):
    first, second, tail, sizes = _three_calls(Index, monkeypatch, "sq_euclid", shape, "clean", {}, always=always)
    for st, s in zip((first, second, tail), sizes):
        assert st["search_overflows"] == 0 and st["link_launches"] == hb.host_link_launches(s)
    if "lat" in always:
        assert second["lat_launches"] > 0 and tail["lat_launches"] > 0


# ---- 2. mixed batches -------------------------------------------------------------------------------------------------------------
def _mixed(Index, monkeypatch, metric, shape, rows_kind, trigger, always=None):
    first, second, tail, sizes = _three_calls(Index, monkeypatch, metric, shape, rows_kind, trigger, always)
    # part of the call was handed back, not all of it: selections of both origins were linked together
    assert 0 < second["search_overflows"] < shape.second, (metric, shape, second["search_overflows"])
    assert second["launches"] > 0                                          # the lock-step engine measured for them
    assert len(sizes[1]) <= second["link_launches"] <= hb.host_link_launches(sizes[1])
    if shape is hb.LARGE:
        assert second["link_launches"] >= len(sizes[1]) + 3                # a batch of 2 048 or more went through four sub-batches
    # the first call and the tail: one planned link per batch (the tail on the mirror the mixed call left) and nothing handed back --
    # except that clean rows added behind unsafe ones still meet them: that tail is mixed again, and every batch below 2 048 items
    assert first["search_overflows"] == 0 and first["link_launches"] == len(sizes[0])
    assert tail["link_launches"] == len(sizes[2])
    if rows_kind == "unsafe":
        assert 0 < tail["search_overflows"] < shape.tail
    else:
        assert tail["search_overflows"] == 0
    return second


@pytest.mark.parametrize("shape", [hb.SMALL, hb.LARGE], ids=repr)
@pytest.mark.parametrize("metric", hb.MIXED_KINDS)
def test_candidate_heap_overflow_in_part_of_a_batch(Index, monkeypatch, metric, shape):
    """The second call on the two-heap traversal with a candidate heap of 24 entries and a spill area sized to the shape
    (handbacks.OVERFLOW_SPILL).  Handed back of 2 000 (small) / 6 000 (large) items, measured on an MI355X: sq_euclid 758 / 2 520,
    ucosine 599 / 2 069, sq_euclid_i8 769 / 2 482; the large shape's call made 9 link launches (both batches of 2 048 or more in
    four sub-batches).  The counts are fixed by the rows and the caps: every search is deterministic."""
    _mixed(Index, monkeypatch, metric, shape, "clean", hb.overflow(shape))


@pytest.mark.parametrize("shape", [hb.SMALL, hb.LARGE], ids=repr)
@pytest.mark.parametrize("metric", hb.MIXED_KINDS)
def test_unsafe_rows_in_the_second_call(Index, monkeypatch, metric, shape):
    """Three rows no distance to which is a number, in the first batch of the second call: they are handed back themselves, and so
    is every later item whose search measures one of them.  The first call is linked on the planned path, the second alternates.
    Handed back of 2 000 (small) / 6 000 (large) items, measured on an MI355X: sq_euclid 1 228 / 130, ucosine 1 153 / 88,
    sq_euclid_i8 1 169 / 142 (9 link launches on the large shape); of the 500 clean rows of the tail 399 / 27, 400 / 15, 370 / 31."""
    _mixed(Index, monkeypatch, metric, shape, "unsafe", {})


def test_unsafe_rows_behind_the_latency_form(Index, monkeypatch):
    """lat=2: the pool form of the insert kernel raises the flag.  Handed back of 2 000 items, measured: 1 228 (as in the plain form)."""
    second = _mixed(Index, monkeypatch, "sq_euclid", hb.SMALL, "unsafe", {}, always={"lat": 2})
    assert second["lat_launches"] > 0


def test_full_visited_table_hands_inserts_back(Index, monkeypatch):
    """Visited tables of 512 ids per wave (crowded beyond 384) under the insert kernel: traverse_sorted / traverse leave with
    hash_full and the job is flagged (csrc/dk_sorted_top.h, csrc/dk_traverse_exact.h).  An efc-100 search visits far more ids
    than that, so the whole call is handed back (measured: 2 000 of 2 000): every selection comes from the lock-step path here."""
    first, second, tail, sizes = _three_calls(Index, monkeypatch, "sq_euclid", hb.SMALL, "clean", hb.TABLE)
    assert 0 < second["search_overflows"] <= hb.SMALL.second and second["visited_hash_launches"] > 0
    assert tail["search_overflows"] == 0 and tail["visited_hash_launches"] == 0


# ---- 3. the exact window ------------------------------------------------------------------------------------------------------
WINDOW_N, WINDOW_DIM = 3000, 24
WINDOW_UNSAFE = (2300, 2600, 2800)
_SEQ = {}


def _sequential(rows_kind):
    """The strictly sequential oracle (one Add per item) of the window cases, once per module."""
    if rows_kind not in _SEQ:
        x = uniform(WINDOW_N, WINDOW_DIM, 911).copy()
        if rows_kind == "unsafe":
            x[list(WINDOW_UNSAFE), [1, 9, 23]] = np.nan
        q = uniform(hb.NQ, WINDOW_DIM, 912)
        ref = oracle.OracleIndex(WINDOW_DIM, collection_size=WINDOW_N)
        assert (ref.add(x) == np.arange(WINDOW_N)).all()
        _SEQ[rows_kind] = (x, q, hb.snapshot(ref, q))
    return _SEQ[rows_kind]


@pytest.mark.parametrize("W", [16, 64])
@pytest.mark.parametrize("rows_kind", ["overflow", "unsafe"])
def test_exact_window_with_items_handed_back(Index, monkeypatch, rows_kind, W):
    """set_insert_batch(-W) against one Add per item.  overflow: the two-heap traversal with the small shape's heap, so that some
    searches of every window come back flagged; unsafe: three NaN rows past row 1 000 (2 300, 2 600, 2 800: nearly every later
    item meets one, and an item that goes alone costs 5 ms).  A flagged item is inserted alone and every speculative result is
    void after it.  Measured, the same for both W: overflow 157 flagged searches and
    69 items alone; unsafe 5 400 flagged searches (a flagged item is searched again in every round until it is the frontier) and
    632 items alone."""
    x, q, want = _sequential("unsafe" if rows_kind == "unsafe" else "clean")
    if rows_kind == "overflow":
        set_diag(monkeypatch, **hb.overflow("window"))
    ix = Index(WINDOW_DIM); ix.set_collection_size(WINDOW_N); ix.set_insert_batch(-W)
    assert (ix.add(x) == np.arange(WINDOW_N)).all()
    st, xw = ix.stats(), ix.exact_window_stats()
    print(f"exact window {rows_kind} W={W}: search_overflows {st['search_overflows']}, window stats {xw}")
    _holds(ix, want, q, (rows_kind, W))
    assert st["search_overflows"] > 0 and xw["alone"] > 0 and xw["linked"] + xw["alone"] == WINDOW_N - 1


# ---- 4. Remove ------------------------------------------------------------------------------------------------------------------
REMOVE_N, REMOVE_DIM, REMOVE_CAP = 6000, 16, 256
REMOVE_VICTIMS = {"clean": 2000, "unsafe": 400}      # (every search of the unsafe index is drawn to a NaN row and comes back: 5 ms each)
REMOVE_UNSAFE_VICTIMS, REMOVE_UNSAFE_KEPT = (700, 1500, 2300), (3100, 3900, 4700)
_REMOVED = {}


def _remove_rows(rows_kind):
    x = uniform(REMOVE_N, REMOVE_DIM, 921).copy()
    if rows_kind == "unsafe":
        x[list(REMOVE_UNSAFE_VICTIMS + REMOVE_UNSAFE_KEPT), [0, 5, 15, 3, 8, 11]] = np.nan
    return x


def _removal_reference(rows_kind, B):
    """The oracle built in batches of 256, its victims (2 000; 400 of the unsafe index) removed (one after the other: B = 1, else
    in the batched schedule), then 300 rows added into the vacated slots; a snapshot after each step, once per module.  The
    victims of the unsafe index hold three NaN rows and four out-neighbours of each of three others, which stay."""
    key = (rows_kind, B)
    if key not in _REMOVED:
        x, q, more = _remove_rows(rows_kind), uniform(hb.NQ, REMOVE_DIM, 922), uniform(300, REMOVE_DIM, 923)
        ref = oracle.OracleIndex(REMOVE_DIM, collection_size=REMOVE_N)
        ref.add_batched(x, REMOVE_CAP, threads=8)
        built = hb.snapshot(ref, q)
        forced = list(REMOVE_UNSAFE_VICTIMS) if rows_kind == "unsafe" else []
        if rows_kind == "unsafe":
            for i in REMOVE_UNSAFE_KEPT:
                forced += [int(v) for v in ref.edges(i, 0)[:4] if int(v) not in REMOVE_UNSAFE_KEPT]
        rest = [int(v) for v in np.random.default_rng(924).permutation(REMOVE_N) if int(v) not in REMOVE_UNSAFE_KEPT]
        victims = np.array(list(dict.fromkeys(forced + rest))[:REMOVE_VICTIMS[rows_kind]], dtype=np.int32)
        victims = np.random.default_rng(925).permutation(victims).astype(np.int32)
        if B == 1:
            ref.remove(victims)
        else:
            ref.remove_batched(victims, B)
        removed = hb.snapshot(ref, q)
        ids = ref.add_batched(more, REMOVE_CAP, threads=8)
        _REMOVED[key] = (x, q, more, victims, built, removed, ids, hb.snapshot(ref, q))
    return _REMOVED[key]


@pytest.mark.parametrize("B", [1, 16, 128])
@pytest.mark.parametrize("rows_kind", ["overflow", "unsafe"])
def test_remove_with_flagged_steps(Index, monkeypatch, rows_kind, B):
    """Nodes of a 6 000-node index removed one after the other (B = 1) and in snapshot batches of 16 and 128.  overflow: a clean
    index, 2 000 victims, the removal under a small candidate heap (handbacks.OVERFLOW_SPILL["remove"]); unsafe: six NaN rows, three
    of them victims, the others neighbours of victims -- 400 victims, because every search of that index is drawn to a NaN row
    (CompareTo puts NaN in front of every number) and comes back.  A flagged search step is repeated on the lock-step path, in the
    sequential form together with its re-links.  search_overflows / lock-step launches of the removal, measured: overflow 182 /
    31 561 (B = 1), 89 / 9 063 (B = 16), 94 / 9 579 (B = 128); unsafe 800 / 136 279 (B = 1: the sorted-list and the exact search of
    every step both come back), 401 / 40 667, 401 / 40 653."""
    x, q, more, victims, built, removed, more_ids, after = _removal_reference("unsafe" if rows_kind == "unsafe" else "clean", B)
    ix = Index(REMOVE_DIM); ix.set_collection_size(REMOVE_N); ix.set_insert_batch(REMOVE_CAP); ix.set_remove_batch(B)
    ix.add(x)
    _holds(ix, built, q, (rows_kind, B, "built"))
    ix.reset_stats()
    with monkeypatch.context() as m:
        if rows_kind == "overflow":
            set_diag(m, **hb.overflow("remove"))
        ix.remove(victims)
    st = ix.stats()
    print(f"remove {rows_kind} B={B}: search_overflows {st['search_overflows']}, lock-step launches {st['launches']}, search_launches {st['search_launches']}")
    assert ix.count == REMOVE_N - victims.size
    _holds(ix, removed, q, (rows_kind, B, "removed"))
    assert st["search_overflows"] > 0 and st["launches"] > 0
    assert (ix.add(more) == more_ids).all()                      # the vacated slots, last out first
    _holds(ix, after, q, (rows_kind, B, "slots reused"))


# ---- 5. the query junctions -----------------------------------------------------------------------------------------------------
def test_query_lanes_that_meet_a_hand_back(Index):
    """Six host threads on one handle (tests/test_gpu_concurrent_queries.py), two of the query sets with three NaN queries each: a
    lane whose launch flags a job returns the whole call to the exclusive path, which redoes the flagged queries on the lock-step
    engine.  Every call answers as the oracle does.  Measured: search_overflows 36 (six NaN queries, three rounds, flagged on the
    lane and again on the exclusive path)."""
    n, dim, T = 20000, 64, 6
    x = uniform(n, dim, 31)
    sets = [uniform(300 + 1700 * t, dim, 100 + t).copy() for t in range(T)]
    sets[3] = uniform(9000, dim, 777).copy()
    sets[1][[0, 777, 1999], [0, 31, 63]] = np.nan
    sets[4][[5, 3000, 7099], [1, 2, 3]] = np.nan
    ref = oracle.OracleIndex(dim, collection_size=n, min_nn=48)
    ref.add_batched(x, default_cap(), threads=8)
    want = [ref.knn_query(s, 10, threads=8) for s in sets]
    ix = Index(dim); ix.set_collection_size(n); ix.set_min_nn(48)
    ix.add(x)
    assert ix.graph_hash() == ref.graph_hash()
    ix.reset_stats()
    got = [None] * T
    errs = []

    def worker(t):
        try:
            for _ in range(3):
                got[t] = ix.knn_query(sets[t], 10)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs
    for t in range(T):
        assert hb.same_answers(got[t], want[t]), t
    st = ix.stats()
    print(f"query lanes: search_overflows {st['search_overflows']}, search_launches {st['search_launches']}, lock-step launches {st['launches']}")
    assert st["search_overflows"] >= 2 * 3 * 3 and st["launches"] > 0      # six NaN queries, three rounds (a lane's flagged launch and the exclusive path both count)


STREAM_WORKER = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
import hnswindex
dim, n, nq = 128, 3000, 33000
x = np.random.default_rng(5).random((n, dim), dtype=np.float32)
q = np.random.default_rng(931).random((nq, dim), dtype=np.float32)
q[[0, 4095, 4096, 20000, 32999], [0, 1, 2, 3, 127]] = np.nan
ix = hnswindex.Index(dim); ix.set_collection_size(n)
ix.add(x)
ix.reset_stats()
ids, d = ix.knn_query(q, 10)
st = ix.stats()
np.savez({out!r}, ids=ids, d=d)
print(json.dumps({{"graph_hash": int(ix.graph_hash()), "search_overflows": int(st["search_overflows"]), "launches": int(st["launches"])}}))
"""


def test_streamed_upload_with_hand_backs_among_its_jobs(tmp_path):
    """One call of 33 000 queries (the streamed upload: 32 768 and more) at dim 128 on a 3 000-node index, five of them with a NaN
    element -- in the head of the upload, at its edge and in the rows that arrive behind the launch.  A process of its own, as
    in tests/test_gpu_streamed_queries.py.  Measured: search_overflows 5."""
    import json
    out = str(tmp_path / "answers.npz")
    env = dict(os.environ, HNSW_MI355X_DIAG=",".join(f"{k}={v}" for k, v in dict(diag_values(), stream_queries=1).items()))
    r = subprocess.run([sys.executable, "-c", STREAM_WORKER.format(root=str(ROOT), out=out)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    print(f"streamed call: {rep}")
    got = np.load(out)
    dim, n, nq = 128, 3000, 33000
    x = np.random.default_rng(5).random((n, dim), dtype=np.float32)
    q = np.random.default_rng(931).random((nq, dim), dtype=np.float32)
    q[[0, 4095, 4096, 20000, 32999], [0, 1, 2, 3, 127]] = np.nan
    ref = oracle.OracleIndex(dim, collection_size=n)
    ref.add_batched(x, default_cap(), threads=8)
    assert ref.graph_hash() == rep["graph_hash"]
    want = ref.knn_query(q, 10, threads=8)
    assert hb.same_answers((got["ids"], got["d"]), want)
    assert np.isnan(want[1][[0, 4095, 4096, 20000, 32999]]).all()
    assert rep["search_overflows"] >= 5 and rep["launches"] > 0
