"""CPU tier: the reference of the exact k-NN call (tests/exact_knn_model.py) orders as the contract says -- (distance, id)
ascending, -0 == +0, +inf before NaN, NaNs by id, padding -- and the surfaces of the call exist: header, exports, bindings, the
five counters appended to hnswdev_stats."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from common import uniform
from exact_knn_model import PAD_ID, exact_knn, select

ROOT = Path(__file__).resolve().parent.parent


def test_nan_orders_last_by_id():
    d = np.array([np.nan, 2.0, np.nan, 1.0, np.inf], np.float32)
    ids = np.array([9, 4, 3, 7, 1], np.int32)
    got_ids, got_d = select(d, ids, 5)
    assert got_ids.tolist() == [7, 4, 1, 3, 9]
    assert got_d[:3].tolist() == [1.0, 2.0, np.inf] and np.isnan(got_d[3:]).all()


def test_signed_zeros_tie_by_id():
    d = np.array([0.0, -0.0, 0.0, -0.0, 1.0], np.float32)
    ids = np.array([8, 6, 2, 4, 0], np.int32)
    assert select(d, ids, 5)[0].tolist() == [2, 4, 6, 8, 0]


def test_inf_orders_before_nan():
    d = np.array([np.nan, np.inf, -np.inf], np.float32)
    ids = np.array([0, 1, 2], np.int32)
    assert select(d, ids, 3)[0].tolist() == [2, 1, 0]
    assert select(d, ids, 2)[0].tolist() == [2, 1]


def test_k_beyond_the_candidates_pads():
    got_ids, got_d = select(np.array([3.0, 1.0], np.float32), np.array([5, 6], np.int32), 4)
    assert got_ids.tolist() == [6, 5, PAD_ID, PAD_ID]
    assert got_d[:2].tolist() == [1.0, 3.0] and np.isnan(got_d[2:]).all()
    e_ids, e_d = select(np.zeros(0, np.float32), np.zeros(0, np.int32), 2)
    assert e_ids.tolist() == [PAD_ID, PAD_ID] and np.isnan(e_d).all()


def test_select_rows_is_select_row_by_row():
    from exact_knn_model import select_rows
    rng = np.random.default_rng(5)
    d = rng.integers(0, 6, (7, 40)).astype(np.float32)          # equal distances abound
    d[1, 3] = d[1, 30] = np.nan; d[2, 5] = np.inf; d[3, :4] = [0.0, -0.0, -0.0, 0.0]
    ids = np.sort(rng.choice(1000, 40, replace=False)).astype(np.int32)
    for k in (1, 7, 40, 50):
        got = select_rows(d, ids, k)
        want = [select(d[i], ids, k) for i in range(7)]
        assert (got[0] == np.stack([w[0] for w in want])).all() and got[1].tobytes() == np.stack([w[1] for w in want]).tobytes()
    e_ids, e_d = select_rows(np.zeros((2, 0), np.float32), np.zeros(0, np.int32), 3)
    assert (e_ids == PAD_ID).all() and np.isnan(e_d).all()


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_every_id_left_out_is_greater_than_the_last_returned(metric):
    import oracle
    from exact_knn_model import stored
    rng = np.random.default_rng(3)
    x = rng.integers(1, 4, (200, 8)).astype(np.float32)   # grid data: equal distances abound
    q = rng.integers(1, 4, (5, 8)).astype(np.float32)
    mask = rng.random(200) < 0.6
    live = np.setdiff1d(np.arange(200), rng.choice(200, 30, replace=False))
    k = 12
    ids, d = exact_knn(metric, x, q, k, mask=mask, live=live)
    base, rows = stored(metric, x)
    cand = np.array([i for i in live if mask[i]], np.int32)
    for i in range(q.shape[0]):
        assert np.isin(ids[i], cand).all() and len(set(ids[i].tolist())) == k
        assert d[i].tobytes() == oracle.dist_query_rows(base, rows, q[i], ids[i]).tobytes()
        keys = list(zip(d[i].tolist(), ids[i].tolist()))
        assert keys == sorted(keys)
        rest = np.setdiff1d(cand, ids[i]).astype(np.int32)
        rd = oracle.dist_query_rows(base, rows, q[i], rest)
        assert all((float(a), int(b)) > keys[-1] for a, b in zip(rd, rest))


def test_f16_model_is_the_f32_model_on_rounded_rows():
    x, q = uniform(100, 24, 1), uniform(4, 24, 2)
    a = exact_knn("ucosine_f16", x, q, 7)
    b = exact_knn("ucosine", x.astype(np.float16).astype(np.float32), q, 7)
    assert (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()


PLAN_PINS = [   # (nq, m, k, pitch, forced chunk) -> (qtile, chunk, n_chunks, round), worked by hand from exact_plan at 256 CUs
    ((9, 20000, 10, 8, 0), (16, 1152, 18, 9)),
    ((67, 20000, 10, 8, 0), (32, 1152, 18, 67)),
    ((9, 20000, 1024, 8, 0), (4, 1152, 18, 9)),
    ((9, 1500, 10, 16, 0), (16, 1536, 1, 9)),
    ((16400, 300, 1024, 8, 0), (4, 384, 1, 16384)),
    ((600, 20000, 64, 8, 5), (32, 5, 4000, 524)),
]


@pytest.mark.parametrize("args,want", PLAN_PINS)
def test_plan_restates_the_picker(args, want):
    from exact_knn_model import plan
    nq, m, k, pitch, forced = args
    p = plan(nq, m, k, pitch, forced_chunk=forced)
    assert (p["qtile"], p["chunk"], p["n_chunks"], p["round"]) == want
    assert p["piece"] == pitch                                   # rows this short are staged whole
    for cu in (32, 64, 304):                                     # tiles <= 3 in every unforced line but the 16400-query one,
        assert plan(nq, m, k, pitch, forced_chunk=forced, num_cu=cu) == p   # whose m // 1024 is 0: no CU count changes any


def test_plan_pieces_caps_and_forced_tiles():
    from exact_knn_model import plan
    # rows beyond the 16 KB staging area at the smallest tile: pieces of 1024 words
    assert plan(5, 300, 10, 1100)["qtile"] == 4 and plan(5, 300, 10, 1100)["piece"] == 1024
    assert plan(5, 300, 10, 1056)["piece"] == 1024 and plan(5, 300, 10, 1024)["piece"] == 1024
    assert plan(40, 300, 10, 264, forced_qtile=32)["piece"] == 128
    # the 4096-chunk cap: 4096 chunks of one id; beyond it the list is divided again
    assert plan(9, 4096, 10, 8, forced_chunk=1)["n_chunks"] == 4096
    p = plan(9, 5000, 10, 8, forced_chunk=1)
    assert (p["chunk"], p["n_chunks"]) == (2, 2500)
    p = plan(600, 4097, 128, 8, forced_chunk=1)
    assert (p["chunk"], p["n_chunks"], p["round"]) == (2, 2049, 511)
    # a forced tile is taken as it is (no multiple of the register tile needed); a forced chunk gives the number of chunks, over
    # which the list is divided evenly (ceil(20000 / 1153) = 18 chunks of ceil(20000 / 18) ids), not rounded to 128
    p = plan(67, 20000, 10, 8, forced_qtile=3, forced_chunk=1153)
    assert (p["qtile"], p["chunk"], p["n_chunks"]) == (3, 1112, 18)
    assert plan(67, 20000, 10, 8, forced_chunk=128)["n_chunks"] == 157
    assert plan(65600, 64, 10, 16)["round"] == 65600 and plan(65600, 64, 10, 16)["qtile"] == 32


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)


def test_header_declares_both_entry_points_and_the_library_exports_them():
    import hnswindex
    text = _header()
    for sym in ("hnsw_mi355x_exact_knn_query", "hnswdev_exact_knn"):
        assert re.search(r"\bint\s+" + sym + r"\s*\(", text), sym
        assert hasattr(hnswindex.net_amd.lib, sym), sym


EXACT_FIELDS = ["exact_launches", "exact_evals", "exact_timed_launches", "exact_timed_evals", "exact_kernel_ms"]


def test_bindings_have_the_methods_and_the_appended_counters():
    import hnswindex
    import importlib
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)   # the bindings module: Stats is not re-exported
    assert callable(net.Index.exact_knn_query) and callable(net.DeviceBackend.exact_knn)
    # hnswdev_stats in Python is DeviceStats: the earlier struct (Stats, whose own field list stays as it was) with the five new
    # counters laid out behind it, so every earlier counter keeps its offset
    assert issubclass(net.DeviceStats, net.Stats)
    assert [n for n, _ in net.DeviceStats._fields_] == EXACT_FIELDS
    assert net.DeviceStats._fields_[-1][1] is ct.c_double and all(t is ct.c_uint64 for _, t in net.DeviceStats._fields_[:-1])
    names = net.DeviceStats.field_names()
    assert names[-5:] == EXACT_FIELDS and names[:-5] == [n for n, _ in net.Stats._fields_]
    assert net.DeviceStats.exact_launches.offset == ct.sizeof(net.Stats) and ct.sizeof(net.DeviceStats) == ct.sizeof(net.Stats) + 40
    assert list(net.DeviceStats().as_dict()) == names
    # the short struct cannot reach a get_stats call: ctypes refuses it before the library could write past its end
    for fn in (net.lib.hnswdev_get_stats, net.lib.hnsw_mi355x_get_stats):
        with pytest.raises(ct.ArgumentError):
            fn(None, ct.byref(net.Stats()))
    # ... and in the header, in the same order, as the struct's last members
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    members = re.findall(r"\b([a-z_0-9]+)\s*[,;]", body)
    assert members[-5:] == EXACT_FIELDS
    assert members == names


def test_null_handle_returns_what_the_filtered_call_returns():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), np.float32)
    o = np.full((2, 3), 7, np.int32)
    d = np.full((2, 3), 7, np.float32)
    bits = np.ones(1, np.uint32)
    args = (v.ctypes.data_as(F), 2, 4, 3, bits.ctypes.data_as(U), 32, o.ctypes.data_as(I), d.ctypes.data_as(F))
    assert lib.hnsw_mi355x_exact_knn_query(None, *args) == lib.hnsw_mi355x_knn_query_filtered(None, *args) == 0
    assert (o == 7).all() and (d == 7).all()     # nothing written
    assert lib.hnswdev_exact_knn(None, v.ctypes.data_as(F), 2, 10, 3, None, 0, o.ctypes.data_as(I), d.ctypes.data_as(F)) == -1
