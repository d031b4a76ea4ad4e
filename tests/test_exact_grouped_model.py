"""CPU tier: the reference of the grouped exact k-NN call (tests/exact_grouped_model.py) on hand-made cases -- an empty group, a
group smaller than k, scrambled query order -- and the surfaces of the call: header, exports, INTEGRATION.md, bindings, with
hnswdev_stats left as it was and the NULL-handle conventions of the ungrouped calls."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from exact_grouped_model import evals, exact_knn_grouped, group_mask, info, members
from exact_knn_model import exact_knn, stored

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("hnsw_mi355x_exact_knn_query_grouped", "hnsw_mi355x_exact_grouped_info", "hnswdev_exact_knn_grouped", "hnswdev_exact_grouped_info",
           "hnswdev_exact_grouped_list_ms")


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_the_model_is_the_brute_force_loop(metric):
    import oracle
    rng = np.random.default_rng(5)
    n, k, n_groups = 40, 4, 5
    x = rng.integers(1, 4, (n, 8)).astype(np.float32)   # grid data: equal distances abound
    q = rng.integers(1, 4, (9, 8)).astype(np.float32)
    row_group = (np.arange(n) % 4).astype(np.int32)     # group 4 is empty
    row_group[row_group == 3] = np.where(np.arange(10) < 3, 3, 0)   # group 3 has 3 members: smaller than k
    row_group[[0, 1]] = [-1, 7]                         # in no group
    query_group = np.array([4, 2, 0, 3, 1, 0, 4, 3, 2], np.int32)   # scrambled, the empty group named twice
    live = np.setdiff1d(np.arange(n), [5, 6, 20])
    base, rows = stored(metric, x)
    ids, d = exact_knn_grouped(metric, x, q, k, row_group, query_group, n_groups, live=live)
    assert ids.dtype == np.int32 and d.dtype == np.float32 and ids.shape == d.shape == (9, k)
    ties = 0
    for i in range(9):
        want = []
        for c in range(n):
            if c in live and row_group[c] == query_group[i]:
                want.append((float(oracle.dist_query_rows(base, rows, q[i], np.array([c], np.int32))[0]), c))
        want.sort()
        ties += len(want) > k and want[k - 1][0] == want[k][0]
        want = (want + [(np.nan, -1)] * k)[:k]
        assert ids[i].tolist() == [c for _, c in want], (metric, i)
        assert d[i].tobytes() == np.array([v for v, _ in want], np.float32).tobytes(), (metric, i)
    assert (ids[[0, 6]] == -1).all() and np.isnan(d[[0, 6]]).all()          # the empty group: padding
    assert (ids[[3, 7], :3] >= 0).all() and (ids[[3, 7], 3:] == -1).all()   # the group of 3: padded from rank 3
    assert ties >= 1                                                          # the id order decided something


def test_the_model_is_the_ungrouped_model_per_group():
    rng = np.random.default_rng(6)
    x, q = rng.random((60, 8), dtype=np.float32), rng.random((11, 8), dtype=np.float32)
    row_group = rng.integers(-1, 4, 60).astype(np.int32)
    query_group = rng.integers(0, 3, 11).astype(np.int32)
    ids, d = exact_knn_grouped("sq_euclid", x, q, 5, row_group, query_group, 3)
    for g in range(3):
        sel = query_group == g
        w_ids, w_d = exact_knn("sq_euclid", x, q[sel], 5, mask=row_group == g)
        assert (ids[sel] == w_ids).all() and d[sel].tobytes() == w_d.tobytes()
    assert not np.isin(ids, np.flatnonzero(row_group == 3)).any()          # a value >= n_groups is in no group
    # a row_group shorter than the rows: the ids past its end are in no group
    short, _ = exact_knn_grouped("sq_euclid", x, q, 5, row_group[:30], query_group, 3)
    assert short.max() < 30
    assert group_mask(row_group, 3, 3).sum() == 0 and group_mask(row_group, -1, 3).sum() == 0


def test_the_counters_of_the_model():
    row_group = np.array([0, 0, 1, 2, 2, 2, -1, 9], np.int32)
    assert members(8, row_group, 4).tolist() == [2, 1, 3, 0]
    assert members(8, row_group, 4, live=[0, 2, 3, 4, 6, 7]).tolist() == [1, 1, 2, 0]
    assert members(5, row_group, 4).tolist() == [2, 1, 2, 0]               # n below the array: clamped
    assert evals(8, row_group, [2, 2, 0, 3], 4) == 3 + 3 + 2 + 0
    assert info(8, row_group, [2, 2, 0, 3], 4) == (2, 6)                   # groups 0 and 2 have a query and a candidate


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)


def test_header_declares_the_entry_points_the_library_exports_them_and_the_guide_names_them():
    import hnswindex
    text = _header()
    guide = (ROOT / "INTEGRATION.md").read_text()
    section4 = guide[guide.index("## 4."):]
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", text), sym
        assert hasattr(hnswindex.net_amd.lib, sym), sym
        assert sym in section4, sym


def test_bindings_have_the_methods_and_the_counters_are_where_they_were():
    import hnswindex
    import importlib
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)
    for cls, names in ((net.Index, ("exact_knn_query_grouped", "exact_grouped_info")), (net.DeviceBackend, ("exact_knn_grouped", "exact_grouped_info", "exact_grouped_list_ms"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    # hnswdev_stats did not change: the grouped call's own counters go through hnswdev_exact_grouped_info
    assert ct.sizeof(net.DeviceStats) == ct.sizeof(net.Stats) + 40
    assert net.DeviceStats.field_names()[-5:] == ["exact_launches", "exact_evals", "exact_timed_launches", "exact_timed_evals", "exact_kernel_ms"]
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    ix = net.Index(4, "sq_euclid")
    assert ix.exact_grouped_info() == {"calls": 0, "groups_scanned": 0, "scan_blocks": 0, "ids_listed": 0}
    # an index nothing was added to: padding, and n_groups worked out from the arrays
    ids, d = ix.exact_knn_query_grouped(np.zeros((3, 4), np.float32), 2, np.zeros(5, np.int32), [0, 0, 0])
    assert ids.shape == (3, 2) and (ids == -1).all() and np.isnan(d).all()
    with pytest.raises(ValueError, match="query_group"):
        ix.exact_knn_query_grouped(np.zeros((3, 4), np.float32), 2, np.zeros(5, np.int32), [0, 0])
    assert net._group_args([0, 3, -1], [1, 1], None, 2)[2] == 4 and net._group_args([-1], [0], None, 1)[2] == 1
    assert net._group_args(np.zeros(0, np.int32), [0], None, 1)[2] == 1 and net._group_args([0, 1], [5], None, 1)[2] == 6


def test_null_handle_returns_what_the_ungrouped_calls_return():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    v = np.zeros((2, 4), np.float32)
    rg, qg = np.zeros(8, np.int32), np.zeros(2, np.int32)
    ids, d = np.full((2, 3), 7, np.int32), np.full((2, 3), 7.0, np.float32)
    out_args = (ids.ctypes.data_as(I), d.ctypes.data_as(F))
    grouped = (rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 1)
    # a NULL handle: 0 and nothing written, as hnsw_mi355x_exact_knn_query
    assert lib.hnsw_mi355x_exact_knn_query_grouped(None, v.ctypes.data_as(F), 2, 4, 3, *grouped, *out_args) == \
        lib.hnsw_mi355x_exact_knn_query(None, v.ctypes.data_as(F), 2, 4, 3, None, 0, *out_args) == 0
    assert (ids == 7).all() and (d == 7.0).all()
    out = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_exact_grouped_info(None, out) == lib.hnsw_mi355x_exact_range_info(None, out) == -1 and list(out) == [9] * 4
    # a NULL context: -1, as hnswdev_exact_knn
    assert lib.hnswdev_exact_knn_grouped(None, v.ctypes.data_as(F), 2, 10, 3, *grouped, *out_args) == \
        lib.hnswdev_exact_knn(None, v.ctypes.data_as(F), 2, 10, 3, None, 0, *out_args) == -1
    assert lib.hnswdev_exact_grouped_info(None, out) == -1 and list(out) == [9] * 4
    ms = ct.c_double(9.0)
    assert lib.hnswdev_exact_grouped_list_ms(None, ct.byref(ms)) == -1 and ms.value == 9.0
    assert (ids == 7).all() and (d == 7.0).all()
