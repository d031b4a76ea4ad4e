"""CPU tier: knn_query_grouped (include/hnsw_mi355x.h hnsw_mi355x_knn_query_grouped) -- its surfaces (header, exports, INTEGRATION.md,
bindings, the NULL-handle conventions of the filtered call, argument errors raised before anything native runs) and the plain-Python
statement of its contract (tests/grouped_query_model.py) pinned to the oracle on one graph."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from common import uniform
from filtered_model import filtered_knn_batch
from grouped_query_model import group_mask, grouped_knn_batch

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("hnsw_mi355x_knn_query_grouped", "hnsw_mi355x_knn_grouped_info", "hnswdev_knn_search_grouped", "hnswdev_knn_grouped_info")


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
    assert "hnsw_mi355x_knn_query_grouped(handle" in guide[:guide.index("## 4.")]   # and the call is shown where the filtered ones are


def test_bindings_have_the_methods_and_hnswdev_stats_is_what_it_was():
    import hnswindex
    import importlib
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)
    for cls, names in ((net.Index, ("knn_query_grouped", "knn_grouped_info")), (net.DeviceBackend, ("knn_search_grouped", "knn_grouped_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    assert net.DeviceStats.field_names()[-1] == "exact_kernel_ms"            # nothing appended: the call's counters have their own entry point
    ix = net.Index(4, "sq_euclid")
    assert ix.knn_grouped_info() == {"calls": 0, "launched": 0, "skipped": 0, "handbacks": 0}
    # an index nothing was added to: padding in knn_query's shape, n_groups worked out from the arrays, any layer
    for layer in (0, 3):
        ids, d = ix.knn_query_grouped(np.zeros((3, 4), np.float32), 2, np.zeros(5, np.int32), [0, 1, 0], layer=layer)
        assert ids.shape == d.shape == (3, 2) and ids.dtype == np.int32 and d.dtype == np.float32
        assert (ids == -1).all() and np.isnan(d).all()


def test_group_argument_errors_are_raised_before_any_native_call(monkeypatch):
    import hnswindex
    import importlib
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)

    def native(*a):
        raise AssertionError("the native call ran")
    monkeypatch.setattr(net.lib, "hnsw_mi355x_knn_query_grouped", native)
    ix = net.Index(4, "sq_euclid")
    with pytest.raises(ValueError, match="query_group has 2 entries for 3 queries"):
        ix.knn_query_grouped(np.zeros((3, 4), np.float32), 2, np.zeros(5, np.int32), [0, 0])
    with pytest.raises(ValueError, match="query_group has 4 entries for 1 queries"):
        ix.knn_query_grouped(np.zeros(4, np.float32), 2, np.zeros(5, np.int32), [0, 0, 0, 0])
    with pytest.raises(ValueError, match="expected dim=4"):
        ix.knn_query_grouped(np.zeros((3, 5), np.float32), 2, np.zeros(5, np.int32), [0, 0, 0])
    with pytest.raises(AssertionError, match="the native call ran"):       # (the stand-in is what a well-formed call reaches)
        ix.knn_query_grouped(np.zeros((3, 4), np.float32), 2, np.zeros(5, np.int32), [0, 0, 0])


def test_null_handle_returns_what_the_filtered_calls_return():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), np.float32)
    rg, qg, w = np.zeros(8, np.int32), np.zeros(2, np.int32), np.ones(1, np.uint32)
    ids, d, flags = np.full((2, 3), 7, np.int32), np.full((2, 3), 7.0, np.float32), np.full(2, 7, np.int32)
    out_args = (ids.ctypes.data_as(I), d.ctypes.data_as(F))
    grouped = (rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 1)
    # a NULL handle: 0 and nothing written, as hnsw_mi355x_knn_query_filtered / _at_layer
    assert lib.hnsw_mi355x_knn_query_grouped(None, v.ctypes.data_as(F), 2, 4, 3, 0, *grouped, *out_args) == \
        lib.hnsw_mi355x_knn_query_filtered(None, v.ctypes.data_as(F), 2, 4, 3, w.ctypes.data_as(U), 32, *out_args) == \
        lib.hnsw_mi355x_knn_query_at_layer(None, v.ctypes.data_as(F), 2, 4, 3, 1, w.ctypes.data_as(U), 32, *out_args) == 0
    assert (ids == 7).all() and (d == 7.0).all()
    out = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_knn_grouped_info(None, out) == lib.hnsw_mi355x_exact_grouped_info(None, out) == -1 and list(out) == [9] * 4
    # a NULL context: -1, as hnswdev_knn_search_filtered
    assert lib.hnswdev_knn_search_grouped(None, v.ctypes.data_as(F), 2, 0, 3, 3, 0, *grouped, *out_args, flags.ctypes.data_as(I)) == \
        lib.hnswdev_knn_search_filtered(None, v.ctypes.data_as(F), 2, 0, 3, 3, w.ctypes.data_as(U), 32, *out_args, flags.ctypes.data_as(I)) == -1
    assert lib.hnswdev_knn_grouped_info(None, out) == -1 and list(out) == [9] * 4
    assert (ids == 7).all() and (d == 7.0).all() and (flags == 7).all()


@pytest.fixture(scope="module")
def graph():
    import oracle
    n, dim, min_nn = 400, 8, 12
    x = uniform(n, dim, 11)
    ix = oracle.OracleIndex(dim, "sq_euclid", max_edges=6, min_nn=min_nn, max_candidates=20, collection_size=n)
    ix.add(x)
    return ix, x, min_nn


def test_the_model_is_the_oracle_on_one_graph(graph):
    """One group that holds every id: OracleIndex.knn_query bit for bit, whatever else the arrays name.  A group of 6 ids: brute
    force over its rows (layer 0 is connected here, and the result heap never fills).  Every result carries its query's group."""
    import oracle
    ix, x, min_nn = graph
    n = x.shape[0]
    q = uniform(14, 8, 12)
    for k in (5, 20):
        want = ix.knn_query(q, k)
        got = grouped_knn_batch(ix, x, "sq_euclid", q, k, min_nn, np.full(n + 50, 2, np.int32), np.full(14, 2, np.int32), 3)
        assert (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes(), k
    rng = np.random.default_rng(5)
    row_group = rng.choice(3, n, p=[0.6, 0.3, 0.1]).astype(np.int32)
    small = rng.choice(n, 6, replace=False)
    row_group[small] = 3
    row_group[rng.choice(np.setdiff1d(np.arange(n), small), 20, replace=False)] = -1
    row_group[np.flatnonzero(row_group == 0)[:5]] = 9                      # a value >= n_groups: no group
    query_group = rng.permutation(np.arange(14) % 5).astype(np.int32)      # group 4: no row carries it
    ids, d = grouped_knn_batch(ix, x, "sq_euclid", q, 4, min_nn, row_group, query_group, 5)
    for i in range(14):
        got = ids[i][ids[i] >= 0]
        assert (row_group[got] == query_group[i]).all(), i
    assert (ids[query_group == 4] == -1).all() and np.isnan(d[query_group == 4]).all()
    srt = np.sort(small)
    for i in np.flatnonzero(query_group == 3):
        bd = oracle.dist_query_rows("sq_euclid", x, q[i], srt)
        order = np.argsort(bd, kind="stable")[:4]
        assert ids[i].tolist() == srt[order].tolist() and d[i].tobytes() == bd[order].astype(np.float32).tobytes()


def test_the_model_is_the_filtered_model_per_group_with_rows_scattered_back(graph):
    ix, x, min_nn = graph
    n = x.shape[0]
    rng = np.random.default_rng(6)
    q = uniform(12, 8, 13)
    row_group = rng.integers(-1, 4, n - 100).astype(np.int32)              # shorter than the rows: ids past its end have no group
    query_group = rng.integers(0, 3, 12).astype(np.int32)
    ids, d = grouped_knn_batch(ix, x, "sq_euclid", q, 5, min_nn, row_group, query_group, 3)
    for g in range(3):
        sel = query_group == g
        mask = np.zeros(n, dtype=bool)
        mask[:n - 100] = row_group == g
        assert (group_mask(row_group, g, 3, n) == mask).all()
        w_ids, w_d = filtered_knn_batch(ix, x, "sq_euclid", q[sel], 5, min_nn, mask)
        assert (ids[sel] == w_ids).all() and d[sel].tobytes() == w_d.tobytes()
    assert ids.max() < n - 100 and not np.isin(ids, np.flatnonzero(row_group == 3)).any()
    assert not group_mask(row_group, 3, 3, n).any() and not group_mask(row_group, -1, 3, n).any()
    with pytest.raises(ValueError):
        grouped_knn_batch(ix, x, "sq_euclid", q, 5, min_nn, row_group, query_group[:5], 3)
    with pytest.raises(ValueError):
        grouped_knn_batch(ix, x, "sq_euclid", q, 5, min_nn, row_group, np.full(12, 3), 3)
