"""CPU tier: the reference of the grouped range traversal (tests/grouped_range_model.py) on hand-made cases of about 50 rows -- held
to the CPU oracle's unfiltered RangeQuery (one group: equal lists; several: the same closure, partitioned) and to the empty-heap
rule -- and the surfaces of the call: header, exports, INTEGRATION.md, bindings, argument errors, hnswdev_stats left as it was."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from grouped_range_model import HeapEmpty, group_mask, grouped_range, heap_empty_closed_form

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("hnsw_mi355x_range_query_grouped", "hnsw_mi355x_range_grouped_info", "hnswdev_range_search_grouped", "hnswdev_range_grouped_info")
INFO = {"calls": 0, "launched": 0, "skipped": 0, "host_finished": 0}
N, DIM, M = 50, 8, 4


def _oracle(metric, x):
    import oracle
    ref = oracle.OracleIndex(DIM, metric, max_edges=M, min_nn=6, collection_size=64)
    ref.add(x)
    return ref


def _case():
    rng = np.random.default_rng(5)
    x = rng.integers(1, 4, (N, DIM)).astype(np.float32)   # grid data: equal distances abound
    q = rng.integers(1, 4, (9, DIM)).astype(np.float32)
    row_group = (np.arange(N) % 3).astype(np.int32)
    row_group[11] = 3                                   # group 3 has one member, group 4 none
    row_group[[0, 1]] = [-1, 7]                         # in no group
    query_group = np.array([4, 2, 0, 3, 1, 0, 4, 3, 2], np.int32)   # scrambled, the empty group named twice
    return x, q, row_group, query_group, 5


def test_one_group_is_the_oracles_unfiltered_range_query():
    x, q, _, _, _ = _case()
    ref = _oracle("sq_euclid", x)
    for radius in (9.0, 16.0):
        ids, d = grouped_range(ref, x, "sq_euclid", q, radius, np.zeros(N, np.int32), np.zeros(9, np.int32), 1)
        w_ids, w_d = ref.range_query(q, radius)
        assert sum(a.size for a in ids) > 9
        assert all(a.tolist() == b.tolist() and c.tobytes() == e.tobytes() for a, b, c, e in zip(ids, w_ids, d, w_d)), radius


def test_groups_partition_the_unfiltered_closure_and_come_back_in_query_order():
    x, q, row_group, query_group, n_groups = _case()
    ref = _oracle("sq_euclid", x)
    radius = 9.0
    ids, d = grouped_range(ref, x, "sq_euclid", q, radius, row_group, query_group, n_groups)
    full_ids, full_d = ref.range_query(q, radius)
    ties = 0
    for i in range(9):
        member = group_mask(row_group, query_group[i], N)[full_ids[i]]
        # radius >= 0: the closure does not depend on the filter, so the results are its members in the group ...
        assert sorted(ids[i].tolist()) == sorted(full_ids[i][member].tolist()), i
        # ... each with the distance the unfiltered call measured, ascending
        by_id = dict(zip(full_ids[i].tolist(), full_d[i].tolist()))
        assert d[i].tolist() == [by_id[j] for j in ids[i].tolist()] and (np.diff(d[i]) >= 0).all(), i
        ties += int((np.diff(d[i]) == 0).any())
        assert ids[i].dtype == np.int32 and d[i].dtype == np.float32
    assert ids[0].size == ids[6].size == 0 and ties >= 1                     # the empty group; equal distances among results
    assert set(ids[3].tolist()) <= {11} and set(ids[7].tolist()) <= {11}     # the one-row group
    assert not np.isin(np.concatenate(ids), [0, 1]).any()                    # labels outside [0, n_groups) are in no group
    short, _ = grouped_range(ref, x, "sq_euclid", q, radius, row_group[:20], query_group, n_groups)   # ids past the array's end too
    assert np.concatenate(short).max() < 20


def test_heap_empty_propagates():
    rng = np.random.default_rng(21)
    x = rng.normal(size=(N, DIM)).astype(np.float32)       # unnormalised ucosine: 1 - dot goes negative
    q = rng.normal(size=(12, DIM)).astype(np.float32)
    ref = _oracle("ucosine", x)
    row_group = (np.arange(N) % 3).astype(np.int32)
    query_group = (np.arange(12) % 3).astype(np.int32)
    throws = [heap_empty_closed_form(ref, x, "ucosine", q[i], -1.0, group_mask(row_group, query_group[i], N)) for i in range(12)]
    assert any(throws) and not all(throws)
    with pytest.raises(HeapEmpty):
        grouped_range(ref, x, "ucosine", q, -1.0, row_group, query_group, 3)
    keep = np.flatnonzero(~np.array(throws))
    ids, _ = grouped_range(ref, x, "ucosine", q[keep], -1.0, row_group, query_group[keep], 3)
    assert len(ids) == keep.size


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
    for cls, names in ((net.Index, ("range_query_grouped", "range_grouped_info")), (net.DeviceBackend, ("range_search_grouped", "range_grouped_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    # hnswdev_stats did not change: the grouped call's own counters go through hnswdev_range_grouped_info
    assert ct.sizeof(net.DeviceStats) == ct.sizeof(net.Stats) + 40
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    ix = net.Index(4, "sq_euclid")
    assert ix.range_grouped_info() == INFO
    # an index nothing was added to: empty lists, and n_groups worked out from the arrays
    ids, d = ix.range_query_grouped(np.zeros((3, 4), np.float32), 1.0, np.zeros(5, np.int32), [0, 0, 0])
    assert len(ids) == len(d) == 3 and all(a.size == 0 and a.dtype == np.int32 for a in ids) and all(a.size == 0 and a.dtype == np.float32 for a in d)
    with pytest.raises(ValueError, match="query_group"):
        ix.range_query_grouped(np.zeros((3, 4), np.float32), 1.0, np.zeros(5, np.int32), [0, 0])


def test_null_handle_and_argument_errors():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    v = np.zeros((2, 4), np.float32)
    rg, qg = np.zeros(8, np.int32), np.zeros(2, np.int32)
    counts = np.full(2, 7, np.int32)
    flags = np.full(2, 7, np.int32)
    pp_i, pp_d = (ct.c_void_p * 2)(0x1234, 0x1234), (ct.c_void_p * 2)(0x1234, 0x1234)
    grouped = (rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 1)
    out_args = (pp_i, pp_d, counts.ctypes.data_as(I))
    # a NULL handle: 0 and nothing written, as hnsw_range_query
    assert lib.hnsw_mi355x_range_query_grouped(None, v.ctypes.data_as(F), 2, 4, ct.c_float(1.0), 0, *grouped, *out_args) == 0
    assert (counts == 7).all() and list(pp_i) == [0x1234] * 2 and list(pp_d) == [0x1234] * 2
    out = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_range_grouped_info(None, out) == -1 and list(out) == [9] * 4
    # a NULL context: -1, as hnswdev_range_search
    assert lib.hnswdev_range_search_grouped(None, v.ctypes.data_as(F), 2, 0, ct.c_float(1.0), 0, *grouped, counts.ctypes.data_as(I), flags.ctypes.data_as(I)) == -1
    assert lib.hnswdev_range_grouped_info(None, out) == -1 and list(out) == [9] * 4
    # the header states the call's contract and its failure
    full = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    doc = full[full.index("RangeQuery with a GROUP FILTER PER QUERY"):full.index("int hnsw_mi355x_range_query_grouped(")]
    for word in ("Heap is empty", "every array", "range >= 0", "hnsw_mi355x_knn_query_grouped"):
        assert word in doc, word
    if lib.hnswdev_device_count() <= 0:
        return   # (a handle needs a device; tests/test_gpu_grouped_range.py makes the same calls on both layers)
    h = lib.hnsw_create(b"sq_euclid")
    assert h
    bad = np.array([0, 3], np.int32)
    cases = (((rg.ctypes.data_as(I), 8, bad.ctypes.data_as(I), 3), r"query_group\[1\]"), ((None, 8, qg.ctypes.data_as(I), 1), "row_group"),
             ((rg.ctypes.data_as(I), -1, qg.ctypes.data_as(I), 1), "n_row_group"), ((rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 65537), "65536"),
             ((rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 0), "65536"))
    for args, word in cases:
        counts[:] = 7
        pp_i[0] = pp_i[1] = pp_d[0] = pp_d[1] = 0x1234
        assert lib.hnsw_mi355x_range_query_grouped(h, v.ctypes.data_as(F), 2, 4, ct.c_float(1.0), 0, *args, *out_args) == -1, word
        assert (counts == 0).all() and all(p is None for p in pp_i) and all(p is None for p in pp_d), word
        assert re.search(word, hnswindex.net_amd.last_error()), (word, hnswindex.net_amd.last_error())
    lib.hnsw_free(h)
