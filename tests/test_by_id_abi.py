"""CPU tier: the surfaces of the by-id calls -- the header's declarations, the exported symbols and their ctypes
signatures, the bindings' methods, and the conventions the filtered calls set for a NULL handle, count <= 0 and k < 1."""
import ctypes as ct
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
OUTER = ("hnsw_mi355x_get_vectors", "hnsw_mi355x_knn_query_by_id", "hnsw_mi355x_exact_knn_query_by_id", "hnsw_mi355x_by_id_info")
INNER = ("hnswdev_gather_rows", "hnswdev_knn_search_by_id", "hnswdev_exact_knn_by_id", "hnswdev_by_id_info")
F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
C_TYPES = {"void *": ct.c_void_p, "float *": F, "int *": I, "uint32_t *": U, "uint64_t []": ct.POINTER(ct.c_uint64), "int": ct.c_int,
           "long long": ct.c_longlong}
# the signatures the issue states, spelled out (the header is checked against them as well)
STATED = {
    "hnsw_mi355x_get_vectors": [ct.c_void_p, I, ct.c_int, F],
    "hnsw_mi355x_knn_query_by_id": [ct.c_void_p, I, ct.c_int, ct.c_int, ct.c_int, I, F],
    "hnsw_mi355x_exact_knn_query_by_id": [ct.c_void_p, I, ct.c_int, ct.c_int, U, ct.c_longlong, I, F],
    "hnsw_mi355x_by_id_info": [ct.c_void_p, ct.POINTER(ct.c_uint64)],
    "hnswdev_gather_rows": [ct.c_void_p, I, ct.c_int, F],
}


def _net():
    import hnswindex
    return importlib.import_module(hnswindex.net_amd.Index.__module__)


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)


def _declared(sym):
    params = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1)
    out = []
    for p in params.split(","):
        p = re.sub(r"\bconst\b", "", " ".join(p.split())).strip()
        m = re.fullmatch(r"(.*?)(\w+)(\[\d+\])?", p)
        out.append(C_TYPES[re.sub(r"\s*\*", " *", m.group(1).strip() + (" []" if m.group(3) else ""))])
    return out


def test_symbols_exist_with_the_stated_argtypes():
    net = _net()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for sym in OUTER + INNER:
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int, sym
        assert list(fn.argtypes) == _declared(sym), sym
        assert sym in guide, sym
    for sym, want in STATED.items():
        assert list(getattr(net.lib, sym).argtypes) == want, sym
    for sym in OUTER[:3]:
        assert "partial int " + sym + "(" in guide, sym                  # the P/Invoke lines


def test_bindings_have_the_methods():
    net = _net()
    for cls, names in ((net.Index, ("get_vectors", "items", "knn_query_by_id", "exact_knn_query_by_id", "exact_knn_graph", "by_id_info")),
                       (net.DeviceBackend, ("gather_rows", "knn_search_by_id", "exact_knn_by_id", "by_id_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    ix = net.Index(4, "sq_euclid")                                       # nothing added: no live id, no row
    assert ix.by_id_info() == {"calls": 0, "traversed": 0, "handbacks": 0, "scanned": 0, "rows_gathered": 0, "self_skipped": 0}
    assert ix.items().shape == (0, 4) and ix.get_vectors([]).shape == (0, 4)
    assert ix.knn_query_by_id([], 3)[0].shape == (0, 3) and ix.exact_knn_graph(3)[1].shape == (0, 3)
    for call in (lambda: ix.get_vectors([0]), lambda: ix.knn_query_by_id([2, 0], 3), lambda: ix.exact_knn_query_by_id(5, 3)):
        with pytest.raises(RuntimeError, match=r"ids\[0\] = \d is not a live id"):
            call()
    with pytest.raises(TypeError, match="ids must be integers"):
        ix.get_vectors([0.5])


def test_null_handle_count_and_k_behave_like_the_filtered_calls():
    lib = _net().lib
    v, w = np.zeros((2, 4), np.float32), np.ones(1, np.uint32)
    own = np.zeros(2, np.int32)
    ids, d, flags, rows = np.full((2, 3), 7, np.int32), np.full((2, 3), 7.0, np.float32), np.full(2, 7, np.int32), np.full((2, 4), 7.0, np.float32)
    out_args = (ids.ctypes.data_as(I), d.ctypes.data_as(F))
    filtered = lambda h, count, k: lib.hnsw_mi355x_knn_query_filtered(h, v.ctypes.data_as(F), count, 4, k, w.ctypes.data_as(U), 32, *out_args)
    exact = lambda h, count, k: lib.hnsw_mi355x_exact_knn_query(h, v.ctypes.data_as(F), count, 4, k, w.ctypes.data_as(U), 32, *out_args)
    by_id = lambda h, count, k: lib.hnsw_mi355x_knn_query_by_id(h, own.ctypes.data_as(I), count, k, 0, *out_args)
    exact_by_id = lambda h, count, k: lib.hnsw_mi355x_exact_knn_query_by_id(h, own.ctypes.data_as(I), count, k, None, 0, *out_args)
    # a NULL handle: 0 and nothing written, whatever count and k are
    for count, k in ((2, 3), (0, 3), (-1, 3), (2, 0), (2, -4)):
        assert by_id(None, count, k) == filtered(None, count, k) == 0, (count, k)
        assert exact_by_id(None, count, k) == exact(None, count, k) == 0, (count, k)
        assert lib.hnsw_mi355x_get_vectors(None, own.ctypes.data_as(I), count, rows.ctypes.data_as(F)) == 0
    assert (ids == 7).all() and (d == 7.0).all() and (rows == 7.0).all()
    out = (ct.c_uint64 * 6)(*[9] * 6)
    assert lib.hnsw_mi355x_by_id_info(None, out) == lib.hnsw_mi355x_exact_tagged_info(None, out) == -1
    # a NULL context: -1, as hnswdev_knn_search_filtered and hnswdev_exact_knn
    assert lib.hnswdev_knn_search_by_id(None, own.ctypes.data_as(I), 2, 0, 3, 3, 0, *out_args, flags.ctypes.data_as(I)) == \
        lib.hnswdev_knn_search_filtered(None, v.ctypes.data_as(F), 2, 0, 3, 3, w.ctypes.data_as(U), 32, *out_args, flags.ctypes.data_as(I)) == -1
    assert lib.hnswdev_exact_knn_by_id(None, own.ctypes.data_as(I), 2, 8, 3, None, 0, *out_args) == \
        lib.hnswdev_exact_knn(None, v.ctypes.data_as(F), 2, 8, 3, None, 0, *out_args) == -1
    assert lib.hnswdev_gather_rows(None, own.ctypes.data_as(I), 2, rows.ctypes.data_as(F)) == lib.hnswdev_by_id_info(None, out) == -1
    assert list(out) == [9] * 6 and (ids == 7).all() and (d == 7.0).all() and (flags == 7).all() and (rows == 7.0).all()


def test_the_self_kernel_is_built_where_the_filtered_kernels_are_and_the_gather_kernel_moved():
    csrc = ROOT / "hnswindex.net_amd" / "csrc"
    unit = re.search(r"#define HNSW_UNIT_filtered\(DO, M\)(.*)", (csrc / "device_kernels.h").read_text()).group(1)
    assert all(f"HNSW_##DO##_{kind}" in unit for kind in ("FILTERED", "GROUPED", "TAGGED", "SELF"))
    assert "exact_self_scan_launch<kUnitMetric>" in (csrc / "exact_unit.hip").read_text()
    assert "gather_rows_kernel(" in (csrc / "dk_misc_kernels.h").read_text()
    assert "graph_repair_gather_kernel" not in "".join(f.read_text() for f in csrc.iterdir() if f.is_file())
