"""CPU tier: the surfaces of the near-duplicate calls over the graph's edges -- the exported symbols with their
ctypes signatures, their P/Invoke lines in INTEGRATION.md, the bindings' methods on an index without items, the conventions of a
NULL handle, the diag name and the kernel's place in the host unit."""
import ctypes as ct
import importlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hnswindex.net_amd" / "csrc"
F, I, U, U64, LL = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_longlong)
STATED = {
    "hnsw_mi355x_graph_duplicate_groups": [ct.c_void_p, ct.c_float, U, ct.c_longlong, I, ct.c_longlong, U64],
    "hnsw_mi355x_near_edges": [ct.c_void_p, ct.c_float, U, ct.c_longlong, LL],
    "hnsw_mi355x_near_edges_results": [ct.c_void_p, I, I, F, ct.c_longlong],
    "hnswdev_graph_edge_groups": [ct.c_void_p, ct.c_longlong, ct.c_float, U, ct.c_longlong, I, U64],
    "hnswdev_graph_near_edges": [ct.c_void_p, ct.c_longlong, ct.c_float, U, ct.c_longlong, LL],
    "hnswdev_graph_near_edges_results": [ct.c_void_p, I, I, F, ct.c_longlong],
}


def _net():
    import hnswindex
    return importlib.import_module(hnswindex.net_amd.Index.__module__)


def test_symbols_exist_with_the_stated_argtypes():
    net = _net()
    guide = (ROOT / "INTEGRATION.md").read_text()
    header = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    for sym, want in STATED.items():
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int and list(fn.argtypes) == want, sym
        assert "partial int " + sym + "(" in guide and "int " + sym + "(" in header, sym


def test_bindings_on_an_index_without_items():
    net = _net()
    for cls, names in ((net.Index, ("graph_duplicate_groups", "near_edges")), (net.DeviceBackend, ("graph_edge_groups", "graph_near_edges"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    ix = net.Index(4, "sq_euclid")
    labels, info = ix.graph_duplicate_groups(1.0)
    assert labels.shape == (0,) and labels.dtype == np.int32
    assert info == {"members": 0, "groups": 0, "edges_within": 0, "edges_measured": 0, "launches": 0}
    src, dst, d = ix.near_edges(1.0)
    assert src.size == dst.size == d.size == 0 and (src.dtype, dst.dtype, d.dtype) == (np.int32, np.int32, np.float32)


def test_null_handle_and_null_outputs():
    lib = _net().lib
    info = (ct.c_uint64 * 5)(*[9] * 5)
    assert lib.hnsw_mi355x_graph_duplicate_groups(None, 1.0, None, 0, None, 0, info) == 0 and list(info) == [0] * 5
    count = ct.c_longlong(9)
    assert lib.hnsw_mi355x_near_edges(None, 1.0, None, 0, ct.byref(count)) == 0 and count.value == 0
    assert lib.hnsw_mi355x_near_edges_results(None, None, None, None, 0) == 0
    assert lib.hnswdev_graph_edge_groups(None, 0, 1.0, None, 0, None, info) == -1
    assert lib.hnswdev_graph_near_edges(None, 0, 1.0, None, 0, ct.byref(count)) == -1
    assert lib.hnswdev_graph_near_edges_results(None, None, None, None, 0) == -1


def test_the_kernel_lives_in_the_host_unit_and_the_diag_name_is_listed():
    backend = (CSRC / "device_backend.hip").read_text()
    assert '#include "dk_edge_groups.h"' in backend and backend.index("#define HNSW_HOST_TU") < backend.index('#include "dk_edge_groups.h"')
    assert "dk_edge_groups.h" not in (CSRC / "kernel_unit.hip").read_text() + (CSRC / "exact_unit.hip").read_text() + (CSRC / "device_kernels.h").read_text()
    assert 'diag("edge_round", 0)' in backend and "edge_round [0 = 65 536" in (CSRC / "diag.h").read_text()
