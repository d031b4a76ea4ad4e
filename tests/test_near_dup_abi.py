"""CPU tier: the surfaces of the near-duplicate calls -- the header's declarations, the exported symbols and their
ctypes signatures, the bindings' methods, the conventions of a NULL handle and count <= 0, and the two sinks in the exact units.
(cap < length needs an index with an item, so that case runs on the GPU tier, at the end of this file.)"""
import ctypes as ct
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hnswindex.net_amd" / "csrc"
F, I, U, PP, U64 = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_uint64)
C_TYPES = {"void *": ct.c_void_p, "void * *": PP, "float *": F, "int *": I, "uint32_t *": U, "uint64_t []": U64, "int": ct.c_int, "float": ct.c_float,
           "long long": ct.c_longlong}
# the signatures the issue states, spelled out (the header is checked against them as well)
STATED = {
    "hnsw_mi355x_exact_range_query_by_id": [ct.c_void_p, I, ct.c_int, ct.c_float, U, ct.c_longlong, PP, PP, I],
    "hnsw_mi355x_duplicate_groups": [ct.c_void_p, ct.c_float, U, ct.c_longlong, I, ct.c_longlong, U64],
    "hnswdev_exact_range_by_id": [ct.c_void_p, I, ct.c_int, ct.c_longlong, ct.c_float, U, ct.c_longlong, I],
    "hnswdev_exact_range_groups": [ct.c_void_p, ct.c_longlong, ct.c_float, U, ct.c_longlong, I, U64],
}


def _net():
    import hnswindex
    return importlib.import_module(hnswindex.net_amd.Index.__module__)


def _declared(sym):
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)
    params = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\)\s*;", header, flags=re.S).group(1)
    out = []
    for p in params.split(","):
        p = re.sub(r"\bconst\b", "", " ".join(p.split())).strip()
        m = re.fullmatch(r"(.*?)(\w+)(\[\d+\])?", p)
        out.append(C_TYPES[" ".join(re.sub(r"\*", " * ", m.group(1) + (" []" if m.group(3) else "")).split())])
    return out


def test_symbols_exist_with_the_stated_argtypes():
    net = _net()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for sym, want in STATED.items():
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int, sym
        assert list(fn.argtypes) == want == _declared(sym), sym
        assert sym in guide, sym
    for sym in ("hnsw_mi355x_exact_range_query_by_id", "hnsw_mi355x_duplicate_groups"):
        assert "partial int " + sym + "(" in guide, sym                  # the P/Invoke lines


def test_bindings_have_the_methods():
    net = _net()
    for cls, names in ((net.Index, ("exact_range_query_by_id", "exact_radius_graph", "duplicate_groups")),
                       (net.DeviceBackend, ("exact_range_by_id", "exact_range_groups"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    ix = net.Index(4, "sq_euclid")                                       # nothing added: no live id, no member
    assert ix.exact_range_query_by_id([], 1.0) == ([], []) and ix.exact_radius_graph(1.0) == ([], [])
    labels, info = ix.duplicate_groups(1.0)
    assert labels.shape == (0,) and labels.dtype == np.int32 and info == {"members": 0, "groups": 0, "pairs_within": 0, "pairs_measured": 0}
    with pytest.raises(RuntimeError, match=r"hnsw_mi355x_exact_range_query_by_id: ids\[0\] = 2 is not a live id"):
        ix.exact_range_query_by_id([2, 0], 1.0)
    with pytest.raises(TypeError, match="ids must be integers"):
        ix.exact_range_query_by_id([0.5], 1.0)


def test_null_handle_and_count_behave_like_exact_range_query():
    lib = _net().lib
    v, own = np.zeros((2, 4), np.float32), np.zeros(2, np.int32)
    ids_pp, dists_pp, counts = (ct.c_void_p * 2)(7, 7), (ct.c_void_p * 2)(7, 7), (ct.c_int * 2)(7, 7)
    by_id = lambda h, count: lib.hnsw_mi355x_exact_range_query_by_id(h, own.ctypes.data_as(I), count, 1.0, None, 0, ids_pp, dists_pp, counts)
    plain = lambda h, count: lib.hnsw_mi355x_exact_range_query(h, v.ctypes.data_as(F), count, 4, 1.0, None, 0, ids_pp, dists_pp, counts)
    for count in (2, 0, -1):                                             # a NULL handle: 0 and nothing written, whatever count is
        assert by_id(None, count) == plain(None, count) == 0, count
    assert list(ids_pp) == list(dists_pp) == [7, 7] and list(counts) == [7, 7]
    # the groups with a NULL handle: 0, out_info zeroed, the labels and cap not looked at
    labels, info = np.full(3, 7, np.int32), (ct.c_uint64 * 4)(9, 9, 9, 9)
    for cap in (3, 0, -5):
        info[:] = [9, 9, 9, 9]
        assert lib.hnsw_mi355x_duplicate_groups(None, 1.0, None, 0, labels.ctypes.data_as(I), cap, info) == 0 and list(info) == [0, 0, 0, 0]
    assert lib.hnsw_mi355x_duplicate_groups(None, 1.0, None, 0, None, 0, None) == 0 and (labels == 7).all()
    # a NULL context: -1, as hnswdev_exact_range
    cnt = np.full(2, 7, np.int32)
    assert lib.hnswdev_exact_range_by_id(None, own.ctypes.data_as(I), 2, 8, 1.0, None, 0, cnt.ctypes.data_as(I)) == \
        lib.hnswdev_exact_range(None, v.ctypes.data_as(F), 2, 8, 1.0, None, 0, cnt.ctypes.data_as(I)) == -1
    info[:] = [9, 9, 9, 9]
    assert lib.hnswdev_exact_range_groups(None, 8, 1.0, None, 0, labels.ctypes.data_as(I), info) == -1
    assert (cnt == 7).all() and (labels == 7).all() and list(info) == [9, 9, 9, 9]


def test_the_sinks_are_instantiated_in_the_exact_units_and_the_union_find_has_a_header_of_its_own():
    unit = (CSRC / "exact_unit.hip").read_text()
    assert "exact_range_self_scan_launch<kUnitMetric>" in unit and "exact_range_union_scan_launch<kUnitMetric>" in unit
    scan = (CSRC / "dk_exact.h").read_text()
    for sink in ("ExactRangeSelf", "ExactRangeUnion"):
        assert re.search(r"struct " + sink + r" \{[^}]*kRange = true;[^}]*kSelf = true;[^}]*const int \*self;", scan), sink
        assert f"exact_scan_kernel<METRIC, {sink}>" in scan, sink
    assert '#include "dk_union_find.h"' in scan and '#include "dk_union_find.h"' in (CSRC / "dk_graph_info.h").read_text()
    uf = (CSRC / "dk_union_find.h").read_text()
    assert "int uf_find(int *parent, int v)" in uf and "void uf_union(int *parent, int a, int b)" in uf
    assert "uf_find(int *parent" not in (CSRC / "dk_graph_info.h").read_text()
    assert "exact_union_round" in (CSRC / "diag.h").read_text()


@pytest.mark.gpu
def test_cap_below_the_length_is_an_error():
    import hnswindex
    lib = _net().lib
    ix = hnswindex.Index(4, "sq_euclid")
    ix.add(np.arange(12, dtype=np.float32).reshape(3, 4))
    labels, info = np.full(3, 7, np.int32), (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_duplicate_groups(ix._h, 1.0, None, 0, labels.ctypes.data_as(I), 2, info) == -1
    assert "hnsw_mi355x_duplicate_groups: cap = 2 is below the index's length of 3" in _net().last_error()
    assert (labels == 7).all() and list(info) == [0, 0, 0, 0]
    assert lib.hnsw_mi355x_duplicate_groups(ix._h, 1.0, None, 0, labels.ctypes.data_as(I), 3, info) == 0
    assert labels.tolist() == [0, 1, 2] and list(info) == [3, 3, 0, 3]
