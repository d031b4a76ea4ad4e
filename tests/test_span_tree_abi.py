"""CPU tier: the surfaces of the single-linkage tree -- the header's declarations, the exported symbols and their
ctypes signatures, the bindings' methods, the conventions of a NULL handle and a NULL context, the new diag name, and that the scan
is no row of the sink list.  (cap, a NULL output and nbits < 0 need an index with items: that case runs on the GPU tier, at the end.)"""
import ctypes as ct
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hnswindex.net_amd" / "csrc"
I, F, U, U64 = ct.POINTER(ct.c_int), ct.POINTER(ct.c_float), ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_uint64)
C_TYPES = {"void *": ct.c_void_p, "int *": I, "float *": F, "uint32_t *": U, "uint64_t []": U64, "long long": ct.c_longlong}
# the signatures the issue states, spelled out (the header is checked against them as well)
STATED = {
    "hnsw_mi355x_single_linkage_tree": [ct.c_void_p, U, ct.c_longlong, I, I, F, ct.c_longlong, U64],
    "hnswdev_exact_span_tree": [ct.c_void_p, ct.c_longlong, U, ct.c_longlong, I, I, F, ct.c_longlong, U64],
}
INFO = ("members", "edges", "components", "rounds", "pairs_measured", "pairs_skipped", "launches", "reserved")


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


def test_bindings_have_the_methods_and_an_empty_index_has_no_edge():
    net = _net()
    for cls, names in ((net.Index, ("single_linkage_tree", "single_linkage_cut")), (net.DeviceBackend, ("exact_span_tree",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    ix = net.Index(4, "sq_euclid")                                       # nothing added: no live id, no member
    a, b, d, info = ix.single_linkage_tree()
    assert a.shape == b.shape == d.shape == (0,) and a.dtype == b.dtype == np.int32 and d.dtype == np.float32
    assert info == dict.fromkeys(INFO, 0) and tuple(info) == INFO
    assert ix.single_linkage_cut((a, b, d, info), 1.0).shape == (0,)


def test_null_handle_and_null_context():
    lib = _net().lib
    a, b, d, info = np.full(3, 7, np.int32), np.full(3, 7, np.int32), np.full(3, 7, np.float32), (ct.c_uint64 * 8)()
    ptrs = (a.ctypes.data_as(I), b.ctypes.data_as(I), d.ctypes.data_as(F))
    for cap in (3, 0, -5):                                                # a NULL handle: 0, out_info zeroed, nothing else looked at
        info[:] = [9] * 8
        assert lib.hnsw_mi355x_single_linkage_tree(None, None, 0, *ptrs, cap, info) == 0
        assert list(info) == [0] * 8
    assert lib.hnsw_mi355x_single_linkage_tree(None, None, -1, None, None, None, 0, None) == 0
    info[:] = [9] * 8                                                     # a NULL context: -1, nothing written
    assert lib.hnswdev_exact_span_tree(None, 8, None, 0, *ptrs, 3, info) == -1
    assert (a == 7).all() and (b == 7).all() and (d == 7).all() and list(info) == [9] * 8


def test_the_scan_is_no_sink_and_has_its_round_knob():
    scan = (CSRC / "dk_exact.h").read_text()
    rows = re.findall(r"X\((\w+)\)", re.search(r"#define HNSW_FOR_EACH_EXACT_SINK\(X\)((?:.*\\\n)*.*)", scan).group(1))
    assert len(rows) == 10                                                # the sink list still has its 10 rows
    assert "template hipError_t span_scan_launch<kUnitMetric>(" in (CSRC / "exact_unit.hip").read_text()
    assert "span_round" in (CSRC / "diag.h").read_text() and '"span_round"' in (CSRC / "device_backend.hip").read_text()


@pytest.mark.gpu
def test_cap_null_outputs_and_nbits_are_errors_that_name_the_call():
    import hnswindex
    net = _net()
    call = net.lib.hnsw_mi355x_single_linkage_tree
    ix = hnswindex.Index(4, "sq_euclid")
    ix.add(np.array([[0, 0, 0, 0], [3, 0, 0, 0], [1, 0, 0, 0]], dtype=np.float32))
    a, b, d, info = np.full(2, 7, np.int32), np.full(2, 7, np.int32), np.full(2, 7, np.float32), (ct.c_uint64 * 8)(*[9] * 8)
    pa, pb, pd = a.ctypes.data_as(I), b.ctypes.data_as(I), d.ctypes.data_as(F)
    assert call(ix._h, None, 0, pa, pb, pd, 1, info) == -1
    assert "hnsw_mi355x_single_linkage_tree: cap = 1 is below members - 1 = 2" in net.last_error() and list(info) == [0] * 8
    for ptrs, name in (((None, pb, pd), "out_a"), ((pa, None, pd), "out_b"), ((pa, pb, None), "out_dist")):
        assert call(ix._h, None, 0, *ptrs, 2, info) == -1 and "hnsw_mi355x_single_linkage_tree: " + name in net.last_error()
    assert call(ix._h, (ct.c_uint32 * 1)(7), -1, pa, pb, pd, 2, info) == -1
    assert "hnsw_mi355x_single_linkage_tree: nbits must be >= 0" in net.last_error()
    assert call(ix._h, None, 0, pa, pb, pd, 2, None) == -1 and "hnsw_mi355x_single_linkage_tree: out_info" in net.last_error()
    assert (a == 7).all() and (b == 7).all() and (d == 7).all()
    assert call(ix._h, None, 0, pa, pb, pd, 2, info) == 0                 # three rows on a line at 0, 3, 1: two edges
    assert (a.tolist(), b.tolist(), d.tolist()) == ([0, 1], [2, 2], [1.0, 4.0])
    assert dict(zip(INFO, info)) == {"members": 3, "edges": 2, "components": 1, "rounds": 1, "pairs_measured": 3, "pairs_skipped": 0, "launches": 1,
                                     "reserved": 0}
    dev = hnswindex.DeviceBackend(4, "sq_euclid", capacity=4)
    dev.upload_rows(0, np.arange(12, dtype=np.float32).reshape(3, 4))
    with pytest.raises(RuntimeError, match="exact_span_tree: cap = 0 is below members - 1 = 2"):
        net.DeviceBackend._check(dev, net.lib.hnswdev_exact_span_tree(dev._ctx, 3, None, 0, pa, pb, pd, 0, info))
