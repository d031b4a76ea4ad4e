"""CPU tier: the surfaces of the density clusters -- the header's declarations, the exported symbols and their ctypes
signatures, the bindings' methods, the conventions of a NULL handle and of min_samples < 1, and the two sinks in the exact units.
(cap < length needs an index with an item, so that case runs on the GPU tier, at the end of this file.)"""
import ctypes as ct
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "hnswindex.net_amd" / "csrc"
I, U, U64 = ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_uint64)
C_TYPES = {"void *": ct.c_void_p, "int *": I, "uint32_t *": U, "uint64_t []": U64, "int": ct.c_int, "float": ct.c_float, "long long": ct.c_longlong}
# the signatures the issue states, spelled out (the header is checked against them as well)
STATED = {
    "hnsw_mi355x_density_clusters": [ct.c_void_p, ct.c_float, ct.c_int, U, ct.c_longlong, I, I, ct.c_longlong, U64],
    "hnswdev_exact_range_density": [ct.c_void_p, ct.c_longlong, ct.c_float, ct.c_int, U, ct.c_longlong, I, I, U64],
}
INFO = ("members", "clusters", "core", "border", "noise", "pairs_within", "pairs_measured", "scans")


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
    assert "uint64_t out_info[8]" in (ROOT / "include" / "hnsw_mi355x.h").read_text()


def test_bindings_have_the_methods():
    net = _net()
    for cls, names in ((net.Index, ("density_clusters", "neighbor_counts")), (net.DeviceBackend, ("exact_range_density",))):
        for name in names:
            assert callable(getattr(cls, name)), name
    ix = net.Index(4, "sq_euclid")                                       # nothing added: no live id, no member
    labels, counts, info = ix.density_clusters(1.0, 3)
    assert labels.shape == counts.shape == (0,) and labels.dtype == counts.dtype == np.int32 and info == dict.fromkeys(INFO, 0)
    counts = ix.neighbor_counts(1.0)
    assert counts.shape == (0,) and counts.dtype == np.int32


def test_min_samples_below_one_fails_with_a_message_that_names_the_call():
    net = _net()
    ix = net.Index(4, "sq_euclid")
    for bad in (0, -3):                                                   # an index that holds nothing has no handle yet: the binding says it
        with pytest.raises(ValueError, match=r"density_clusters: min_samples = %d is below 1" % bad):
            ix.density_clusters(1.0, bad)
    # ... and the library says it wherever there is a handle (run on the GPU tier, below); the text is in the index layer and the device layer
    assert '"System.ArgumentException: hnsw_mi355x_density_clusters: min_samples = "' in (CSRC / "hnsw_index.cpp").read_text()
    assert '": min_samples = " + std::to_string(min_samples) + " is below 1"' in (CSRC / "device_backend.hip").read_text()


def test_null_handle_returns_zeros():
    lib = _net().lib
    labels, counts, info = np.full(3, 7, np.int32), np.full(3, 7, np.int32), (ct.c_uint64 * 8)()
    for cap, ms in ((3, 2), (0, 2), (-5, 0)):                             # a NULL handle: 0, out_info zeroed, nothing else looked at
        info[:] = [9] * 8
        assert lib.hnsw_mi355x_density_clusters(None, 1.0, ms, None, 0, labels.ctypes.data_as(I), counts.ctypes.data_as(I), cap, info) == 0
        assert list(info) == [0] * 8
    assert lib.hnsw_mi355x_density_clusters(None, 1.0, 2, None, 0, None, None, 0, None) == 0
    assert (labels == 7).all() and (counts == 7).all()
    # a NULL context: -1, as hnswdev_exact_range_groups
    info[:] = [9] * 8
    assert lib.hnswdev_exact_range_density(None, 8, 1.0, 2, None, 0, labels.ctypes.data_as(I), counts.ctypes.data_as(I), info) == -1
    assert (labels == 7).all() and (counts == 7).all() and list(info) == [9] * 8


def test_the_sinks_are_instantiated_in_the_exact_units():
    unit = (CSRC / "exact_unit.hip").read_text()
    assert "exact_range_density_scan_launch<kUnitMetric>" in unit and "exact_range_density_join_scan_launch<kUnitMetric>" in unit
    scan = (CSRC / "dk_exact.h").read_text()
    for sink in ("ExactRangeDensity", "ExactRangeDensityJoin"):
        assert re.search(r"struct " + sink + r" \{[^}]*kRange = true;[^}]*kSelf = true;[^}]*kDensity = true;[^}]*const int \*self;", scan), sink
        assert f"exact_scan_kernel<METRIC, {sink}>" in scan, sink
    # every sink says whether it is a density sink, so that the others compile as they did
    assert len(re.findall(r"static constexpr bool kDensity = (?:true|false);", scan)) == len(re.findall(r"static constexpr bool kUnion = (?:true|false);", scan)) == 10
    for kernel in ("density_init_kernel", "density_pairs_kernel", "density_labels_kernel"):
        assert "void __launch_bounds__(256) " + kernel in scan, kernel
    assert "density_pair_cap" in (CSRC / "diag.h").read_text() and 'diag("density_pair_cap"' in (CSRC / "device_backend.hip").read_text()


@pytest.mark.gpu
def test_cap_below_the_length_is_an_error():
    import hnswindex
    net = _net()
    ix = hnswindex.Index(4, "sq_euclid")
    ix.add(np.arange(12, dtype=np.float32).reshape(3, 4))
    labels, counts, info = np.full(3, 7, np.int32), np.full(3, 7, np.int32), (ct.c_uint64 * 8)(*[9] * 8)
    call = lambda ms, lp, cp, cap: net.lib.hnsw_mi355x_density_clusters(ix._h, 1.0, ms, None, 0, lp, cp, cap, info)
    assert call(1, labels.ctypes.data_as(I), counts.ctypes.data_as(I), 2) == -1
    assert "hnsw_mi355x_density_clusters: cap = 2 is below the index's length of 3" in net.last_error()
    assert (labels == 7).all() and (counts == 7).all() and list(info) == [0] * 8
    assert call(1, labels.ctypes.data_as(I), None, 3) == -1 and "hnsw_mi355x_density_clusters: out_counts" in net.last_error()
    assert call(0, labels.ctypes.data_as(I), counts.ctypes.data_as(I), 3) == -1
    assert "hnsw_mi355x_density_clusters: min_samples = 0 is below 1" in net.last_error()
    words = (ct.c_uint32 * 1)(7)
    assert net.lib.hnsw_mi355x_density_clusters(ix._h, 1.0, 1, words, -1, labels.ctypes.data_as(I), counts.ctypes.data_as(I), 3, info) == -1
    assert "hnsw_mi355x_density_clusters: nbits must be >= 0" in net.last_error()
    assert net.lib.hnsw_mi355x_density_clusters(ix._h, 1.0, 1, None, 0, labels.ctypes.data_as(I), counts.ctypes.data_as(I), 3, None) == -1
    assert "hnsw_mi355x_density_clusters: out_info" in net.last_error()
    dev = hnswindex.DeviceBackend(4, "sq_euclid", capacity=4)
    dev.upload_rows(0, np.arange(12, dtype=np.float32).reshape(3, 4))
    with pytest.raises(RuntimeError, match="exact_range_density: min_samples = 0 is below 1"):
        dev.exact_range_density(1.0, 0, 3)
    assert (labels == 7).all() and (counts == 7).all()
    assert call(1, labels.ctypes.data_as(I), counts.ctypes.data_as(I), 3) == 0
    assert labels.tolist() == [0, 1, 2] and counts.tolist() == [0, 0, 0] and list(info) == [3, 3, 3, 0, 0, 0, 3, 1]
    labels[:] = 7
    assert call(2, None, counts.ctypes.data_as(I), 3) == 0                # no labels: the counts alone
    assert (labels == 7).all() and counts.tolist() == [0, 0, 0] and list(info) == [3, 0, 0, 0, 0, 0, 3, 1]
