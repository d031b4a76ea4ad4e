"""The counters of the spanning trees' MFMA prefilter through the ABI, without a GPU: both getters are declared with
out[4] and exported, a NULL handle is an error that writes nothing, an index without a native handle reports the four named zeros, and
the kernel's launcher is instantiated per metric in exact_unit.hip."""
import ctypes as ct
import importlib
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "hnsw_mi355x.h").read_text()
SLOTS = ("launches", "pairs_on_tile", "pairs_remeasured", "reserved")


@pytest.mark.parametrize("name,arg", [("hnsw_mi355x_span_prefilter_stats", "handle"), ("hnswdev_span_prefilter_stats", "ctx")])
def test_getter_is_declared_exported_and_refuses_null(name, arg):
    import hnswindex
    assert re.search(r"\bint %s\(void \*%s, uint64_t out\[4\]\);" % (name, arg), HEADER), name
    fn = getattr(importlib.import_module(hnswindex.net_amd.Index.__module__).lib, name)      # AttributeError: not exported
    assert fn.restype is ct.c_int and list(fn.argtypes) == [ct.c_void_p, ct.POINTER(ct.c_uint64)], name
    out = (ct.c_uint64 * 4)(7, 7, 7, 7)
    assert fn(None, out) == -1 and list(out) == [7, 7, 7, 7], name


def test_index_without_a_handle_reports_zeros():
    import hnswindex
    ix = hnswindex.Index.__new__(hnswindex.Index)
    ix._h = None
    assert ix.span_prefilter_stats() == dict.fromkeys(SLOTS, 0)
    assert callable(hnswindex.DeviceBackend.span_prefilter_stats)


def test_the_launcher_is_instantiated_per_metric():
    assert "template hipError_t span_pf_launch<kUnitMetric>(" in (ROOT / "hnswindex.net_amd" / "csrc" / "exact_unit.hip").read_text()
