"""CPU tier (one case with a live handle on the GPU tier, at the end): the surface of the 8-bit row prefilter -- the two new exports with their ctypes signatures, declared in
the header and named in INTEGRATION.md, the bindings' methods, and the argument errors: -1 with a message."""
import ctypes as ct
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
U64, U8 = ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_uint8)
STATED = {
    "hnsw_mi355x_row_prefilter8_stats": [ct.c_void_p, U64],
    "hnsw_mi355x_row_prefilter8_peek": [ct.c_void_p, ct.c_int, ct.c_int, U64, U8],
}
FIELDS = ("launches", "rows_packed", "rows_on_shadow", "rows_reread", "full_packs", "fallbacks_to_f16")


def _net():
    import hnswindex
    return importlib.import_module(hnswindex.net_amd.Index.__module__)


def test_the_two_symbols_exist_and_are_declared_and_documented():
    net = _net()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)
    guide = (ROOT / "INTEGRATION.md").read_text()
    for sym, want in STATED.items():
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int and list(fn.argtypes) == want, sym
        assert re.search(r"\bint\s+" + sym + r"\s*\(", header), sym
        assert sym in guide, sym
    assert "uint64_t out[6]" in header and "uint64_t out[4], uint8_t *codes" in header


def test_argument_errors_return_minus_one_with_a_message():
    net = _net()
    lib = net.lib
    out, codes = (ct.c_uint64 * 6)(9, 9, 9, 9, 9, 9), np.full(128, 7, np.uint8)
    assert lib.hnsw_mi355x_row_prefilter8_stats(None, out) == -1
    assert "hnsw_mi355x_row_prefilter8_stats" in net.last_error() and list(out) == [9] * 6
    assert lib.hnsw_mi355x_row_prefilter8_peek(None, 0, 1, out, codes.ctypes.data_as(U8)) == -1
    assert "hnsw_mi355x_row_prefilter8_peek" in net.last_error() and (codes == 7).all()


def test_the_bindings_answer_without_an_index_behind_them():
    net = _net()
    ix = net.Index(128, "sq_euclid")                                     # nothing added: no shadow of either width
    assert callable(net.Index.row_prefilter8_stats) and callable(net.Index.row_prefilter8_peek)
    assert ix.row_prefilter8_stats() == dict.fromkeys(FIELDS, 0)
    peek = ix.row_prefilter8_peek()
    assert peek["packed"] == 0 and peek["codes"].shape == (0, 128) and peek["codes"].dtype == np.uint8
    with pytest.raises(RuntimeError, match="8-bit shadow rows"):
        ix.row_prefilter8_peek(0, 1)
    assert ix.row_prefilter_form_stats() == {"runtime_dim": 0, "fixed_dim": 0}       # unchanged: the 8-bit form is neither slot


def test_the_form_and_the_mode_are_where_the_design_says():
    csrc = ROOT / "hnswindex.net_amd" / "csrc"
    assert "kFormLeanPF8Fixed = 5" in (csrc / "dk_base.h").read_text()
    units = (csrc / "device_kernels.h").read_text()
    for ns, hashed in ((2, "false"), (4, "false"), (2, "true"), (4, "true")):
        assert f"X(M, {ns}, {hashed}, kFormLeanPF8Fixed)" in units
    assert "3 = the 8-bit form" in (csrc / "diag.h").read_text()


@pytest.mark.gpu
def test_a_live_index_without_a_shadow_reports_zeros_and_checks_its_arguments():
    """(hnsw_create needs a device: the cases with a live handle run on the GPU tier)"""
    net = _net()
    lib = net.lib
    ix = net.Index(128, "sq_euclid")
    ix._initialize()
    out = (ct.c_uint64 * 6)(9, 9, 9, 9, 9, 9)
    assert lib.hnsw_mi355x_row_prefilter8_stats(ix._h, None) == -1 and "hnsw_mi355x_row_prefilter8_stats" in net.last_error()
    assert lib.hnsw_mi355x_row_prefilter8_peek(ix._h, 0, 0, None, None) == -1 and "hnsw_mi355x_row_prefilter8_peek" in net.last_error()
    assert lib.hnsw_mi355x_row_prefilter8_peek(ix._h, 0, 1, out, None) == -1 and "hnsw_mi355x_row_prefilter8_peek" in net.last_error()
    assert net.lib.hnsw_mi355x_row_prefilter8_stats(ix._h, out) == 0 and list(out) == [0] * 6
    peek = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert net.lib.hnsw_mi355x_row_prefilter8_peek(ix._h, 0, 0, peek, None) == 0 and list(peek) == [0] * 4
    assert net.lib.hnsw_mi355x_row_prefilter8_peek(ix._h, 0, 2, peek, np.zeros(256, np.uint8).ctypes.data_as(U8)) == -1
    assert "no 8-bit shadow rows" in net.last_error()
