"""CPU tier: the surfaces of the mutual reachability tree -- the header's declarations against the stated signatures,
the exported symbols and their ctypes argtypes, the bindings' methods, an empty index, and the conventions of a NULL handle and a NULL
context.  (cap, NULL outputs and nbits < 0 need an index with items: the GPU tier.)"""
import ctypes as ct

import numpy as np

from test_span_tree_abi import F, I, ROOT, U, U64, _net

LL = ct.c_longlong
STATED = {
    "hnsw_mi355x_mutual_reachability_tree": [ct.c_void_p, ct.c_int, U, LL, I, I, F, LL, F, LL, U64],
    "hnswdev_exact_mreach_tree": [ct.c_void_p, LL, ct.c_int, U, LL, I, I, F, LL, F, LL, U64],
}
TAIL = ("int min_samples, const uint32_t *allow_words, long long nbits, int *out_a, int *out_b, float *out_dist, long long cap, float *out_core, "
        "long long core_len, uint64_t out_info[8]);")
DECLARED = {"hnsw_mi355x_mutual_reachability_tree": "(void *handle, " + TAIL, "hnswdev_exact_mreach_tree": "(void *ctx, long long n_rows, " + TAIL}
INFO = ("members", "edges", "components", "rounds", "pairs_measured", "pairs_skipped", "launches", "core_launches")


def test_symbols_exist_with_the_stated_argtypes():
    net = _net()
    guide = (ROOT / "INTEGRATION.md").read_text()
    header = " ".join((ROOT / "include" / "hnsw_mi355x.h").read_text().split())
    for sym, stated in STATED.items():
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int and list(fn.argtypes) == stated, sym
        assert "int " + sym + DECLARED[sym] in header and sym in guide, sym
    assert "template hipError_t mreach_scan_launch<kUnitMetric>(" in (ROOT / "hnswindex.net_amd" / "csrc" / "exact_unit.hip").read_text()


def test_bindings_have_the_methods_and_an_empty_index_has_no_edge():
    net = _net()
    assert callable(net.Index.mutual_reachability_tree) and callable(net.DeviceBackend.exact_mreach_tree)
    ix = net.Index(4, "sq_euclid")                                        # nothing added: no live id, no member
    a, b, d, core, info = ix.mutual_reachability_tree(5)
    assert a.shape == b.shape == d.shape == core.shape == (0,) and a.dtype == b.dtype == np.int32 and d.dtype == core.dtype == np.float32
    assert info == dict.fromkeys(INFO, 0) and tuple(info) == INFO
    assert ix.single_linkage_cut((a, b, d, info), 1.0).shape == (0,)


def test_null_handle_and_null_context():
    lib = _net().lib
    a, b, d, core, info = np.full(3, 7, np.int32), np.full(3, 7, np.int32), np.full(3, 7, np.float32), np.full(4, 7, np.float32), (ct.c_uint64 * 8)()
    ptrs = (a.ctypes.data_as(I), b.ctypes.data_as(I), d.ctypes.data_as(F))
    for cap in (3, 0, -5):                                                # a NULL handle: 0, out_info zeroed, nothing else looked at
        info[:] = [9] * 8
        assert lib.hnsw_mi355x_mutual_reachability_tree(None, 0, None, 0, *ptrs, cap, core.ctypes.data_as(F), cap, info) == 0
        assert list(info) == [0] * 8
    assert lib.hnsw_mi355x_mutual_reachability_tree(None, 5, None, -1, None, None, None, 0, None, 0, None) == 0
    info[:] = [9] * 8                                                     # a NULL context: -1, nothing written
    assert lib.hnswdev_exact_mreach_tree(None, 4, 5, None, 0, *ptrs, 3, core.ctypes.data_as(F), 4, info) == -1
    assert (a == 7).all() and (b == 7).all() and (d == 7).all() and (core == 7).all() and list(info) == [9] * 8
