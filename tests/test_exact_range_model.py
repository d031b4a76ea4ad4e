"""CPU tier: the reference of the exact range call (tests/exact_range_model.py) keeps what the contract says -- d <= radius as the
IEEE float compare, then (distance, id) ascending -- and the surfaces of the call exist: header, exports, INTEGRATION.md, bindings,
with hnswdev_stats left as it was."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from exact_knn_model import stored
from exact_range_model import exact_range, within

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("hnsw_mi355x_exact_range_query", "hnsw_mi355x_exact_range_info", "hnswdev_exact_range", "hnswdev_exact_range_results",
           "hnswdev_exact_range_info")


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "ucosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_the_model_is_the_brute_force_loop(metric):
    import oracle
    rng = np.random.default_rng(4)
    x = rng.integers(1, 4, (50, 8)).astype(np.float32)   # grid data: equal distances abound
    q = rng.integers(1, 4, (5, 8)).astype(np.float32)
    mask = rng.random(50) < 0.7
    live = np.setdiff1d(np.arange(50), rng.choice(50, 8, replace=False))
    base, rows = stored(metric, x)
    every = np.arange(50, dtype=np.int32)
    d_all = np.stack([oracle.dist_query_rows(base, rows, q[i], every) for i in range(5)])
    radius = float(np.sort(d_all[0])[20])                # a value the data holds: the pairs on the boundary are in
    ids, d = exact_range(metric, x, q, radius, mask=mask, live=live)
    sizes = []
    for i in range(5):
        want = []
        for c in range(50):
            if c in live and mask[c] and d_all[i, c] <= np.float32(radius):
                want.append((float(d_all[i, c]), c))
        want.sort()
        assert ids[i].dtype == np.int32 and d[i].dtype == np.float32
        assert list(zip(d[i].tolist(), ids[i].tolist())) == want, (metric, i)
        assert d[i].tobytes() == d_all[i, ids[i]].tobytes()
        sizes.append(len(want))
    assert max(sizes) >= 2                               # something was ordered
    assert any(np.any(d[i][1:] == d[i][:-1]) for i in range(5))   # ... among equal distances too


def test_radii_that_are_no_ordinary_numbers():
    d = np.array([0.0, -0.0, 1.0, np.inf, np.nan, -1.0, -np.inf, 2.0], np.float32)
    ids = np.array([7, 3, 5, 1, 0, 6, 2, 4], np.int32)
    assert within(d, ids, np.nan)[0].size == 0
    i, v = within(d, ids, np.inf)                        # every number, +inf included; the NaN never
    assert i.tolist() == [2, 6, 3, 7, 5, 4, 1] and v.tolist() == [-np.inf, -1.0, 0.0, 0.0, 1.0, 2.0, np.inf]
    assert not np.signbit(v[2:4]).any()                  # -0 is returned as +0 (and ties with +0 by id)
    i, v = within(d, ids, -0.0)                          # -0.0 admits distance 0
    assert i.tolist() == [2, 6, 3, 7] and v.tobytes() == np.array([-np.inf, -1.0, 0.0, 0.0], np.float32).tobytes()
    assert within(d, ids, -np.inf)[0].tolist() == [2]
    assert within(d, ids, -0.5)[0].tolist() == [2, 6]    # a negative radius is an ordinary one
    assert within(d, ids, np.nextafter(np.float32(1.0), np.float32(0.0)))[0].tolist() == [2, 6, 3, 7]
    e = within(np.zeros(0, np.float32), np.zeros(0, np.int32), 1.0)
    assert e[0].size == 0 and e[0].dtype == np.int32 and e[1].dtype == np.float32


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
    for cls, names in ((net.Index, ("exact_range_query", "exact_range_info")), (net.DeviceBackend, ("exact_range", "exact_range_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    # hnswdev_stats did not change: the range form's own counters go through hnswdev_exact_range_info
    assert ct.sizeof(net.DeviceStats) == ct.sizeof(net.Stats) + 40
    assert net.DeviceStats.field_names()[-5:] == ["exact_launches", "exact_evals", "exact_timed_launches", "exact_timed_evals", "exact_kernel_ms"]
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    assert list(net.Index(4, "sq_euclid").exact_range_info()) == ["device_sorted", "host_sorted", "repeated_rounds", "results"]


def test_null_handle_returns_what_the_filtered_range_call_returns():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), np.float32)
    bits = np.ones(1, np.uint32)
    marker = 0x1234
    pp_i, pp_d = (ct.c_void_p * 2)(marker, marker), (ct.c_void_p * 2)(marker, marker)
    counts = np.full(2, 7, np.int32)
    args = (v.ctypes.data_as(F), 2, 4, ct.c_float(1.0), bits.ctypes.data_as(U), 32, pp_i, pp_d, counts.ctypes.data_as(I))
    assert lib.hnsw_mi355x_exact_range_query(None, *args) == lib.hnsw_mi355x_range_query_filtered(None, *args) == 0
    assert list(pp_i) == [marker] * 2 and list(pp_d) == [marker] * 2 and (counts == 7).all()     # nothing written
    out = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_exact_range_info(None, out) == -1 and list(out) == [9] * 4
    assert lib.hnswdev_exact_range(None, v.ctypes.data_as(F), 2, 10, ct.c_float(1.0), None, 0, counts.ctypes.data_as(I)) == -1
    assert lib.hnswdev_exact_range_results(None, None, None) == -1 and lib.hnswdev_exact_range_info(None, out) == -1
    assert (counts == 7).all()
