"""CPU tier: the reference of the grouped exact range call (tests/exact_range_grouped_model.py) on hand-made cases -- an empty group, a
one-row group, scrambled query order, the radii with a rule of their own -- and the surfaces of the call: header, exports,
INTEGRATION.md, bindings, argument errors, with hnswdev_stats left as it was and the NULL-handle conventions of the ungrouped call."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from exact_knn_model import distances, stored
from exact_range_grouped_model import exact_range_grouped, from_matrix
from exact_range_model import exact_range

ROOT = Path(__file__).resolve().parent.parent
SYMBOLS = ("hnsw_mi355x_exact_range_query_grouped", "hnsw_mi355x_exact_range_grouped_info", "hnswdev_exact_range_grouped",
           "hnswdev_exact_range_grouped_info")
INFO = {"calls": 0, "device_sorted": 0, "host_sorted": 0, "repeated_pieces": 0}


def _case():
    rng = np.random.default_rng(5)
    n = 50
    x = rng.integers(1, 4, (n, 8)).astype(np.float32)   # grid data: equal distances abound
    q = rng.integers(1, 4, (9, 8)).astype(np.float32)
    row_group = (np.arange(n) % 4).astype(np.int32)
    row_group[row_group == 3] = 0
    row_group[11] = 3                                   # group 3 has one member, group 4 none
    row_group[[0, 1]] = [-1, 7]                         # in no group
    query_group = np.array([4, 2, 0, 3, 1, 0, 4, 3, 2], np.int32)   # scrambled, the empty group named twice
    live = np.setdiff1d(np.arange(n), [5, 6, 20])
    return x, q, row_group, query_group, 5, live


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_the_model_is_the_brute_force_loop(metric):
    import oracle
    x, q, row_group, query_group, n_groups, live = _case()
    base, rows = stored(metric, x)
    dist = lambda i, c: np.float32(oracle.dist_query_rows(base, rows, q[i], np.array([c], np.int32))[0])   # noqa: E731
    all_d = np.sort(np.array([dist(i, c) for i in range(9) for c in live], np.float32))
    ties = 0
    for radius in (float(all_d[all_d.size // 3]), float("inf"), float("nan"), -0.0, float(np.nextafter(all_d[0], np.float32(-np.inf)))):
        ids, d = exact_range_grouped(metric, x, q, radius, row_group, query_group, n_groups, live=live)
        assert len(ids) == len(d) == 9
        for i in range(9):
            want = sorted((float(dist(i, c)), int(c)) for c in live if row_group[c] == query_group[i] and dist(i, c) <= np.float32(radius))
            ties += any(a[0] == b[0] for a, b in zip(want, want[1:]))
            assert ids[i].dtype == np.int32 and d[i].dtype == np.float32
            assert ids[i].tolist() == [c for _, c in want], (metric, radius, i)
            assert d[i].tobytes() == np.array([v for v, _ in want], np.float32).tobytes(), (metric, radius, i)
        assert ids[0].size == ids[6].size == 0                              # the empty group
        if radius == float("inf"):
            assert ids[3].tolist() == ids[7].tolist() == [11]               # the one-row group
            assert sum(a.size for a in ids) == sum(int((row_group[live] == g).sum()) for g in query_group)
        if radius != radius or radius < all_d[0]:
            assert sum(a.size for a in ids) == 0
    assert ties >= 1                                                        # the id order decided something


def test_the_model_is_the_ungrouped_model_per_group():
    rng = np.random.default_rng(6)
    x, q = rng.random((60, 8), dtype=np.float32), rng.random((11, 8), dtype=np.float32)
    row_group = rng.integers(-1, 4, 60).astype(np.int32)
    query_group = rng.integers(0, 3, 11).astype(np.int32)
    ids, d = exact_range_grouped("sq_euclid", x, q, 0.9, row_group, query_group, 3)
    assert sum(a.size for a in ids) > 20
    for g in range(3):
        sel = np.flatnonzero(query_group == g)
        w_ids, w_d = exact_range("sq_euclid", x, q[sel], 0.9, mask=row_group == g)
        for j, i in enumerate(sel):
            assert ids[i].tolist() == w_ids[j].tolist() and d[i].tobytes() == w_d[j].tobytes()
    assert not np.isin(np.concatenate(ids), np.flatnonzero(row_group == 3)).any()      # a value >= n_groups is in no group
    m_ids, m_d = from_matrix(distances("sq_euclid", x, q, np.arange(60, dtype=np.int32)), 0.9, row_group, query_group, 3)   # the same from a matrix
    assert all(a.tolist() == b.tolist() and c.tobytes() == e.tobytes() for a, b, c, e in zip(ids, m_ids, d, m_d))
    short, _ = exact_range_grouped("sq_euclid", x, q, float("inf"), row_group[:30], query_group, 3)   # ids past the array's end are in no group
    assert np.concatenate(short).max() < 30
    # negative radius on ucosine: an ordinary radius
    xn = x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    n_ids, n_d = exact_range_grouped("ucosine", xn, xn[:11], -1e-9, np.zeros(60, np.int32), np.zeros(11, np.int32), 1)
    assert all((v < 0).all() for v in n_d)


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
    for cls, names in ((net.Index, ("exact_range_query_grouped", "exact_range_grouped_info")), (net.DeviceBackend, ("exact_range_grouped", "exact_range_grouped_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    # hnswdev_stats did not change: the grouped call's own counters go through hnswdev_exact_range_grouped_info
    assert ct.sizeof(net.DeviceStats) == ct.sizeof(net.Stats) + 40
    assert net.DeviceStats.field_names()[-5:] == ["exact_launches", "exact_evals", "exact_timed_launches", "exact_timed_evals", "exact_kernel_ms"]
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    ix = net.Index(4, "sq_euclid")
    assert ix.exact_range_grouped_info() == INFO
    # an index nothing was added to: empty lists, and n_groups worked out from the arrays
    ids, d = ix.exact_range_query_grouped(np.zeros((3, 4), np.float32), 1.0, np.zeros(5, np.int32), [0, 0, 0])
    assert len(ids) == len(d) == 3 and all(a.size == 0 and a.dtype == np.int32 for a in ids) and all(a.size == 0 and a.dtype == np.float32 for a in d)
    with pytest.raises(ValueError, match="query_group"):
        ix.exact_range_query_grouped(np.zeros((3, 4), np.float32), 1.0, np.zeros(5, np.int32), [0, 0])


def test_null_handle_and_argument_errors():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    v = np.zeros((2, 4), np.float32)
    rg, qg = np.zeros(8, np.int32), np.zeros(2, np.int32)
    counts = np.full(2, 7, np.int32)
    pp_i, pp_d = (ct.c_void_p * 2)(0x1234, 0x1234), (ct.c_void_p * 2)(0x1234, 0x1234)
    grouped = (rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 1)
    out_args = (pp_i, pp_d, counts.ctypes.data_as(I))
    # a NULL handle: 0 and nothing written, as hnsw_mi355x_exact_range_query
    assert lib.hnsw_mi355x_exact_range_query_grouped(None, v.ctypes.data_as(F), 2, 4, ct.c_float(1.0), *grouped, *out_args) == \
        lib.hnsw_mi355x_exact_range_query(None, v.ctypes.data_as(F), 2, 4, ct.c_float(1.0), None, 0, *out_args) == 0
    assert (counts == 7).all() and list(pp_i) == [0x1234] * 2 and list(pp_d) == [0x1234] * 2
    out = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_exact_range_grouped_info(None, out) == -1 and list(out) == [9] * 4
    # a NULL context: -1, as hnswdev_exact_range
    assert lib.hnswdev_exact_range_grouped(None, v.ctypes.data_as(F), 2, 10, ct.c_float(1.0), *grouped, counts.ctypes.data_as(I)) == \
        lib.hnswdev_exact_range(None, v.ctypes.data_as(F), 2, 10, ct.c_float(1.0), None, 0, counts.ctypes.data_as(I)) == -1
    assert lib.hnswdev_exact_range_grouped_info(None, out) == -1 and list(out) == [9] * 4
    # the header states the argument errors of the call
    full = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    doc = full[full.index("hnsw_mi355x_exact_range_query with a candidate group per query"):full.index("int hnsw_mi355x_exact_range_query_grouped(")]
    for word in ("row_group NULL", "n_row_group < 0", "1 .. 65 536", "query_group value outside", "every out pointer NULL and every count 0"):
        assert word in doc, word
    if lib.hnswdev_device_count() <= 0:
        return   # (a handle needs a device; tests/test_gpu_exact_range_grouped.py makes the same calls on both layers)
    # a handle and bad group arguments: -1 with a message, every pointer NULL and every count 0
    h = lib.hnsw_create(b"sq_euclid")
    assert h
    bad = np.array([0, 3], np.int32)
    cases = (((rg.ctypes.data_as(I), 8, bad.ctypes.data_as(I), 3), r"query_group\[1\]"), ((None, 8, qg.ctypes.data_as(I), 1), "row_group"),
             ((rg.ctypes.data_as(I), -1, qg.ctypes.data_as(I), 1), "n_row_group"), ((rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 65537), "65536"),
             ((rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 0), "65536"))
    for args, word in cases:
        counts[:] = 7
        pp_i[0] = pp_i[1] = pp_d[0] = pp_d[1] = 0x1234
        assert lib.hnsw_mi355x_exact_range_query_grouped(h, v.ctypes.data_as(F), 2, 4, ct.c_float(1.0), *args, *out_args) == -1, word
        assert (counts == 0).all() and all(p is None for p in pp_i) and all(p is None for p in pp_d), word
        assert re.search(word, hnswindex.net_amd.last_error()), (word, hnswindex.net_amd.last_error())
    lib.hnsw_free(h)
