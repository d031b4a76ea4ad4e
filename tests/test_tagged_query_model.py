"""CPU tier: the tagged calls (include/hnsw_mi355x.h hnsw_mi355x_knn_query_tagged / hnsw_mi355x_exact_knn_query_tagged) -- their
surfaces (header, exports, INTEGRATION.md, bindings and their ctypes signatures, the NULL-handle conventions of the filtered call,
argument errors raised before anything native runs), where the list builder is compiled, and the plain-Python statement of the
contract (tests/tagged_query_model.py) pinned to the oracle on one graph, for both modes."""
import ctypes as ct
import importlib
import importlib.util
import re
from pathlib import Path

import numpy as np
import pytest

from common import uniform
from filtered_model import filtered_knn_batch
from tagged_query_model import tag_mask, tagged_knn_batch

ROOT = Path(__file__).resolve().parent.parent
OUTER = ("hnsw_mi355x_knn_query_tagged", "hnsw_mi355x_exact_knn_query_tagged", "hnsw_mi355x_knn_tagged_info", "hnsw_mi355x_exact_tagged_info")
INNER = ("hnswdev_knn_search_tagged", "hnswdev_exact_knn_tagged", "hnswdev_knn_tagged_info", "hnswdev_exact_tagged_info", "hnswdev_tag_list_ms")
SYMBOLS = OUTER + INNER
C_TYPES = {"void *": ct.c_void_p, "float *": ct.POINTER(ct.c_float), "int *": ct.POINTER(ct.c_int), "uint32_t *": ct.POINTER(ct.c_uint32),
           "double *": ct.POINTER(ct.c_double), "uint64_t []": ct.POINTER(ct.c_uint64), "int": ct.c_int, "long long": ct.c_longlong}


def _header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "hnsw_mi355x.h").read_text(), flags=re.S)


def _net():
    import hnswindex
    return importlib.import_module(hnswindex.net_amd.Index.__module__)


def _declared(sym):
    """The ctypes argument types the header's declaration of `sym` asks for."""
    params = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\)\s*;", _header(), flags=re.S).group(1)
    out = []
    for p in params.split(","):
        p = re.sub(r"\bconst\b", "", " ".join(p.split())).strip()
        m = re.fullmatch(r"(.*?)(\w+)(\[\d+\])?", p)          # type, name, array bound
        ctype = m.group(1).strip() + (" []" if m.group(3) else "")
        out.append(C_TYPES[re.sub(r"\s*\*", " *", ctype)])
    return out


def test_header_declares_the_entry_points_the_library_exports_them_and_the_guide_names_them():
    net = _net()
    text = _header()
    guide = (ROOT / "INTEGRATION.md").read_text()
    section4 = guide[guide.index("## 4."):]
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", text), sym
        assert hasattr(net.lib, sym), sym
        assert sym in section4, sym
    front = guide[:guide.index("## 4.")]
    for sym in ("hnsw_mi355x_knn_query_tagged", "hnsw_mi355x_exact_knn_query_tagged", "hnswdev_knn_search_tagged", "hnswdev_exact_knn_tagged"):
        assert "partial int " + sym + "(" in front, sym                    # the P/Invoke lines, beside the grouped ones
    assert "hnsw_mi355x_knn_query_tagged(handle" in front and "hnsw_mi355x_exact_knn_query_tagged(handle" in front
    assert not re.search(r"HNSWDEV_[A-Z0-9_]*(ANY|ALL)\s*=", text)          # the mode is a plain int: no enum constant


def test_ctypes_signatures_are_the_header_s():
    net = _net()
    for sym in SYMBOLS:
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int, sym
        assert list(fn.argtypes) == _declared(sym), sym


def test_bindings_have_the_methods_and_hnswdev_stats_is_what_it_was():
    net = _net()
    for cls, names in ((net.Index, ("knn_query_tagged", "exact_knn_query_tagged", "knn_tagged_info", "exact_tagged_info")),
                       (net.DeviceBackend, ("knn_search_tagged", "exact_knn_tagged", "knn_tagged_info", "exact_tagged_info", "tag_list_ms"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    assert net.DeviceStats.field_names()[-1] == "exact_kernel_ms"            # nothing appended: the calls' counters have their own entry points
    ix = net.Index(4, "sq_euclid")
    assert ix.knn_tagged_info() == {"calls": 0, "masks": 0, "launched": 0, "skipped": 0, "handbacks": 0}
    assert ix.exact_tagged_info() == {"calls": 0, "masks": 0, "scanned": 0, "skipped": 0, "ids_listed": 0, "batches": 0}
    # an index nothing was added to: padding in knn_query's shape, either mode, any layer
    for match in ("any", "all"):
        for call in (lambda: ix.knn_query_tagged(np.zeros((3, 4), np.float32), 2, np.ones(5, np.uint32), [1, 0x80000000, 0], match, layer=3),
                     lambda: ix.exact_knn_query_tagged(np.zeros((3, 4), np.float32), 2, np.ones(5, np.uint32), [1, 0x80000000, 0], match)):
            ids, d = call()
            assert ids.shape == d.shape == (3, 2) and ids.dtype == np.int32 and d.dtype == np.float32
            assert (ids == -1).all() and np.isnan(d).all()


def test_argument_errors_are_raised_before_any_native_call(monkeypatch):
    net = _net()

    def native(*a):
        raise AssertionError("the native call ran")
    monkeypatch.setattr(net.lib, "hnsw_mi355x_knn_query_tagged", native)
    monkeypatch.setattr(net.lib, "hnsw_mi355x_exact_knn_query_tagged", native)
    ix = net.Index(4, "sq_euclid")
    q3, tags = np.zeros((3, 4), np.float32), np.ones(5, np.uint32)
    for call in (ix.knn_query_tagged, ix.exact_knn_query_tagged):
        with pytest.raises(ValueError, match="query_tags has 2 entries for 3 queries"):
            call(q3, 2, tags, [1, 1])
        with pytest.raises(ValueError, match="query_tags has 4 entries for 1 queries"):
            call(np.zeros(4, np.float32), 2, tags, [1, 1, 1, 1])
        with pytest.raises(ValueError, match="expected dim=4"):
            call(np.zeros((3, 5), np.float32), 2, tags, [1, 1, 1])
        with pytest.raises(ValueError, match="match = 'some' is neither 'any' nor 'all'"):
            call(q3, 2, tags, [1, 1, 1], "some")
        with pytest.raises(ValueError, match="query_tags holds a value outside 0 .. 2\\^32 - 1"):
            call(q3, 2, tags, [1, -1, 1])
        with pytest.raises(ValueError, match="row_tags holds a value outside 0 .. 2\\^32 - 1"):
            call(q3, 2, [1 << 32], [1, 1, 1])
        with pytest.raises(ValueError, match="row_tags must hold integers"):
            call(q3, 2, [0.5, 1.0], [1, 1, 1])
        with pytest.raises(ValueError, match="query_tags holds 65537 distinct masks, more than 65536"):
            call(np.zeros((65537, 4), np.float32), 2, tags, np.arange(65537))
        with pytest.raises(AssertionError, match="the native call ran"):       # (the stand-in is what a well-formed call reaches)
            call(q3, 2, tags, [1, 0xFFFFFFFF, 0])


def test_null_handle_returns_what_the_filtered_calls_return():
    net = _net()
    lib = net.lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), np.float32)
    rt, qt, w = np.ones(8, np.uint32), np.ones(2, np.uint32), np.ones(1, np.uint32)
    ids, d, flags = np.full((2, 3), 7, np.int32), np.full((2, 3), 7.0, np.float32), np.full(2, 7, np.int32)
    out_args = (ids.ctypes.data_as(I), d.ctypes.data_as(F))
    tagged = (rt.ctypes.data_as(U), 8, qt.ctypes.data_as(U), 0)
    # a NULL handle: 0 and nothing written, as hnsw_mi355x_knn_query_filtered / _at_layer / hnsw_mi355x_exact_knn_query
    assert lib.hnsw_mi355x_knn_query_tagged(None, v.ctypes.data_as(F), 2, 4, 3, 0, *tagged, *out_args) == \
        lib.hnsw_mi355x_knn_query_filtered(None, v.ctypes.data_as(F), 2, 4, 3, w.ctypes.data_as(U), 32, *out_args) == \
        lib.hnsw_mi355x_knn_query_at_layer(None, v.ctypes.data_as(F), 2, 4, 3, 1, w.ctypes.data_as(U), 32, *out_args) == 0
    assert lib.hnsw_mi355x_exact_knn_query_tagged(None, v.ctypes.data_as(F), 2, 4, 3, *tagged, *out_args) == \
        lib.hnsw_mi355x_exact_knn_query(None, v.ctypes.data_as(F), 2, 4, 3, w.ctypes.data_as(U), 32, *out_args) == 0
    assert (ids == 7).all() and (d == 7.0).all()
    out = (ct.c_uint64 * 6)(*[9] * 6)
    assert lib.hnsw_mi355x_knn_tagged_info(None, out) == lib.hnsw_mi355x_exact_tagged_info(None, out) == lib.hnsw_mi355x_knn_grouped_info(None, out) == -1
    assert list(out) == [9] * 6
    # a NULL context: -1, as hnswdev_knn_search_filtered
    assert lib.hnswdev_knn_search_tagged(None, v.ctypes.data_as(F), 2, 0, 3, 3, 0, *tagged, *out_args, flags.ctypes.data_as(I)) == \
        lib.hnswdev_knn_search_filtered(None, v.ctypes.data_as(F), 2, 0, 3, 3, w.ctypes.data_as(U), 32, *out_args, flags.ctypes.data_as(I)) == -1
    assert lib.hnswdev_exact_knn_tagged(None, v.ctypes.data_as(F), 2, 8, 3, *tagged, *out_args) == -1
    ms = ct.c_double(9.0)
    assert lib.hnswdev_knn_tagged_info(None, out) == lib.hnswdev_exact_tagged_info(None, out) == lib.hnswdev_tag_list_ms(None, ct.byref(ms)) == -1
    assert list(out) == [9] * 6 and ms.value == 9.0
    assert (ids == 7).all() and (d == 7.0).all() and (flags == 7).all()


def test_the_list_builder_is_compiled_in_the_host_unit_alone():
    """dk_tag_lists.h has no metric: device_backend.hip includes it, as it includes dk_graph_info.h; no unit table, unit source or
    umbrella header names it, so no per-metric unit carries its kernels."""
    spec = importlib.util.spec_from_file_location("hnsw_build_for_tags", ROOT / "hnswindex.net_amd" / "build.py")
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    csrc = ROOT / "hnswindex.net_amd" / "csrc"
    assert (csrc / "dk_tag_lists.h").is_file()
    assert "dk_tag_lists" not in (ROOT / "hnswindex.net_amd" / "build.py").read_text()
    assert all("tag" not in src for _, src, _ in build.units())
    including = sorted(f.name for f in csrc.iterdir() if f.is_file() and f.name != "dk_tag_lists.h" and '#include "dk_tag_lists.h"' in f.read_text())
    assert including == ["device_backend.hip"]
    for name in ("kernel_unit.hip", "exact_unit.hip", "device_kernels.h", "dk_exact.h"):
        assert "dk_tag_lists" not in (csrc / name).read_text(), name
    # ... while the traversal kernel is instantiated where the grouped one is: in the units of the `filtered` kind
    unit = re.search(r"#define HNSW_UNIT_filtered\(DO, M\)(.*)", (csrc / "device_kernels.h").read_text()).group(1)
    assert "HNSW_##DO##_FILTERED" in unit and "HNSW_##DO##_GROUPED" in unit and "HNSW_##DO##_TAGGED" in unit


def test_tag_mask_is_the_predicate():
    rt = np.array([0, 1, 2, 3, 0x80000000, 0x80000001, 0xFFFFFFFF, 5], np.uint32)
    assert tag_mask(rt, 1, "any", 10).tolist() == [False, True, False, True, False, True, True, True, False, False]      # ids 8, 9: past the array
    assert tag_mask(rt, 3, "any", 8).tolist() == [False, True, True, True, False, True, True, True]
    assert tag_mask(rt, 3, "all", 8).tolist() == [False, False, False, True, False, False, True, False]
    assert tag_mask(rt, 0x80000000, "any", 8).tolist() == [False, False, False, False, True, True, True, False]           # bit 31 is a tag like the others
    assert tag_mask(rt, 0x80000001, "all", 8).tolist() == [False, False, False, False, False, True, True, False]
    assert tag_mask(rt, 0xFFFFFFFF, "all", 8).tolist() == [False] * 6 + [True, False]
    assert tag_mask(rt, 0xFFFFFFFF, "any", 8).tolist() == [False] + [True] * 7
    for match in ("any", "all"):
        assert not tag_mask(rt, 0, match, 8).any()                                                                      # the mask 0 has no candidate
        assert not tag_mask(rt, 1 << 4, match, 8)[:6].any()
        assert (tag_mask(rt, 4, match, 8) == tag_mask(rt.astype(np.int64), 4, match, 8)).all()
    with pytest.raises(ValueError):
        tag_mask(rt, 1, "some", 8)


@pytest.fixture(scope="module")
def graph():
    import oracle
    n, dim, min_nn = 400, 8, 12
    x = uniform(n, dim, 11)
    ix = oracle.OracleIndex(dim, "sq_euclid", max_edges=6, min_nn=min_nn, max_candidates=20, collection_size=n)
    ix.add(x)
    return ix, x, min_nn


def test_the_model_is_the_oracle_on_one_graph(graph):
    """Every id tagged with the bit every query asks for: OracleIndex.knn_query bit for bit, in both modes.  A tag on 6 ids: brute
    force over its rows (layer 0 is connected here, and the result heap never fills).  Every result matches its query's mask."""
    import oracle
    ix, x, min_nn = graph
    n = x.shape[0]
    q = uniform(14, 8, 12)
    for match in ("any", "all"):
        for k in (5, 20):
            want = ix.knn_query(q, k)
            got = tagged_knn_batch(ix, x, "sq_euclid", q, k, min_nn, np.full(n + 50, 0x80000004, np.uint32), np.full(14, 0x80000000, np.uint32), match)
            assert (got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes(), (match, k)
    rng = np.random.default_rng(5)
    row_tags = ((rng.random(n) < 0.6) * 1 + (rng.random(n) < 0.3) * 2 + (rng.random(n) < 0.1) * 4).astype(np.uint32)
    small = rng.choice(n, 6, replace=False)
    row_tags[small] |= 8
    row_tags[rng.choice(np.setdiff1d(np.arange(n), small), 20, replace=False)] = 0
    masks = np.array([1, 2, 4, 8, 16, 3, 5, 0], np.uint32)                 # 16: no row carries it; 0: no candidate by definition
    query_tags = masks[rng.permutation(np.arange(14) % masks.size)]
    for match in ("any", "all"):
        ids, d = tagged_knn_batch(ix, x, "sq_euclid", q, 4, min_nn, row_tags, query_tags, match)
        for i in range(14):
            got = ids[i][ids[i] >= 0]
            hit = row_tags[got] & query_tags[i]
            assert (hit != 0).all() if match == "any" else (hit == query_tags[i]).all(), (match, i)
        none = (query_tags == 16) | (query_tags == 0)
        assert (ids[none] == -1).all() and np.isnan(d[none]).all()
        srt = np.sort(small)
        for i in np.flatnonzero(query_tags == 8):
            bd = oracle.dist_query_rows("sq_euclid", x, q[i], srt)
            order = np.argsort(bd, kind="stable")[:4]
            assert ids[i].tolist() == srt[order].tolist() and d[i].tobytes() == bd[order].astype(np.float32).tobytes()
    any_rows = tagged_knn_batch(ix, x, "sq_euclid", q, 4, min_nn, row_tags, query_tags, "any")
    all_rows = tagged_knn_batch(ix, x, "sq_euclid", q, 4, min_nn, row_tags, query_tags, "all")
    single = np.isin(query_tags, [1, 2, 4, 8])
    assert (any_rows[0][single] == all_rows[0][single]).all()              # one bit: the modes agree
    assert (any_rows[0][~single] != all_rows[0][~single]).any()            # 3 and 5: they do not


def test_the_model_is_the_filtered_model_per_mask_with_rows_scattered_back(graph):
    ix, x, min_nn = graph
    n = x.shape[0]
    rng = np.random.default_rng(6)
    q = uniform(12, 8, 13)
    row_tags = rng.integers(0, 8, n - 100).astype(np.uint32)               # shorter than the rows: ids past its end carry no tag
    row_tags[::7] |= 0x80000000
    query_tags = rng.choice(np.array([1, 6, 0x80000001], np.uint32), 12)
    for match in ("any", "all"):
        ids, d = tagged_knn_batch(ix, x, "sq_euclid", q, 5, min_nn, row_tags, query_tags, match)
        for m in np.unique(query_tags):
            sel = query_tags == m
            hit = row_tags.astype(np.int64) & int(m)
            mask = np.zeros(n, dtype=bool)
            mask[:n - 100] = hit != 0 if match == "any" else hit == int(m)
            assert (tag_mask(row_tags, m, match, n) == mask).all()
            w_ids, w_d = filtered_knn_batch(ix, x, "sq_euclid", q[sel], 5, min_nn, mask)
            assert (ids[sel] == w_ids).all() and d[sel].tobytes() == w_d.tobytes()
        assert ids.max() < n - 100
    with pytest.raises(ValueError):
        tagged_knn_batch(ix, x, "sq_euclid", q, 5, min_nn, row_tags, query_tags[:5])
    with pytest.raises(ValueError):
        tagged_knn_batch(ix, x, "sq_euclid", q, 5, min_nn, row_tags, query_tags, "none")
