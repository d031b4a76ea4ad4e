"""CPU tier: the tagged range calls (hnsw_mi355x_range_query_tagged / hnsw_mi355x_exact_range_query_tagged) -- the
plain-Python statement of their contract (tests/tagged_range_model.py) held to the CPU oracle's unfiltered RangeQuery on 50-row
grids (every id tagged: equal lists; several masks: the same closure partitioned), to a brute-force loop for the scan and to the
empty-heap rule, in both modes -- and the surfaces of the calls: header, exports, ctypes signatures, INTEGRATION.md, bindings,
argument errors raised before anything native runs, the NULL-handle conventions of the grouped range exports, hnswdev_stats left
as it was."""
import ctypes as ct
import importlib
import re
from pathlib import Path

import numpy as np
import pytest

from exact_knn_model import stored
from tagged_range_model import HeapEmpty, exact_range_tagged, heap_empty_closed_form, tag_mask, tagged_range

ROOT = Path(__file__).resolve().parent.parent
OUTER = ("hnsw_mi355x_range_query_tagged", "hnsw_mi355x_exact_range_query_tagged", "hnsw_mi355x_range_tagged_info", "hnsw_mi355x_exact_range_tagged_info")
INNER = ("hnswdev_range_search_tagged", "hnswdev_exact_range_tagged", "hnswdev_range_tagged_info", "hnswdev_exact_range_tagged_info")
SYMBOLS = OUTER + INNER
RANGE_INFO = {"calls": 0, "masks": 0, "launched": 0, "skipped": 0, "host_finished": 0, "long_finished": 0}
EXACT_INFO = {"calls": 0, "masks": 0, "scanned": 0, "skipped": 0, "ids_listed": 0, "batches": 0, "device_sorted": 0, "host_sorted": 0, "repeated_pieces": 0}
C_TYPES = {"void *": ct.c_void_p, "void * *": ct.POINTER(ct.c_void_p), "float *": ct.POINTER(ct.c_float), "int *": ct.POINTER(ct.c_int),
           "uint32_t *": ct.POINTER(ct.c_uint32), "uint64_t []": ct.POINTER(ct.c_uint64), "int": ct.c_int, "long long": ct.c_longlong, "float": ct.c_float}
N, DIM, M = 50, 8, 4
MODES = ("any", "all")


def _oracle(metric, x):
    import oracle
    ref = oracle.OracleIndex(DIM, metric, max_edges=M, min_nn=6, collection_size=64)
    ref.add(x)
    return ref


def _case():
    rng = np.random.default_rng(5)
    x = rng.integers(1, 4, (N, DIM)).astype(np.float32)   # grid data: equal distances abound
    q = rng.integers(1, 4, (9, DIM)).astype(np.float32)
    row_tags = ((np.arange(N) % 2 == 0) * 1 + (np.arange(N) % 3 == 0) * 2 + (np.arange(N) % 5 == 0) * 0x80000000).astype(np.uint32)
    row_tags[11] |= 8                                     # the tag 8 is on one id, the tag 16 on none
    row_tags[[7, 13]] = 0                                 # no tag at all
    query_tags = np.array([16, 3, 1, 8, 0x80000002, 1, 0, 8, 0xFFFFFFFF], np.uint32)   # scrambled; a tag nobody carries, and the mask 0
    return x, q, row_tags, query_tags


@pytest.mark.parametrize("match", MODES)
def test_every_id_tagged_is_the_oracles_unfiltered_range_query(match):
    x, q, _, _ = _case()
    ref = _oracle("sq_euclid", x)
    for radius in (9.0, 16.0):
        ids, d = tagged_range(ref, x, "sq_euclid", q, radius, np.full(N, 0x80000004, np.uint32), np.full(9, 0x80000000, np.uint32), match)
        w_ids, w_d = ref.range_query(q, radius)
        assert sum(a.size for a in ids) > 9
        assert all(a.tolist() == b.tolist() and c.tobytes() == e.tobytes() for a, b, c, e in zip(ids, w_ids, d, w_d)), radius


@pytest.mark.parametrize("match", MODES)
def test_masks_partition_the_unfiltered_closure_and_come_back_in_query_order(match):
    x, q, row_tags, query_tags = _case()
    ref = _oracle("sq_euclid", x)
    radius = 9.0
    ids, d = tagged_range(ref, x, "sq_euclid", q, radius, row_tags, query_tags, match)
    full_ids, full_d = ref.range_query(q, radius)
    ties = 0
    for i in range(9):
        member = tag_mask(row_tags, int(query_tags[i]), match, N)[full_ids[i]]
        # radius >= 0: the closure does not depend on the filter, so the results are its members that match the mask ...
        assert sorted(ids[i].tolist()) == sorted(full_ids[i][member].tolist()), i
        # ... each with the distance the unfiltered call measured, ascending
        by_id = dict(zip(full_ids[i].tolist(), full_d[i].tolist()))
        assert d[i].tolist() == [by_id[j] for j in ids[i].tolist()] and (np.diff(d[i]) >= 0).all(), i
        ties += int((np.diff(d[i]) == 0).any())
        assert ids[i].dtype == np.int32 and d[i].dtype == np.float32
    assert ids[0].size == ids[6].size == 0 and ties >= 1                     # the tag nobody carries and the mask 0; equal distances among results
    assert set(ids[3].tolist()) <= {11} and set(ids[7].tolist()) <= {11}     # the one-row tag
    assert not np.isin(np.concatenate(ids), [7, 13]).any()                   # the word 0 matches nothing
    short, _ = tagged_range(ref, x, "sq_euclid", q, radius, row_tags[:20], query_tags, match)   # ids past the array's end too
    assert np.concatenate(short).max() < 20
    if match == "all":   # 0x80000002 asks for both tags: fewer ids than either
        both = tag_mask(row_tags, 0x80000002, "all", N)
        assert both.sum() < tag_mask(row_tags, 0x80000002, "any", N).sum() and set(ids[4].tolist()) <= set(np.flatnonzero(both).tolist())


@pytest.mark.parametrize("match", MODES)
@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_i8", "sq_euclid_f16"])
def test_the_scan_model_is_the_brute_force_loop(metric, match):
    import oracle
    x, q, row_tags, query_tags = _case()
    row_tags = row_tags[:N - 6]                                             # ids past row_tags carry no tag
    live = np.setdiff1d(np.arange(N), [5, 6, 20])                           # removed ids stay tagged and match nothing
    base, rows = stored(metric, x)
    dist = lambda i, c: np.float32(oracle.dist_query_rows(base, rows, q[i], np.array([c], np.int32))[0])   # noqa: E731
    word = lambda c: int(row_tags[c]) if c < row_tags.size else 0                                         # noqa: E731
    hit = lambda w, m: (w & m) != 0 if match == "any" else (m != 0 and (w & m) == m)                        # noqa: E731
    all_d = np.sort(np.array([dist(i, c) for i in range(9) for c in live], np.float32))
    ties = 0
    for radius in (float(all_d[all_d.size // 3]), float("inf"), float("nan"), -0.0, float(np.nextafter(all_d[0], np.float32(-np.inf)))):
        ids, d = exact_range_tagged(metric, x, q, radius, row_tags, query_tags, match, live=live)
        assert len(ids) == len(d) == 9
        for i in range(9):
            want = sorted((float(dist(i, c)), int(c)) for c in live if hit(word(c), int(query_tags[i])) and dist(i, c) <= np.float32(radius))
            ties += any(a[0] == b[0] for a, b in zip(want, want[1:]))
            assert ids[i].dtype == np.int32 and d[i].dtype == np.float32
            assert ids[i].tolist() == [c for _, c in want], (metric, radius, i)
            assert d[i].tobytes() == np.array([v for v, _ in want], np.float32).tobytes(), (metric, radius, i)
        assert ids[0].size == ids[6].size == 0                              # a tag on no row; the mask 0
        if radius == float("inf"):
            assert ids[3].tolist() == ids[7].tolist() == [11]               # the one-row tag
            assert 0 in ids[4].tolist() and 30 in ids[4].tolist()           # bit 31 is a tag like the others (ids 0 and 30 carry it)
            assert not np.isin(np.concatenate(ids), [5, 6, 20, 7, 13]).any() and np.concatenate(ids).max() < N - 6
    assert ties >= 1                                                        # the id order decided something


def test_heap_empty_propagates():
    rng = np.random.default_rng(21)
    x = rng.normal(size=(N, DIM)).astype(np.float32)       # unnormalised ucosine: 1 - dot goes negative
    q = rng.normal(size=(12, DIM)).astype(np.float32)
    ref = _oracle("ucosine", x)
    row_tags = (1 << (np.arange(N) % 3)).astype(np.uint32)
    query_tags = (1 << (np.arange(12) % 3)).astype(np.uint32)
    throws = [heap_empty_closed_form(ref, x, "ucosine", q[i], -1.0, tag_mask(row_tags, int(query_tags[i]), "any", N)) for i in range(12)]
    assert any(throws) and not all(throws)
    with pytest.raises(HeapEmpty):
        tagged_range(ref, x, "ucosine", q, -1.0, row_tags, query_tags)
    keep = np.flatnonzero(~np.array(throws))
    ids, _ = tagged_range(ref, x, "ucosine", q[keep], -1.0, row_tags, query_tags[keep])
    assert len(ids) == keep.size
    with pytest.raises(ValueError):
        tagged_range(ref, x, "ucosine", q, 1.0, row_tags, query_tags[:5])
    with pytest.raises(ValueError):
        tagged_range(ref, x, "ucosine", q, 1.0, row_tags, query_tags, "some")


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


def test_ctypes_signatures_are_the_header_s():
    net = _net()
    for sym in SYMBOLS:
        fn = getattr(net.lib, sym)
        assert fn.restype is ct.c_int, sym
        assert list(fn.argtypes) == _declared(sym), sym


def test_bindings_have_the_methods_the_info_dicts_are_zero_and_hnswdev_stats_is_what_it_was():
    net = _net()
    for cls, names in ((net.Index, ("range_query_tagged", "exact_range_query_tagged", "range_tagged_info", "exact_range_tagged_info")),
                       (net.DeviceBackend, ("range_search_tagged", "exact_range_tagged", "range_tagged_info", "exact_range_tagged_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    assert ct.sizeof(net.DeviceStats) == ct.sizeof(net.Stats) + 40              # sizeof(hnswdev_stats) unchanged
    body = re.search(r"typedef struct hnswdev_stats \{(.*?)\} hnswdev_stats;", _header(), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_0-9]+)\s*[,;]", body) == net.DeviceStats.field_names()
    assert net.DeviceStats.field_names()[-1] == "exact_kernel_ms"               # nothing appended: the calls' counters have their own entry points
    ix = net.Index(4, "sq_euclid")
    assert ix.range_tagged_info() == RANGE_INFO and ix.exact_range_tagged_info() == EXACT_INFO
    # an index nothing was added to: empty lists in range_query's shape, either mode, any layer
    for match in MODES:
        for call in (lambda: ix.range_query_tagged(np.zeros((3, 4), np.float32), 1.0, np.ones(5, np.uint32), [1, 0x80000000, 0], match, layer=3),
                     lambda: ix.exact_range_query_tagged(np.zeros((3, 4), np.float32), 1.0, np.ones(5, np.uint32), [1, 0x80000000, 0], match)):
            ids, d = call()
            assert len(ids) == len(d) == 3 and all(a.size == 0 and a.dtype == np.int32 for a in ids) and all(a.size == 0 and a.dtype == np.float32 for a in d)


def test_argument_errors_are_raised_before_any_native_call(monkeypatch):
    net = _net()

    def native(*a):
        raise AssertionError("the native call ran")
    monkeypatch.setattr(net.lib, "hnsw_mi355x_range_query_tagged", native)
    monkeypatch.setattr(net.lib, "hnsw_mi355x_exact_range_query_tagged", native)
    ix = net.Index(4, "sq_euclid")
    q3, tags = np.zeros((3, 4), np.float32), np.ones(5, np.uint32)
    for call in (ix.range_query_tagged, ix.exact_range_query_tagged):
        with pytest.raises(ValueError, match="query_tags has 2 entries for 3 queries"):
            call(q3, 1.0, tags, [1, 1])
        with pytest.raises(ValueError, match="query_tags has 4 entries for 1 queries"):
            call(np.zeros(4, np.float32), 1.0, tags, [1, 1, 1, 1])
        with pytest.raises(ValueError, match="expected dim=4"):
            call(np.zeros((3, 5), np.float32), 1.0, tags, [1, 1, 1])
        with pytest.raises(ValueError, match="match = 'some' is neither 'any' nor 'all'"):
            call(q3, 1.0, tags, [1, 1, 1], "some")
        with pytest.raises(ValueError, match="query_tags holds a value outside 0 .. 2\\^32 - 1"):
            call(q3, 1.0, tags, [1, -1, 1])
        with pytest.raises(ValueError, match="row_tags holds a value outside 0 .. 2\\^32 - 1"):
            call(q3, 1.0, [1 << 32], [1, 1, 1])
        with pytest.raises(ValueError, match="row_tags must hold integers"):
            call(q3, 1.0, [0.5, 1.0], [1, 1, 1])
        with pytest.raises(ValueError, match="query_tags holds 65537 distinct masks, more than 65536"):
            call(np.zeros((65537, 4), np.float32), 1.0, tags, np.arange(65537))
        with pytest.raises(AssertionError, match="the native call ran"):       # (the stand-in is what a well-formed call reaches)
            call(q3, 1.0, tags, [1, 0xFFFFFFFF, 0])


def test_null_handle_returns_what_the_grouped_range_exports_return():
    lib = _net().lib
    F, I, U = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int), ct.POINTER(ct.c_uint32)
    v = np.zeros((2, 4), np.float32)
    rt, qt = np.ones(8, np.uint32), np.ones(2, np.uint32)
    rg, qg = np.zeros(8, np.int32), np.zeros(2, np.int32)
    counts, flags = np.full(2, 7, np.int32), np.full(2, 7, np.int32)
    pp_i, pp_d = (ct.c_void_p * 2)(0x1234, 0x1234), (ct.c_void_p * 2)(0x1234, 0x1234)
    tagged = (rt.ctypes.data_as(U), 8, qt.ctypes.data_as(U), 0)
    grouped = (rg.ctypes.data_as(I), 8, qg.ctypes.data_as(I), 1)
    out_args = (pp_i, pp_d, counts.ctypes.data_as(I))
    r = ct.c_float(1.0)
    # a NULL handle: 0 and nothing written
    assert lib.hnsw_mi355x_range_query_tagged(None, v.ctypes.data_as(F), 2, 4, r, 0, *tagged, *out_args) == \
        lib.hnsw_mi355x_range_query_grouped(None, v.ctypes.data_as(F), 2, 4, r, 0, *grouped, *out_args) == 0
    assert lib.hnsw_mi355x_exact_range_query_tagged(None, v.ctypes.data_as(F), 2, 4, r, *tagged, *out_args) == \
        lib.hnsw_mi355x_exact_range_query_grouped(None, v.ctypes.data_as(F), 2, 4, r, *grouped, *out_args) == 0
    assert (counts == 7).all() and list(pp_i) == [0x1234] * 2 and list(pp_d) == [0x1234] * 2
    out = (ct.c_uint64 * 9)(*[9] * 9)
    assert lib.hnsw_mi355x_range_tagged_info(None, out) == lib.hnsw_mi355x_exact_range_tagged_info(None, out) == lib.hnsw_mi355x_range_grouped_info(None, out) == -1
    assert list(out) == [9] * 9
    # a NULL context: -1
    assert lib.hnswdev_range_search_tagged(None, v.ctypes.data_as(F), 2, 0, r, 0, *tagged, counts.ctypes.data_as(I), flags.ctypes.data_as(I)) == \
        lib.hnswdev_range_search_grouped(None, v.ctypes.data_as(F), 2, 0, r, 0, *grouped, counts.ctypes.data_as(I), flags.ctypes.data_as(I)) == -1
    assert lib.hnswdev_exact_range_tagged(None, v.ctypes.data_as(F), 2, 8, r, *tagged, counts.ctypes.data_as(I)) == \
        lib.hnswdev_exact_range_grouped(None, v.ctypes.data_as(F), 2, 8, r, *grouped, counts.ctypes.data_as(I)) == -1
    assert lib.hnswdev_range_tagged_info(None, out) == lib.hnswdev_exact_range_tagged_info(None, out) == -1
    assert list(out) == [9] * 9 and (counts == 7).all() and (flags == 7).all()
    # the header states the calls' contract and their argument errors
    full = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    doc = full[full.index("TAG MASK PER QUERY"):full.index("int hnsw_mi355x_range_query_tagged(")]
    for word in ("Heap is empty", "every array", "range >= 0", "row_tags NULL", "n_row_tags < 0", "match other than 0 and 1", "65 536 distinct masks", "2^27"):
        assert word in doc, word
