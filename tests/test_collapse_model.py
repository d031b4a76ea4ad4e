"""CPU tier: the collapsed k-NN contract and the way the device keeps it (tests/collapse_model.py).

The chunk lemma -- an id of the global collapsed top-k that lies in chunk C is in C's collapsed top-k -- and the insert step that
maintains a collapsed list under offers in any order are what the device's result rests on.  Both are held against the plain walk
here, on integer grids (dozens of ties, so the id decides), with small labels, with one label that holds 90 % of the rows, and with
chunk sizes that put a label's best members into different chunks.  The native interface is checked as far as it goes without a GPU:
symbols, methods, and the argument errors that are raised before anything native runs."""
import ctypes as ct
import re
from pathlib import Path

import numpy as np
import pytest

from collapse_model import EMPTY, CollapsedList, chunked, collapsed_rows, merge, scan_chunk, walk

ROOT = Path(__file__).resolve().parent.parent
KS = (1, 3, 64, 65, 130)


def _ms(k):
    return sorted({m for m in (1, 2, 3, k) if m <= k})


def _keys(n, seed, spread):
    """n keys in id order: integer distances in [0, spread) above the id -- spread << n makes most keys tie in distance."""
    d = np.random.default_rng(seed).integers(0, spread, n)
    return [(int(d[i]) << 32) | i for i in range(n)]


def _labels(n, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "small":          # labels of 1 to 5 members, scattered over the ids; some negative
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(rng.integers(1, 6)))
        lab = np.repeat(np.arange(len(sizes)) - 7, sizes)[:n]
        return lab[rng.permutation(n)]
    if kind == "heavy":          # one label holds 90 % of the rows, the rest are their own
        lab = np.arange(n) + 10
        lab[rng.permutation(n)[: n * 9 // 10]] = -1
        return lab
    raise ValueError(kind)


def test_walk_states_the_contract():
    lab = {0: 5, 1: 5, 2: 5, 3: -2, 4: -2, 5: 9}.__getitem__
    assert walk(range(6), lab, 10, 1) == [0, 3, 5]
    assert walk(range(6), lab, 10, 2) == [0, 1, 3, 4, 5]
    assert walk(range(6), lab, 2, 2) == [0, 1]
    assert walk(range(6), lab, 4, 3) == [0, 1, 2, 3]
    assert walk([], lab, 3, 1) == []
    ids, d = collapsed_rows([[4, 2, -1, 0, 5], []], [[.5, .5, np.nan, 1., 2.], []], np.array([5, 5, 5, -2, -2, 9]), 3, 1)
    assert ids.tolist() == [[4, 2, 5], [-1, -1, -1]] and d[0].tolist() == [.5, .5, 2.] and np.isnan(d[1]).all()
    assert ids.dtype == np.int32 and d.dtype == np.float32


@pytest.mark.parametrize("kind", ["small", "heavy"])
@pytest.mark.parametrize("k", KS)
def test_a_list_under_offers_in_any_order_is_the_walk(k, kind):
    n = 400
    keys, lab = _keys(n, 11 + k, 6), _labels(n, 12 + k, kind)
    label_of = lambda x: int(lab[x & 0xffffffff])
    for m in _ms(k):
        want = walk(sorted(keys), label_of, k, m)
        for seed in range(3):
            rng = np.random.default_rng(seed)
            L = scan_chunk(keys, label_of, k, m, rng)              # through the scan's filter
            assert L.entries() == want, (k, m, kind, seed)
            U = CollapsedList(k, m)                                # and with every key offered: the filter only saves work
            for i in rng.permutation(n):
                U.offer(keys[i], label_of(keys[i]))
            assert U.entries() == want and U.keys[len(want):] == [EMPTY] * (k - len(want)), (k, m, kind, seed)
            per = {}
            for x in U.entries():
                per[label_of(x)] = per.get(label_of(x), 0) + 1
            assert max(per.values()) <= m
        if m == k:                                                 # the cap cannot bind: the plain k smallest
            assert want == sorted(keys)[:k]


@pytest.mark.parametrize("kind", ["small", "heavy"])
@pytest.mark.parametrize("k", KS)
def test_merged_chunk_lists_are_the_walk_over_the_whole_order(k, kind):
    n = 900
    keys, lab = _keys(n, 21 + k, 9), _labels(n, 22 + k, kind)
    label_of = lambda x: int(lab[x & 0xffffffff])
    for m in _ms(k):
        want = walk(sorted(keys), label_of, k, m)
        for chunk in (1, 7, 128, 333, n):
            assert chunked(keys, label_of, k, m, chunk, np.random.default_rng(chunk)) == want, (k, m, kind, chunk)


def test_a_labels_best_members_in_different_chunks():
    """Label 7's three nearest members are ids 699, 700 and 1400 -- the last and the first entry of two chunks and the first of a
    third (chunks of 700) -- and it has farther members in every chunk, nearer ones of other labels between them."""
    n, chunk = 2100, 700
    d = np.random.default_rng(5).integers(10, 40, n)
    lab = np.arange(n) + 100
    lab[[5, 650, 699, 700, 1399, 1400, 2000]] = 7
    d[[699, 700, 1400]] = [3, 2, 1]
    d[[0, 1401]] = [2, 0]                                          # other labels, tied with and below the members
    keys = [(int(d[i]) << 32) | i for i in range(n)]
    label_of = lambda x: int(lab[x & 0xffffffff])
    for k in (3, 10, 65):
        for m, members in ((1, [1400]), (2, [700, 1400]), (3, [699, 700, 1400])):
            if m > k:
                continue
            got = chunked(keys, label_of, k, m, chunk, np.random.default_rng(m))
            assert got == walk(sorted(keys), label_of, k, m)
            of7 = sorted(x & 0xffffffff for x in got if label_of(x) == 7)
            assert of7 == (members if k >= 5 else of7) and len(of7) <= m, (k, m, of7)


def test_the_merge_leaves_a_list_where_nothing_more_can_enter():
    """A key not below the merged list's k-th never enters, whatever its label: in a full list every entry of its label is below it."""
    label_of = lambda x: x % 3
    a = [1, 2, 3, 4, 5, 6]
    out = merge([a[:3] + [EMPTY], [4, 5, 6, EMPTY]], label_of, 4, 2)
    assert out.entries() == walk(a, label_of, 4, 2) == [1, 2, 3, 4]
    full = merge([[10, 11, 12, 13], [1, 14, 15, EMPTY]], label_of, 4, 4)
    assert full.entries() == [1, 10, 11, 12] and full.evicted + full.dropped == 0


def test_rows_with_padding_inside_and_caps_of_more_than_64():
    """The inputs tests/test_gpu_knn_collapsed_edges.py adds: a row of 7 entries and 33 paddings of which two share a label, and a
    row long enough that each of two labels is capped at 60 kept entries."""
    ids = np.full((1, 40), -1, np.int32)
    ids[0, :7] = [11, 3, 8, 0, 5, 9, 2]
    d = np.full((1, 40), np.nan, np.float32)
    d[0, :7] = np.arange(7)
    lab = np.arange(12, dtype=np.int32)
    lab[8] = lab[11]
    out, od = collapsed_rows(ids, d, lab, 10, 1)
    assert out[0].tolist() == [11, 3, 0, 5, 9, 2, -1, -1, -1, -1] and od[0, :6].tolist() == [0, 1, 3, 4, 5, 6] and np.isnan(od[0, 6:]).all()
    order = np.random.default_rng(6).permutation(400).astype(np.int32)[None, :]
    out, _ = collapsed_rows(order, np.arange(400, dtype=np.float32)[None, :], np.arange(400) % 2, 120, 60)
    assert ((out[0] % 2) == 0).sum() == ((out[0] % 2) == 1).sum() == 60
    assert out[0].tolist() == walk(order[0].tolist(), lambda i: i % 2, 120, 60)


def test_the_case_of_the_two_forms_reaches_every_row_and_has_no_ties():
    """tests/test_gpu_knn_collapsed_edges.py holds knn_query_collapsed at a beam of the whole index against the flat scan.  That needs
    a graph on which the traversal returns every row, in the scan's order: here the oracle's graph of the case (one row at a time, as
    the GPU test builds it) is walked from the entry point, and the oracle's knn_query at k = FULL_N must return all rows for every
    query, ascending by (distance, id) with no two distances equal."""
    import oracle
    from collapse_model import FULL_DIM, FULL_M, FULL_METRICS, FULL_N, full_case, reached_from_entry
    x, q = full_case()
    for metric in FULL_METRICS:
        ref = oracle.OracleIndex(FULL_DIM, metric, max_edges=FULL_M, collection_size=FULL_N)
        assert (ref.add(x) == np.arange(FULL_N)).all()
        assert reached_from_entry(ref) == FULL_N, metric
        ids, d = ref.knn_query(q, FULL_N)
        assert (np.sort(ids, axis=1) == np.arange(FULL_N)).all(), metric
        assert (d[:, 1:] > d[:, :-1]).all(), metric


def _header():
    return (ROOT / "include" / "hnsw_mi355x.h").read_text()


SYMBOLS = ("hnsw_mi355x_exact_knn_query_collapsed", "hnsw_mi355x_exact_collapsed_info", "hnswdev_exact_knn_collapsed", "hnswdev_exact_collapsed_info")


def test_header_library_and_bindings_have_the_call():
    import importlib

    import hnswindex
    text = _header()
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\s*\(", text), sym
        assert hasattr(hnswindex.net_amd.lib, sym), sym
    net = importlib.import_module(hnswindex.net_amd.Index.__module__)
    for cls, names in ((net.Index, ("exact_knn_query_collapsed", "exact_collapsed_info")), (net.DeviceBackend, ("exact_knn_collapsed", "exact_collapsed_info"))):
        for name in names:
            assert callable(getattr(cls, name)), name
    ix = net.Index(4, "sq_euclid")
    assert ix.exact_collapsed_info() == {"calls": 0, "queries": 0, "dropped": 0, "evicted": 0}
    q = np.zeros((3, 4), np.float32)
    ids, d = ix.exact_knn_query_collapsed(q, 2, np.zeros(0, np.int32))     # an index nothing was added to: padding
    assert ids.shape == (3, 2) and (ids == -1).all() and np.isnan(d).all()
    # argument breaches are ValueErrors before anything native runs
    with pytest.raises(ValueError, match=r"per_group = 0 is outside \[1, k = 2\]"):
        ix.exact_knn_query_collapsed(q, 2, [], per_group=0)
    with pytest.raises(ValueError, match=r"per_group = 3 is outside \[1, k = 2\]"):
        ix.exact_knn_query_collapsed(q, 2, [], per_group=3)
    with pytest.raises(ValueError, match="k = 1025 is above the limit of 1024"):
        ix.exact_knn_query_collapsed(q, 1025, [])
    with pytest.raises(ValueError, match="row_group must hold integers"):
        ix.exact_knn_query_collapsed(q, 2, [0.5])
    with pytest.raises(ValueError, match="row_group has 2 entries, the index's length is 3"):
        net._collapse_args([1, 2], 2, 1, 3)
    assert net._collapse_args([-5, 2 ** 31 - 1], 2, 2, 2).dtype == np.int32
    for bad in ([0, 2 ** 31], np.array([-2 ** 31 - 1, 0]), np.array([2 ** 32 + 5, 5], np.uint64)):   # wrapped, two labels could become one
        with pytest.raises(ValueError, match="row_group holds a value outside the int32 range"):
            net._collapse_args(bad, 2, 1, 2)
    with pytest.raises(ValueError, match="beam = 1 is below k = 2"):
        ix.knn_query_collapsed(q, 2, [], beam=1)
    assert callable(net.Index.knn_query_collapsed) and hasattr(hnswindex.net_amd.lib, "hnsw_mi355x_knn_query_collapsed")
    ids, d = ix.knn_query_collapsed(q, 2, np.zeros(0, np.int32))
    assert ids.shape == (3, 2) and (ids == -1).all() and np.isnan(d).all()


def test_null_handle_returns_what_the_plain_call_returns():
    import hnswindex
    lib = hnswindex.net_amd.lib
    F, I = ct.POINTER(ct.c_float), ct.POINTER(ct.c_int)
    v, rg = np.zeros((2, 4), np.float32), np.zeros(8, np.int32)
    ids, d = np.full((2, 3), 7, np.int32), np.full((2, 3), 7.0, np.float32)
    out_args = (ids.ctypes.data_as(I), d.ctypes.data_as(F))
    assert lib.hnsw_mi355x_exact_knn_query_collapsed(None, v.ctypes.data_as(F), 2, 4, 3, rg.ctypes.data_as(I), 8, 1, None, 0, *out_args) == \
        lib.hnsw_mi355x_exact_knn_query(None, v.ctypes.data_as(F), 2, 4, 3, None, 0, *out_args) == 0
    out = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_exact_collapsed_info(None, out) == -1 and list(out) == [9] * 4
    assert lib.hnswdev_exact_knn_collapsed(None, v.ctypes.data_as(F), 2, 10, 3, rg.ctypes.data_as(I), 8, 1, None, 0, *out_args) == \
        lib.hnswdev_exact_knn(None, v.ctypes.data_as(F), 2, 10, 3, None, 0, *out_args) == -1
    assert lib.hnswdev_exact_collapsed_info(None, out) == -1 and list(out) == [9] * 4
    assert (ids == 7).all() and (d == 7.0).all()
