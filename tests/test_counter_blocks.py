"""CPU tier: the counter blocks are one table in C (HNSW_FOR_EACH_COUNTER_BLOCK, csrc/counter_blocks.h) and one in Python
(bindings.COUNTER_BLOCKS); the two agree, the ABI header declares both getters of every block with the table's slot count, the library
exports them, and they answer a NULL handle / context and an index without a native handle as the hand-written ones did."""
import ctypes as ct
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "hnswindex.net_amd" / "csrc" / "counter_blocks.h"
ABI = ROOT / "include" / "hnsw_mi355x.h"
SUMMED = {"knn_grouped_info", "knn_tagged_info", "by_id_info"}   # every other block is the primary context's alone
SENTINEL = 0xA5A5A5A5DEADBEEF


def _c_rows():
    """(block name, scope, slot names) of every row of HNSW_FOR_EACH_COUNTER_BLOCK, in order."""
    m = re.search(r"^#define HNSW_FOR_EACH_COUNTER_BLOCK\(X\)((?:.*\\\n)*.*)$", HEADER.read_text(), flags=re.M)
    assert m
    body = m.group(1).replace("\\\n", " ")
    rows = re.findall(r"X\(\s*(\w+)\s*,\s*(\w+)\s*,\s*([\w\s,]+?)\s*\)", body)
    assert len(rows) == body.count("X(") and rows, body
    return [(name, scope, tuple(s.strip() for s in slots.split(","))) for name, scope, slots in rows]


@pytest.fixture(scope="module")
def net():
    import hnswindex
    return hnswindex.net_amd


def test_the_c_table_and_the_python_table_agree(net):
    rows = _c_rows()
    py = net.bindings.COUNTER_BLOCKS
    assert [name for name, _, _ in rows] == list(py)                       # the same blocks in the same order
    for name, scope, slots in rows:
        assert slots == tuple(py[name][0]), name                           # the same slot names in the same order
        assert len(set(slots)) == len(slots) and all(re.fullmatch(r"[a-z_]+", s) for s in slots), name
        assert scope in ("summed", "primary"), name
        assert isinstance(py[name][1], str) and ("hnsw_mi355x_" + name) in py[name][1], name   # the docstring names its getter
    assert len(rows) == 14 and max(len(s) for _, _, s in rows) == 9


def test_the_summed_blocks_are_the_three_that_run_on_every_context():
    assert {name for name, scope, _ in _c_rows() if scope == "summed"} == SUMMED
    assert {name for name, scope, _ in _c_rows() if scope == "primary"} == {name for name, _, _ in _c_rows()} - SUMMED


def test_the_abi_header_declares_both_getters_with_the_slot_count():
    text = ABI.read_text()
    for name, _, slots in _c_rows():
        n = len(slots)
        assert f"int hnsw_mi355x_{name}(void *handle, uint64_t out[{n}]);" in text, name
        assert f"int hnswdev_{name}(void *ctx, uint64_t out[{n}]);" in text, name
        assert len(re.findall(r"\b(?:hnsw_mi355x|hnswdev)_" + name + r"\(", text)) == 2, name   # and declares neither twice


def test_the_library_exports_both_getters(net):
    for name in net.bindings.COUNTER_BLOCKS:
        for sym in ("hnsw_mi355x_" + name, "hnswdev_" + name):
            fn = getattr(net.lib, sym)                                     # AttributeError: the symbol is not exported
            assert fn.restype is ct.c_int, sym
            assert list(fn.argtypes) == [ct.c_void_p, ct.POINTER(ct.c_uint64)], sym


def test_a_null_handle_or_context_is_minus_one_and_writes_nothing(net):
    for name, (slots, _) in net.bindings.COUNTER_BLOCKS.items():
        for sym in ("hnsw_mi355x_" + name, "hnswdev_" + name):
            out = (ct.c_uint64 * (len(slots) + 1))(*([SENTINEL] * (len(slots) + 1)))
            assert getattr(net.lib, sym)(None, out) == -1, sym
            assert list(out) == [SENTINEL] * (len(slots) + 1), sym
    buf = ct.create_string_buffer(256)                                     # the inner level says why; the outer level sets no text
    net.lib.hnswdev_last_error(buf, len(buf))
    assert b"null hnswdev context" in buf.value


def test_an_index_without_a_native_handle_reports_zeros_in_table_order(net):
    ix = net.Index(4, "sq_euclid")
    assert ix._h is None
    for name, (slots, doc) in net.bindings.COUNTER_BLOCKS.items():
        got = getattr(ix, name)()
        assert list(got) == list(slots) and all(type(v) is int and v == 0 for v in got.values()), name
        assert getattr(net.Index, name).__doc__ == doc and getattr(net.Index, name).__name__ == name
        assert callable(getattr(net.DeviceBackend, name)) and ("hnswdev_" + name) in getattr(net.DeviceBackend, name).__doc__
    assert ix._h is None                                                   # asking created nothing
