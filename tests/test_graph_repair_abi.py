"""CPU tier: the C ABI of repair_reachability where no device is needed -- NULL handles and contexts, the struct.  (Creating
an index needs a device, so the argument ranges are tested in the GPU tier: tests/test_gpu_graph_repair.py.)"""
import ctypes as ct
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def net():
    import hnswindex
    return hnswindex.net_amd


def test_null_handle_gives_zero_and_writes_nothing(net):
    lib = net.lib
    layers = (net.LayerRepair * 2)()
    for i in range(2):
        layers[i].layer_id = layers[i].linked = -7
    assert lib.hnsw_mi355x_repair_reachability(None, 8, 8, layers, 2) == 0
    assert lib.hnsw_mi355x_repair_reachability(None, 0, 99, layers, 2) == 0   # (a NULL handle is answered before the arguments are read)
    counters = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_graph_repair_counters(None, counters) == -1
    assert list(counters) == [9, 9, 9, 9]
    assert all(layers[i].layer_id == -7 and layers[i].linked == -7 for i in range(2))


def test_null_context_is_an_error(net):
    lib = net.lib
    words = np.zeros(1, np.uint32)
    U, I = ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_int)
    n = ct.c_int(-7)
    out = np.full(8, -7, np.int32)
    p = out.ctypes.data_as(I)
    assert lib.hnswdev_graph_repair_propose(None, 0, None, 0, words.ctypes.data_as(U), 1, 8, 8, ct.byref(n), p, p, p, 1) != 0
    counters = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnswdev_graph_repair_counters(None, counters) != 0
    assert n.value == -7 and (out == -7).all() and list(counters) == [9, 9, 9, 9]


def test_the_struct_is_24_bytes_here_and_in_the_header(net):
    fields = ["layer_id", "unreachable_before", "linked", "evicted", "rounds", "unreachable_after"]
    assert ct.sizeof(net.LayerRepair) == 24
    assert [n for n, _ in net.LayerRepair._fields_] == fields
    text = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    m = re.search(r"typedef struct hnsw_mi355x_layer_repair \{\s*int32_t ([a-z_, ]+);.*?\} hnsw_mi355x_layer_repair; /\* (\d+) bytes \*/", text, flags=re.S)
    assert m and [f.strip() for f in m.group(1).split(",")] == fields and int(m.group(2)) == 24
    src = '#include "hnsw_mi355x.h"\n_Static_assert(sizeof(hnsw_mi355x_layer_repair) == 24, "24 bytes");\n'
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc:
        r = subprocess.run([cc, "-fsyntax-only", "-x", "c", "-I", str(ROOT / "include"), "-"], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
