"""CPU tier: the C ABI of the reachability calls where no device is needed -- NULL handles and contexts, the struct."""
import ctypes as ct
import re
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
    layers = (net.LayerReach * 2)()
    for i in range(2):
        layers[i].layer_id = layers[i].reached = -7
    ids = np.full(4, -7, np.int32)
    I = ct.POINTER(ct.c_int)
    assert lib.hnsw_mi355x_reachability(None, layers, 2) == 0
    assert lib.hnsw_mi355x_unreachable_ids(None, 0, ids.ctypes.data_as(I), 4) == 0
    assert lib.hnsw_mi355x_hop_counts(None, 0, ids.ctypes.data_as(I), 4) == 0
    counters = (ct.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hnsw_mi355x_graph_reach_counters(None, counters) == -1
    assert (ids == -7).all() and list(counters) == [9, 9, 9, 9]
    assert all(layers[i].layer_id == -7 and layers[i].reached == -7 for i in range(2))


def test_null_context_is_an_error(net):
    lib = net.lib
    words = np.zeros(1, np.uint32)
    U = ct.POINTER(ct.c_uint32)
    summary = (ct.c_uint64 * 4)(9, 9, 9, 9)
    layers = (net.LayerReach * 1)()
    assert lib.hnswdev_graph_reach_layer(None, 0, None, 0, words.ctypes.data_as(U), 1, None, None, summary) != 0
    assert lib.hnswdev_graph_reach(None, 0, None, 0, 0, layers, 1, None, None) < 0
    assert lib.hnswdev_graph_reach_counters(None, summary) != 0
    assert list(summary) == [9, 9, 9, 9]


def test_the_struct_is_20_bytes_here_and_in_the_header(net):
    assert ct.sizeof(net.LayerReach) == 20
    assert [n for n, _ in net.LayerReach._fields_] == ["layer_id", "nodes_count", "seeds", "reached", "max_hops"]
    text = (ROOT / "include" / "hnsw_mi355x.h").read_text()
    m = re.search(r"typedef struct hnsw_mi355x_layer_reach \{\s*int32_t ([a-z_, ]+);.*?\} hnsw_mi355x_layer_reach; /\* (\d+) bytes \*/", text, flags=re.S)
    assert m and [f.strip() for f in m.group(1).split(",")] == [n for n, _ in net.LayerReach._fields_] and int(m.group(2)) == 20
    # compiled against the header: an array of two is laid out 20 bytes apart (the library wrote the second entry where ctypes reads it
    # is the GPU tier's business; here the compiler's view)
    src = '#include "hnsw_mi355x.h"\n_Static_assert(sizeof(hnsw_mi355x_layer_reach) == 20, "20 bytes");\n'
    import shutil
    import subprocess
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc:
        r = subprocess.run([cc, "-fsyntax-only", "-x", "c", "-I", str(ROOT / "include"), "-"], input=src, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
