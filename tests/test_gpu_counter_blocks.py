"""GPU tier: every counter block of csrc/counter_blocks.h counts, is read back with exactly its slot count at both levels (the C ABI
getters against the Python methods), and is cleared by reset_stats.  One tiny graph -- 64 rows, dim 8, max_edges 8, built once and
imported with every in-edge of one layer-0 node taken out, so that repair has something to link.

That the three `summed` blocks add up over contexts is asserted by
tests/test_gpu_grouped_query.py::test_hashed_visited_sets_host_traversal_and_two_contexts (set_devices=2: calls == 4, launched + skipped == 48)."""
import ctypes as ct

import numpy as np
import pytest

from common import uniform

pytestmark = pytest.mark.gpu

N, DIM, M, STRIDE, NQ = 64, 8, 8, 2 * 8 + 2, 12
SENTINEL = 0x5EED5EED5EED5EED
FIRST_SLOT = {"exact_range_info": "results"}   # every other block: its first slot


@pytest.fixture(scope="module")
def graph():
    """Rows, queries, the graph Add builds at a fixed seed with the in-edges of `lost` removed, and the calls' arguments."""
    import hnswindex
    x, q = uniform(N, DIM, 41), uniform(NQ, DIM, 42)
    src = hnswindex.Index(DIM, "sq_euclid")
    src.set_max_edges(M)
    src.set_collection_size(N)
    src.set_random_seed(31337)
    src.set_insert_batch(1)
    src.add(x)
    levels, ep = src.levels(), src.entry_point
    layers = [src.export_edges(layer, STRIDE) for layer in range(src.top_layer() + 1)]
    lost = int(np.flatnonzero((levels == 0) & (np.arange(N) != ep))[3])
    counts, edges = layers[0]
    for v in range(N):
        keep = [e for e in edges[v, :counts[v]] if e != lost]
        counts[v] = len(keep)
        edges[v] = 0
        edges[v, :len(keep)] = keep
    d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return dict(x=x, q=q, levels=levels, ep=ep, layers=layers, lost=lost,
                radius=1.01 * float(np.sort(d, axis=1)[:, 3].max()),              # every query has at least four rows inside (1 %: far above
                                                                                  # what numpy's and the device's summation orders differ by)
                row_group=(np.arange(N) % 3).astype(np.int32), query_group=(np.arange(NQ) % 3).astype(np.int32),
                row_tags=(1 + (np.arange(N) % 2)).astype(np.uint32), query_tags=np.array([1, 2, 3], np.uint32)[np.arange(NQ) % 3],
                own=np.array([0, N - 1, lost], np.int32))


@pytest.fixture(scope="module")
def blocks():
    import hnswindex
    return hnswindex.net_amd.bindings.COUNTER_BLOCKS


def _index_after_the_calls(g):
    """An Index over the graph after one small call of every family; repair last, it edits lists."""
    import hnswindex
    ix = hnswindex.Index(DIM, "sq_euclid")
    ix.set_max_edges(M)
    ix.set_collection_size(N)
    ix.import_graph(g["x"], g["levels"], g["ep"], g["layers"])
    assert ix.unreachable_ids(0).tolist() == [g["lost"]]
    ix.reset_stats()
    q, r, rg, qg, rt, qt = g["q"], g["radius"], g["row_group"], g["query_group"], g["row_tags"], g["query_tags"]
    ix.knn_query_grouped(q, 5, rg, qg, 3)
    ix.knn_query_tagged(q, 5, rt, qt)
    ix.knn_query_by_id(g["own"], 5)
    ix.range_query_grouped(q, r, rg, qg, 3)
    ix.range_query_tagged(q, r, rt, qt)
    assert min(a.size for a in ix.exact_range_query(q, r)[0]) >= 4
    ix.exact_knn_query_grouped(q, 5, rg, qg, 3)
    ix.exact_knn_query_collapsed(q, 5, rg, 2)
    ix.exact_knn_query_tagged(q, 5, rt, qt)
    ix.exact_range_query_grouped(q, r, rg, qg, 3)
    ix.exact_range_query_tagged(q, r, rt, qt)
    ix.get_info()
    ix.connected_component_counts()
    ix.reachability()
    rep = ix.repair_reachability()
    assert rep[0]["unreachable_before"] == 1 and rep[0]["linked"] >= 1
    return ix


def _backend_after_the_calls(g):
    """A DeviceBackend over the same rows and graph after the same families through hnswdev_*."""
    import hnswindex
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=N)
    dev.upload_rows(0, g["x"])
    dev.set_graph(g["levels"], g["layers"], M)
    dev.reset_stats()
    q, ep, r, rg, qg, rt, qt = g["q"], g["ep"], g["radius"], g["row_group"], g["query_group"], g["row_tags"], g["query_tags"]
    dev.knn_search_grouped(q, ep, 10, 5, rg, qg, 3)
    dev.knn_search_tagged(q, ep, 10, 5, rt, qt)
    dev.knn_search_by_id(g["own"], ep, 10, 5)
    dev.range_search_grouped(q, ep, r, rg, qg, 3)
    dev.range_search_tagged(q, ep, r, rt, qt)
    assert min(a.size for a in dev.exact_range(q, r)[0]) >= 4
    dev.exact_knn_grouped(q, 5, rg, qg, 3)
    dev.exact_knn_collapsed(q, 5, rg, 2)
    dev.exact_knn_tagged(q, 5, rt, qt)
    dev.exact_range_grouped(q, r, rg, qg, 3)
    dev.exact_range_tagged(q, r, rt, qt)
    dev.graph_info(0)
    dev.graph_components(0)
    reached = dev.graph_reach(ep)[1]
    U, _, _ = dev.graph_repair_propose(0, reached)
    assert U.tolist() == [g["lost"]]
    return dev


def _raw(fn, handle, n):
    """The block as the C getter writes it into an array one word longer than the block: (status, the n words, the word behind them)."""
    out = (ct.c_uint64 * (n + 1))(*([SENTINEL] * (n + 1)))
    rc = fn(handle, out)
    return rc, [int(v) for v in out[:n]], int(out[n])


def _check_level(obj, handle, prefix, blocks, lib):
    for name, (slots, _) in blocks.items():
        got = getattr(obj, name)()
        assert list(got) == list(slots), name
        assert got[FIRST_SLOT.get(name, slots[0])] > 0, (prefix, name, got)                # the family's call was counted
        rc, words, behind = _raw(getattr(lib, prefix + name), handle, len(slots))
        assert rc == 0 and behind == SENTINEL, (prefix, name)                              # exactly the block's slots were written
        assert words == list(got.values()), (prefix, name)
    obj.reset_stats()
    for name, (slots, _) in blocks.items():
        assert getattr(obj, name)() == dict.fromkeys(slots, 0), (prefix, name)
        assert _raw(getattr(lib, prefix + name), handle, len(slots)) == (0, [0] * len(slots), SENTINEL), (prefix, name)


def test_every_block_counts_reads_back_exactly_and_resets_on_an_index(graph, blocks):
    import hnswindex
    ix = _index_after_the_calls(graph)
    _check_level(ix, ix._h, "hnsw_mi355x_", blocks, hnswindex.net_amd.lib)


def test_every_block_counts_reads_back_exactly_and_resets_on_a_device_backend(graph, blocks):
    import hnswindex
    dev = _backend_after_the_calls(graph)
    _check_level(dev, dev._ctx, "hnswdev_", blocks, hnswindex.net_amd.lib)
