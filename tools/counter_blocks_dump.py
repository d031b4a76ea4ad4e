#!/usr/bin/env python3
"""Every counter block (csrc/counter_blocks.h) of an Index and of a DeviceBackend after one fixed sequence of calls, as JSON: the
record that a change to the counting code left every value where it was.  Run it on two commits on the same machine and compare
everything but the "order_dependent" section (profiles/counter_blocks_dump.json is the committed one).  Only methods that every commit since the collapsed k-NN has are used.

    python3 tools/counter_blocks_dump.py [out.json]      (default: stdout)
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BLOCKS = ("knn_grouped_info", "knn_tagged_info", "by_id_info", "range_grouped_info", "range_tagged_info", "exact_range_info",
          "exact_grouped_info", "exact_collapsed_info", "exact_tagged_info", "exact_range_grouped_info", "exact_range_tagged_info",
          "graph_info_counters", "graph_reach_counters", "graph_repair_counters")
N, DIM, M, STRIDE = 300, 24, 6, 2 * 6 + 2


def scenario():
    """(rows, queries, levels, entry point, per-layer lists with every in-edge of one layer-0 node taken out, that node, labels, tag
    words, a radius that gives every query a few results)."""
    import hnswindex
    rng = np.random.default_rng(20261)
    x = rng.random((N, DIM), dtype=np.float32)
    q = rng.random((40, DIM), dtype=np.float32)
    src = hnswindex.Index(DIM, "sq_euclid")
    src.set_max_edges(M)
    src.set_collection_size(N)
    src.set_random_seed(31337)
    src.set_insert_batch(1)
    src.add(x)
    levels, ep = src.levels(), src.entry_point
    layers = [src.export_edges(layer, STRIDE) for layer in range(src.top_layer() + 1)]
    lost = int(np.flatnonzero((levels == 0) & (np.arange(N) != ep))[7])
    counts, edges = layers[0]
    for v in range(N):
        keep = [e for e in edges[v, :max(counts[v], 0)] if e != lost]
        if counts[v] >= 0:
            counts[v] = len(keep)
            edges[v] = 0
            edges[v, :len(keep)] = keep
    d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    radius = float(np.sort(d, axis=1)[:, 5].mean())
    ids = np.arange(N)
    row_group = (ids % 5).astype(np.int32)                       # group 4 of 6 asked for below; group 5 holds no id
    row_tags = ((ids % 2 == 0) * 1 + (ids % 3 == 0) * 2 + (ids % 7 == 0) * 0x80000000).astype(np.uint32)
    return x, q, levels, ep, layers, lost, row_group, row_tags, radius


def index_calls(x, q, levels, ep, layers, lost, row_group, row_tags, radius):
    import hnswindex
    ix = hnswindex.Index(DIM, "sq_euclid")
    ix.set_max_edges(M)
    ix.set_collection_size(N)
    ix.import_graph(x, levels, ep, layers)
    nq = q.shape[0]
    query_group = (np.arange(nq) % 6).astype(np.int32)
    query_tags = np.array([1, 3, 0x80000002, 0, 4], np.uint32)[np.arange(nq) % 5]
    own = np.array([ep, 0, N - 1, 7, 7, lost], np.int32)
    ix.reset_stats()
    for k in (5, 20):
        ix.knn_query_grouped(q, k, row_group, query_group, 6)
        for match in ("any", "all"):
            ix.knn_query_tagged(q, k, row_tags, query_tags, match)
            ix.exact_knn_query_tagged(q, k, row_tags, query_tags, match)
        ix.knn_query_by_id(own, k)
        ix.exact_knn_query_by_id(own, k)
        ix.exact_knn_query_grouped(q, k, row_group, query_group, 6)
        ix.exact_knn_query_collapsed(q, k, row_group, 2)
    ix.get_vectors(own)
    for r in (radius, 4 * radius):
        ix.range_query_grouped(q, r, row_group, query_group, 6)
        ix.exact_range_query(q, r)
        ix.exact_range_query_grouped(q, r, row_group, query_group, 6)
        for match in ("any", "all"):
            ix.range_query_tagged(q, r, row_tags, query_tags, match)
            ix.exact_range_query_tagged(q, r, row_tags, query_tags, match)
    ix.get_info()
    ix.connected_component_counts()
    ix.reachability()
    ix.unreachable_ids(0)
    ix.repair_reachability()
    return {b: getattr(ix, b)() for b in BLOCKS}


def backend_calls(x, q, levels, ep, layers, lost, row_group, row_tags, radius):
    import hnswindex
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=N)
    dev.upload_rows(0, x)
    dev.set_graph(levels, layers, M)
    nq = q.shape[0]
    query_group = (np.arange(nq) % 6).astype(np.int32)
    query_tags = np.array([1, 3, 0x80000002, 0, 4], np.uint32)[np.arange(nq) % 5]
    own = np.array([ep, 0, N - 1, 7, 7, lost], np.int32)
    dev.reset_stats()
    dev.knn_search_grouped(q, ep, 20, 5, row_group, query_group, 6)
    for match in ("any", "all"):
        dev.knn_search_tagged(q, ep, 20, 5, row_tags, query_tags, match)
        dev.exact_knn_tagged(q, 5, row_tags, query_tags, match)
        dev.range_search_tagged(q, ep, radius, row_tags, query_tags, match)
        dev.exact_range_tagged(q, radius, row_tags, query_tags, match)
    dev.knn_search_by_id(own, ep, 20, 5)
    dev.exact_knn_by_id(own, 5)
    dev.gather_rows(own)
    dev.range_search_grouped(q, ep, radius, row_group, query_group, 6)
    dev.exact_range(q, radius)
    dev.exact_knn_grouped(q, 5, row_group, query_group, 6)
    dev.exact_knn_collapsed(q, 5, row_group, 2)
    dev.exact_range_grouped(q, radius, row_group, query_group, 6)
    for layer in range(len(layers)):
        dev.graph_info(layer)
        dev.graph_components(layer)
    dev.graph_reach(ep)
    dev.graph_repair_propose(0, [ep])
    return {b: getattr(dev, b)() for b in BLOCKS}


# Counted by the collapsed scan's waves as their keys arrive (csrc/counter_blocks.h): these differ from run to run of one build, so
# they are recorded apart from the values two commits are compared on.
ORDER_DEPENDENT = (("exact_collapsed_info", "dropped"), ("exact_collapsed_info", "evicted"))


def main():
    s = scenario()
    dump = {"index": index_calls(*s), "device_backend": backend_calls(*s), "order_dependent": {}}
    for level in ("index", "device_backend"):
        dump["order_dependent"][level] = {f"{b}.{k}": dump[level][b].pop(k) for b, k in ORDER_DEPENDENT}
    text = json.dumps(dump, indent=1) + "\n"
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
