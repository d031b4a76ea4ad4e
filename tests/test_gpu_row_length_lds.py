"""GPU tier: rows at and past the 64 KB LDS budget, and Remove on either side of 2048 elements.

Device::traversal_fits sends Add, the queries, Remove and repair to the lock-step host path when a row no longer fits LDS beside
the traversal's heaps.  Add's link launches need more than its searches (the shortcut's scratch, link_lds_bytes), and that amount is
part of the rule: tests/row_lengths.py restates it, tests/test_row_length_inputs.py derives the lengths used here -- the last length
of each side and the first of the other, in steps of four elements -- and shows the window in which Add used to be admitted with a
link launch above 64 KB: 5344 and 5348 for (M 8, efc 4), 4996 and up for (M 63, efc 1).  Those run here too, and must now link on
the host.

Every case holds graph hash, levels, entry point and the answers (ids, distance bytes) to the oracle, and reads off stats() which
side did the work: insert_launches and link_launches for Add on the device, the lock-step engine's `launches` for the host,
search_launches for the queries.  Where everything runs on the host, RangeQuery, the query by stored id, the tagged query, the
reachability repair and Remove are checked as well: a path that is rarely taken is still a path.  The repair runs on a copy of the
index (import_graph) and is held to tests/graph_repair_model.py -- one of the three graphs has a node for it to link, the others
none (row_lengths.LDS_HOST_ONLY, derived from the oracle on the CPU) -- and Remove runs on the index as built, against the oracle."""
import numpy as np
import pytest

import oracle
import row_lengths as rl
import wide_beams as wb
import graph_repair_model as rp
from by_id_model import knn_by_id_loop
from common import default_cap
from tagged_query_model import tagged_knn_batch

pytestmark = pytest.mark.gpu

N, NQ, K = rl.LDS_N, rl.LDS_NQ, rl.LDS_K
MIN_NN = 5
CASES = [(kind, m, efc, dim) for (m, efc), dims in rl.LDS_CASES.items() for dim in dims for kind in rl.LDS_KINDS]
CASES += [(rl.I8_KIND, 8, 40, dim) for dim in rl.LDS_I8_DIMS]


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _graph(ix, stride):
    """(levels, live mask, (counts, edges) per layer) of an index, as tests/graph_repair_model.py takes them."""
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.ids()] = True
    return levels, live, [ix.export_edges(layer, stride) for layer in range(ix.top_layer() + 1)]


def _equal_lists(a, b):
    return len(a) == len(b) and all((ca == cb).all() and all((ea[i, :max(ca[i], 0)] == eb[i, :max(cb[i], 0)]).all() for i in range(ca.size))
                                    for (ca, ea), (cb, eb) in zip(a, b))


def _same(got, want):
    pad = np.isnan(want[1])
    return bool((got[0] == want[0]).all() and (np.isnan(got[1]) == pad).all() and got[1][~pad].tobytes() == want[1][~pad].tobytes())


def _same_lists(got, want):
    return len(got[0]) == len(want[0]) and all(a.tolist() == c.tolist() and b.tobytes() == d.tobytes() for a, b, c, d in zip(got[0], got[1], want[0], want[1]))


@pytest.mark.parametrize("kind,m,efc,dim", CASES, ids=lambda v: str(v))
def test_rows_at_the_lds_budget(Index, kind, m, efc, dim):
    add_dev, knn_dev, range_dev = rl.add_fits(kind, dim, m, efc), rl.query_fits(kind, dim, m, max(MIN_NN, K)), rl.query_fits(kind, dim, m, 1)
    assert add_dev <= rl.link_fits(kind, dim, m)                  # never a device Add whose link launch is past the budget
    x, q = rl.lds_rows(kind, dim)
    xr, base = wb.oracle_rows(kind, x), wb.base_metric(kind)
    ref = oracle.OracleIndex(dim, base, max_edges=m, max_candidates=efc, min_nn=MIN_NN, collection_size=N)
    assert (ref.add_batched(xr, rl.LDS_CAP, threads=8) == np.arange(N)).all()
    tag = (kind, m, efc, dim, add_dev, knn_dev)
    assert (not knn_dev) == ((kind, m, efc, dim) in rl.LDS_HOST_ONLY), tag

    ix = Index(dim, kind)
    ix.set_collection_size(N); ix.set_max_edges(m); ix.set_max_candidates(efc); ix.set_min_nn(MIN_NN); ix.set_insert_batch(rl.LDS_CAP)
    assert (ix.add(x) == np.arange(N)).all()
    st = ix.stats()
    if add_dev:
        assert st["insert_launches"] > 0 and st["link_launches"] > 0 and st["launches"] == 0, tag + (st,)
    else:
        assert st["insert_launches"] == 0 and st["link_launches"] == 0 and st["launches"] > 0, tag + (st,)
    assert st["search_overflows"] == 0, tag
    assert ix.graph_hash() == ref.graph_hash() and ix.levels().tolist() == ref.levels().tolist() and ix.entry_point == ref.entry_point, tag

    ix.reset_stats()
    want = ref.knn_query(q, K)
    assert _same(ix.knn_query(q, K), want), tag
    st = ix.stats()
    if knn_dev:
        assert st["search_launches"] > 0 and st["launches"] == 0 and st["search_overflows"] == 0, tag + (st,)
    else:
        assert st["search_launches"] == 0 and st["launches"] > 0, tag + (st,)
    radius = float(np.median(want[1][:, 3]))
    ix.reset_stats()
    assert _same_lists(ix.range_query(q, radius), ref.range_query(q, radius)), tag
    st = ix.stats()
    assert (st["range_launches"] > 0) == range_dev and (st["launches"] == 0) == range_dev, tag + (st,)
    if knn_dev:
        return

    # everything on the host: the newer calls, the repair and Remove
    ix.reset_stats()
    own = np.array([ref.entry_point, 0, N - 1, 7, 150], np.int32)
    assert _same(ix.knn_query_by_id(own, K), knn_by_id_loop(ix, own, K)), tag
    tags = ((np.arange(N) % 2 == 0) * 1 + (np.arange(N) % 3 == 0) * 2 + (np.arange(N) % 5 == 0) * 0x80000000).astype(np.uint32)
    qt = np.array([1, 3, 0x80000002, 0], np.uint32)[np.arange(8) % 4]
    for match in ("any", "all"):
        assert _same(ix.knn_query_tagged(q[:8], K, tags, qt, match), tagged_knn_batch(ref, xr, base, q[:8], K, MIN_NN, tags, qt, match)), tag + (match,)
    assert ix.stats()["search_launches"] == 0, tag

    # repair_reachability on a copy of the graph, against the model (cand_fn / dist_fn from existing calls, as in
    # tests/test_gpu_graph_repair.py): the reports equal, the lists equal, and where nothing was unreachable the hash unchanged
    import hnswindex
    stride = 2 * m + 2
    levels, live, before = _graph(ix, stride)
    cp = hnswindex.Index(dim, kind)
    cp.set_collection_size(N); cp.set_max_edges(m); cp.set_max_candidates(efc); cp.set_min_nn(MIN_NN)
    cp.import_graph(x, levels, ix.entry_point, [ix.export_edges(L, 2 * m + 2 if L == 0 else m + 2) for L in range(len(before))])
    assert cp.graph_hash() == ix.graph_hash() == ref.graph_hash(), tag
    lost = cp.unreachable_ids(0)
    assert lost.size == rl.LDS_HOST_ONLY[kind, m, efc, dim], tag + (lost,)
    dev = hnswindex.DeviceBackend(dim, kind, capacity=N)
    dev.upload_rows(0, x)
    stored = dev.download_rows(0, N)
    want_lists, want_rep = rp.repair(levels, live, before, cp.entry_point, lambda layer, U, reached, C: cp.exact_knn_query(stored[U], C, allowed=reached)[0],
                                     dev.dist_pair_batch, m, 8, 8)
    fixed = cp.repair_reachability()
    assert fixed == want_rep and len(fixed) == int(levels[ix.entry_point]) + 1, tag + (fixed, want_rep)
    assert fixed[0]["unreachable_before"] == lost.size, tag
    assert _equal_lists(_graph(cp, stride)[2], want_lists), tag
    if lost.size == 0:
        assert cp.graph_hash() == ref.graph_hash() and _equal_lists(want_lists, before), tag
    else:                                                         # (what the repair achieves is the model's to say: `fixed == want_rep`)
        assert cp.unreachable_ids(0).size == fixed[0]["unreachable_after"] and (fixed[0]["linked"] > 0) == (not _equal_lists(want_lists, before)), tag

    # Remove on the index as built
    victims = np.arange(0, N, 6, dtype=np.int32)
    ix.reset_stats()
    ix.remove(victims)
    ref.remove(victims)
    st = ix.stats()
    assert st["search_launches"] == 0 and st["launches"] > 0, tag + (st,)
    assert ix.graph_hash() == ref.graph_hash() and ix.ids().tolist() == ref.active_ids().tolist() and ix.entry_point == ref.entry_point, tag
    assert _same(ix.knn_query(q, K), ref.knn_query(q, K)), tag


@pytest.mark.parametrize("batch", [1, 16])
@pytest.mark.parametrize("dim", rl.REMOVE_DIMS)
@pytest.mark.parametrize("kind", ["sq_euclid", rl.I8_KIND])
def test_remove_on_either_side_of_2048_elements(Index, kind, dim, batch):
    """Remove searches and re-links on the device for rows of up to 2048 elements and on the host beyond (HnswIndex::remove):
    every third id of 600 removed, one after the other and in snapshot batches of 16.  The batched schedule is the device's: where
    Remove leaves the device the ids go one after the other whatever set_remove_batch says (include/hnsw_mi355x.h), so at 2049 the
    reference of both settings is the sequential oracle."""
    n = 600
    on_device = rl.remove_fits(kind, dim, 16)
    assert on_device == (dim <= 2048)
    x, q = rl.lds_rows(kind, dim, n=n, seed=7900)
    ref = oracle.OracleIndex(dim, kind, collection_size=n)
    assert (ref.add_batched(x, default_cap(), threads=8) == np.arange(n)).all()
    ix = Index(dim, kind)
    ix.set_collection_size(n); ix.set_remove_batch(batch)
    assert (ix.add(x) == np.arange(n)).all()
    assert ix.graph_hash() == ref.graph_hash()
    victims = np.arange(0, n, 3, dtype=np.int32)
    if batch == 1 or not on_device:
        ref.remove(victims)
    else:
        ref.remove_batched(victims, batch)
    ix.reset_stats()
    ix.remove(victims)
    st = ix.stats()
    tag = (kind, dim, batch, {k: st[k] for k in ("search_launches", "launches", "search_overflows")})
    if on_device:
        assert st["search_launches"] > 0, tag
    else:
        assert st["search_launches"] == 0 and st["launches"] > 0, tag
    assert ix.count == n - victims.size
    assert ix.graph_hash() == ref.graph_hash() and ix.ids().tolist() == ref.active_ids().tolist() and ix.entry_point == ref.entry_point, tag
    assert _same(ix.knn_query(q, K), ref.knn_query(q, K)), tag
