"""GPU tier: repair_reachability (hnsw_mi355x_repair_reachability, hnswdev_graph_repair_propose).  Every expectation
comes from tests/graph_repair_model.py, which the CPU tier pins to a graph the oracle builds; the model's candidates are
DeviceBackend.exact_knn's for the stored rows and its distances dist_pair_batch's -- two existing calls with tests of their own."""
import numpy as np
import pytest

import graph_reach_model as rm
import graph_repair_model as rp
from common import set_diag, uniform

pytestmark = pytest.mark.gpu

COUNTERS0 = dict(rounds=0, pairs=0, distances=0, lists_patched=0)
DIM = 20   # (no multiple of 8: the metrics' scalar tail runs)


# ---------------------------------------------------------------- hand-made graphs through DeviceBackend.set_graph
def _backend(rows, metric, max_edges, levels, layer_edges):
    import hnswindex
    dev = hnswindex.DeviceBackend(rows.shape[1], metric, capacity=max(rows.shape[0], 1))
    dev.upload_rows(0, rows)
    dev.set_graph(levels, layer_edges, max_edges)
    return dev


def _rows(n, metric, seed, grid=False):
    rng = np.random.default_rng(seed)
    if grid:   # small integers: many pairs at exactly the same distance
        return rng.integers(-1, 2, (n, DIM)).astype(np.float32)
    return rng.random((n, DIM), dtype=np.float32) + np.float32(0.05)


def _dense_graph(n, max_edges, seed, top=1):
    """Levels 0 .. top and, per layer, lists among the layer's members: about half of them full (MaxEdges(layer) entries, some with the
    MaxEdges + 1 that a list of the mirror can hold), the rest short or empty; targets drawn with replacement (duplicates, self-loops) from
    three quarters of the members, so that the others have no in-edge."""
    rng = np.random.default_rng(seed)
    levels = np.minimum(rng.geometric(0.5, n) - 1, top).astype(np.int32)
    levels[rng.integers(n)] = top
    stride = 2 * max_edges + 2
    layer_edges = []
    for layer in range(top + 1):
        mem = np.nonzero(levels >= layer)[0]
        me = 2 * max_edges if layer == 0 else max_edges
        counts = np.full(n, -1, np.int32)
        edges = np.zeros((n, stride), np.int32)
        inside = mem[rng.random(mem.size) < 0.75]
        inside = inside if inside.size else mem[:1]
        for v in mem:
            kind = rng.random()
            c = 0 if kind < 0.15 else me + 1 if kind < 0.25 else me if kind < 0.6 else int(rng.integers(1, 3))
            if v == np.argmax(levels):
                c = me           # (the tests' one seed: it reaches something)
            counts[v] = c
            edges[v, :c] = rng.choice(inside, c)
            if kind > 0.95:
                edges[v, 0] = v   # a self-loop
        layer_edges.append((counts, edges))
    return levels, layer_edges


def _mask(n, live):
    return None if live is None else rm.as_mask(n, live)


def _check_round(dev, levels, layer_edges, layer, seeds, live, max_edges, cands, tally):
    """One hnswdev_graph_repair_propose against the model; adds the model's (rounds, pairs, distances) to tally."""
    n = levels.size
    counts, edges = layer_edges[layer]
    cap, me = (2 * max_edges + 1, 2 * max_edges) if layer == 0 else (max_edges + 1, max_edges)
    hops = rm.reach_layer(levels, _mask(n, live), layer, counts, edges, seeds, cap)
    U = rm.unreachable_ids(hops)
    got_u, got_c, got_code = dev.graph_repair_propose(layer, seeds, live=live, cands=cands)
    assert got_u.tolist() == U.tolist(), (layer, "U")
    assert got_c.shape == got_code.shape == (U.size, cands)
    if U.size == 0:
        return hops
    reached = hops >= 0
    if reached.any():
        want_c, _ = dev.exact_knn(dev.download_rows(0, n)[U], cands, allowed=reached)
    else:
        want_c = np.full((U.size, cands), -1, np.int32)
    assert got_c.tolist() == want_c.tolist(), (layer, "candidates")
    want_code, measured = rp.propose(levels, _mask(n, live), layer, counts, edges, hops, want_c, dev.dist_pair_batch, me, cap)
    assert got_code.tolist() == want_code.tolist(), (layer, "codes")
    tally += (int(reached.any()), int((want_c >= 0).sum()), measured)      # (a round with nothing reached launches no proposal)
    return hops


@pytest.mark.parametrize("metric", ["sq_euclid", "cosine", "sq_euclid_f16", "sq_euclid_i8"])
@pytest.mark.parametrize("max_edges", [4, 16])
@pytest.mark.parametrize("n", [2, 33, 65, 257])
def test_hand_made_graphs_match_the_model(n, max_edges, metric):
    levels, layer_edges = _dense_graph(n, max_edges, 100 * n + max_edges)
    rows = _rows(n, metric, n + max_edges, grid=(n == 65))      # one size on the integer grid: equal distances, the larger slot wins
    dev = _backend(rows, metric, max_edges, levels, layer_edges)
    dev.reset_stats()
    rng = np.random.default_rng(n * max_edges)
    tally = np.zeros(3, np.int64)
    top_node = int(np.argmax(levels))
    few = np.zeros(n, bool)
    few[top_node] = True                                        # one seed: append and evict proposals, long hop chains
    some = rng.random(n) < 0.2
    some[top_node] = True
    live = rng.random(n) < 0.7                                  # dead targets in the lists of the living
    live[top_node] = True
    seen = set()
    for layer in range(len(layer_edges)):
        for seeds, lv, c in ((few, None, 8), (np.nonzero(some)[0], live, 3), (some, np.nonzero(live)[0], 64), (few, live, 1)):
            hops = _check_round(dev, levels, layer_edges, layer, seeds, lv, max_edges, c, tally)
            seen.add(("U", bool((hops == -1).any())))
    assert n < 33 or ("U", True) in seen
    c = dev.graph_repair_counters()
    assert (c["rounds"], c["pairs"], c["distances"], c["lists_patched"]) == (*tally.tolist(), 0)
    # every member a seed: U is empty, nothing is proposed and the counters stay
    u, cd, code = dev.graph_repair_propose(0, np.ones(n, bool))
    assert u.size == 0 and cd.shape == (0, 8) and dev.graph_repair_counters() == c
    # nobody a seed: every member is in U, there is no candidate and no code
    u, cd, code = dev.graph_repair_propose(0, np.zeros(0, bool), cands=2)
    assert u.tolist() == list(range(n)) and (cd == -1).all() and (code == -1).all()
    assert dev.graph_repair_counters() == c                              # ... and no proposal launch: the counters stay
    dev.reset_stats()
    assert dev.graph_repair_counters() == COUNTERS0


def test_lists_of_64_entries_take_two_lane_passes():
    """MaxEdges(0) = 64: full lists of 64 and of 65 entries, the evictable entries spread over both passes."""
    n, max_edges = 300, 32
    rng = np.random.default_rng(5)
    levels = np.zeros(n, np.int32)
    counts = np.zeros(n, np.int32)
    edges = np.zeros((n, 2 * max_edges + 2), np.int32)
    for v in range(200):                     # 0 .. 199 point at each other; 200 .. 299 have no in-edge
        counts[v] = 64 + (v % 3 == 0)
        edges[v, :counts[v]] = rng.choice(200, counts[v], replace=False)
    edges[0, :64] = np.arange(1, 65)
    layer_edges = [(counts, edges)]
    for metric, grid in (("sq_euclid", False), ("sq_euclid", True), ("cosine", False)):
        dev = _backend(_rows(n, metric, 9, grid), metric, max_edges, levels, layer_edges)
        tally = np.zeros(3, np.int64)
        hops = _check_round(dev, levels, layer_edges, 0, [0], None, max_edges, 8, tally)
        assert (hops == -1).sum() == 100 and tally[2] > 64 * 100
        codes = dev.graph_repair_propose(0, [0], cands=8)[2]
        assert (codes >= 0).any() and codes.max() >= 32 and codes.max() <= 64


def test_the_rule_on_a_graph_small_enough_to_read():
    """MaxEdges(0) = 2 (M = 1).  0 -> 1, 2; 1 -> 0, 1 (a self-loop); 2 -> 0, 0 (a duplicate); 3 -> 1; 3 and 4 have no in-edge.  The list
    of 0 is full of tree edges (-1); in the list of 1 both entries are evictable and 1 -> 0 is the longer one (the self-loop has
    distance 0); in the list of 2 the two entries tie and the larger slot wins."""
    n, max_edges = 5, 1
    levels = np.zeros(n, np.int32)
    counts = np.array([2, 2, 2, 1, 0], np.int32)
    edges = np.zeros((n, 4), np.int32)
    edges[0, :2], edges[1, :2], edges[2, :2], edges[3, :1] = [1, 2], [0, 1], [0, 0], [1]
    rows = np.zeros((n, DIM), np.float32)
    rows[1, 0], rows[2, 1], rows[3, 0], rows[4, 1] = 1, 1, 2, 2
    dev = _backend(rows, "sq_euclid", max_edges, levels, [(counts, edges)])
    u, cd, code = dev.graph_repair_propose(0, [0], cands=3)
    assert u.tolist() == [3, 4]
    assert cd.tolist() == [[1, 0, 2], [2, 0, 1]]
    assert code.tolist() == [[0, -1, 1], [1, -1, 0]]
    tally = np.zeros(3, np.int64)
    _check_round(dev, levels, [(counts, edges)], 0, [0], None, max_edges, 3, tally)
    # 4 is not live: 3 alone is lost; fewer reached members than candidates: padding
    u, cd, code = dev.graph_repair_propose(0, [0], live=[0, 1, 2, 3], cands=5)
    assert u.tolist() == [3] and cd.tolist() == [[1, 0, 2, -1, -1]] and code.tolist() == [[0, -1, 1, -1, -1]]


def test_what_is_no_member_is_never_dereferenced_and_never_evicted(monkeypatch):
    """Lists that no build writes (diag graph_unchecked): entries of -1, n, 2^31 - 1, of an id that is not live and, on layer 1, of a
    level-0 id, in full lists.  None of them is evictable; the round comes back and equals the model."""
    n, max_edges = 40, 2
    levels = np.zeros(n, np.int32)
    levels[[0, 1, 2, 3, 4]] = 1
    c0 = np.zeros(n, np.int32)
    e0 = np.zeros((n, 2 * max_edges + 2), np.int32)
    c0[0], e0[0, :4] = 4, [-1, n, 1, 5]                 # 5 is not live below
    c0[1], e0[1, :4] = 4, [2 ** 31 - 1, 2, -2 ** 31, 0]
    c0[2], e0[2, :5] = 5, [5, 5, n + 7, -1, 5]
    c1 = np.full(n, -1, np.int32)
    e1 = np.zeros((n, 2 * max_edges + 2), np.int32)
    c1[0], e1[0, :2] = 2, [9, 1]                        # 9 has level 0: no member of layer 1
    c1[1], e1[1, :2] = 2, [0, n + 3]
    c1[2], c1[3], c1[4] = 0, 0, 0
    layer_edges = [(c0, e0), (c1, e1)]
    set_diag(monkeypatch, graph_unchecked=1)
    dev = _backend(_rows(n, "sq_euclid", 3), "sq_euclid", max_edges, levels, layer_edges)
    set_diag(monkeypatch, graph_unchecked=0)
    live = np.ones(n, bool)
    live[5] = False
    tally = np.zeros(3, np.int64)
    for layer in (0, 1):
        for seeds in ([0], [0, 1, 2], np.ones(n + 9, bool)):
            _check_round(dev, levels, layer_edges, layer, seeds, live, max_edges, 4, tally)
    u, cd, code = dev.graph_repair_propose(0, [0], live=live, cands=4)
    reached = sorted(set(cd.ravel().tolist()) - {-1})
    assert reached == [0, 1, 2] and 5 not in u.tolist()
    by_v = {int(v): int(c) for v, c in zip(cd.ravel(), code.ravel())}
    assert by_v[0] == -1 and by_v[2] == -1 and by_v[1] == 3           # 0: a tree edge and three non-members; 2: non-members only; 1: 1 -> 0 in slot 3


def test_arguments():
    import hnswindex
    dev = hnswindex.DeviceBackend(DIM, "sq_euclid", capacity=8)
    with pytest.raises(RuntimeError, match="no graph committed"):
        dev.graph_repair_propose(0, [0])
    levels, layer_edges = _dense_graph(8, 4, 1)
    dev = _backend(_rows(8, "sq_euclid", 1), "sq_euclid", 4, levels, layer_edges)
    for cands in (0, 65, -1):
        with pytest.raises(RuntimeError, match="cands"):
            dev.graph_repair_propose(0, [0], cands=cands)
    for me in (0, 10, -1):                  # a layer-0 list of the mirror holds 2 * 4 + 1 entries
        with pytest.raises(RuntimeError, match="max_edges"):
            dev.graph_repair_propose(0, [0], max_edges=me)
    for bad in (-1, len(layer_edges)):
        with pytest.raises(RuntimeError, match="layer"):
            dev.graph_repair_propose(bad, [0])
    ix = hnswindex.Index(16)
    for cands, max_rounds in ((0, 8), (65, 8), (-1, 8), (8, 0), (8, 65), (8, -3)):
        with pytest.raises(RuntimeError, match=r"ArgumentOutOfRangeException: hnsw_mi355x_repair_reachability: cands = %d and max_rounds = %d" % (cands, max_rounds)):
            ix.repair_reachability(cands, max_rounds)
    out = (hnswindex.net_amd.LayerRepair * 1)()
    lib = hnswindex.net_amd.lib
    assert lib.hnsw_mi355x_repair_reachability(ix._h, 8, 8, out, -1) == -1 and "ArgumentNullException" in hnswindex.net_amd.last_error()
    assert lib.hnsw_mi355x_repair_reachability(ix._h, 8, 8, None, 1) == -1
    # an empty index: no layer, no error, whatever the (legal) arguments
    assert ix.repair_reachability() == [] and ix.repair_reachability(1, 64) == [] and ix.repair_reachability(64, 1) == []
    assert ix.graph_repair_counters() == COUNTERS0


# ---------------------------------------------------------------- Index.repair_reachability
def _graph(ix, stride):
    levels = ix.levels()
    live = np.zeros(levels.size, bool)
    live[ix.ids()] = True
    return levels, live, [ix.export_edges(layer, stride) for layer in range(ix.top_layer() + 1)]


def _model_fns(ix, x, metric):
    """cand_fn and dist_fn of the model from existing calls: exact_knn_query of this index for the stored rows, and dist_pair_batch of
    a context that holds the same rows."""
    import hnswindex
    dev = hnswindex.DeviceBackend(x.shape[1], metric, capacity=x.shape[0])
    dev.upload_rows(0, x)
    stored = dev.download_rows(0, x.shape[0])

    def cand_fn(layer, U, reached, C):
        return ix.exact_knn_query(stored[U], C, allowed=reached)[0]
    return cand_fn, dev.dist_pair_batch, stored


def _monotone(before, after):
    old = before >= 0
    assert (after[old] >= 0).all() and (after[old] <= before[old]).all()


def _build(metric, n=2000, host=False):
    import hnswindex
    x = uniform(n, 64, 13)
    ix = hnswindex.Index(64, metric)
    ix.set_max_edges(4)
    ix.set_collection_size(4096)
    ix.set_insert_batch(1)
    if host:
        ix.set_device_traversal(False)
    ix.add(x)
    return ix, x


def _same_lists(a, b):
    return all((ca == cb).all() and all((ea[i, :max(ca[i], 0)] == eb[i, :max(cb[i], 0)]).all() for i in range(ca.size)) for (ca, ea), (cb, eb) in zip(a, b))


@pytest.mark.parametrize("metric,host", [("sq_euclid", False), ("sq_euclid_f16", False), ("sq_euclid", True)])
def test_a_built_index_is_repaired_as_the_model_says(metric, host, tmp_path):
    import hnswindex
    M, stride = 4, 10
    ix, x = _build(metric, host=host)
    n = x.shape[0]
    levels, live, before = _graph(ix, stride)
    lost = ix.unreachable_ids(0)
    assert lost.size > 0 and not (ix.knn_query(x[lost], 1)[0][:, 0] == lost).any()
    cand_fn, dist_fn, stored = _model_fns(ix, x, metric)
    want, want_rep = rp.repair(levels, live, before, ix.entry_point, cand_fn, dist_fn, M, 8, 8, _monotone)
    ix.reset_stats()
    rep = ix.repair_reachability()
    assert rep == want_rep
    assert rep[0]["unreachable_before"] <= lost.size                     # (layer 0 starts from the repaired layer 1)
    after = _graph(ix, stride)[2]
    assert _same_lists(after, want) and not _same_lists(after, before)
    left = rm.reach_chain(levels, live, want, ix.entry_point)[2]
    for layer in range(len(rep)):
        assert ix.unreachable_ids(layer).tolist() == rm.unreachable_ids(left[layer]).tolist()
        assert rep[layer]["unreachable_after"] == 0 == ix.unreachable_ids(layer).size
    c = ix.graph_repair_counters()
    assert c["rounds"] == sum(r["rounds"] for r in rep) and c["lists_patched"] == sum(r["linked"] for r in rep) and c["pairs"] > 0
    # the formerly lost ids can be found now: some self-queries return them, and the flat scan agrees on those
    found = ix.knn_query(stored[lost], 1)[0][:, 0]
    hit = found == lost
    assert hit.sum() > 0
    assert (ix.exact_knn_query(stored[lost][hit], 1)[0][:, 0] == lost[hit]).all()
    # a second call finds nothing to do and changes no list
    second = ix.repair_reachability()
    assert second == rp.repair(levels, live, want, ix.entry_point, cand_fn, dist_fn, M, 8, 8)[1]
    assert all(tuple(r[f] for f in rp.FIELDS[1:]) == (0, 0, 0, 0, 0) for r in second)
    assert _same_lists(_graph(ix, stride)[2], after)
    # the index still works: a snapshot round trip with equal lists, more rows, removals, out-degrees within MaxEdges
    path = tmp_path / "repaired.bin"
    ix.serialize(path)
    back = hnswindex.Index.deserialize(path, metric)
    assert _same_lists(_graph(back, stride)[2], after) and back.unreachable_ids(0).tolist() == ix.unreachable_ids(0).tolist()
    more = uniform(100, 64, 99)
    ids = ix.add(more)
    assert ids.tolist() == list(range(n, n + 100))
    assert (ix.exact_knn_query(more, 1)[0][:, 0] == ids).all() and ix.count == n + 100
    levels1, live1, edges1 = _graph(ix, stride)
    assert ix.reachability() == rm.reach_chain(levels1, live1, edges1, ix.entry_point)[0]      # Add went on from the repaired lists
    got, _ = ix.knn_query(more, 5)
    assert live1[got[got >= 0]].all() and (got[:, 0] >= 0).all()
    ix.remove(np.arange(0, n + 100, 2))
    assert ix.count == (n + 100) // 2
    info = ix.get_info()
    assert info[0]["max_out_edges"] <= 2 * M and all(i["max_out_edges"] <= M for i in info[1:])
    levels2, live2, edges2 = _graph(ix, stride)
    for layer, (counts, edges) in enumerate(edges2):
        for i in np.nonzero(live2 & (levels2 >= layer))[0]:
            own = edges[i, :counts[i]]
            assert np.unique(own).size == own.size and live2[own].all() and (levels2[own] >= layer).all()
    # ... and can be repaired again, with a live set that is a real bitset
    cand_fn2, dist_fn2, _ = _model_fns(ix, np.vstack([x, more]), metric)
    want2, want_rep2 = rp.repair(levels2, live2, edges2, ix.entry_point, cand_fn2, dist_fn2, M, 8, 8, _monotone)
    assert ix.repair_reachability() == want_rep2 and _same_lists(_graph(ix, stride)[2], want2)


def test_one_candidate_and_one_round_leave_the_models_remainder():
    ix, x = _build("sq_euclid")
    levels, live, before = _graph(ix, 10)
    cand_fn, dist_fn, _ = _model_fns(ix, x, "sq_euclid")
    want, want_rep = rp.repair(levels, live, before, ix.entry_point, cand_fn, dist_fn, 4, 1, 1, _monotone)
    assert ix.repair_reachability(cands=1, max_rounds=1) == want_rep
    assert _same_lists(_graph(ix, 10)[2], want)
    left = rm.unreachable_ids(rm.reach_chain(levels, live, want, ix.entry_point)[1])
    assert left.size > 0 and ix.unreachable_ids(0).tolist() == left.tolist()
    assert sum(r["unreachable_after"] for r in want_rep) > 0


def test_nothing_unreachable_nothing_changed_and_a_one_item_index():
    import hnswindex
    x = uniform(300, 32, 3)
    ix = hnswindex.Index(32)
    ix.set_collection_size(1024)
    ix.set_insert_batch(1)
    ix.add(x)
    assert all(ix.unreachable_ids(layer).size == 0 for layer in range(ix.top_layer() + 1))      # M = 16 on 300 rows: everything is reached
    h, (ids0, d0) = ix.graph_hash(), ix.knn_query(x[:50], 10)
    ix.reset_stats()
    rep = ix.repair_reachability()
    assert len(rep) == ix.top_layer() + 1 and all(tuple(r[f] for f in rp.FIELDS[1:]) == (0, 0, 0, 0, 0) for r in rep)
    assert ix.graph_hash() == h and ix.graph_repair_counters() == COUNTERS0
    ids1, d1 = ix.knn_query(x[:50], 10)
    assert (ids0 == ids1).all() and d0.tobytes() == d1.tobytes()
    one = hnswindex.Index(32)
    one.add(x[:1])
    assert one.repair_reachability() == [dict(layer_id=L, unreachable_before=0, linked=0, evicted=0, rounds=0, unreachable_after=0) for L in range(one.top_layer() + 1)]
    # cap below the count is no error: the count comes back, cap entries are written
    out = (hnswindex.net_amd.LayerRepair * 2)()
    out[1].linked = -7
    assert hnswindex.net_amd.lib.hnsw_mi355x_repair_reachability(ix._h, 8, 8, out, 1) == ix.top_layer() + 1 and out[0].as_dict() == rep[0] and out[1].linked == -7
