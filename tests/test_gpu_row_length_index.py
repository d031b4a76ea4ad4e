"""GPU tier: Add, the neighbour heuristic, the link launches, Remove and the newer query calls at the row lengths of
tests/row_lengths.py -- small builds (700 rows, MaxEdges 16 so that layer-0 lists pass 24 ids, efc 48, MinNN 32) held to the oracle.

Per (row kind, length), with everything at its default and again under lat=2 (the latency forms of the insert and search kernels):
the graph of the default batched Add and of a sequential build of the first 300 rows; KnnQuery at k 1, 10 and 40 and RangeQuery at the
median fourth-neighbour radius; knn_query_by_id against the per-id filtered calls and knn_query_tagged against the tag model;
100 ids removed, 100 rows added into the vacated slots, and the graph, the Ids() order and the answers again.  Graph hash, levels,
entry point and ids equal, distances equal byte for byte.  stats() must show that the device did the work wherever the restated
traversal_fits says the shape fits: no lock-step launch -- and Remove at rows of more than 2048 elements must leave the device.

The int8 lengths all run the run-time-length measure pass (records of 64 words and more); 1017 and 4200 (int8), 257 and above
(f32), 1024 (f16) are past the 1 KB rule and the heuristic's prefetch limit.  One more build per f32 metric at efc 300 runs the
eight-set insert kernel with the grouped heuristic below the MFMA threshold at 200 and 250 elements."""
import numpy as np
import pytest

import gram_prefilter as gp
import oracle
import row_lengths as rl
import wide_beams as wb
from by_id_model import knn_by_id_loop
from common import default_cap, set_diag
from tagged_query_model import tagged_knn_batch

pytestmark = pytest.mark.gpu

N, M, EFC, MIN_NN, NQ = rl.INDEX_N, rl.INDEX_M, rl.INDEX_EFC, rl.INDEX_MIN_NN, rl.INDEX_NQ
N_SEQ, N_SIDE, N_OUT = 300, 24, 100
MODES = {"device": {}, "lat2": {"lat": 2}}
CASES = [(k, d) for k in rl.ROW_KINDS for d in rl.index_lengths(k)]
QUERY_TAGS = np.array([1, 3, 0x80000002, 0], np.uint32)
_REFS = {}


@pytest.fixture(scope="module")
def Index():
    import hnswindex
    assert hnswindex.net_amd.lib.hnswdev_device_count() > 0, "GPU tier needs a HIP device"
    return hnswindex.Index


def _oracle(kind, dim, efc=EFC, n=N):
    return oracle.OracleIndex(dim, wb.base_metric(kind), max_edges=M, max_candidates=efc, min_nn=MIN_NN, collection_size=n)


def _row_tags(ids):
    return ((ids % 2 == 0) * 1 + (ids % 3 == 0) * 2 + (ids % 5 == 0) * 0x80000000).astype(np.uint32)


def _snapshot(ref, q):
    return {"hash": ref.graph_hash(), "levels": ref.levels(), "entry": ref.entry_point, "ids": ref.active_ids(),
            "knn": {k: ref.knn_query(q, k) for k in (1, 10, 40)}}


def reference(kind, dim):
    """The oracle's side of a case, once per module: the batched build, its answers, the sequential build of the first rows, and
    the state after the removal and the re-use of the slots."""
    key = (kind, dim)
    if key not in _REFS:
        x, q, extra = rl.index_rows(kind, dim)
        xr, er = wb.oracle_rows(kind, x), wb.oracle_rows(kind, extra)
        ref = _oracle(kind, dim)
        assert (ref.add_batched(xr, default_cap(), threads=8) == np.arange(N)).all()
        out = {"x": x, "q": q, "extra": extra, "built": _snapshot(ref, q)}
        radius = float(np.median(out["built"]["knn"][10][1][:, 3]))
        out["radius"], out["range"] = radius, ref.range_query(q, radius)
        tags = _row_tags(np.arange(N))
        qt = QUERY_TAGS[np.arange(N_SIDE) % 4]
        out["tags"], out["qt"] = tags, qt
        out["tagged"] = {m: tagged_knn_batch(ref, xr, wb.base_metric(kind), q[:N_SIDE], 10, MIN_NN, tags, qt, m) for m in ("any", "all")}
        seq = _oracle(kind, dim)
        assert (seq.add(xr[:N_SEQ]) == np.arange(N_SEQ)).all()
        out["seq"] = {"hash": seq.graph_hash(), "levels": seq.levels(), "entry": seq.entry_point}
        victims = np.random.default_rng(7600 + dim).permutation(N)[:N_OUT].astype(np.int32)
        ref.remove(victims)
        out["victims"], out["removed"] = victims, _snapshot(ref, q)
        out["extra_ids"] = ref.add_batched(er, default_cap(), threads=8)
        out["reused"] = _snapshot(ref, q)
        _REFS[key] = out
    return _REFS[key]


def _index(Index, kind, dim, efc=EFC, n=N, batch=None):
    ix = Index(dim, kind)
    ix.set_collection_size(n); ix.set_max_edges(M); ix.set_max_candidates(efc); ix.set_min_nn(MIN_NN)
    if batch is not None:
        ix.set_insert_batch(batch)
    return ix


def _same(got, want):
    return bool((got[0] == want[0]).all() and got[1].tobytes() == want[1].tobytes())


def _same_padded(got, want):
    pad = np.isnan(want[1])
    return bool((got[0] == want[0]).all() and (np.isnan(got[1]) == pad).all() and got[1][~pad].tobytes() == want[1][~pad].tobytes())


def _same_lists(got, want):
    return len(got[0]) == len(want[0]) and all(a.tolist() == c.tolist() and b.tobytes() == d.tobytes() for a, b, c, d in zip(got[0], got[1], want[0], want[1]))


def _holds(ix, want, q, tag, ks=(10,)):
    assert ix.graph_hash() == want["hash"], tag
    assert ix.levels().tolist() == want["levels"].tolist() and ix.entry_point == want["entry"], tag
    assert ix.ids().tolist() == want["ids"].tolist(), tag
    for k in ks:
        assert _same(ix.knn_query(q, k), want["knn"][k]), tag + (k,)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,dim", CASES, ids=lambda v: str(v))
def test_index_at_row_length(Index, monkeypatch, kind, dim, mode):
    want = reference(kind, dim)
    x, q = want["x"], want["q"]
    set_diag(monkeypatch, **MODES[mode])
    tag = (kind, dim, mode)
    on_device = rl.add_fits(kind, dim, M, EFC) and rl.query_fits(kind, dim, M, 40)
    assert on_device                                            # (tests/test_row_length_inputs.py: every length here fits)

    # Add under the default schedule, and the queries
    ix = _index(Index, kind, dim)
    assert (ix.add(x) == np.arange(N)).all()
    st = ix.stats()
    assert st["insert_launches"] > 0 and st["link_launches"] > 0 and st["launches"] == 0 and st["search_overflows"] == 0, tag + (st,)
    if mode == "lat2":
        assert st["lat_launches"] > 0, tag
    ix.reset_stats()
    _holds(ix, want["built"], q, tag + ("built",), ks=(1, 10, 40))
    assert _same_lists(ix.range_query(q, want["radius"]), want["range"]), tag
    st = ix.stats()
    assert st["search_launches"] >= 3 and st["range_launches"] >= 1 and st["launches"] == 0 and st["search_overflows"] == 0, tag + (st,)

    # by stored id and by tag
    own = np.concatenate(([want["built"]["entry"], 0, N - 1], np.random.default_rng(7700 + dim).choice(N, N_SIDE - 3, replace=False))).astype(np.int32)
    assert _same_padded(ix.knn_query_by_id(own, 10), knn_by_id_loop(ix, own, 10)), tag
    for match in ("any", "all"):
        assert _same_padded(ix.knn_query_tagged(q[:N_SIDE], 10, want["tags"], want["qt"], match), want["tagged"][match]), tag + (match,)
    assert ix.stats()["launches"] == 0, tag

    # Remove, and Add into the vacated slots
    ix.reset_stats()
    ix.remove(want["victims"])
    st = ix.stats()
    assert ix.count == N - N_OUT
    if rl.remove_fits(kind, dim, M):
        assert st["search_launches"] > 0 and st["launches"] == 0, tag + (st,)
    else:
        assert st["search_launches"] == 0 and st["launches"] > 0, tag + (st,)
    _holds(ix, want["removed"], q, tag + ("removed",))
    assert (ix.add(want["extra"]) == want["extra_ids"]).all(), tag
    _holds(ix, want["reused"], q, tag + ("slots reused",))

    # one item after the other
    seq = _index(Index, kind, dim, batch=1)
    assert (seq.add(x[:N_SEQ]) == np.arange(N_SEQ)).all()
    st = seq.stats()
    assert st["insert_launches"] > 0 and st["launches"] == 0, tag + (st,)
    assert seq.graph_hash() == want["seq"]["hash"] and seq.levels().tolist() == want["seq"]["levels"].tolist() and seq.entry_point == want["seq"]["entry"], tag


def _wide_leg(Index, monkeypatch, kind, dim, mfma):
    """One build at efc 300 under mfma=<mfma>, held to the oracle; returns insert_evals of the build."""
    x, q, _ = rl.index_rows(kind, dim)
    ref = _oracle(kind, dim, efc=rl.WIDE_EFC)
    assert (ref.add_batched(x, default_cap(), threads=8) == np.arange(N)).all()
    with monkeypatch.context() as m:
        set_diag(m, mfma=mfma)
        ix = _index(Index, kind, dim, efc=rl.WIDE_EFC)
        assert (ix.add(x) == np.arange(N)).all()
        st = ix.stats()
        assert st["insert_launches"] > 0 and st["launches"] == 0 and st["search_overflows"] == 0, (kind, dim, mfma, st)
        assert ix.graph_hash() == ref.graph_hash() and ix.levels().tolist() == ref.levels().tolist() and ix.entry_point == ref.entry_point
        assert _same(ix.knn_query(q, 10), ref.knn_query(q, 10)), (kind, dim, mfma)
    return st["insert_evals"]


@pytest.mark.parametrize("dim", rl.WIDE_LENGTHS + (256,))
@pytest.mark.parametrize("kind", rl.F32_KINDS)
def test_eight_set_insert_with_the_grouped_heuristic(Index, monkeypatch, kind, dim):
    """efc 300: the insert search on eight register sets, its heuristic in the grouped form (the MFMA tiles start at 256 elements),
    at lengths that are no multiple of 128 -- 200 = 16 + 8 + 1 blocks, 250 with a scalar tail.  stats() has no counter per form, so
    which one ran is read off insert_evals as tests/test_gpu_gram_prefilter.py does: the tile form is instantiated for the eight-set
    kernel only and measures other pairs than the exact forms, so a build counts differently with the tiles allowed (mfma=1) and
    forbidden (mfma=0) exactly where they run.  At 256 elements -- the control, same efc, M and row count -- the counters differ:
    the builds of this shape are on the eight-set kernel.  At 200 and 250 they are equal: no tile ran, the heuristic was the grouped one."""
    on, off = _wide_leg(Index, monkeypatch, kind, dim, 1), _wide_leg(Index, monkeypatch, kind, dim, 0)
    print(f"{kind} {dim}: insert_evals {on} with the tiles allowed, {off} without")
    assert gp.prefilter_applies(kind, dim, rl.WIDE_EFC) == (dim == 256)
    assert (on != off) == (dim == 256), (kind, dim, on, off)
