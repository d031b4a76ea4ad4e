"""CPU tier: the inputs of tests/test_gpu_write_handbacks.py do what that file relies on, checked against the oracle alone.

The batch schedule: handbacks.batch_sizes restates Add's batch rule; the GPU tests take from it that the second call of the large
shape has batches of 2 048 items or more (the four-sub-batch form of the host-grouped link half) and how many link launches a call
makes on either link path.  The prediction is held to the oracle: an oracle fed the call batch by batch, in calls of exactly the
predicted sizes, must end in the one-call graph -- a wrong size merges or splits a batch.

The unsafe rows: the oracle builds them, distances to them are NaN (all of them for the float kinds, those with a non-positive
element opposite the inf for int8), and the oracle's graph and answers do not depend on its thread count."""
import numpy as np
import pytest

import handbacks as hb
import oracle
import wide_beams as wb


def _fed_by(metric, shape, x, sizes):
    """The oracle after the first call in one piece and the second in calls of `sizes` items."""
    ref = hb.make_oracle(metric, shape)
    ref.add_batched(x[:shape.first], shape.cap, threads=8)
    lo = shape.first
    for s in sizes:
        ref.add_batched(x[lo:lo + s], shape.cap, threads=8)
        lo += s
    assert lo == shape.first + shape.second
    return ref


@pytest.mark.parametrize("shape", [hb.SMALL, hb.LARGE], ids=repr)
def test_batch_sizes_predict_the_oracles_schedule(shape):
    metric = "sq_euclid"
    want = hb.reference(metric, shape)
    lv = want["tail"]["levels"]
    assert (lv == oracle.random_levels(31337, 1.0 / np.log(16), shape.n)).all()         # levels are the generator's alone
    sizes = hb.batch_sizes(lv, shape.first, shape.second, shape.cap)
    print(f"{shape}: second call in batches of {sizes}")
    assert sum(sizes) == shape.second
    big = [s for s in sizes if s >= hb.SUB_BATCH_MIN]
    if shape is hb.LARGE:
        assert len(big) >= 2 and sizes[0] == shape.first // 16
        assert hb.host_link_launches(sizes) == len(sizes) + 3 * len(big)
    else:
        assert not big and max(sizes) <= shape.cap and hb.host_link_launches(sizes) == len(sizes)
    x = want["x"]
    assert _fed_by(metric, shape, x, sizes).graph_hash() == want["second"]["hash"]
    # the check can fail: one item moved from the first batch to the second is another schedule and another graph
    moved = [sizes[0] - 1, sizes[1] + 1] + sizes[2:]
    assert _fed_by(metric, shape, x, moved).graph_hash() != want["second"]["hash"]


def test_batch_sizes_on_the_rules_edges():
    lv = np.zeros(140000, np.int32)
    # an empty index: the first node is the entry point without a batch; 12 / 16 = 0 leaves no early phase, and linked / 16 = 0 is
    # raised to one item
    assert hb.batch_sizes(lv, 0, 12, 256) == [1] * 11
    # an item above the top layer ends the batch in front of it and goes alone; the next batch starts behind it
    lv2 = lv.copy(); lv2[1000 + 10] = 3
    assert hb.batch_sizes(lv2, 1000, 200, 256) == [10, 1, 63, 67, 59]
    # ... but not an item AT the top layer
    lv3 = lv2.copy(); lv3[5] = 3
    assert hb.batch_sizes(lv3, 1000, 200, 256) == [62, 66, 70, 2]
    # early phase: linked / 4 while fewer than (count after the call) / 16 are linked, linked / 16 afterwards; capped
    # (32 000 / 16 = 2 000: 1 000, 1 250, 1 562 and 1 952 linked nodes are early, 2 440 are not)
    assert hb.batch_sizes(lv, 1000, 31000, 4096)[:5] == [250, 312, 390, 488, 152]
    # the early phase ends at 65 536 linked nodes however large the call: 1 260 000 / 16 = 78 750 would keep 75 000 early
    assert hb.batch_sizes(np.zeros(1260000, np.int32), 60000, 1200000, 10 ** 6)[:2] == [15000, 4687]
    assert hb.batch_sizes(lv, 64000, 70000, 4096)[:2] == [4000, 4096]
    assert hb.batch_sizes(lv, 40000, 3000, 4096) == [2500, 500]
    assert hb.batch_sizes(lv, 40000, 3000, 1000) == [1000, 1000, 1000]


@pytest.mark.parametrize("shape", [hb.SMALL, hb.LARGE], ids=repr)
@pytest.mark.parametrize("metric", hb.MIXED_KINDS)
def test_unsafe_rows_are_built_by_the_oracle_whatever_its_threads(metric, shape):
    x = hb.unsafe_rows(metric, shape)
    clean = hb.clean_rows(metric, shape)
    ids = hb.unsafe_ids(shape)
    changed = np.flatnonzero((x != clean).any(axis=1) | np.isnan(x).any(axis=1))
    assert changed.tolist() == ids.tolist() and (ids >= shape.first).all() and (ids < shape.first + shape.second).all()
    sizes = hb.batch_sizes(hb.reference(metric, shape, "unsafe")["tail"]["levels"], shape.first, shape.second, shape.cap)
    assert ids.max() - shape.first < sizes[0] and len(sizes) >= 3            # all in the first batch, later batches can meet them
    # distances to an unsafe row
    others = np.setdiff1d(np.arange(shape.first + shape.second, dtype=np.int32), ids)[:2000]
    for i in ids:
        d = oracle.dist_query_rows(wb.base_metric(metric), x, x[i], others)
        share = float(np.isnan(d).mean())
        print(f"{metric} {shape}: row {i}: share of NaN distances {share:.3f}")
        if metric == "sq_euclid_i8":
            assert 0.3 < share < 0.7 and np.isinf(d[~np.isnan(d)]).all()
        else:
            assert share == 1.0
    if metric == "sq_euclid_i8":     # a NaN element would have done nothing
        y = clean.copy(); y[ids[0], 2] = np.nan
        assert np.isfinite(oracle.dist_query_rows(metric, y, y[ids[0]], others)).all()
    # one thread and eight: the same graph after every call, the same answers
    a, b = hb.reference(metric, shape, "unsafe", threads=1), hb.reference(metric, shape, "unsafe", threads=8)
    for stage in ("first", "second", "tail"):
        assert a[stage]["hash"] == b[stage]["hash"] and a[stage]["entry"] == b[stage]["entry"]
        assert (a[stage]["knn"][0] == b[stage]["knn"][0]).all() and a[stage]["knn"][1].tobytes() == b[stage]["knn"][1].tobytes()
    assert a["second"]["hash"] != hb.reference(metric, shape)["second"]["hash"]      # the rows matter
    assert a["first"]["hash"] == hb.reference(metric, shape)["first"]["hash"]        # ... in the second call only
