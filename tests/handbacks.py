"""Inputs, triggers and counting rules of the write-side hand-back tests (test_handback_inputs.py on the CPU, test_gpu_write_handbacks.py
on the device).

Every device traversal can give a job back to the host: on a NaN or -0 distance (key_unsafe, csrc/dk_heaps.h), on a full candidate
heap and spill area, on a full visited table.  In Add such an item is searched again on the lock-step path (search_half_lockstep,
csrc/hnsw_index.cpp) and its whole batch is then linked by the host-grouped form of link_half_device instead of the planned one; in
the exact window it goes alone; Remove repeats the flagged step.  The tests force these paths with the diagnostics below (read by
the library on every call, so a test switches them per phase) and with rows no distance to which is a number.

Shapes.  SMALL: 4 000 + 2 000 rows of dim 24 under a cap of 256 -- every batch below 2 048 items, one sub-batch per batch
(S = 1 in link_half_device).  LARGE: 36 000 + 6 000 rows of dim 16, M 8, efc 40 under a cap of 4 096 -- the second call's batches hold
linked / 16 >= 2 250 items, which the host-grouped form cuts into four sub-batches on two staging sets (S = 4).  `batch_sizes`
restates Add's batch rule, so that the tests rest on a schedule the CPU tier has checked against the oracle."""
import numpy as np

import oracle
import wide_beams as wb
from common import uniform

ROW_KINDS = wb.ROW_KINDS
MIXED_KINDS = ("sq_euclid", "ucosine", "sq_euclid_i8")


class Shape:
    def __init__(self, name, dim, M, efc, cap, first, second, tail=500):
        self.name, self.dim, self.M, self.efc, self.cap, self.first, self.second, self.tail = name, dim, M, efc, cap, first, second, tail

    @property
    def n(self):
        return self.first + self.second + self.tail

    def __repr__(self):
        return self.name


SMALL = Shape("small", 24, 16, 100, 256, 4000, 2000)
SMALL_M32 = Shape("small_m32", 24, 32, 100, 256, 4000, 2000)       # layer-0 lists of 64 entries: the widest the latency forms take
LARGE = Shape("large", 16, 8, 40, 4096, 36000, 6000)
SUB_BATCH_MIN = 2048                 # link_half_device: a batch of this many items goes in four sub-batches
NQ = 300

# ---- triggers (HNSW_MI355X_DIAG) -------------------------------------------------------------------------------------------------
PLAN0 = {"link_plan": 0}             # the host-grouped link half alone: searches stay on the device
# The two-heap traversal with a candidate heap of cand_cap entries in LDS and spill_cap behind it; a search whose heap outgrows
# both is handed back.  cand_cap 24 / spill_cap 8 (tests/test_gpu_index.py) hand back EVERY insert of these shapes: the entry
# point's 2 M neighbours alone fill 32 entries.  The mixed cases need batches that are partly handed back, so the spill area is
# sized to about the median peak of the heap, which is narrow: measured on an MI355X, of the small shape's 2 000 items 1 505 come
# back at 180 entries, 758 at 195, 212 at 210 and 4 at 240; of the large shape's 6 000 (M 8, efc 40) 4 143 at 60, 2 520 at 70, 1 146
# at 80 and none at 150.  "window": the 3 000 x 24 sequential build (157 at 195, 7 386 at 165); "remove": Remove's searches with 100
# candidates on 6 000 x 16 (43 % of the steps at 140, none at 180).
OVERFLOW_SPILL = {"small": 195, "large": 70, "window": 195, "remove": 155}
TABLE = {"vis_hash": 1, "vis_hash_cap": 64, "novis_insert": 0}    # per-wave visited tables of 512 ids: crowded beyond 384


def overflow(name):
    """The overflow trigger of a shape (by name): part of its searches outgrow LDS heap + spill area."""
    return {"sorted_top": 0, "cand_cap": 24, "spill_cap": OVERFLOW_SPILL[str(name)]}


# ---- rows --------------------------------------------------------------------------------------------------------------------
ROW_SEED, QUERY_SEED = 901, 902
# positions, within the SECOND call, of the rows no distance to which is a number: all inside its first batch, so that every later
# batch of the call can meet them
UNSAFE_AT = (3, 57, 140)


def _shape(metric, x):
    return wb._shape(metric, x)


def clean_rows(metric, shape):
    """All rows of a case (first call, second call, tail), i.i.d. uniform -- centred for the int8 kind (see unsafe_rows), unit
    length for the ucosine kinds."""
    x = uniform(shape.n, shape.dim, ROW_SEED + shape.dim)
    if metric == "sq_euclid_i8":
        x = x - np.float32(0.5)
    return _shape(metric, x)


def unsafe_rows(metric, shape, at=UNSAFE_AT):
    """clean_rows with the rows first + at[i] made unsafe.  Float kinds: one NaN element, so every distance to the row is NaN.
    sq_euclid_i8: a NaN element does nothing there (fmaxf drops it from the scale and the element itself clamps to -127: a finite
    record), so the row gets one +inf element instead -- scale inf, that element -127, all others 0 -- and its distance to a row b
    is inf - 2 inf (-127 q_b) = NaN where q_b <= 0 at that element, +inf otherwise: about half of each on centred rows."""
    x = clean_rows(metric, shape).copy()
    rows = shape.first + np.asarray(at)
    cols = (np.arange(len(at)) * 7 + 2) % shape.dim
    x[rows, cols] = np.inf if metric == "sq_euclid_i8" else np.nan
    return x


def unsafe_ids(shape, at=UNSAFE_AT):
    return (shape.first + np.asarray(at)).astype(np.int32)


def queries(metric, shape, nq=NQ):
    q = uniform(nq, shape.dim, QUERY_SEED + shape.dim)
    if metric == "sq_euclid_i8":
        q = q - np.float32(0.5)
    return _shape(metric, q)


# ---- the batch rule --------------------------------------------------------------------------------------------------------------
def batch_sizes(levels, linked_before, m, cap):
    """The snapshot batches of ONE Add call (HnswIndex::add, csrc/hnsw_index.cpp; orc_add_batched): `levels` are the levels of all
    nodes up to the end of the call, the first `linked_before` of them linked already, the next `m` the call's items (nothing was
    ever removed, so ids ascend); `cap` is the insert-batch cap.  A batch holds min(cap, max(1, linked / 4)) items while fewer than
    min(65 536, count after the call / 16) nodes are linked and min(cap, max(1, linked / 16)) afterwards; it ends in front of an item
    whose level exceeds the top layer, and such an item is a batch of its own that raises the top layer.  The very first node of an
    index becomes the entry point without a batch."""
    lv = np.asarray(levels)
    count = linked_before + m
    assert lv.size >= count
    early = min(65536, count // 16)
    out, p = [], 0
    if linked_before == 0:
        top, p = int(lv[0]), 1
    else:
        top = int(lv[:linked_before].max())          # the entry point is the first node of the highest level
    while p < m:
        i = linked_before + p
        if lv[i] > top:
            out.append(1)
            top = int(lv[i])
            p += 1
            continue
        linked = count - (m - p)
        b = min(cap, max(1, linked // (4 if linked < early else 16)))
        s = 1
        while s < b and p + s < m and lv[i + s] <= top:
            s += 1
        out.append(s)
        p += s
    return out


def host_link_launches(sizes):
    """link_launches of a call whose every batch takes the host-grouped link half: one launch per sub-batch (four for a batch of
    2 048 items or more), against one per batch on the planned path."""
    return sum(4 if s >= SUB_BATCH_MIN else 1 for s in sizes)


# ---- references ------------------------------------------------------------------------------------------------------------------
_REFS = {}


def make_oracle(metric, shape, n=None):
    return oracle.OracleIndex(shape.dim, wb.base_metric(metric), max_edges=shape.M, max_candidates=shape.efc, collection_size=n or shape.n)


def reference(metric, shape, rows_kind="clean", threads=8):
    """The oracle of a case after each of its three calls, once per process: a dict with the rows `x`, the queries `q` and per
    stage ("first", "second", "tail") the graph hash, levels, entry point, ids and the answers to the queries."""
    key = (metric, shape.name, rows_kind, threads)
    if key not in _REFS:
        x = clean_rows(metric, shape) if rows_kind == "clean" else unsafe_rows(metric, shape)
        q = queries(metric, shape)
        ref = make_oracle(metric, shape)
        xr = wb.oracle_rows(metric, x)
        out = {"x": x, "q": q}
        for stage, lo, hi in (("first", 0, shape.first), ("second", shape.first, shape.first + shape.second), ("tail", shape.first + shape.second, shape.n)):
            ids = ref.add_batched(xr[lo:hi], shape.cap, threads=threads)
            assert (ids == np.arange(lo, hi)).all()
            out[stage] = snapshot(ref, q, threads)
        x.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def snapshot(ref, q, threads=8):
    return {"hash": ref.graph_hash(), "levels": ref.levels(), "entry": ref.entry_point, "ids": ref.active_ids(), "knn": ref.knn_query(q, 10, threads=threads)}


def same_answers(got, want):
    """knn answers equal: the ids, and the distances byte for byte.  Where the oracle's distance is a NaN the product must have a
    NaN too, but not the same one: the device computes a - b as a + (-b), which flips the sign of a NaN operand (0xFFC00000 against
    the oracle's 0x7FC00000, tests/test_gpu_gram_prefilter.py) -- IEEE 754 leaves a NaN's sign open."""
    gi, gd = got
    wi, wd = want
    isn = np.isnan(wd)
    return bool((gi == wi).all() and (np.isnan(gd) == isn).all() and gd[~isn].tobytes() == wd[~isn].tobytes())
