"""Row lengths of the traversal and insert tests (test_row_length_inputs.py on the CPU; test_gpu_row_length_passes.py,
test_gpu_row_length_index.py and test_gpu_row_length_lds.py on the device), and the rules of the library that make them special.

The kernels choose their code by row length: the measure passes (csrc/dk_measure.h) work in chunks, the int8 pass has compiled
lengths and a run-time one, the plan (Device::plan_traversal, csrc/device_backend.hip) drops the visited sets up to 1 KB per row,
the heuristic (csrc/dk_heuristic.h) prefetches up to 256 words, and Device::traversal_fits sends a shape to the host when its row
no longer fits 64 KB of LDS.  Every rule is restated here with its source line beside it, and the tables name, per row kind, the
lengths that reach each class -- the minimum sets; the CPU test asserts that each length hits the class named.

  f32 (sq_euclid, cosine, ucosine): 8-lane pass = 16-block chunks + single blocks + scalar tail; 2-lane pass = 16 + 8 + up to 7 blocks
    136   16 + 1 blocks
    192   16 + 8
    200   16 + 8 + 1
    248   16 + 8 + 7
    250   the same with a tail of 2: under lat=2 the 8-lane form runs, because dim & 7 != 0
    256   the last row of 1 KB: no visited sets, the heuristic prefetches
    257   the first beyond it, with a tail of 1
    1024  eight 16-block chunks
    2056  257 blocks = 16 x 16 + 1
  f16 (sq_euclid_f16, ucosine_f16): pairs of blocks in chunks of 8 and 4, single pairs, an odd block, the tail
    192   8 + 4 pairs
    232   8 + 4 + 2 pairs and an odd block
    250   8 + 4 + 3 pairs, an odd block and a tail of 2
    392   three 8-pair chunks and an odd block
    1024, 2056
  int8 (sq_euclid_i8), on both sides of each step of the record's pitch
    120 | 121    pitch 32 | 48 words, both compiled lengths
    184 | 185    48 | 64: the first record of run-time length
    248 | 249    64 | 80
    768          pitch 208
    1016 | 1017  pitch 256 | 272: the 1 KB rule and the prefetch limit change
    4200         pitch 1056

The LDS rules end in `lds_boundaries`: for a parameter set (M, efc) the last length at which Add runs on the device, at which a
link launch stays within 64 KB, and at which queries run on the device.  Before the link launches' LDS was part of
traversal_fits (`link_term=False` restates that), Add was admitted at lengths whose link launch asked for more than 64 KB:

  (M, efc)   Add fits up to   link LDS <= 64 KB up to
  (8, 40)    5324             5340
  (8, 4)     5348             5340       5344 and 5348 in the gap
  (63, 1)    5204             4992       4996 .. 5204 in the gap
"""
import numpy as np

import wide_beams as wb
from common import normalize_f32, uniform

ROW_KINDS = wb.ROW_KINDS
F32_KINDS = ("sq_euclid", "cosine", "ucosine")
F16_KINDS = ("sq_euclid_f16", "ucosine_f16")
I8_KIND = "sq_euclid_i8"

LDS_BUDGET = 64 * 1024
ND_BYTES = 8                 # struct ND { int id; float dist; }                                     csrc/dk_heaps.h:22
K_NEW_MAX = 4                # kNewMax                                                               csrc/dk_search_common.h:7
TEAM_LDS = 576 + 16          # kTeamLds = ((sizeof(TeamMail) + 15) & ~15) + 16, TeamMail of 576 B    csrc/device_backend.hip:1187, dk_team.h:59
K_PRE = 4                    # kPre: the heuristic prefetches rows of up to 64 * kPre words          csrc/dk_heuristic.h:185


# ---- records ---------------------------------------------------------------------------------------------------------------------
def i8_pitch(dim):
    """32-bit words of an int8 record: the elements, a scale and a sum of squares, rounded up to 64 B.  device_backend.hip:282"""
    return ((dim + 3) // 4 + 2 + 15) & ~15


def f16_row_words(dim):
    """32-bit words of a half-precision record: 8 per 16 elements.  dk_base.h:97"""
    return ((dim + 15) >> 4) << 3


def pitch_of(kind, dim):
    """What the kernels get as `dim` and what a query occupies in LDS, in words: the int8 record, else the elements (the f16 kinds'
    queries stay f32).  device_backend.h:587"""
    return i8_pitch(dim) if kind == I8_KIND else dim


# ---- the chunks of each pass -------------------------------------------------------------------------------------------------------
def pass8_chunks(dim):
    """measure_pass (dk_measure.h:26-72): (16-block chunks, single blocks behind them, scalar tail elements)."""
    nblk = dim >> 3
    return nblk // 16, nblk % 16, dim & 7


def pass2_chunks(dim):
    """measure_pass2 (dk_measure.h:198-230), which measure_all takes under the latency form only where dim & 7 == 0 (:424):
    (16-block chunks, 8-block chunks -- at most one, single blocks -- at most 7)."""
    assert dim & 7 == 0
    nblk = dim >> 3
    rest = nblk % 16
    return nblk // 16, rest // 8, rest % 8


def passh_chunks(dim):
    """measure_pass_h / measure_pass2_h (dk_measure.h:283-337, :354-393): (8-pair chunks, 4-pair chunks -- at most one, single
    pairs -- at most 3, an odd last block, scalar tail elements)."""
    nblk = dim >> 3
    npair = nblk >> 1
    rest = npair % 8
    return npair // 8, rest // 4, rest % 4, nblk & 1, dim & 7


def i8_blocks(dim):
    """measure_pass_i8_any (dk_measure.h:162-169): (blocks of 8 words, compiled) -- compiled lengths are the pitches 16, 32 and 48."""
    p = i8_pitch(dim)
    return p >> 3, p in (16, 32, 48)


def two_lane_form(kind, dim):
    """Under the latency form, lists of more than 8 ids are measured two lanes per row -- float and half rows of a multiple of 8
    elements only (measure_all, dk_measure.h:409, :424)."""
    return kind != I8_KIND and dim & 7 == 0


# ---- LDS ---------------------------------------------------------------------------------------------------------------------------
def _pad4(dim):
    return (dim + 3) & ~3


def search_lds_bytes(k, cand_cap, dim, heur, nbcap):
    """dk_search_common.h:24-29.  dim: pitch_of(kind, dim)."""
    b = ((ND_BYTES * (k + 1 + cand_cap) + 15) & ~15) + 4 * _pad4(dim) + 2 * 4 * nbcap
    if heur:
        b += 2 * 4 * _pad4(dim) + 4 * nbcap + 4 * 3 * 40
    return b


def cand_lds_cap(k, dim, heur, nbcap):
    """device_backend.hip:1118-1124 with no diagnostic set."""
    cap = min(max(4 * k, 256), 4096)
    while cap > 64 and search_lds_bytes(k, cap, dim, heur, nbcap) > LDS_BUDGET:
        cap //= 2
    return cap


def nbcap_of(max_edges):
    """The id / distance scratch: the longest list (2 M + 1 words with its count) rounded up to 8.  traversal_fits,
    device_backend.hip:1563; Device::nbcap, device_backend.h:256."""
    return max(8, (2 * max_edges + 1 + 7) & ~7)


def link_lds_bytes(dim, nbcap):
    """link_lds_bytes, dk_search_common.h:34: what graph_link_kernel and its dry-run forms are launched with (the four launches of
    device_backend.hip go through link_lds_or_error)."""
    return ((search_lds_bytes(nbcap, 0, dim, True, nbcap) + 15) & ~15) + 4 * (K_NEW_MAX + 1) * nbcap


def traversal_fits(k, heur, max_edges, pitch, link_term=True):
    """Device::traversal_fits (device_backend.hip:1560-1568): the traversal of beam k, the relink of a full list and -- for Add
    (heur) -- the link launch all within 64 KB.  link_term=False: the rule before the link launches' LDS was part of it."""
    if k < 1 or 2 * max_edges + 1 > 128:
        return False
    nb = nbcap_of(max_edges)
    cap = cand_lds_cap(k, pitch, heur, nb)
    ok = search_lds_bytes(k, cap, pitch, heur, nb) <= LDS_BUDGET and search_lds_bytes(nb, 0, pitch, True, nb) <= LDS_BUDGET
    if heur and link_term:
        ok = ok and link_lds_bytes(pitch, nb) <= LDS_BUDGET
    return ok


def add_fits(kind, dim, max_edges, efc, link_term=True):
    """Add on the device: hnsw_index.cpp:1029."""
    return traversal_fits(efc, True, max_edges, pitch_of(kind, dim), link_term)


def query_fits(kind, dim, max_edges, beam):
    """KnnQuery on the device with a beam of max(MinNN, k): hnsw_index.cpp:1596; RangeQuery asks with beam 1 (:2796)."""
    return traversal_fits(beam, False, max_edges, pitch_of(kind, dim))


def remove_fits(kind, dim, max_edges, remove_max_candidates=100):
    """Remove on the device: rows of up to 2048 elements, and a search of RemoveMaxCandidates + 1 fits.  hnsw_index.cpp:2859"""
    return dim <= 2048 and traversal_fits(remove_max_candidates + 1, False, max_edges, pitch_of(kind, dim))


def link_fits(kind, dim, max_edges):
    return link_lds_bytes(pitch_of(kind, dim), nbcap_of(max_edges)) <= LDS_BUDGET


def last_true(pred, lo=4, hi=6000):
    """The largest length in lo .. hi with pred true, by bisection: the rules are monotonic in the length (the exhaustive scans of
    test_row_length_inputs.py hold that for the parameter sets used)."""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid
    return lo


def lds_boundaries(max_edges, efc, beam, kind="sq_euclid", link_term=True):
    """(last length with Add on the device, last length whose link launch is within 64 KB, last length with queries of that beam
    on the device)."""
    return (last_true(lambda d: add_fits(kind, d, max_edges, efc, link_term)), last_true(lambda d: link_fits(kind, d, max_edges)),
            last_true(lambda d: query_fits(kind, d, max_edges, beam)))


# ---- the plan of a search launch -------------------------------------------------------------------------------------------------
def novis_rule(kind, dim):
    """Rows of up to 1 KB are searched without visited sets: (size_t)pitch_ * sizeof(float) <= 1024, device_backend.hip:1290."""
    return pitch_of(kind, dim) * 4 <= 1024


def prefetch_rule(kind, dim):
    """The heuristic prefetches the next candidate's row, and the grouped form stages four at once, up to dim <= 64 * kPre words
    (dk_heuristic.h:186, :188)."""
    return pitch_of(kind, dim) <= 64 * K_PRE


def search_plan(kind, dim, beam, max_edges, diag=None):
    """What plan_traversal and place_traversal (device_backend.hip:1268-1294, :1351-1369) decide for a search launch of a few jobs
    (fewer than the latency form's resident waves) under the diagnostics `diag`: {"ns", "exact_only", "novis", "lat_ok", "form"}
    with form one of "lat", "lean", "plain".  The row prefilter is a variant of "lean"."""
    diag = diag or {}
    ns = 0 if diag.get("sorted_top", 1) == 0 else wb.sets_for(beam)
    exact_only = ns == 0
    nb = nbcap_of(max_edges)
    pitch = pitch_of(kind, dim)
    lds = search_lds_bytes(beam, cand_lds_cap(beam, pitch, False, nb), pitch, False, nb)
    short_lists = 2 * max_edges <= 64                                    # g_stride0_ - 2 <= 64
    novis = short_lists and diag.get("overlap", 1) != 0 and novis_rule(kind, dim) and diag.get("novis", 2) == 2
    lat_ok = not exact_only and short_lists and lds + TEAM_LDS <= LDS_BUDGET
    if lat_ok and diag.get("lat", 1) != 0:
        form = "lat"
    elif novis and not exact_only and diag.get("lean", 1) != 0 and ns <= 4:
        form = "lean"
    else:
        form = "plain"
    return {"ns": 2 if exact_only else ns, "exact_only": exact_only, "novis": novis, "lat_ok": lat_ok, "form": form, "lds": lds}


# ---- the lengths -------------------------------------------------------------------------------------------------------------------
# per length: what pass8_chunks / pass2_chunks (None where dim & 7 != 0) give
F32_LENGTHS = {
    136: ((1, 1, 0), (1, 0, 1)),
    192: ((1, 8, 0), (1, 1, 0)),
    200: ((1, 9, 0), (1, 1, 1)),
    248: ((1, 15, 0), (1, 1, 7)),
    250: ((1, 15, 2), None),
    256: ((2, 0, 0), (2, 0, 0)),
    257: ((2, 0, 1), None),
    1024: ((8, 0, 0), (8, 0, 0)),
    2056: ((16, 1, 0), (16, 0, 1)),
}
# per length: passh_chunks
F16_LENGTHS = {
    192: (1, 1, 0, 0, 0),
    232: (1, 1, 2, 1, 0),
    250: (1, 1, 3, 1, 2),
    392: (3, 0, 0, 1, 0),
    1024: (8, 0, 0, 0, 0),
    2056: (16, 0, 0, 1, 0),
}
# per length: the pitch
I8_LENGTHS = {120: 32, 121: 48, 184: 48, 185: 64, 248: 64, 249: 80, 768: 208, 1016: 256, 1017: 272, 4200: 1056}
I8_SHIFTED = 185             # one int8 case on rows and queries shifted by -0.5 (negative elements in the records)


def lengths_of(kind):
    return tuple(F32_LENGTHS) if kind in F32_KINDS else tuple(F16_LENGTHS) if kind in F16_KINDS else tuple(I8_LENGTHS)


def pass_cases():
    """(kind, dim, shifted) of test_gpu_row_length_passes.py."""
    out = [(k, d, False) for k in ROW_KINDS for d in lengths_of(k)]
    return out + [(I8_KIND, I8_SHIFTED, True)]


# the index builds of test_gpu_row_length_index.py
INDEX_LENGTHS = {"f32": (200, 250, 257, 1024, 2056), "f16": (192, 250, 1024), "i8": (185, 768, 1017, 4200)}
INDEX_N, INDEX_M, INDEX_EFC, INDEX_MIN_NN, INDEX_NQ = 700, 16, 48, 32, 100
WIDE_EFC, WIDE_LENGTHS = 300, (200, 250)     # the 8-set insert kernel with the grouped heuristic below the MFMA threshold (dim >= 256)


def index_lengths(kind):
    return INDEX_LENGTHS["f32" if kind in F32_KINDS else "f16" if kind in F16_KINDS else "i8"]


# rows at and past the LDS budget (test_gpu_row_length_lds.py): (M, efc) -> lengths; MinNN 5 and k = 10, so queries ask with beam 10
LDS_N, LDS_NQ, LDS_K = 300, 40, 10
LDS_CAP = 16                 # Add's snapshot batches, on both sides: the graph, and with it LDS_HOST_ONLY below, is the same on every host
LDS_KINDS = ("sq_euclid", "ucosine_f16")
LDS_CASES = {(8, 40): (5324, 5328, 5380, 5384), (8, 4): (5340, 5344, 5348, 5352), (63, 1): (4992, 4996)}
LDS_I8_DIMS = (21490, 21506)                 # pitch 5376, the last with device queries at M 8, and four words more
# the cases in which everything runs on the host, and how many nodes of the oracle's graph the entry point does not reach on layer 0
# (test_row_length_inputs.py derives both): repair_reachability has a node to link in the f16 case and nothing to do in the others
LDS_HOST_ONLY = {("sq_euclid", 8, 40, 5384): 0, ("ucosine_f16", 8, 40, 5384): 1, (I8_KIND, 8, 40, 21506): 0}
REMOVE_DIMS = (2048, 2049)                   # Remove leaves the device above 2048 elements


# ---- the hand-made graph of the pass tests -------------------------------------------------------------------------------------------
# Layer-0 list lengths of the hubs: measure_all's NP = 1 .. 4 selections on either side (8 | 9, 16 | 17, 24 | 25, 32), its second
# round of 32 rows (33, 40, 57) and the widest list the latency form takes (64).  FULL holds them all: 327 nodes, which a beam of
# 327 searches on eight register sets -- the plain and the latency forms.  The lean forms exist for up to four sets (beams up to
# 256), so two smaller graphs carry the same lengths between them for those.
GRAPH_M = 32
HUB_LISTS = (1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 57, 64)
LEAN_LISTS = ((1, 8, 9, 16, 17, 24, 25, 32, 33, 40), (9, 57, 64, 40, 33, 17))
NQ = 12


def hub_graph(lists):
    """A chain of hubs on layer 0: hub i (id i) lists hub i + 1 and its own leaves, lists[i] ids in all; a leaf lists its hub.
    -> (n, levels, [(counts, edges)]) in the layout of DeviceBackend.set_graph / import_graph; the entry point is id 0."""
    h = len(lists)
    assert all(1 <= c <= 2 * GRAPH_M for c in lists) and lists[-1] >= 1
    leaves = [c - (1 if i + 1 < h else 0) for i, c in enumerate(lists)]
    n = h + sum(leaves)
    counts = np.zeros(n, np.int32)
    edges = np.zeros((n, 2 * GRAPH_M + 2), np.int32)
    nxt = h
    for i, c in enumerate(lists):
        own = list(range(nxt, nxt + leaves[i]))
        nxt += leaves[i]
        # the next hub in the middle of the list, so that it sits in another 8-row group from hub to hub
        lst = own[:len(own) // 2] + ([i + 1] if i + 1 < h else []) + own[len(own) // 2:]
        assert len(lst) == c
        counts[i] = c
        edges[i, :c] = lst
        for leaf in own:
            counts[leaf] = 1
            edges[leaf, 0] = i
    return n, np.zeros(n, np.int32), [(counts, edges)]


def shape_rows(kind, x):
    """Rows or queries as a row kind takes them: unit length for the ucosine kinds."""
    return normalize_f32(x) if wb.base_metric(kind) == "ucosine" else x


_PASS_ROWS = {}


def distinct_distances(kind, x, q):
    """True when, by the oracle's metric, no query of q has two equal distances among the rows x."""
    import oracle
    rows, ids = wb.oracle_rows(kind, x), np.arange(x.shape[0], dtype=np.int32)
    return all(np.unique(oracle.dist_query_rows(wb.base_metric(kind), rows, qi, ids)).size == ids.size for qi in q)


def pass_rows(kind, dim, shifted=False):
    """(rows, queries) of a pass case, for the full graph (the lean graphs take a prefix of the rows): i.i.d. uniform, unit length
    for the ucosine kinds, minus 0.5 where shifted.  327 distances of 24 bits tie now and then (about one query in a hundred), and
    a tie's place in an answer is the heap's business, not the measure pass's: of the seeds 0, 1, ... the first whose queries
    have no two equal distances by the ORACLE's metric is taken (test_row_length_inputs.py holds that one exists below 8)."""
    key = (kind, dim, shifted)
    if key not in _PASS_ROWS:
        n = hub_graph(HUB_LISTS)[0]
        for seed in range(8):
            x, q = uniform(n, dim, 7100 + dim + 10000 * seed), uniform(NQ, dim, 7200 + dim + 10000 * seed)
            if shifted:
                x, q = x - np.float32(0.5), q - np.float32(0.5)
            x, q = shape_rows(kind, x), shape_rows(kind, q)
            if distinct_distances(kind, x, q):
                break
        else:
            raise AssertionError(f"no tie-free seed for {key}")
        x.setflags(write=False)
        q.setflags(write=False)
        _PASS_ROWS[key] = (x, q)
    return _PASS_ROWS[key]


def index_rows(kind, dim, n=INDEX_N, nq=INDEX_NQ, extra=100):
    """(rows, queries, rows for the vacated slots) of an index case."""
    return (shape_rows(kind, uniform(n, dim, 7300 + dim)), shape_rows(kind, uniform(nq, dim, 7400 + dim)),
            shape_rows(kind, uniform(extra, dim, 7500 + dim)))


def lds_rows(kind, dim, n=LDS_N, nq=LDS_NQ, seed=7800):
    """(rows, queries) of a case at the LDS budget (seed 7900: of a Remove case)."""
    return shape_rows(kind, uniform(n, dim, seed + dim)), shape_rows(kind, uniform(nq, dim, seed + 50 + dim))
