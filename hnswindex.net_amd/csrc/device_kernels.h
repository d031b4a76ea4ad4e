// device_kernels.h -- all gfx950 device code of the backend (included by device_backend.hip, which holds the host side, and by
// kernel_unit.hip, which only instantiates one kind of the big traversal kernel templates for one metric -- the build compiles it
// once per (kind, metric), in parallel).  The code lives in the dk_*.h parts, in dependency order:
//   dk_base.h            includes, wave_sync / wave_lds_sync, half-precision rows
//   dk_metric.h          the reference's lane arithmetic (EuclideanMetric.cs / CosineMetric.cs), int8 records, slot_distance_kernel
//   dk_heaps.h           integer keys, the two BinaryHeaps in LDS with the reference's sift rules
//   dk_measure.h         measure passes (rows of one expansion in one memory round trip)
//   dk_search_common.h   LDS carve-up, graph view, visited set, read log, a persistent wave's prologue, FindEntryAtLayer
//   dk_sorted_top.h      SearchLayer on one sorted register list (the loaded launches), tie rules, no visited set
//   dk_team.h            the latency variants' memory wave and its mailbox
//   dk_pool_top.h        SearchLayer on an unsorted register pool (the latency variants' logic wave)
//   dk_traverse_exact.h  the exact two-heap traversal
//   dk_heuristic.h       RelativeNeighborPruning (with its MFMA Gram-block prefilter)
//   dk_range_finish.h   RangeQuery's order on the device: ranking by counting, the heaps replayed on known distances
//   dk_search_kernels.h  graph_search_kernel, graph_search_filtered_kernel, graph_search_grouped_kernel, graph_search_tagged_kernel, graph_search_self_kernel, graph_multilayer_kernel, graph_range_kernel
//   dk_insert_kernels.h  graph_insert_search_kernel
//   dk_link.h            the link half of Add, Remove's re-link
//   dk_misc_kernels.h    small kernels
// (dk_exact.h, the flat scan behind hnswdev_exact_knn, is not part of this umbrella: its kernels are compiled in the exact_unit.hip
// units alone and reached through launchers, so no other unit carries their code.)
// See device_backend.hip's header comment for what the kernels replace and the numerical contract.
#pragma once
#include "dk_base.h"
#include "dk_metric.h"
#include "dk_heaps.h"
#include "dk_measure.h"
#include "dk_search_common.h"
#include "dk_sorted_top.h"
#include "dk_team.h"
#include "dk_pool_top.h"
#include "dk_traverse_exact.h"
#include "dk_heuristic.h"
#include "dk_search_kernels.h"
#include "dk_range_finish.h"
#include "dk_insert_kernels.h"
#include "dk_link.h"
#include "dk_misc_kernels.h"

namespace hnsw {

// Explicit instantiations of the traversal kernels live in the kernel_unit.hip units, one per (kind, metric) -- the kinds are listed
// below, the metrics in device_backend.h; every other unit only declares them.
// Ten forms per metric and kernel (eighteen until round 5) plus four lean ones: register sets NS in {2, 4, 8} (beams up to 128 / 256 / 512; a beam of
// up to 64 runs in the two-set form), the visited set as a bitset or (graphs above 4M nodes, NS <= 4) a per-wave hash table, and the
// latency variant of each.  What used to be forms of their own: NS = 1 (same code with one register less), NS = 0 (the exact
// two-heap traversal alone: now launch flag 0x200 of the two-set form), hash tables for NS = 8 (such launches keep bitsets).
#define HNSW_FOR_EACH_TRAVERSAL(X, M) \
    X(M, 2, false, kFormPlain) X(M, 4, false, kFormPlain) X(M, 8, false, kFormPlain) \
    X(M, 2, true, kFormPlain) X(M, 4, true, kFormPlain)
// the latency variants: units of their own
#define HNSW_FOR_EACH_TRAVERSAL_LAT(X, M) \
    X(M, 2, false, kFormLat) X(M, 4, false, kFormLat) X(M, 8, false, kFormLat) \
    X(M, 2, true, kFormLat) X(M, 4, true, kFormLat)
// the lean forms of graph_search_kernel (round 5; kFormLean in dk_base.h): beams up to 256 entries, launches without visited sets;
// units of their own.  (The insert kernel has none: measured, its f32 form loses 6 % that way.)  Beside them their row-prefilter
// variants (kFormLeanPF, kFormLeanPFFixed with the row length compiled in, and kFormLeanPF8Fixed on the 8-bit shadow): real kernels for sq_euclid, empty ones for every other
// metric (graph_search_kernel), never launched there.
#define HNSW_FOR_EACH_TRAVERSAL_LEAN(X, M) \
    X(M, 2, false, kFormLean) X(M, 4, false, kFormLean) X(M, 2, true, kFormLean) X(M, 4, true, kFormLean) \
    X(M, 2, false, kFormLeanPF) X(M, 4, false, kFormLeanPF) X(M, 2, true, kFormLeanPF) X(M, 4, true, kFormLeanPF) \
    X(M, 2, false, kFormLeanPFFixed) X(M, 4, false, kFormLeanPFFixed) X(M, 2, true, kFormLeanPFFixed) X(M, 4, true, kFormLeanPFFixed) \
    X(M, 2, false, kFormLeanPF8Fixed) X(M, 4, false, kFormLeanPF8Fixed) X(M, 2, true, kFormLeanPF8Fixed) X(M, 4, true, kFormLeanPF8Fixed)

// The kinds of kernel unit, X(kind, ...), and what each instantiates for a metric M: HNSW_UNIT_<kind>(DEFINE, M) is the unit's
// content (kernel_unit.hip), HNSW_UNIT_<kind>(DECLARE, M) the extern template declarations of everyone else.  build.py's KINDS
// is the same list: a unit is compiled with -DHNSW_UNIT_KIND=<kind>.  A grid over metrics x kinds is two lines where it is needed:
//     #define PER_UNIT(KIND, ID, TAG) ...
//     #define PER_METRIC(ID, TAG, NAME) HNSW_FOR_EACH_KIND(PER_UNIT, ID, TAG)
//     HNSW_FOR_EACH_METRIC(PER_METRIC)
#define HNSW_FOR_EACH_KIND(X, ...) \
    X(insert, __VA_ARGS__) X(insert_lat, __VA_ARGS__) X(search, __VA_ARGS__) X(search_lat, __VA_ARGS__) X(search_lean, __VA_ARGS__) \
    X(filtered, __VA_ARGS__) X(multilayer, __VA_ARGS__)
#define HNSW_UNIT_insert(DO, M) HNSW_FOR_EACH_TRAVERSAL(HNSW_##DO##_INSERT, M)
#define HNSW_UNIT_insert_lat(DO, M) HNSW_FOR_EACH_TRAVERSAL_LAT(HNSW_##DO##_INSERT, M)
#define HNSW_UNIT_search(DO, M) HNSW_FOR_EACH_TRAVERSAL(HNSW_##DO##_SEARCH, M)
#define HNSW_UNIT_search_lat(DO, M) HNSW_FOR_EACH_TRAVERSAL_LAT(HNSW_##DO##_SEARCH, M)
#define HNSW_UNIT_search_lean(DO, M) HNSW_FOR_EACH_TRAVERSAL_LEAN(HNSW_##DO##_SEARCH, M)
#define HNSW_UNIT_filtered(DO, M) HNSW_FOR_EACH_FILTERED(HNSW_##DO##_FILTERED, M) HNSW_FOR_EACH_FILTERED(HNSW_##DO##_GROUPED, M) HNSW_FOR_EACH_FILTERED(HNSW_##DO##_TAGGED, M) HNSW_FOR_EACH_FILTERED(HNSW_##DO##_SELF, M) // (graph_search_grouped_kernel, graph_search_tagged_kernel, graph_search_self_kernel: the same traversal, built beside it)
#define HNSW_UNIT_multilayer(DO, M) HNSW_FOR_EACH_MULTILAYER(HNSW_##DO##_MULTILAYER, M)

} // namespace hnsw
