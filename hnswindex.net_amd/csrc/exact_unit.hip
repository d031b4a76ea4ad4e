// exact_unit.hip -- one unit of the flat scan (dk_exact.h): exact_scan_kernel, with each of its sinks, for one metric, and the other kernel that
// measures stored rows with the metric outside a traversal: graph_repair_propose_kernel (dk_graph_repair.h).  build.py compiles this file once
// per metric with -DHNSW_UNIT_METRIC=<tag> (device_backend.h, HNSW_FOR_EACH_METRIC); the split into units exists for build time.
// The metric-independent kernels (exact_compact_kernel, exact_merge_kernel, exact_range_sort_kernel, the group-list kernels, exact_merge_grouped_kernel, exact_merge_collapsed_kernel, exact_union_init_kernel, exact_union_labels_kernel, density_init_kernel, density_pairs_kernel, density_labels_kernel) live in exactly one of the units: sq's.
#define HNSW_EXACT_COMMON_IN_sq 1
#define HNSW_CAT_(A, B) A##B
#define HNSW_CAT(A, B) HNSW_CAT_(A, B)
#if HNSW_CAT(HNSW_EXACT_COMMON_IN_, HNSW_UNIT_METRIC) // defined for that one tag, 0 for every other
#define HNSW_EXACT_COMMON
#endif
#define HNSW_EXACT_UNIT
#include "dk_exact.h"
#include "dk_graph_repair.h"

namespace hnsw {
constexpr int kUnitMetric = HNSW_UNIT_METRIC_ID;
static_assert(kUnitMetric >= 0, "HNSW_UNIT_METRIC is no tag of HNSW_FOR_EACH_METRIC");
template hipError_t exact_scan_launch<kUnitMetric>(const ExactScanArgs &, unsigned, size_t, hipStream_t);
template hipError_t exact_range_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactRange &, unsigned, size_t, hipStream_t);
template hipError_t exact_self_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactTopKSelf &, unsigned, size_t, hipStream_t);
template hipError_t exact_range_self_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactRangeSelf &, unsigned, size_t, hipStream_t);
template hipError_t exact_range_union_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactRangeUnion &, unsigned, size_t, hipStream_t);
template hipError_t exact_range_density_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactRangeDensity &, unsigned, size_t, hipStream_t);
template hipError_t exact_range_density_join_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactRangeDensityJoin &, unsigned, size_t, hipStream_t);
template hipError_t exact_collapsed_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactTopKCollapse &, unsigned, size_t, hipStream_t);
template hipError_t exact_grouped_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactTopKGrouped &, unsigned, size_t, hipStream_t);
template hipError_t exact_range_grouped_scan_launch<kUnitMetric>(const ExactScanArgs &, const ExactRangeGrouped &, unsigned, size_t, hipStream_t);
template hipError_t graph_repair_propose_launch<kUnitMetric>(const RepairProposeArgs &, unsigned, hipStream_t);
} // namespace hnsw
