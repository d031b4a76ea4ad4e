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
#include "dk_exact_mfma.h" // exact_scan_pf_kernel: the plain top-k scan behind an f16 MFMA tile; a kernel of its own, no sink
#include "dk_exact_mfma_ip.h" // exact_scan_ip_pf_kernel: that scan for the cosine family, the bound on the dot product, LDS up to the device's limit
#include "dk_exact_mfma_i8.h" // exact_scan_i8_mfma_kernel: that scan for the int8 rows, the exact dot product on the i8 MFMA tile
#include "dk_exact_tri.h" // exact_tri_pf_kernel: the fixed-radius triangle scans behind the same tile, with the three pair sinks
#include "dk_span_tree.h" // span_scan_kernel: a kernel of its own over the scan's triangle, no sink; its round kernels sit with the common ones
#include "dk_mreach_tree.h" // mreach_scan_kernel: that scan under the mutual reachability distance, the offers on all eight lanes; its two core-key kernels likewise
#include "dk_span_tree_pf.h" // span_pf_kernel: both trees' scans behind the f16 MFMA tile, the bound per component and live

namespace hnsw {
constexpr int kUnitMetric = HNSW_UNIT_METRIC_ID;
static_assert(kUnitMetric >= 0, "HNSW_UNIT_METRIC is no tag of HNSW_FOR_EACH_METRIC");
#define HNSW_EXACT_SINK_UNIT(SINK) template hipError_t exact_scan_launch<kUnitMetric, SINK>(const ExactScanArgs &, const SINK &, unsigned, size_t, hipStream_t);
HNSW_FOR_EACH_EXACT_SINK(HNSW_EXACT_SINK_UNIT)
#undef HNSW_EXACT_SINK_UNIT
template hipError_t graph_repair_propose_launch<kUnitMetric>(const RepairProposeArgs &, unsigned, hipStream_t);
template hipError_t span_scan_launch<kUnitMetric>(const ExactScanArgs &, const SpanScanArgs &, unsigned, size_t, hipStream_t);
template hipError_t mreach_scan_launch<kUnitMetric>(const ExactScanArgs &, const MreachScanArgs &, unsigned, size_t, hipStream_t);
template hipError_t exact_scan_pf_launch<kUnitMetric>(const ExactScanArgs &, unsigned long long *, unsigned, size_t, hipStream_t); // a kernel for sq and sqh, an error for the rest
template hipError_t exact_scan_ip_pf_launch<kUnitMetric>(const ExactScanArgs &, unsigned long long *, unsigned, int, size_t, size_t, hipStream_t); // a kernel for cos, ucos and ucosh, an error for the rest
template hipError_t exact_scan_i8_mfma_launch<kUnitMetric>(const ExactScanArgs &, unsigned long long *, unsigned, size_t, hipStream_t); // a kernel for i8, an error for the rest
#define HNSW_EXACT_TRI_UNIT(SINK) template hipError_t exact_tri_pf_launch<kUnitMetric, SINK>(const ExactScanArgs &, const SINK &, unsigned long long *, unsigned, size_t, hipStream_t);
HNSW_EXACT_TRI_UNIT(ExactRangeUnion) HNSW_EXACT_TRI_UNIT(ExactRangeDensity) HNSW_EXACT_TRI_UNIT(ExactRangeDensityJoin) // ... likewise
#undef HNSW_EXACT_TRI_UNIT
template hipError_t span_pf_launch<kUnitMetric>(const ExactScanArgs &, const SpanPfArgs &, bool, unsigned, size_t, hipStream_t); // ... likewise, with and without core keys
} // namespace hnsw
