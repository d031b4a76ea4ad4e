// exact_sq.hip -- instantiates exact_scan_kernel for M_SQ (sq_euclid) and holds the metric-independent kernels of the flat scan
// (exact_compact_kernel, exact_merge_kernel).  Device code: dk_exact.h; the split exists for build time.
#define HNSW_EXACT_UNIT
#define HNSW_EXACT_COMMON
#include "dk_exact.h"

namespace hnsw {
template hipError_t exact_scan_launch<M_SQ>(const ExactScanArgs &, unsigned, size_t, hipStream_t);
} // namespace hnsw
