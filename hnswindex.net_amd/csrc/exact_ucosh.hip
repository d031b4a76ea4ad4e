// exact_ucosh.hip -- instantiates exact_scan_kernel for M_UCOSH (ucosine_f16).  Device code: dk_exact.h; the split exists for build time.
#define HNSW_EXACT_UNIT
#include "dk_exact.h"

namespace hnsw {
template hipError_t exact_scan_launch<M_UCOSH>(const ExactScanArgs &, unsigned, size_t, hipStream_t);
} // namespace hnsw
