// traverse_sqh_search_lean.hip -- instantiates the lean forms of graph_search_kernel for M_SQH (sq_euclid on half-precision rows) (launches without visited sets:
// dk_base.h, kFormLean).  Device code: device_kernels.h; the split exists for build time.
#include "device_kernels.h"

namespace hnsw {
HNSW_FOR_EACH_TRAVERSAL_LEAN(HNSW_DEFINE_SEARCH, M_SQH)
} // namespace hnsw
HNSW_PHASE_BIND(sqh_search_lean)
