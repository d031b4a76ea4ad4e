// traverse_sqh_filtered.hip -- instantiates graph_search_filtered_kernel for M_SQH (sq_euclid on half-precision rows) (KnnQuery with an allow-set; both visited-set
// representations).  Device code: device_kernels.h; the split exists for build time.
#include "device_kernels.h"

namespace hnsw {
HNSW_FOR_EACH_FILTERED(HNSW_DEFINE_FILTERED, M_SQH)
} // namespace hnsw
