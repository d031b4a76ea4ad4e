// traverse_ucosh_filtered.hip -- instantiates graph_search_filtered_kernel for M_UCOSH (ucosine on half-precision rows) (KnnQuery with an allow-set; both visited-set
// representations).  Device code: device_kernels.h; the split exists for build time.
#include "device_kernels.h"

namespace hnsw {
HNSW_FOR_EACH_FILTERED(HNSW_DEFINE_FILTERED, M_UCOSH)
} // namespace hnsw
