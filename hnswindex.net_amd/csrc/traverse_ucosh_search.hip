// traverse_ucosh_search.hip -- instantiates graph_search_kernel for M_UCOSH (ucosine on half-precision rows) (every register-set count,
// both visited-set representations).  Device code: device_kernels.h; the split exists for build time.
#include "device_kernels.h"

namespace hnsw {
HNSW_FOR_EACH_TRAVERSAL(HNSW_DEFINE_SEARCH, M_UCOSH)
} // namespace hnsw
HNSW_PHASE_BIND(ucosh_search)
