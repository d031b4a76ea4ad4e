// traverse_ucosh_multilayer.hip -- instantiates graph_multilayer_kernel for M_UCOSH (ucosine on half-precision rows) (MultiLayerKnnQuery's chain of searches; both
// visited-set representations).  Device code: device_kernels.h; the split exists for build time.
#include "device_kernels.h"

namespace hnsw {
HNSW_FOR_EACH_MULTILAYER(HNSW_DEFINE_MULTILAYER, M_UCOSH)
} // namespace hnsw
