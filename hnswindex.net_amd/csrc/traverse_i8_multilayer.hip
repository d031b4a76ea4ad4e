// traverse_i8_multilayer.hip -- instantiates graph_multilayer_kernel for M_I8 (MultiLayerKnnQuery's chain of searches; both
// visited-set representations).  Device code: device_kernels.h; the split exists for build time.
#include "device_kernels.h"

namespace hnsw {
HNSW_FOR_EACH_MULTILAYER(HNSW_DEFINE_MULTILAYER, M_I8)
} // namespace hnsw
