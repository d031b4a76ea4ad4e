// kernel_unit.hip -- one traversal kernel unit: the explicit instantiations of one kind (device_kernels.h, HNSW_FOR_EACH_KIND) for
// one metric (device_backend.h, HNSW_FOR_EACH_METRIC), and the unit's phase-clock bind.  build.py compiles this file once per
// (kind, metric) with -DHNSW_UNIT_KIND=<kind> -DHNSW_UNIT_METRIC=<tag>; the split into units exists for build time.
#include "device_kernels.h"

#define HNSW_UNIT_(KIND, TAG)                                                                  \
    namespace hnsw {                                                                           \
    constexpr int kUnitMetric = HNSW_UNIT_METRIC_ID;                                           \
    static_assert(kUnitMetric >= 0, "HNSW_UNIT_METRIC is no tag of HNSW_FOR_EACH_METRIC");     \
    HNSW_UNIT_##KIND(DEFINE, kUnitMetric)                                                      \
    }                                                                                          \
    HNSW_PHASE_BIND(TAG##_##KIND)
#define HNSW_UNIT(KIND, TAG) HNSW_UNIT_(KIND, TAG)
HNSW_UNIT(HNSW_UNIT_KIND, HNSW_UNIT_METRIC)
