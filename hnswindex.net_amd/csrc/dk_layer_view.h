// dk_layer_view.h -- one layer of the graph mirror as the graph-info, graph-reach and graph-repair kernels see it.
// A header of its own so that a per-metric unit can take the view without dk_graph_info.h's kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hnsw {

struct LayerView {
    const int *adj0, *level, *pool;
    const int64_t *upper;
    long long n, pool_cap;
    int stride0, strideU, layer;
    const unsigned *live; // nullptr: every id of 0 .. n - 1; else nbits bits in the allow-sets' format, ids >= nbits not live
    long long nbits;

    __device__ __forceinline__ bool member(long long v) const
    {
        if ((unsigned long long)v >= (unsigned long long)n) return false;
        if (live && (v >= nbits || !((live[v >> 5] >> (v & 31)) & 1u))) return false;
        return level[v] >= layer;
    }
    __device__ __forceinline__ int stride() const { return layer == 0 ? stride0 : strideU; }
    // the list of MEMBER v on this layer, nullptr where the mirror has no such block (a member above layer 0 has upper[v] >= 0)
    __device__ __forceinline__ const int *list(long long v) const
    {
        if (layer == 0) return adj0 + v * stride0;
        const long long off = upper[v];
        if (off < 0) return nullptr;
        const long long at = off + (long long)(layer - 1) * strideU;
        return at + strideU <= pool_cap ? pool + at : nullptr;
    }
    __device__ __forceinline__ int count(const int *l) const
    {
        const int c = l[0], cap = stride() - 1;
        return c < 0 ? 0 : c > cap ? cap : c;
    }
};

} // namespace hnsw
