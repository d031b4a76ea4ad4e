// dk_graph_info.h -- device code of GetInfo / GetConnectedComponentCounts on the graph mirror (the reference:
// src/HNSWIndex/HNSWInfo.cs:5-53, GraphNavigator.cs:331-419).  Included by device_backend.hip only: these kernels read no rows, so
// they have no metric and live in that unit beside the small kernels.
//
// A layer's MEMBERS are the ids v < n that are live and have level[v] >= layer (LayerView::member).  Every kernel is an ordinary
// grid-stride launch: no kernel waits for another wave, none is launched until "nothing changes".  The mirror is read, never
// written; what is written is the call's own scratch (GraphAcc, in_deg, parent, the in-degree histogram).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dk_layer_view.h"
#include "dk_union_find.h"

namespace hnsw {

constexpr int kGraphInfoMaxStride = 132; // ints of the longest list the mirror takes (set_graph: MaxEdges(0) + 1 <= 129), count word included
constexpr int kGraphInfoBlock = 256;
constexpr int kGraphInfoLdsBins = 2048;  // in-degree histogram: bins below this are counted in LDS first

// What a call's kernels add up (one block of device memory, zeroed in front of the first launch)
struct GraphAcc {
    unsigned long long entries; // list entries read: the sum of the members' out-degrees
    unsigned long long in_sum;  // sum of the members' in-degrees
    unsigned long long roots;   // members that are the root of their tree
    int in_max, in_min_inv;     // max in-degree; max of (INT_MAX - in-degree), so that zeroed memory is the neutral element
    int out_hist[kGraphInfoMaxStride]; // members per out-degree
};

// (GI_RELAXED, uf_find and uf_union -- the union-find of the component count -- are dk_union_find.h's)

// ---- the edge pass ----------------------------------------------------------------------------------------------------------
// Thread i handles word i of the layer's lists taken as one flat array of n * stride words: node i / stride, slot i % stride, slot 0
// the count word.  On layer 0 that array IS adj0, read coalesced; above, the node's block of the pool, where it is a member.
// UNION == false, the degree pass: the count word of a member goes into the out-degree histogram (LDS, one atomic per bin and
// block at the end); an entry u -> v with v a member adds one to in_deg[v] (in_deg == nullptr: no in-degrees).
// UNION == true, the component pass: such an entry joins u and v.
// Either way acc->entries counts the entries of members' lists, whatever they point to.  A target that is no member is never
// dereferenced.
template <bool UNION>
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_edge_pass_kernel(LayerView g, int *__restrict__ in_deg_or_parent, GraphAcc *__restrict__ acc)
{
    __shared__ int s_hist[kGraphInfoMaxStride];
    __shared__ unsigned s_entries;
    for (int b = threadIdx.x; b < kGraphInfoMaxStride; b += kGraphInfoBlock) s_hist[b] = 0;
    if (threadIdx.x == 0) s_entries = 0u;
    __syncthreads();
    const int stride = g.stride();
    const long long total = g.n * stride, step = (long long)gridDim.x * kGraphInfoBlock;
    unsigned mine = 0u;
    for (long long i = (long long)blockIdx.x * kGraphInfoBlock + threadIdx.x; i < total; i += step) {
        const long long u = i / stride;
        const int slot = (int)(i - u * stride);
        if (!g.member(u)) continue;
        const int *l = g.list(u);
        if (!l) continue;
        const int cnt = g.count(l);
        if (slot == 0) {
            if (!UNION) atomicAdd(&s_hist[cnt], 1);
            continue;
        }
        if (slot > cnt) continue;
        ++mine;
        const int v = l[slot];
        if (!g.member(v)) continue;
        if (UNION) uf_union(in_deg_or_parent, (int)u, v);
        else if (in_deg_or_parent) (void)__hip_atomic_fetch_add(in_deg_or_parent + v, 1, GI_RELAXED);
    }
    if (mine) atomicAdd(&s_entries, mine);
    __syncthreads();
    if (!UNION)
        for (int b = threadIdx.x; b < kGraphInfoMaxStride; b += kGraphInfoBlock)
            if (s_hist[b]) (void)__hip_atomic_fetch_add(&acc->out_hist[b], s_hist[b], GI_RELAXED);
    if (threadIdx.x == 0 && s_entries) (void)__hip_atomic_fetch_add(&acc->entries, (unsigned long long)s_entries, GI_RELAXED);
}

// ---- in-degrees of the members: max, min and sum; then their histogram with max + 1 bins ------------------------------------
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_indeg_reduce_kernel(LayerView g, const int *__restrict__ in_deg, GraphAcc *__restrict__ acc)
{
    __shared__ int s_max, s_min_inv;
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) { s_max = 0; s_min_inv = 0; s_sum = 0ull; }
    __syncthreads();
    int mx = 0, mn_inv = 0;
    unsigned long long sum = 0ull;
    const long long step = (long long)gridDim.x * kGraphInfoBlock;
    for (long long v = (long long)blockIdx.x * kGraphInfoBlock + threadIdx.x; v < g.n; v += step) {
        if (!g.member(v)) continue;
        const int d = in_deg[v];
        mx = d > mx ? d : mx;
        mn_inv = 0x7fffffff - d > mn_inv ? 0x7fffffff - d : mn_inv;
        sum += (unsigned long long)d;
    }
    if (mn_inv) { atomicMax(&s_max, mx); atomicMax(&s_min_inv, mn_inv); atomicAdd(&s_sum, sum); } // (mn_inv == 0: the thread met no member)
    __syncthreads();
    if (threadIdx.x == 0 && s_min_inv) {
        (void)__hip_atomic_fetch_max(&acc->in_max, s_max, GI_RELAXED);
        (void)__hip_atomic_fetch_max(&acc->in_min_inv, s_min_inv, GI_RELAXED);
        (void)__hip_atomic_fetch_add(&acc->in_sum, s_sum, GI_RELAXED);
    }
}

// hist has `bins` ints (max in-degree + 1); the bins below kGraphInfoLdsBins -- where all but the hubs are -- are counted in LDS first
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_indeg_hist_kernel(LayerView g, const int *__restrict__ in_deg, int *__restrict__ hist, long long bins)
{
    __shared__ int s_hist[kGraphInfoLdsBins];
    const int low = bins < kGraphInfoLdsBins ? (int)bins : kGraphInfoLdsBins;
    for (int b = threadIdx.x; b < low; b += kGraphInfoBlock) s_hist[b] = 0;
    __syncthreads();
    const long long step = (long long)gridDim.x * kGraphInfoBlock;
    for (long long v = (long long)blockIdx.x * kGraphInfoBlock + threadIdx.x; v < g.n; v += step) {
        if (!g.member(v)) continue;
        const int d = in_deg[v];
        if (d < 0 || d >= bins) continue; // (cannot be: bins is the maximum + 1)
        if (d < low) atomicAdd(&s_hist[d], 1);
        else (void)__hip_atomic_fetch_add(hist + d, 1, GI_RELAXED);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < low; b += kGraphInfoBlock)
        if (s_hist[b]) (void)__hip_atomic_fetch_add(hist + b, s_hist[b], GI_RELAXED);
}

// ---- components: every member its own root (others: -1, never read), the edge pass with UNION, then the roots counted --------
__global__ void __launch_bounds__(kGraphInfoBlock)
graph_uf_init_kernel(LayerView g, int *__restrict__ parent)
{
    const long long step = (long long)gridDim.x * kGraphInfoBlock;
    for (long long v = (long long)blockIdx.x * kGraphInfoBlock + threadIdx.x; v < g.n; v += step) parent[v] = g.member(v) ? (int)v : -1;
}

__global__ void __launch_bounds__(kGraphInfoBlock)
graph_uf_roots_kernel(LayerView g, const int *__restrict__ parent, GraphAcc *__restrict__ acc)
{
    __shared__ unsigned s_roots;
    if (threadIdx.x == 0) s_roots = 0u;
    __syncthreads();
    unsigned mine = 0u;
    const long long step = (long long)gridDim.x * kGraphInfoBlock;
    for (long long v = (long long)blockIdx.x * kGraphInfoBlock + threadIdx.x; v < g.n; v += step)
        if (g.member(v) && parent[v] == (int)v) ++mine;
    if (mine) atomicAdd(&s_roots, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_roots) (void)__hip_atomic_fetch_add(&acc->roots, (unsigned long long)s_roots, GI_RELAXED);
}

#undef GI_RELAXED

} // namespace hnsw
