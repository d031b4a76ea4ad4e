// dk_edge_groups.h -- device code of the near-duplicate calls over the graph's edges: graph_edge_kernel measures,
// for every OWNER of a round, the layer-0 neighbours that are members and hands those within the radius to a sink -- a union-find
// (EdgeUnion: graph_duplicate_groups) or the owner's segment of a key arena (EdgeList: near_edges).  No traversal: no visited set,
// no descent, no atomic besides the job claim and what the union-find needs.  Included by device_backend.hip alone (HNSW_HOST_TU),
// as graph_range_kernel is: twelve instantiations, launched from one place.
#pragma once
#include "dk_search_common.h"
#include "dk_union_find.h"

namespace hnsw {

#ifdef HNSW_HOST_TU

// The sink of graph_duplicate_groups: every within-edge is a union; totals[0] += the job's within-edges, totals[1] += its measured ones.
struct EdgeUnion {
    int *parent;
    unsigned long long *totals;
    static constexpr bool kList = false;
};
// The sink of near_edges: job j's within-edges go to keys[j * seg, ...) as (distance bits << 32 | id), ascending by (distance, id)
// with -0 == +0 -- the order of exact_range_query_by_id's list -- and counts[j] is their number.  seg >= the longest list: the
// segments are disjoint, so nothing is claimed.
struct EdgeList {
    unsigned long long *keys;
    int *counts;
    int seg;
    static constexpr bool kList = true;
};

// Persistent, one wave per block, jobs from a counter (claim_job).  Job j: the owner owners[j], whose gathered row is query j of
// `queries` (stage_query).  The owner's layer-0 list is read once; the entries that `members` holds are compacted into nbuf in list
// order (a ballot per 64 entries: lists of MaxEdges > 32 have up to 2 MaxEdges), measured by measure_all -- the metric's own bits,
// the owner's row as the query -- and those with d <= range (the float compare: NaN admits nothing) go to the sink.  nbcap >=
// stride0 - 1.  A list length outside [0, stride0) is read as clamped, an id below 0 as no member: no row outside the members'
// is ever touched.  (no `continue` behind a lane-0 branch; lane 0's stores stand at the end of the body.)
template <int METRIC, class Sink>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3)))
graph_edge_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                  const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0, const int *__restrict__ owners,
                  const AllowSet members, float range, const Sink sink, int nbcap, int njobs, int *__restrict__ job_counter)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    const SearchLds L = carve_lds(smem, 0, 0, dim, nbcap);
    int *nbuf = L.nbuf;
    float *dbuf = L.dbuf;
    for (;;) {
        int job;
        if (!claim_job(job_counter, njobs, lane, job)) break;
        const int owner = __builtin_amdgcn_readfirstlane(owners[job]);
        const double sb = stage_query<METRIC>(queries, q_sn, job, dim, L, lane);
        const int *l = adj0 + (size_t)owner * stride0;
        const int n = min(max(__builtin_amdgcn_readfirstlane(l[0]), 0), min(stride0 - 1, nbcap));
        int m = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int x = 0;
            bool in = false;
            if (i < n) {
                x = l[1 + i];
                in = x >= 0 && members.has(x);
            }
            const unsigned long long mk = __ballot(in);
            const int pp = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0));
            if (in) nbuf[m + pp] = x;
            m += __popcll(mk);
        }
        wave_sync();
        if (m > 0) measure_all<METRIC>(rows, row_sn, dim, L.qs, sb, nbuf, dbuf, m, lane);
        wave_sync();
        int within = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            const float di = i < m ? dbuf[i] : 0.0f;
            const int xi = i < m ? nbuf[i] : 0;
            const bool in = i < m && di <= range;
            if constexpr (Sink::kList) {
                // the counting rank of range_sort_kernel on (distance, id, place): every lane reads entry j at once (an LDS broadcast)
                int below = 0;
                for (int j = 0; j < m; ++j) {
                    const float dj = dbuf[j];
                    const int xj = nbuf[j];
                    below += (dj <= range && (dj < di || (dj == di && (xj < xi || (xj == xi && j < i))))) ? 1 : 0;
                }
                if (in) sink.keys[(size_t)job * (size_t)sink.seg + (size_t)below] = ((unsigned long long)__float_as_uint(di) << 32) | (unsigned)xi;
            } else {
                if (in) uf_union(sink.parent, owner, xi);
            }
            within += __popcll(__ballot(in));
        }
        if (lane == 0) {
            if constexpr (Sink::kList) sink.counts[job] = within;
            else {
                if (within) atomicAdd(sink.totals, (unsigned long long)within);
                atomicAdd(sink.totals + 1, (unsigned long long)m);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

#endif // HNSW_HOST_TU

} // namespace hnsw
