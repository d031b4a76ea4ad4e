// dk_graph_repair.h -- device code of repair_reachability: one round links members of a layer that the entry point
// does not reach (U: hop == -1 after dk_graph_reach.h's BFS) into the lists of reached members.
//   graph_repair_collect_kernel    hop[] -> a bitset of the nodes with hop == -1 (or hop >= 0) and its set bits per block of
//   graph_repair_offsets_kernel    kExactCompactWords words, their exclusive prefix: what exact_compact_kernel (dk_exact.h) turns
//                                  into the ASCENDING id list -- U, and the reached members the flat scan measures
//   gather_rows_kernel             (dk_misc_kernels.h) the stored rows of U as f32 rows in element order: hnswdev_download_rows' values
//   graph_repair_propose_kernel<M> one wave per (u, j): where in the list of v = cand[u][j] the id u could go -- the append
//                                  position, the evictable entry of largest (d(v, w), slot), or -1
// The first two read no rows through a metric and live in device_backend.hip's unit (HNSW_HOST_TU), as gather_rows_kernel does; the proposal kernel measures
// with group_metric, so it is compiled in the exact_<metric> units (exact_unit.hip, HNSW_EXACT_UNIT) and reached through the
// launcher declared here.  Every kernel is an ordinary grid-stride launch of 256-thread blocks; none waits for another wave.
//
// The loops that hold a ballot, a shuffle or group_metric's cross-lane collapse have a WAVE-UNIFORM trip count: they step over the
// wave's first item and no lane `continue`s ahead of them (range_sort_kernel's hang).
#pragma once
#include "dk_layer_view.h"

namespace hnsw {

constexpr int kRepairBlock = 256;
constexpr int kRepairMaxCands = 64;

struct RepairProposeArgs {
    LayerView g;
    const float *rows;      // stored rows (f32 rows, int8 records, f16 records)
    const double *row_sn;   // cosine: sqrt((double)|row|^2)
    int dim;                // what the metric gets as `dim`
    long long n_rows;       // uploaded rows: an id at or beyond it is never measured
    const int *hop;         // this round's hop array (graph_reach_run)
    const int *cand;        // [n_pairs]: pair p = (u index p / C, j = p % C); -1: padding
    long long n_pairs;
    int max_edges;          // MaxEdges(layer), at most stride() - 1
    int *code;              // out [n_pairs]
    unsigned long long *measured; // out: distances measured, added up over the waves
};

template <int METRIC>
hipError_t graph_repair_propose_launch(const RepairProposeArgs &a, unsigned blocks, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_HOST_TU
#include "dk_exact.h"

namespace hnsw {

// ---- thread per node: the selected nodes as a bitset in the allow-sets' format, and how many there are per block of words ------
// unreached: hop == -1 (U), else hop >= 0 (the reached set).  A wave's ballot is two words (its first node is a multiple of 64);
// block_cnt[] (zeroed before the launch) has one int per kExactCompactWords words.
__global__ void __launch_bounds__(kRepairBlock)
graph_repair_collect_kernel(long long n, const int *__restrict__ hop, int unreached, unsigned *__restrict__ bits, int *__restrict__ block_cnt)
{
    const int lane = (int)(threadIdx.x & 63u);
    const long long step = (long long)gridDim.x * kRepairBlock, words = (n + 31) / 32;
    for (long long first = (long long)blockIdx.x * kRepairBlock + (threadIdx.x & ~63u); first < n; first += step) {
        const long long v = first + lane;
        const int h = v < n ? hop[v] : -2;
        const unsigned long long b = __ballot(unreached ? h == -1 : h >= 0);
        const long long w = (first >> 5) + (lane >> 5);
        if ((lane & 31) == 0 && w < words) bits[w] = (unsigned)(b >> (lane & 32));
        if (lane == 0 && b) (void)__hip_atomic_fetch_add(block_cnt + (first >> 5) / kExactCompactWords, __popcll(b), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- one wave: block_off[b] = the counts in front of block b (exact_compact_kernel's block offsets) ----------------------------
// A layer of 1M nodes has 123 blocks: one wave walks them 64 at a time with a shuffle prefix.
__global__ void __launch_bounds__(64)
graph_repair_offsets_kernel(const int *__restrict__ block_cnt, int n_blocks, long long *__restrict__ block_off)
{
    const int lane = (int)threadIdx.x;
    long long base = 0;
    for (int first = 0; first < n_blocks; first += 64) { // (wave-uniform: every lane goes round ceil(n_blocks / 64) times)
        const int b = first + lane;
        const int c = b < n_blocks ? block_cnt[b] : 0;
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (b < n_blocks) block_off[b] = base + (incl - c);
        base += __shfl(incl, 63, 64);
    }
}

} // namespace hnsw
#endif // HNSW_HOST_TU

#ifdef HNSW_EXACT_UNIT
#include "dk_base.h"
#include "dk_metric.h"

namespace hnsw {

// One wave per pair p: v = cand[p].  count(v) < max_edges: the code is count(v) (an append).  Otherwise entry s (0-based) with
// target w is EVICTABLE iff w is a member with 0 <= hop[w] <= hop[v]; a target that is no member is not dereferenced beyond the
// member test.  Lane l of pass t looks at entry 64 t + l; the evictable entries are then measured eight at a time, an 8-lane group
// each (group_metric on the rows of v and w: pair_distance_kernel's bits), a group without an entry shadowing the pair (v, v) and
// discarding it.  The wave keeps the largest (distance, slot) by the float compare -- a NaN distance is not evictable -- and lane
// 0 writes the slot, or -1.
template <int METRIC>
__global__ void __launch_bounds__(kRepairBlock)
graph_repair_propose_kernel(RepairProposeArgs a)
{
    const LayerView &g = a.g;
    const int lane = (int)(threadIdx.x & 63u), grp = lane >> 3, j = lane & 7;
    const long long waves = (long long)gridDim.x * (kRepairBlock / 64);
    unsigned measured = 0u; // the wave's, the same in every lane
    for (long long p = (long long)blockIdx.x * (kRepairBlock / 64) + (threadIdx.x >> 6); p < a.n_pairs; p += waves) { // (p is the wave's: uniform)
        const int v = __builtin_amdgcn_readfirstlane(a.cand[p]);
        int code = -1;
        const bool ok = v >= 0 && (long long)v < a.n_rows && g.member(v);
        const int *l = ok ? g.list(v) : nullptr;
        if (l) {
            const int cnt = g.count(l);
            if (cnt < a.max_edges) code = cnt;
            else {
                const int hv = a.hop[v];
                const double sv = METRIC == M_COS ? a.row_sn[v] : 0.0;
                const float *rv = row_at<METRIC>(a.rows, (size_t)v, a.dim);
                float best_d = 0.0f;
                int best_s = -1;
                for (int s0 = 0; s0 < cnt; s0 += 64) { // cnt is the wave's: uniform
                    const int s = s0 + lane;
                    int w = -1;
                    bool ev = false;
                    if (s < cnt) {
                        w = l[1 + s];
                        if ((long long)w < a.n_rows && g.member(w)) {
                            const int hw = a.hop[w];
                            ev = hw >= 0 && hw <= hv;
                        }
                    }
                    const unsigned long long evb = __ballot(ev);
                    for (int t = 0; t < 8; ++t) {
                        if ((evb >> (8 * t)) & 0xffull) { // (the wave's ballot: every lane takes the same side)
                            const int src = 8 * t + grp;
                            const int wt = __shfl(w, src, 64);
                            const bool act = (evb >> src) & 1ull;
                            const int id = act ? wt : v;
                            const double sw = METRIC == M_COS ? a.row_sn[id] : 0.0;
                            const float d = group_metric<METRIC>(rv, row_at<METRIC>(a.rows, (size_t)id, a.dim), a.dim, j, sv, sw);
                            const int st = s0 + src;
                            if (act && j == 0 && d == d && (best_s < 0 || d > best_d || (d == best_d && st > best_s))) { best_d = d; best_s = st; }
                        }
                    }
                    measured += (unsigned)__popcll(evb);
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) { // (every lane of the wave is here)
                    const float od = __shfl_xor(best_d, o, 64);
                    const int os = __shfl_xor(best_s, o, 64);
                    if (os >= 0 && (best_s < 0 || od > best_d || (od == best_d && os > best_s))) { best_d = od; best_s = os; }
                }
                code = best_s;
            }
        }
        if (lane == 0) a.code[p] = code;
    }
    if (lane == 0 && measured) (void)__hip_atomic_fetch_add(a.measured, (unsigned long long)measured, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int METRIC>
hipError_t graph_repair_propose_launch(const RepairProposeArgs &a, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL(graph_repair_propose_kernel<METRIC>, dim3(blocks), dim3(kRepairBlock), 0, st, a);
    return hipGetLastError();
}

} // namespace hnsw
#endif // HNSW_EXACT_UNIT
