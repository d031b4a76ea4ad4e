// dk_mreach_tree.h -- the minimum spanning forest of the members under the MUTUAL REACHABILITY distance: HDBSCAN*'s
// tree, by the Boruvka rounds of dk_span_tree.h with another scan.  core[v] is the distance from member v to its (min_samples - 1)-th
// nearest other member, kept as exact_key's 32-bit distance key; the weight of members a < b whose distance d -- the stored row of a
// as the query, span_scan_kernel's bits -- is a number is max(K(d), core[a], core[b]) in key space, which is monotone, so the maximum
// of the keys is the key of the maximum.  Edges are ordered by (weight key, a, b): a strict total order, a unique forest.
//   mreach_scan_kernel<M>   span_scan_kernel's blocks, tiles, component tests and measuring core; behind the collapse every lane of a
//                           group holds the 16 distances of its register tile, and the 16 offers are spread over the eight lanes:
//                           lane j takes query (j & 3) against rows 2 (j >> 2) and 2 (j >> 2) + 1.  The query side is completed by one
//                           exchange with lane j ^ 4, the row side by two inside the quad (DPP, no LDS), in front of the one LDS /
//                           global 64-bit minimum.
//   mreach_core_fill_kernel core[id] = one key for the m ids of the list (min_samples == 1: the key of -inf, below every distance)
//   mreach_core_take_kernel core[self[i]] = the key of column k - 1 of row i of a top-k result; padding and NaN read +inf
// The round kernels are dk_span_tree.h's, unchanged: they only see keys.  mreach_scan_kernel is instantiated per metric in
// exact_unit.hip through mreach_scan_launch<kUnitMetric>; the two core kernels live with the metric-free ones (HNSW_EXACT_COMMON).
#pragma once
#include "dk_span_tree.h"

namespace hnsw {

struct MreachScanArgs {
    const int *label;              // [every id of the list]: its component -- the component's smallest id
    unsigned long long *best;      // [every id of the list]: the smallest (weight key << 32 | other id) offered in this round
    const int *seg_label;          // [ceil(m / kExactIterRows)]: span_reset_kernel's
    const unsigned *core;          // [every id of the list]: its core distance as exact_key's 32-bit distance key
    long long q_off;               // query q of the launch is entry q_off + q of the id list (ExactScanArgs::ids)
    unsigned long long *skipped;   // out: pairs of the triangle not measured, both ends in one component, added up over the blocks
};

// LDS of one block: the staged query words (exact_scan_lds' first part), then per query slot of the tile a 64-bit minimum, the
// query's label, its id and its core key, then the block's two pair counters
inline size_t mreach_scan_lds(int qtile, int piece, int dim)
{
    const size_t qtr = (size_t)((qtile + kExactRQ - 1) / kExactRQ * kExactRQ), qw = (size_t)(piece < dim ? piece : dim);
    return ((qtr * qw * 4 + 15) & ~(size_t)15) + qtr * (8 + 4 + 4 + 4) + 8;
}

// One launch of mreach_scan_kernel<METRIC>: n_blocks x a.n_chunks blocks; the arguments as span_scan_launch's.
template <int METRIC>
hipError_t mreach_scan_launch(const ExactScanArgs &a, const MreachScanArgs &s, unsigned n_blocks, size_t lds, hipStream_t st);
// core[ids[i]] = exact_key's distance key of d, i < m
hipError_t mreach_core_fill_launch(const int *ids, long long m, float d, unsigned *core, hipStream_t st);
// core[self[i]] = the distance key of dists[i * k + k - 1], +inf's where that is NaN (padding is), i < nq
hipError_t mreach_core_take_launch(const float *dists, int nq, int k, const int *self, unsigned *core, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT
namespace hnsw {

// A 64-bit word of lane ^ 1, ^ 2 (quad permutations) or ^ 4 (row_shl:4 for the lower half of an 8-lane group, row_shr:4 for the upper:
// lane_xor_add's moves, dk_metric.h) -- two DPP moves per half word, no LDS crossbar.  Every lane of the group is active where these
// are called: the branches around them are taken by whole groups.
template <int MASK>
__device__ __forceinline__ int mreach_lane_xor(int x)
{
    if constexpr (MASK == 1) return __builtin_amdgcn_mov_dpp(x, 0xB1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, true);
    else if constexpr (MASK == 2) return __builtin_amdgcn_mov_dpp(x, 0x4E /* quad_perm:[2,3,0,1] */, 0xf, 0xf, true);
    else {
        static_assert(MASK == 4, "mreach_lane_xor: 1, 2 or 4");
        int o = __builtin_amdgcn_update_dpp(0, x, 0x104 /* row_shl:4 */, 0xf, 0x5, false);
        return __builtin_amdgcn_update_dpp(o, x, 0x114 /* row_shr:4 */, 0xf, 0xa, false);
    }
}
template <int MASK>
__device__ __forceinline__ unsigned long long mreach_min_xor(unsigned long long v)
{
    const unsigned lo = (unsigned)mreach_lane_xor<MASK>((int)(unsigned)v), hi = (unsigned)mreach_lane_xor<MASK>((int)(unsigned)(v >> 32));
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    return o < v ? o : v;
}

// Resources (gfx950, profiles/mreach_tree_kernel_resources.json): span_scan_kernel's split -- 256 threads as 32 groups of 8 lanes, a
// 4 x 4 register tile per group, the tile's queries staged in LDS in pieces -- because the measuring core fixes the distance bits.
// Around it: the tile's core keys in LDS beside label and id, the lane's two rows' core keys in registers, and the offers on all
// eight lanes.
template <int METRIC>
__global__ void __launch_bounds__(kExactThreads) mreach_scan_kernel(const ExactScanArgs a, const MreachScanArgs s)
{
    constexpr int RQ = kExactRQ, RR = kExactRR;
    static_assert(RQ == 4 && RR == 4, "lane j offers query (j & 3) against rows 2 (j >> 2) and 2 (j >> 2) + 1");
    extern __shared__ __align__(16) unsigned char mreach_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 3, j = tid & 7;
    const int dim = a.dim, QT = a.qtile, QTR = (QT + RQ - 1) / RQ * RQ;
    const int P = a.piece, qw = P < dim ? P : dim, npieces = (dim + P - 1) / P;
    float *qs = reinterpret_cast<float *>(mreach_lds);
    unsigned long long *qbest = reinterpret_cast<unsigned long long *>(mreach_lds + (((size_t)QTR * qw * 4 + 15) & ~(size_t)15));
    int *qlab = reinterpret_cast<int *>(qbest + QTR);
    int *qself = qlab + QTR;
    unsigned *qcore = reinterpret_cast<unsigned *>(qself + QTR);
    unsigned *cnt = qcore + QTR; // [0] the block's pairs measured, [1] skipped
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT; // the tile's queries: at least one (the grid has no empty tile)
    const int *self = a.ids + s.q_off;
    // nothing to measure where the chunk's last id is not above the tile's first query id (both ascend): the whole block leaves, in
    // front of its first barrier
    if (__builtin_amdgcn_readfirstlane(a.ids[hi - 1]) <= __builtin_amdgcn_readfirstlane(self[q0])) return;
    const int rw = row_words<METRIC>(dim);
    const int nblk = dim >> 3;
    const int jq = j & 3;       // this lane's query of a register tile
    const bool up = j >= 4;     // ... and its rows: 2 and 3 of the group's four, else 0 and 1

    if (tid < QTR) { // past the tile's last query a slot shadows it
        const int v = self[q0 + (tid < nqt ? tid : nqt - 1)];
        qself[tid] = v;
        qlab[tid] = s.label[v];
        qcore[tid] = s.core[v];
        qbest[tid] = kExactEmpty;
    }
    if (tid < 2) cnt[tid] = 0u;
    __syncthreads();
    // the tile's one label, -1 where its queries lie in several components (labels are ids: never negative)
    int tlab = qlab[0];
    for (int i = 1; i < nqt; ++i) tlab = qlab[i] == tlab ? tlab : -1;
    tlab = __builtin_amdgcn_readfirstlane(tlab);

    unsigned measured = 0, skipped = 0; // every lane: its own pairs of the mixed steps; thread q < nqt also: query q's pairs of the skipped steps
    bool staged = false;
    for (long long base = lo; base < hi; base += kExactIterRows) {
        const long long end = base + kExactIterRows < hi ? base + kExactIterRows : hi;
        // a step whose rows all carry the tile's label is not read at all (the test is the same for the whole block: two scalar loads).
        // Its pairs above the diagonal: query q is entry q_off + q0 + q of the list, and the entries behind it are the ids above it.
        bool same = false;
        if (tlab >= 0)
            same = __builtin_amdgcn_readfirstlane(s.seg_label[base / kExactIterRows]) == tlab &&
                   __builtin_amdgcn_readfirstlane(s.seg_label[(end - 1) / kExactIterRows]) == tlab;
        if (same) {
            if (tid < nqt) {
                const long long from = s.q_off + q0 + tid + 1 > base ? s.q_off + q0 + tid + 1 : base;
                if (end > from) skipped += (unsigned)(end - from);
            }
            continue; // (block-uniform: no lane goes on alone)
        }
        // this group's rows; past the chunk's end a group shadows the chunk's last row and discards
        int rid[RR], rlab[RR];
        bool rvalid[RR];
        const float *rp[RR];
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            long long idx = base + grp * RR + r;
            rvalid[r] = idx < hi;
            if (!rvalid[r]) idx = hi - 1;
            rid[r] = a.ids[idx];
            rp[r] = a.rows + (size_t)rid[r] * (size_t)rw;
            rlab[r] = s.label[rid[r]];
        }
        const bool rows_one = rlab[0] == rlab[1] && rlab[1] == rlab[2] && rlab[2] == rlab[3];
        // the lane's own two rows, for the offers: id, label, core key, and the row side's minimum over all the tile's queries
        int mrid[2], mrlab[2];
        bool mrvalid[2];
        unsigned mrcore[2];
        unsigned long long rbest[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            mrid[t] = up ? rid[2 + t] : rid[t];
            mrlab[t] = up ? rlab[2 + t] : rlab[t];
            mrvalid[t] = up ? rvalid[2 + t] : rvalid[t];
            mrcore[t] = s.core[mrid[t]];
            rbest[t] = kExactEmpty;
        }
        for (int qsub = 0; qsub < nqt; qsub += RQ) {
            int ql[RQ], qv0 = qself[qsub];
#pragma unroll
            for (int q = 0; q < RQ; ++q) ql[q] = qlab[qsub + q];
            // the register tile is not measured where its 16 pairs share a label, or where all of them lie on or below the diagonal
            // (rows and queries ascend).  The same in the eight lanes of a group; the staging barriers below stand outside it.
            const bool tile_skip = (rows_one && ql[0] == rlab[0] && ql[1] == rlab[0] && ql[2] == rlab[0] && ql[3] == rlab[0]) || rid[RR - 1] <= qv0;
            float acc[RQ][RR];
            int iacc[RQ][RR], ta[RR], tb[RQ];
            float dist[RQ][RR];
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
                tb[q] = 0;
#pragma unroll
                for (int r = 0; r < RR; ++r) { acc[q][r] = 0.0f; iacc[q][r] = 0; ta[r] = 0; dist[q][r] = 0.0f; }
            }
            for (int p = 0; p < npieces; ++p) {
                const int w0 = p * P, w1 = w0 + P < dim ? w0 + P : dim, len = w1 - w0;
                if (npieces > 1 || !staged) { // the queries of the tile, words [w0, w1); past the last query a slot shadows it
                    __syncthreads();
                    for (int qi = wave; qi < QTR; qi += kExactThreads / 64) {
                        const long long src = q0 + (qi < nqt ? qi : nqt - 1);
                        const float *g = a.queries + (size_t)src * dim + w0;
                        for (int o = lane; o < len; o += 64) qs[(size_t)qi * qw + o] = g[o];
                    }
                    __syncthreads();
                    staged = true;
                }
                if (!tile_skip) {
                    const int s0 = w0 >> 3, s1 = w1 >> 3; // the 8-element steps of this piece (P is a multiple of 16)
                    const float *qb = qs + (size_t)qsub * qw + j;
                    if constexpr (METRIC == M_I8) {
                        const int *qi8 = reinterpret_cast<const int *>(qb);
#pragma unroll 2
                        for (int e = s0; e < s1; ++e) {
                            int wa[RR], wb[RQ];
#pragma unroll
                            for (int r = 0; r < RR; ++r) wa[r] = reinterpret_cast<const int *>(rp[r])[8 * e + j];
#pragma unroll
                            for (int q = 0; q < RQ; ++q) wb[q] = qi8[q * qw + 8 * (e - s0)];
                            if (e == nblk - 1 && j >= 6) { // the record's scale / sumsq words
#pragma unroll
                                for (int r = 0; r < RR; ++r) ta[r] = wa[r];
#pragma unroll
                                for (int q = 0; q < RQ; ++q) tb[q] = wb[q];
                            } else {
#pragma unroll
                                for (int q = 0; q < RQ; ++q)
#pragma unroll
                                    for (int r = 0; r < RR; ++r) iacc[q][r] = dot4_i8(wa[r], wb[q], iacc[q][r]);
                            }
                        }
                    } else if constexpr (metric_f16(METRIC)) {
                        for (int e = s0; e < s1; e += 2) { // one record word holds this lane's element of two consecutive steps
                            unsigned w[RR];
#pragma unroll
                            for (int r = 0; r < RR; ++r) w[r] = reinterpret_cast<const unsigned *>(rp[r])[8 * (e >> 1) + j];
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                if (e + h < s1) {
                                    float y[RQ];
#pragma unroll
                                    for (int q = 0; q < RQ; ++q) y[q] = qb[q * qw + 8 * (e + h - s0)];
#pragma unroll
                                    for (int r = 0; r < RR; ++r) {
                                        const float x = h ? half_hi(w[r]) : half_lo(w[r]);
#pragma unroll
                                        for (int q = 0; q < RQ; ++q) {
                                            if (metric_is_sq(METRIC)) { const float d = x - y[q]; acc[q][r] = __builtin_fmaf(d, d, acc[q][r]); }
                                            else { const float m = x * y[q]; acc[q][r] = acc[q][r] + m; }
                                        }
                                    }
                                }
                            }
                        }
                    } else {
#pragma unroll 2
                        for (int e = s0; e < s1; ++e) {
                            float x[RR], y[RQ];
#pragma unroll
                            for (int r = 0; r < RR; ++r) x[r] = rp[r][8 * e + j];
#pragma unroll
                            for (int q = 0; q < RQ; ++q) y[q] = qb[q * qw + 8 * (e - s0)];
#pragma unroll
                            for (int q = 0; q < RQ; ++q)
#pragma unroll
                                for (int r = 0; r < RR; ++r) {
                                    if (metric_is_sq(METRIC)) { const float d = x[r] - y[q]; acc[q][r] = __builtin_fmaf(d, d, acc[q][r]); }
                                    else { const float m = x[r] * y[q]; acc[q][r] = acc[q][r] + m; }
                                }
                        }
                    }
                    if (p == npieces - 1) { // the last piece holds the tail elements: collapse, scalar tail, epilogue (group_metric's, pair by pair)
                        if constexpr (METRIC == M_I8) {
                            const int g6 = (lane & ~7) | 6, g7 = (lane & ~7) | 7;
                            float sb[RQ];
                            int nb[RQ];
#pragma unroll
                            for (int q = 0; q < RQ; ++q) { sb[q] = __int_as_float(__shfl(tb[q], g6, 64)); nb[q] = __shfl(tb[q], g7, 64); }
#pragma unroll
                            for (int r = 0; r < RR; ++r) {
                                const float sa = __int_as_float(__shfl(ta[r], g6, 64));
                                const int na = __shfl(ta[r], g7, 64);
#pragma unroll
                                for (int q = 0; q < RQ; ++q) dist[q][r] = i8_epilogue(sa, na, sb[q], nb[q], group_sum_i32(iacc[q][r]));
                            }
                        } else {
#pragma unroll
                            for (int q = 0; q < RQ; ++q) {
                                double sqn = 0.0;
                                if constexpr (METRIC == M_COS) sqn = a.q_sn[q0 + (qsub + q < nqt ? qsub + q : nqt - 1)];
#pragma unroll
                                for (int r = 0; r < RR; ++r) {
                                    float t = metric_is_sq(METRIC) ? collapse_l2(acc[q][r]) : collapse_cos(acc[q][r]);
                                    for (int i = dim & ~7; i < dim; ++i) { // every lane redundantly; mul then add, no fma
                                        const float x = row_elem<METRIC>(rp[r], i), y = qs[(size_t)(qsub + q) * qw + (i - w0)];
                                        if (metric_is_sq(METRIC)) { const float d = x - y; const float m = d * d; t = t + m; }
                                        else { const float m = x * y; t = t + m; }
                                    }
                                    if (metric_is_sq(METRIC)) dist[q][r] = t;
                                    else if (metric_is_ucos(METRIC)) dist[q][r] = 1.0f - t;
                                    else {
                                        const float denom = (float)(a.row_sn[rid[r]] * sqn);
                                        dist[q][r] = denom < 1e-30f ? 1.0f : 1.0f - t / denom;
                                    }
                                }
                            }
                        }
                    }
                }
            }
            // The offers, on all eight lanes: every lane holds the tile's 16 distances (the collapses and the int8 sums leave their
            // result in every lane of the group) and takes two of the pairs -- its query (j & 3) against its two rows.  A pair above
            // the diagonal is skipped where its ends share a label and measured otherwise; a distance that is a number offers its
            // weight, the largest of three keys, to both ends.  tile_skip is the group's, so the lanes of a group stay together
            // through the DPP exchanges; the tests on a pair are selects, not branches.
            const int qi = qsub + jq;
            const int mqv = qself[qi];
            const bool qok = qi < nqt;
            if (tile_skip) {
#pragma unroll
                for (int t = 0; t < 2; ++t) skipped += (unsigned)(qok && mrvalid[t] && mrid[t] > mqv);
            } else {
                const int mql = qlab[qi];
                const unsigned mqc = qcore[qi];
                float half[RQ][2]; // the lane's rows of every query, then its query's
#pragma unroll
                for (int q = 0; q < RQ; ++q)
#pragma unroll
                    for (int t = 0; t < 2; ++t) half[q][t] = up ? dist[q][2 + t] : dist[q][t];
                unsigned long long kq = kExactEmpty, kr[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float d = jq == 0 ? half[0][t] : jq == 1 ? half[1][t] : jq == 2 ? half[2][t] : half[3][t];
                    const bool above = qok && mrvalid[t] && mrid[t] > mqv, apart = mrlab[t] != mql;
                    skipped += (unsigned)(above && !apart);
                    measured += (unsigned)(above && apart);
                    const unsigned dk = (unsigned)(exact_key(d, 0) >> 32);
                    unsigned wk = dk > mqc ? dk : mqc;
                    wk = wk > mrcore[t] ? wk : mrcore[t];
                    const bool edge = above && apart && d == d;
                    const unsigned long long kc = edge ? ((unsigned long long)wk << 32) | (unsigned)mrid[t] : kExactEmpty;
                    kr[t] = edge ? ((unsigned long long)wk << 32) | (unsigned)mqv : kExactEmpty;
                    kq = kc < kq ? kc : kq;
                }
                // the query side: lanes j and j ^ 4 hold the same query; then a 64-bit LDS min where a plain read says it is smaller
                kq = mreach_min_xor<4>(kq);
                if (j < 4 && kq < qbest[qi]) (void)__hip_atomic_fetch_min(&qbest[qi], kq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                // the row side: the four lanes of a quad hold the same two rows and the tile's four queries
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const unsigned long long k = mreach_min_xor<2>(mreach_min_xor<1>(kr[t]));
                    rbest[t] = k < rbest[t] ? k : rbest[t];
                }
            }
        }
        // the row side leaves from the first lane of each quad: at most one global atomic per row and step, and only where a plain
        // load says the offer is smaller
        if (jq == 0) {
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (rbest[t] != kExactEmpty && rbest[t] < __hip_atomic_load(s.best + mrid[t], GI_RELAXED)) (void)__hip_atomic_fetch_min(s.best + mrid[t], rbest[t], GI_RELAXED);
        }
    }
    if (measured) (void)__hip_atomic_fetch_add(&cnt[0], measured, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (skipped) (void)__hip_atomic_fetch_add(&cnt[1], skipped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads(); // the LDS minima and the two counters are complete
    if (tid == 0 && cnt[0]) atomicAdd(a.evals, (unsigned long long)cnt[0]);
    if (tid == 1 && cnt[1]) atomicAdd(s.skipped, (unsigned long long)cnt[1]);
    if (tid < nqt) { // the query side leaves: one global atomic per query and block at the most
        const unsigned long long k = qbest[tid];
        unsigned long long *dst = s.best + qself[tid];
        if (k != kExactEmpty && k < __hip_atomic_load(dst, GI_RELAXED)) (void)__hip_atomic_fetch_min(dst, k, GI_RELAXED);
    }
}

template <int METRIC>
hipError_t mreach_scan_launch(const ExactScanArgs &a, const MreachScanArgs &s, unsigned n_blocks, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((mreach_scan_kernel<METRIC>), dim3(n_blocks, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, s);
    return hipGetLastError();
}

#ifdef HNSW_EXACT_COMMON
// ---- the core keys: metric-free, grid-stride ----
__global__ void __launch_bounds__(256) mreach_core_fill_kernel(const int *__restrict__ ids, long long m, float d, unsigned *__restrict__ core)
{
    const long long step = (long long)gridDim.x * 256;
    const unsigned dk = (unsigned)(exact_key(d, 0) >> 32);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) core[ids[i]] = dk;
}
__global__ void __launch_bounds__(256) mreach_core_take_kernel(const float *__restrict__ dists, int nq, int k, const int *__restrict__ self, unsigned *__restrict__ core)
{
    const int step = (int)gridDim.x * 256;
    for (int i = (int)blockIdx.x * 256 + (int)threadIdx.x; i < nq; i += step) {
        const float d = dists[(size_t)i * (size_t)k + (size_t)(k - 1)];
        core[self[i]] = (unsigned)(exact_key(d == d ? d : __builtin_inff(), 0) >> 32);
    }
}
hipError_t mreach_core_fill_launch(const int *ids, long long m, float d, unsigned *core, hipStream_t st)
{
    hipLaunchKernelGGL(mreach_core_fill_kernel, dim3(exact_union_blocks(m)), dim3(256), 0, st, ids, m, d, core);
    return hipGetLastError();
}
hipError_t mreach_core_take_launch(const float *dists, int nq, int k, const int *self, unsigned *core, hipStream_t st)
{
    hipLaunchKernelGGL(mreach_core_take_kernel, dim3(exact_union_blocks(nq)), dim3(256), 0, st, dists, nq, k, self, core);
    return hipGetLastError();
}
#endif // HNSW_EXACT_COMMON

} // namespace hnsw
#endif // HNSW_EXACT_UNIT
