// dk_span_tree.h -- the minimum spanning forest of the members under the metric: Boruvka's rounds over the triangle
// that ExactRangeUnion scans once (dk_exact.h).  An edge is a pair of members a < b whose distance, the stored row of a as the query,
// is a number; edges are ordered by (exact_key's distance key, a, b), a strict total order, so the forest is unique.
//   span_scan_kernel<M>     a tile of queries x a chunk of the member list per block: every pair (self, rid), rid > self, whose ends
//                           lie in different components is measured with the metric's own arithmetic (exact_scan_kernel's: the bits
//                           are exact_range_query_by_id's) and offers exact_key(d, rid) to best[self] and exact_key(d, self) to
//                           best[rid] -- 64-bit minima.  It is no sink of exact_scan_kernel: it keeps no list and stages no key.
//   span_reset_kernel       before a round's scans: best[] = kExactEmpty, comp_w[] / comp_edge[] = all ones for the members, and
//                           seg_label[s] = the label of the s-th kExactIterRows entries of the member list where they share one, else -1
//   span_weight_kernel      every member with a key: its 32-bit distance key -> comp_w[label] (min)
//   span_edge_kernel        every member whose distance key is its component's: (lo << 32 | hi) -> comp_edge[label] (min)
//   span_join_kernel        every root with an edge: uf_union(lo, hi), and the edge appended unless the other component chose it too
//                           and has the smaller label
// The metric-free kernels live in the unit that holds density_*_kernel (HNSW_EXACT_COMMON); span_scan_kernel is instantiated per
// metric in exact_unit.hip through span_scan_launch<kUnitMetric>.
#pragma once
#include "dk_exact.h"

namespace hnsw {

struct SpanScanArgs {
    const int *label;              // [every id of the list]: its component -- the component's smallest id
    unsigned long long *best;      // [every id of the list]: the smallest exact_key(distance, other id) offered in this round
    const int *seg_label;          // [ceil(m / kExactIterRows)]: span_reset_kernel's
    long long q_off;               // query q of the launch is entry q_off + q of the id list (ExactScanArgs::ids)
    unsigned long long *skipped;   // out: pairs of the triangle not measured, both ends in one component, added up over the blocks
};
struct alignas(16) SpanEdge { int a, b; unsigned dkey, zero; }; // a < b, the distance as exact_key's 32-bit key: one vector store

// LDS of one block: the staged query words (exact_scan_lds' first part), then per query slot of the tile a 64-bit minimum, the
// query's label and its id
inline size_t span_scan_lds(int qtile, int piece, int dim)
{
    const size_t qtr = (size_t)((qtile + kExactRQ - 1) / kExactRQ * kExactRQ), qw = (size_t)(piece < dim ? piece : dim);
    return ((qtr * qw * 4 + 15) & ~(size_t)15) + qtr * (8 + 4 + 4);
}

// One launch of span_scan_kernel<METRIC>: n_blocks x a.n_chunks blocks.  a.ids is the member list (never nullptr), a.queries the
// gathered rows of its entries [s.q_off, s.q_off + a.nq); a.k / a.lists are not read; a.evals counts the pairs measured.
template <int METRIC>
hipError_t span_scan_launch(const ExactScanArgs &a, const SpanScanArgs &s, unsigned n_blocks, size_t lds, hipStream_t st);
hipError_t span_reset_launch(const int *ids, long long m, const int *label, unsigned long long *best, unsigned *comp_w, unsigned long long *comp_edge,
                             int *seg_label, hipStream_t st);
// the three kernels behind a round's scans, in order; *cursor counts the edges of edges[0, cap) written so far
hipError_t span_join_launch(const int *ids, long long m, const int *label, const unsigned long long *best, unsigned *comp_w, unsigned long long *comp_edge,
                            int *parent, SpanEdge *edges, unsigned long long cap, unsigned long long *cursor, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT
namespace hnsw {

// Resources (gfx950, profiles/span_tree_kernel_resources.json): the split is exact_scan_kernel's -- 256 threads as 32 groups of 8
// lanes, a 4 x 4 register tile per group, the tile's queries staged in LDS in pieces -- because the measuring core is what fixes the
// registers, and the union sink it is closest to already sits at 4 waves per SIMD on float rows.  What is new sits around the core:
// two label tests in front of it and two minima behind it.
template <int METRIC>
__global__ void __launch_bounds__(kExactThreads) span_scan_kernel(const ExactScanArgs a, const SpanScanArgs s)
{
    constexpr int RQ = kExactRQ, RR = kExactRR;
    extern __shared__ __align__(16) unsigned char span_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 3, j = tid & 7;
    const int dim = a.dim, QT = a.qtile, QTR = (QT + RQ - 1) / RQ * RQ;
    const int P = a.piece, qw = P < dim ? P : dim, npieces = (dim + P - 1) / P;
    float *qs = reinterpret_cast<float *>(span_lds);
    unsigned long long *qbest = reinterpret_cast<unsigned long long *>(span_lds + (((size_t)QTR * qw * 4 + 15) & ~(size_t)15));
    int *qlab = reinterpret_cast<int *>(qbest + QTR);
    int *qself = qlab + QTR;
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT; // the tile's queries: at least one (the grid has no empty tile)
    const int *self = a.ids + s.q_off;
    // nothing to measure where the chunk's last id is not above the tile's first query id (both ascend): the whole block leaves, in
    // front of its first barrier
    if (__builtin_amdgcn_readfirstlane(a.ids[hi - 1]) <= __builtin_amdgcn_readfirstlane(self[q0])) return;
    const int rw = row_words<METRIC>(dim);
    const int nblk = dim >> 3;

    if (tid < QTR) { // past the tile's last query a slot shadows it
        const int v = self[q0 + (tid < nqt ? tid : nqt - 1)];
        qself[tid] = v;
        qlab[tid] = s.label[v];
        qbest[tid] = kExactEmpty;
    }
    __syncthreads();
    // the tile's one label, -1 where its queries lie in several components (labels are ids: never negative)
    int tlab = qlab[0];
    for (int i = 1; i < nqt; ++i) tlab = qlab[i] == tlab ? tlab : -1;
    tlab = __builtin_amdgcn_readfirstlane(tlab);

    unsigned measured = 0, skipped = 0; // lane 0 of a group: its pairs of the mixed steps; thread q < nqt: query q's pairs of the skipped steps
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
        unsigned long long rbest[RR]; // the row side: the smallest key over all the tile's queries, in registers
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            long long idx = base + grp * RR + r;
            rvalid[r] = idx < hi;
            if (!rvalid[r]) idx = hi - 1;
            rid[r] = a.ids[idx];
            rp[r] = a.rows + (size_t)rid[r] * (size_t)rw;
            rlab[r] = s.label[rid[r]];
            rbest[r] = kExactEmpty;
        }
        const bool rows_one = rlab[0] == rlab[1] && rlab[1] == rlab[2] && rlab[2] == rlab[3];
        for (int qsub = 0; qsub < nqt; qsub += RQ) {
            int ql[RQ], qv[RQ];
#pragma unroll
            for (int q = 0; q < RQ; ++q) { ql[q] = qlab[qsub + q]; qv[q] = qself[qsub + q]; }
            // the register tile is not measured where its 16 pairs share a label, or where all of them lie on or below the diagonal
            // (rows and queries ascend).  The same in the eight lanes of a group; the staging barriers below stand outside it.
            const bool tile_skip = (rows_one && ql[0] == rlab[0] && ql[1] == rlab[0] && ql[2] == rlab[0] && ql[3] == rlab[0]) || rid[RR - 1] <= qv[0];
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
            // The offers, from the lane that holds the distances.  A pair above the diagonal is skipped where its ends share a label and
            // measured otherwise; a distance that is a number offers itself to both ends.  The query side: the minimum over the group's
            // rows in registers, then a 64-bit LDS min per query where a plain read says it is smaller.  The row side stays in rbest[].
            // Nothing here waits for another lane, and every test is a nested if: the lanes meet again behind the branch.
            if (j == 0) {
#pragma unroll
                for (int q = 0; q < RQ; ++q) {
                    if (qsub + q < nqt) {
                        unsigned long long kq = kExactEmpty;
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            if (rvalid[r] && rid[r] > qv[q]) {
                                if (tile_skip || rlab[r] == ql[q]) ++skipped;
                                else {
                                    ++measured;
                                    const float d = dist[q][r];
                                    if (d == d) {
                                        const unsigned long long kr = exact_key(d, qv[q]), kc = exact_key(d, rid[r]);
                                        rbest[r] = kr < rbest[r] ? kr : rbest[r];
                                        kq = kc < kq ? kc : kq;
                                    }
                                }
                            }
                        }
                        if (kq < qbest[qsub + q]) (void)__hip_atomic_fetch_min(&qbest[qsub + q], kq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
            }
        }
        // the row side leaves: at most one global atomic per row and step, and only where a plain load says the offer is smaller
        if (j == 0) {
#pragma unroll
            for (int r = 0; r < RR; ++r)
                if (rbest[r] != kExactEmpty && rbest[r] < __hip_atomic_load(s.best + rid[r], GI_RELAXED)) (void)__hip_atomic_fetch_min(s.best + rid[r], rbest[r], GI_RELAXED);
        }
    }
    __syncthreads(); // the LDS minima are complete
    if (measured) atomicAdd(a.evals, (unsigned long long)measured);
    if (skipped) atomicAdd(s.skipped, (unsigned long long)skipped);
    if (tid < nqt) { // the query side leaves: one global atomic per query and block at the most
        const unsigned long long k = qbest[tid];
        unsigned long long *dst = s.best + qself[tid];
        if (k != kExactEmpty && k < __hip_atomic_load(dst, GI_RELAXED)) (void)__hip_atomic_fetch_min(dst, k, GI_RELAXED);
    }
}

template <int METRIC>
hipError_t span_scan_launch(const ExactScanArgs &a, const SpanScanArgs &s, unsigned n_blocks, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((span_scan_kernel<METRIC>), dim3(n_blocks, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, s);
    return hipGetLastError();
}

#ifdef HNSW_EXACT_COMMON
// ---- the round around the scans: metric-free, grid-stride, no kernel waits for another wave ----
// Before a round's scans.  Entries [0, m): the member's key and its own slot of the two component tables (a component's slot is its
// root's, and every root is a member).  Entries [0, segments) as well: a segment's label -- its first entry's where every entry of
// the segment carries it, -1 otherwise (the last segment may be short).
__global__ void __launch_bounds__(256) span_reset_kernel(const int *__restrict__ ids, long long m, const int *__restrict__ label, unsigned long long *__restrict__ best,
                                                         unsigned *__restrict__ comp_w, unsigned long long *__restrict__ comp_edge, int *__restrict__ seg_label)
{
    const long long step = (long long)gridDim.x * 256, nseg = (m + kExactIterRows - 1) / kExactIterRows;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) {
        const int v = ids[i];
        best[v] = kExactEmpty;
        comp_w[v] = 0xffffffffu;
        comp_edge[v] = kExactEmpty;
        if (i < nseg) {
            const long long e0 = i * kExactIterRows, e1 = e0 + kExactIterRows < m ? e0 + kExactIterRows : m;
            int l = label[ids[e0]];
            for (long long e = e0 + 1; e < e1; ++e) l = label[ids[e]] == l ? l : -1;
            seg_label[i] = l;
        }
    }
}
// The lightest distance key a component was offered.  (A member without a key met no foreign member whose distance is a number.)
__global__ void __launch_bounds__(256) span_weight_kernel(const int *__restrict__ ids, long long m, const int *__restrict__ label,
                                                          const unsigned long long *__restrict__ best, unsigned *comp_w)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) {
        const int v = ids[i];
        const unsigned long long k = best[v];
        if (k != kExactEmpty) {
            unsigned *dst = comp_w + label[v];
            const unsigned dk = (unsigned)(k >> 32);
            if (dk < __hip_atomic_load(dst, GI_RELAXED)) (void)__hip_atomic_fetch_min(dst, dk, GI_RELAXED);
        }
    }
}
// The component's lightest outgoing edge under (distance key, lo, hi).  For a fixed v the smallest (d, u) is also its smallest
// (d, lo, hi): the ids below v give (u, v), ordered by u, and come before the ids above it, which give (v, u), ordered by u.
__global__ void __launch_bounds__(256) span_edge_kernel(const int *__restrict__ ids, long long m, const int *__restrict__ label,
                                                        const unsigned long long *__restrict__ best, const unsigned *__restrict__ comp_w,
                                                        unsigned long long *comp_edge)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) {
        const int v = ids[i];
        const unsigned long long k = best[v];
        if (k != kExactEmpty && (unsigned)(k >> 32) == comp_w[label[v]]) {
            const unsigned u = (unsigned)k, lo = u < (unsigned)v ? u : (unsigned)v, hi = u < (unsigned)v ? (unsigned)v : u;
            const unsigned long long e = ((unsigned long long)lo << 32) | hi;
            unsigned long long *dst = comp_edge + label[v];
            if (e < __hip_atomic_load(dst, GI_RELAXED)) (void)__hip_atomic_fetch_min(dst, e, GI_RELAXED);
        }
    }
}
// Every root with an edge joins its two ends and writes the edge, unless the component at the other end chose the same edge and
// has the smaller label: a mutual choice is written once.  label[], comp_w[] and comp_edge[] are read-only here; parent[] is the
// union-find's.  The edges of one round cannot close a cycle: each is its component's minimum under a strict total order.
__global__ void __launch_bounds__(256) span_join_kernel(const int *__restrict__ ids, long long m, const int *__restrict__ label, const unsigned *__restrict__ comp_w,
                                                        const unsigned long long *__restrict__ comp_edge, int *parent, SpanEdge *__restrict__ edges,
                                                        unsigned long long cap, unsigned long long *cursor)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) {
        const int v = ids[i];
        const unsigned long long e = comp_edge[v];
        if (label[v] == v && e != kExactEmpty) {
            const int lo = (int)(unsigned)(e >> 32), hi = (int)(unsigned)e;
            const int other = label[lo] == v ? label[hi] : label[lo];
            uf_union(parent, lo, hi);
            if (!(comp_edge[other] == e && other < v)) {
                const unsigned long long place = atomicAdd(cursor, 1ull);
                if (place < cap) edges[place] = SpanEdge{lo, hi, comp_w[v], 0u};
            }
        }
    }
}
hipError_t span_reset_launch(const int *ids, long long m, const int *label, unsigned long long *best, unsigned *comp_w, unsigned long long *comp_edge,
                             int *seg_label, hipStream_t st)
{
    hipLaunchKernelGGL(span_reset_kernel, dim3(exact_union_blocks(m)), dim3(256), 0, st, ids, m, label, best, comp_w, comp_edge, seg_label);
    return hipGetLastError();
}
hipError_t span_join_launch(const int *ids, long long m, const int *label, const unsigned long long *best, unsigned *comp_w, unsigned long long *comp_edge,
                            int *parent, SpanEdge *edges, unsigned long long cap, unsigned long long *cursor, hipStream_t st)
{
    const dim3 grid(exact_union_blocks(m)), block(256);
    hipLaunchKernelGGL(span_weight_kernel, grid, block, 0, st, ids, m, label, best, comp_w);
    hipLaunchKernelGGL(span_edge_kernel, grid, block, 0, st, ids, m, label, best, comp_w, comp_edge);
    hipLaunchKernelGGL(span_join_kernel, grid, block, 0, st, ids, m, label, comp_w, comp_edge, parent, edges, cap, cursor);
    return hipGetLastError();
}
#endif // HNSW_EXACT_COMMON

} // namespace hnsw
#endif // HNSW_EXACT_UNIT
