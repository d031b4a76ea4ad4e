// dk_exact_tri.h -- the triangle scans with one fixed radius behind dk_exact_mfma.h's f16 MFMA tile.
//   exact_tri_pf_kernel<M, SINK>   the launch shape of Device::exact_triangle_scan: the queries are a contiguous ascending piece of
//                                  the member list (their ids in SINK::self), the candidates the whole list, a pair (self, rid) counts
//                                  where rid > self.  Every such pair is JUDGED on the half-precision tile against the call's radius
//                                  and only a pair that the bound of 3.34 cannot prove to lie beyond it is MEASURED, with the
//                                  metric's own arithmetic, and handed to the sink where its distance is <= the radius.
// SINK is one of the three sinks that exact_scan_kernel serves over the same triangle, read for its fields alone:
//   ExactRangeUnion         uf_union(parent, self, rid), *pairs += 1
//   ExactRangeDensity       counts[self] += 1, counts[rid] += 1, a place on *n_pairs; the record is stored where the place is below arena_cap
//   ExactRangeDensityJoin   density_join on the complete counts
// Labels, counts and info are byte for byte exact_scan_kernel's: the same pairs are admitted (a pair is turned away only with a proof
// that its distance is above the radius) with the same distance bits, and everything the sinks do is independent of order.
//
// What differs from exact_scan_pf_kernel.  The split is its own -- 256 threads, 64 queries, steps of 128 rows, wave w owning rows
// [32 w, 32 w + 32) against both 32-query halves, row operands straight from global memory two MFMA steps ahead, the queries staged
// once as halves -- and so is the epilogue's test, with thr = the radius:
//     s_q = sqrt(max(radius, 1e-30) c) (1 + 2^-20) + e_q      ONCE per query, while it is staged (+inf for a NaN radius: every pair
//                                                              is measured and the sink's own compare admits nothing)
//     turned away  iff  R > (s_q + e_x)^2 (1 + 2^-18)
//   * No lists, no k-th keys, no pending lists: LDS holds the staged halves, three words per query, three per row of the step and
//     the survivor masks -- 21.5 KB at dim 128 against exact_scan_pf_kernel's 27 KB at k = 10 and 46 KB at k = 64.
//   * The triangle.  A block whose chunk ends at or below its tile's first query id leaves before its first barrier, as
//     exact_scan_kernel's does.  A block ON the diagonal then SKIPS the steps of its chunk whose last row id is not above the tile's
//     first query id: the rows of those steps are the tile's own queries' predecessors, no pair of theirs counts.  What a diagonal block
//     measures in vain is therefore at most one step of 128 rows plus the tile's own 64, whatever the chunk -- the chunk no longer
//     decides the double work, only how many blocks there are and how often the queries are staged.
//   * The epilogue masks rid <= self and the rows past the chunk's end before it counts: ExactScanArgs::evals and ctr[0] are the pairs
//     with rid > self, each once, turned away or measured; ctr[1] those that went to the drain.
//   * The barrier of a step is __syncthreads_or over the masks: a step without a survivor -- nearly every step on a near-duplicate
//     workload -- has no drain at all.
//   * The drain hands a within pair to the sink from the lane that holds its distance, one global atomic (or uf_union) per pair.
//     exact_scan_kernel's LDS self-counts and its one-atomic-per-wave arena append are what a path needs on which EVERY pair passes
//     the sink; here pairs arrive one at a time.  A table with many within pairs pays for it (DESIGN.md 3.35 has the number).
#pragma once
#include "dk_exact_mfma.h"

namespace hnsw {

constexpr long long kExactTriPfChunk = 4096; // rows of a chunk of this form unless `exact_chunk` forces them
// what the picker asks of a call before it takes this form by itself (diag exact_prefilter = 1): members of the scan, per sink
// family (DESIGN.md 3.35 has the measurement)
constexpr long long kExactTriPfMinMembersUnion = 16384;
constexpr long long kExactTriPfMinMembersDensity = 16384;

// LDS of one block: the staged halves; n_q, s_q and the id per query; n_x, e_x and the id per row of the step; the survivor masks (two buffers)
inline size_t exact_tri_pf_lds(int dim)
{
    const size_t qt = kExactPfQTile;
    return qt * (size_t)(dim + 8) * 2 + 3 * qt * 4 + 3 * 128 * 4 + 2 * qt * 16;
}

// One launch of exact_tri_pf_kernel<METRIC, SINK>: n_blocks x a.n_chunks blocks of kExactThreads threads; lds: exact_tri_pf_lds(a.dim).
// a.qtile, a.piece, a.k and a.lists are not read.  ctr[0] += the pairs with rid > self, ctr[1] += those of them that were measured;
// a.evals += the former.  A metric the form is not built for: an error.
template <int METRIC, class SINK>
hipError_t exact_tri_pf_launch(const ExactScanArgs &a, const SINK &sink, unsigned long long *ctr, unsigned n_blocks, size_t lds, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT
namespace hnsw {

// A pair (a < b) whose measured distance d is <= the radius, from one lane
__device__ __forceinline__ void tri_pf_admit(const ExactRangeUnion &s, int a, int b, float)
{
    uf_union(s.parent, a, b);
    atomicAdd(s.pairs, 1ull);
}
__device__ __forceinline__ void tri_pf_admit(const ExactRangeDensity &s, int a, int b, float d)
{
    atomicAdd(&s.counts[a], 1);
    atomicAdd(&s.counts[b], 1);
    const unsigned long long place = atomicAdd(s.n_pairs, 1ull); // counts on past the capacity
    if (place < s.arena_cap) s.arena[place] = ExactDensityPair{a, b, __float_as_uint(d), 0u};
}
__device__ __forceinline__ void tri_pf_admit(const ExactRangeDensityJoin &s, int a, int b, float d)
{
    density_join(s.counts, s.min_samples, s.parent, s.attach, a, b, d);
}

// The tile of one step: this lane's row (rp) against the 64 staged queries (qb: the lane's query row and half of the operand) ->
// two 32 x 32 accumulators; the lane's share of n_x, of the rounding-error sum and of `finite`.  exact_scan_pf_kernel's, word for word.
template <bool F16>
__device__ __forceinline__ void tri_pf_tile(const float *rp, const _Float16 *qb, int KP, int nsteps, int hh, pf_float16 &acc0, pf_float16 &acc1, float &nx,
                                            double &ss, bool &finite)
{
    using Raw = typename std::conditional<F16, uint4, float4>::type;
    constexpr int NR = F16 ? 1 : 2; // 16-byte loads per MFMA step
    Raw cur[2][NR], nxt[2][NR];
    const auto load = [&](Raw (&dst)[2][NR], int s) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if constexpr (F16) dst[t][0] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const unsigned *>(rp) + 8 * (s + t) + 4 * hh);
            else {
                dst[t][0] = *reinterpret_cast<const float4 *>(rp + 16 * (s + t) + 8 * hh);
                dst[t][1] = *reinterpret_cast<const float4 *>(rp + 16 * (s + t) + 8 * hh + 4);
            }
        }
    };
    load(cur, 0);
    for (int s = 0; s < nsteps; s += 2) { // operand loads run two MFMA steps (32 elements; dim % 32 == 0) ahead of their use
        if (s + 2 < nsteps) load(nxt, s + 2);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            pf_half8 av;
            if constexpr (F16) {
                av = __builtin_bit_cast(pf_half8, cur[t][0]);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float hf = (float)av[e];
                    nx = __builtin_fmaf(hf, hf, nx);
                    finite = finite && (hf - hf == 0.0f);
                }
            } else {
                const float x[8] = {cur[t][0].x, cur[t][0].y, cur[t][0].z, cur[t][0].w, cur[t][1].x, cur[t][1].y, cur[t][1].z, cur[t][1].w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    av[e] = (_Float16)x[e];
                    const float hf = (float)av[e];
                    nx = __builtin_fmaf(hf, hf, nx);
                    finite = finite && (hf - hf == 0.0f) && (x[e] - x[e] == 0.0f);
                    const double d = (double)(x[e] - hf);
                    ss += d * d;
                }
            }
            const pf_half8 b0 = *reinterpret_cast<const pf_half8 *>(qb + 16 * (s + t));
            const pf_half8 b1 = *reinterpret_cast<const pf_half8 *>(qb + (size_t)32 * KP + 16 * (s + t));
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, b1, acc1, 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < NR; ++r) cur[t][r] = nxt[t][r];
    }
}

template <int METRIC, class SINK>
__global__ void __launch_bounds__(kExactThreads) exact_tri_pf_kernel(const ExactScanArgs a, const SINK sink, unsigned long long *__restrict__ ctr)
{
    static_assert(exact_pf_metric(METRIC), "built for sq_euclid and sq_euclid_f16 only");
    constexpr int QT = kExactPfQTile;
    constexpr bool F16 = metric_f16(METRIC);
    extern __shared__ __align__(16) unsigned char exact_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g8 = lane >> 3, j = lane & 7;
    const int rl = lane & 31, hh = lane >> 5;
    const int dim = a.dim, KP = dim + 8, nsteps = dim >> 4;
    _Float16 *qh = reinterpret_cast<_Float16 *>(exact_lds);
    float *nq_s = reinterpret_cast<float *>(exact_lds + (size_t)QT * KP * 2), *sq_s = nq_s + QT;
    int *self_s = reinterpret_cast<int *>(sq_s + QT);
    float *nx_s = reinterpret_cast<float *>(self_s + QT), *ex_s = nx_s + 128; // [wave][32]: written and read by their wave alone
    int *rid_s = reinterpret_cast<int *>(ex_s + 128);                         // ... and the rows' ids
    unsigned *surv = reinterpret_cast<unsigned *>(rid_s + 128);               // [2][QT][4]: bit 16 (2 w + h) + v of a query's 128
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT; // queries of the round in this tile (>= 1)
    const auto id_at = [&](long long idx) { return a.ids ? a.ids[idx] : (int)idx; };
    // nothing counts where the chunk's last id is not above the tile's first query id (both lists ascend): the whole block leaves, in
    // front of its first barrier; and a block on the diagonal begins at the first step whose last id is above it
    const int self0 = __builtin_amdgcn_readfirstlane(sink.self[q0]);
    if (__builtin_amdgcn_readfirstlane(id_at(hi - 1)) <= self0) return;
    long long first = lo;
    while (first + kExactIterRows < hi && __builtin_amdgcn_readfirstlane(id_at(first + kExactIterRows - 1)) <= self0) first += kExactIterRows;
    const int rw = row_words<METRIC>(dim);
    const float g = 1.001f * (float)((dim >> 3) + 16) * 0x1p-24f, c = 1.0f + 1.5f * g;
    const float eps = 1.01f * (float)(3 * dim + 36) * 0x1p-24f * 1.0000002f; // (the two roundings of the constant itself)
    const float radius = sink.range;
    // s_q without e_q: the radius is the same for every query and never changes
    const float s_r = radius != radius ? __uint_as_float(0x7f800000u) : sqrtf(fmaxf(radius, 1e-30f) * c) * 1.00000095367431640625f;

    // the tile's queries as halves (past the last query a slot shadows it; its pairs are masked in the epilogue), n_q, s_q, the id
    for (int qi = wave; qi < QT; qi += kExactThreads / 64) {
        const long long src = q0 + (qi < nqt ? qi : nqt - 1);
        const float *s = a.queries + (size_t)src * dim;
        float n = 0.0f;
        double ss = 0.0;
        bool finite = true;
        for (int o = lane; o < dim; o += 64) {
            const float v = s[o];
            const _Float16 hv = (_Float16)v; // round to nearest even; beyond the largest half: inf
            const float hf = (float)hv;
            const int pos = F16 ? ((o & ~15) | ((o & 7) << 1) | ((o >> 3) & 1)) : o; // the record's order for the f16 rows
            qh[(size_t)qi * KP + pos] = hv;
            n = __builtin_fmaf(hf, hf, n);
            finite = finite && (hf - hf == 0.0f) && (v - v == 0.0f);
            const double d = (double)(v - hf); // exact in f32 for finite v, hf
            ss += d * d;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o, 64); ss += __shfl_xor(ss, o, 64); }
        const bool all_finite = __ballot(!finite) == 0ull;
        if (lane == 0) { nq_s[qi] = n; sq_s[qi] = s_r + exact_pf_e(ss, all_finite); self_s[qi] = sink.self[src]; }
    }
    __syncthreads();

    unsigned seen = 0, kept = 0; // pairs with rid > self in this lane's masks, and those of them it sent to the drain
    int buf = 0;
    for (long long base = first; base < hi; base += kExactIterRows, buf ^= 1) {
        // ---- the tile: this lane's row against the 64 queries ----
        long long idx = base + wave * 32 + rl;
        if (idx >= hi) idx = hi - 1; // past the chunk's end a lane shadows its last row; the pairs are masked below
        const int rid = id_at(idx);
        const float *rp = a.rows + (size_t)rid * (size_t)rw;
        pf_float16 acc0 = {}, acc1 = {};
        float nx = 0.0f;
        double ss = 0.0;
        bool finite = true;
        tri_pf_tile<F16>(rp, qh + (size_t)rl * KP + 8 * hh, KP, nsteps, hh, acc0, acc1, nx, ss, finite);
        // the row's two lanes join their halves of n_x and of the error sum
        nx += __shfl_xor(nx, 32, 64);
        float ex = 0.0f;
        const bool row_finite = finite && __shfl_xor((int)finite, 32, 64) != 0;
        if constexpr (F16) ex = row_finite ? 0.0f : __uint_as_float(0x7f800000u);
        else { ss += __shfl_xor(ss, 32, 64); ex = exact_pf_e(ss, row_finite); }
        if (hh == 0) { nx_s[wave * 32 + rl] = nx; ex_s[wave * 32 + rl] = ex; rid_s[wave * 32 + rl] = rid; }
        wave_lds_sync();
        // ---- the epilogue: 16 + 16 pairs of this lane -> two survivor masks ----
        const long long rows_left = hi - base - wave * 32; // rows of this wave's 32 that exist
        unsigned any = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qs = 32 * t + rl;
            const float nq = nq_s[qs], sq = sq_s[qs];
            const int self = self_s[qs];
            unsigned mask = 0, counted = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = 8 * (v >> 2) + 4 * hh + (v & 3);
                const float dot = t ? acc1[v] : acc0[v];
                const float N = nx_s[wave * 32 + r] + nq;
                const float D = N - 2.0f * dot;
                const float R = fmaxf(D - eps * N, 0.0f);
                const float tt = sq + ex_s[wave * 32 + r];
                const float T = tt * tt * 1.000003814697265625f;
                if (r < rows_left && rid_s[wave * 32 + r] > self) { // the pair's other half, the query's own row and the shadows: not counted
                    counted |= 1u << v;
                    if (!(R > T)) mask |= 1u << v;
                }
            }
            if (qs >= nqt) mask = counted = 0;
            seen += (unsigned)__popc(counted);
            kept += (unsigned)__popc(mask);
            any |= mask;
            reinterpret_cast<unsigned short *>(surv + ((size_t)buf * QT + qs) * 4)[2 * wave + hh] = (unsigned short)mask;
        }
        // the step's one barrier: every wave's masks are written (and the previous step's were read: two buffers); no survivor in the
        // whole block: no drain
        if (!__syncthreads_or((int)any)) continue;
        // ---- the drain: this wave's queries ----
        for (int qi = wave; qi < nqt; qi += kExactThreads / 64) {
            const uint4 sm = *reinterpret_cast<const uint4 *>(surv + ((size_t)buf * QT + qi) * 4);
            unsigned long long m0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sm.y) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)sm.x);
            unsigned long long m1 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sm.w) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)sm.z);
            if (!(m0 | m1)) continue;
            const float *qp = a.queries + (size_t)(q0 + qi) * dim;
            const int self = self_s[qi];
            while (m0 | m1) {
                // the next up to 32 survivors, the n-th to group n % 8 as its row n / 8; a group without one shadows the first
                int pos[4];
                bool act[4];
                const int first_pos = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pos[r] = first_pos; act[r] = false;
#pragma unroll
                    for (int gg = 0; gg < 8; ++gg) {
                        if (m0 | m1) {
                            const int p = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
                            if (m0) m0 &= m0 - 1; else m1 &= m1 - 1;
                            if (gg == g8) { pos[r] = p; act[r] = true; }
                        }
                    }
                }
                int prid[4];
                const float *prp[4];
                float pacc[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int u = pos[r] >> 4, v = pos[r] & 15; // u = 2 w' + h of the lane that judged the pair
                    // < hi: the mask holds existing rows only.  (From the list, not from rid_s: another wave may be a step ahead and have rewritten its ids)
                    prid[r] = id_at(base + 32 * (u >> 1) + 8 * (v >> 2) + 4 * (u & 1) + (v & 3));
                    prp[r] = a.rows + (size_t)prid[r] * (size_t)rw;
                    pacc[r] = 0.0f;
                }
                for (int kk = 0; kk < (dim >> 3); ++kk) { // the metric's own lane partial: elements j, j + 8, ... in order (dim % 8 == 0: no tail)
                    const float y = qp[8 * kk + j];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float d = row_elem<METRIC>(prp[r], 8 * kk + j) - y;
                        pacc[r] = __builtin_fmaf(d, d, pacc[r]);
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dist = collapse_l2(pacc[r]); // (all 64 lanes)
                    if (j == 0 && act[r] && dist <= radius) tri_pf_admit(sink, self, prid[r], dist); // the sink's compare: a NaN on either side admits nothing
                }
            }
        }
    }
    // one wave, one atomic per counter
    unsigned long long wseen = seen, wkept = kept;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { wseen += __shfl_xor(wseen, o, 64); wkept += __shfl_xor(wkept, o, 64); }
    if (lane == 0 && wseen) {
        atomicAdd(ctr, wseen);
        atomicAdd(a.evals, wseen); // a pair counts once, turned away or measured
        if (wkept) atomicAdd(ctr + 1, wkept);
    }
}

template <int METRIC, class SINK>
hipError_t exact_tri_pf_launch(const ExactScanArgs &a, const SINK &sink, unsigned long long *ctr, unsigned n_blocks, size_t lds, hipStream_t st)
{
    if constexpr (!exact_pf_metric(METRIC)) return hipErrorInvalidValue; // no kernel is built for this metric
    else {
        if (!exact_pf_dim(a.dim) || lds > kExactPfMaxLds || lds < exact_tri_pf_lds(a.dim)) return hipErrorInvalidValue;
        hipLaunchKernelGGL((exact_tri_pf_kernel<METRIC, SINK>), dim3(n_blocks, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink, ctr);
        return hipGetLastError();
    }
}

} // namespace hnsw
#endif
