// dk_exact_mfma.h -- the plain top-k flat scan with an f16 MFMA tile in front of the measuring.
//   exact_scan_pf_kernel<M>   a tile of 64 queries x a chunk of the id list per block, as exact_scan_kernel<M, ExactTopK> (dk_exact.h) and
//                             with its output: lists[nq][n_chunks][k], followed by the unchanged exact_merge_kernel.  Every (query, row)
//                             pair is JUDGED on a dense half-precision tile -- v_mfma_f32_32x32x16_f16 on h(row) . h(query), h = rounded
//                             to binary16 -- and only a pair whose proven lower bound on the library's distance is not above the query's
//                             current k-th distance is MEASURED, with the metric's own arithmetic (the eight lane partials in element
//                             order, collapse_l2), so that every key that reaches a list carries exact_scan_kernel's bits.
// Built for sq_euclid (f32 rows, converted on the fly: no shadow matrix, nothing outlives the call) and sq_euclid_f16 (the records are
// the operand as they are); for the other metrics no kernel exists and the launcher fails.  It is a kernel of its own, like
// span_scan_kernel: no sink of exact_scan_kernel.
//
// The split.  256 threads, 4 waves.  Wave w owns rows [32 w, 32 w + 32) of a step of 128 rows against both 32-query halves of the
// tile: two 32 x 32 f32 accumulators, dim / 16 MFMAs each.
//   * The ROW operand never passes through LDS: a row of the step belongs to exactly one wave, so lane (r = lane % 32, h = lane / 32)
//     loads the 8 elements [16 s + 8 h, 16 s + 8 h + 8) of its row for MFMA s straight from global memory (two steps of s ahead of the
//     MFMAs that use them), rounds them to halves in registers and, on the way, adds up n_x = sum h(x)_i^2 (f32) and
//     sum (x_i - h(x)_i)^2 (double; every difference is exact); the two lanes of a row join their sums with one shuffle.
//   * The QUERY operand is staged once per block as halves in LDS, row stride dim + 8 halves (16 bytes more than a power-of-two
//     multiple: the 16-byte operand reads of 32 consecutive queries spread over the banks), with n_q and e_q computed while staging.
//   * A dot product does not care in which order its elements are paired as long as both operands use the same one, so for the f16
//     records -- word 8 b + j holds elements 16 b + j and 16 b + 8 + j -- the queries are staged in the record's order and a lane's
//     8 halves are simply 16 consecutive bytes of the record.
//   * The epilogue: accumulator register v of lane (c = lane % 32, h) is (row 8 (v / 4) + 4 h + v % 4, query c).  The lane forms
//     D~ = (n_x + n_q) - 2 dot and the test below for its 16 + 16 pairs and leaves a 16-bit survivor mask per accumulator in LDS:
//     surv[query][2 w + h] -- 128 bits per query and step, no atomics, no queue that could overflow (in a chunk's first step every
//     pair survives: the lists are not full).
//   * The drain: wave w owns the lists of queries w, w + 4, ... (as exact_scan_kernel's merging wave does).  After ONE barrier per step
//     (the masks are double-buffered) it reads the 128 bits of each of its queries; for a query that has any, its 8 lane groups
//     measure up to 4 survivors each per pass from global memory (row and f32 query), offer the keys below the k-th to the wave's
//     pending list, and the wave inserts them with exact_list_insert and republishes the k-th and s_q.  No block barrier in the drain.
//
// The test (DESIGN.md 3.34 proves it).  u = 2^-24, K = dim, eps = 1.01 (3 K + 36) u, g = 1.001 (K / 8 + 16) u (3.24's), c = 1 + 1.5 g:
//     R = max(D~ - eps (n_x + n_q), 0)                     <= |h(x) - h(q)|^2
//     s_q = sqrt(max(thr, 1e-30) c) (1 + 2^-20) + e_q      (+inf while the list is not full; refreshed with the k-th)
//     turned away  iff  R > (s_q + e_x)^2 (1 + 2^-18)      (the IEEE compare: a NaN anywhere keeps the pair)
// e >= |x - h(x)|_2: the double sum's root rounded up to f32 and raised as pack_shadow_rows_kernel raises E; +inf for a vector with
// an element that is not finite or does not round to a finite half; exactly 0 for an f16 record without such an element.
#pragma once
#include "dk_exact.h"

namespace hnsw {

constexpr int kExactPfQTile = 64;        // queries per block: two MFMA tiles of 32
constexpr int kExactPfMinDim = 64, kExactPfMaxDim = 256; // dim % 32 == 0 in between
constexpr size_t kExactPfMaxLds = 64 * 1024;
// what the picker asks of a call before it takes this form by itself (diag exact_prefilter = 1; DESIGN.md 3.34 has the measurement)
constexpr int kExactPfMinQueries = 256;
constexpr long long kExactPfMinRows = 65536;
constexpr long long kExactPfMinPairs = 250000000; // queries x candidates: below it the first steps of every chunk, where every pair survives, outweigh the tile
constexpr int kExactPfPickerMaxK = 64;            // the largest k the A/B ran at
constexpr int kExactPfPend = 32;         // keys a wave's pending list holds: 8 groups x 4 survivors of one pass

constexpr bool exact_pf_metric(int metric) { return metric == M_SQ || metric == M_SQH; }
inline bool exact_pf_dim(int dim) { return dim >= kExactPfMinDim && dim <= kExactPfMaxDim && dim % 32 == 0; }
// LDS of one block: the staged halves, the lists and their k-th keys, n_q / e_q / s_q, the waves' n_x / e_x, the survivor masks
// (two buffers), the waves' pending lists and their counts
inline size_t exact_pf_lds(int dim, int k)
{
    const size_t qt = kExactPfQTile;
    return qt * (size_t)(dim + 8) * 2 + qt * (size_t)k * 8 + qt * 8 + 3 * qt * 4 + 2 * 128 * 4 + 2 * qt * 16 + 4 * (size_t)kExactPfPend * 8 + 16;
}
// the largest k the form serves at a row length: what is left of 64 KB
inline int exact_pf_max_k(int dim)
{
    const size_t fixed = exact_pf_lds(dim, 0);
    return fixed >= kExactPfMaxLds ? 0 : (int)((kExactPfMaxLds - fixed) / ((size_t)kExactPfQTile * 8));
}

// One launch of exact_scan_pf_kernel<METRIC>: n_blocks x a.n_chunks blocks of kExactThreads threads; lds: exact_pf_lds(a.dim, a.k).
// a.qtile and a.piece are not read (the tile is kExactPfQTile, the queries are staged whole).  ctr[0] += the pairs the tile judged,
// ctr[1] += those of them that were then measured; a.evals += the pairs, each once.  A metric the form is not built for: an error.
template <int METRIC>
hipError_t exact_scan_pf_launch(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, size_t lds, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT
#include <type_traits>

namespace hnsw {

typedef _Float16 pf_half8 __attribute__((ext_vector_type(8)));
typedef float pf_float16 __attribute__((ext_vector_type(16)));

// sqrt of a double sum of squares as an upper bound in f32: rounded up, then raised as pack_shadow_rows_kernel raises E
__device__ __forceinline__ float exact_pf_e(double ss, bool finite)
{
    if (!finite || !(ss < 1e300)) return __uint_as_float(0x7f800000u);
    const double e = sqrt(ss);
    float f = (float)e;
    if ((double)f < e) f = __uint_as_float(__float_as_uint(f) + 1u); // (f >= 0: the next float up)
    return f * 1.00000095367431640625f + 1e-37f;
}
// s_q of a list whose k-th key is `kth`: +inf while the list is not full (or its k-th distance is no number)
__device__ __forceinline__ float exact_pf_sq(unsigned long long kth, float e_q, float c)
{
    if (kth == kExactEmpty) return __uint_as_float(0x7f800000u);
    const float thr = exact_key_dist(kth);
    if (thr != thr) return __uint_as_float(0x7f800000u); // a NaN's key is above every number's: nothing is turned away on it
    return sqrtf(fmaxf(thr, 1e-30f) * c) * 1.00000095367431640625f + e_q;
}

template <int METRIC>
__global__ void __launch_bounds__(kExactThreads) exact_scan_pf_kernel(const ExactScanArgs a, unsigned long long *__restrict__ ctr)
{
    static_assert(exact_pf_metric(METRIC), "built for sq_euclid and sq_euclid_f16 only");
    constexpr int QT = kExactPfQTile;
    constexpr bool F16 = metric_f16(METRIC);
    extern __shared__ __align__(16) unsigned char exact_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g8 = lane >> 3, j = lane & 7;
    const int rl = lane & 31, hh = lane >> 5;
    const int dim = a.dim, k = a.k, KP = dim + 8, nsteps = dim >> 4;
    _Float16 *qh = reinterpret_cast<_Float16 *>(exact_lds);
    unsigned long long *lists = reinterpret_cast<unsigned long long *>(exact_lds + (size_t)QT * KP * 2);
    unsigned long long *thr = lists + (size_t)QT * k;
    float *nq_s = reinterpret_cast<float *>(thr + QT), *eq_s = nq_s + QT, *sq_s = eq_s + QT;
    float *nx_s = sq_s + QT, *ex_s = nx_s + 128;                 // [wave][32]: written and read by their wave alone
    unsigned *surv = reinterpret_cast<unsigned *>(ex_s + 128);    // [2][QT][4]: bit 16 (2 w + h) + v of a query's 128
    unsigned long long *pend = reinterpret_cast<unsigned long long *>(surv + 2 * QT * 4); // [wave][kExactPfPend]
    int *pend_cnt = reinterpret_cast<int *>(pend + 4 * kExactPfPend);
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT;     // queries of the round in this tile (>= 1)
    const int rw = row_words<METRIC>(dim);
    const float g = 1.001f * (float)((dim >> 3) + 16) * 0x1p-24f, c = 1.0f + 1.5f * g;
    const float eps = 1.01f * (float)(3 * dim + 36) * 0x1p-24f * 1.0000002f; // (the two roundings of the constant itself)

    for (int i = tid; i < QT * k; i += kExactThreads) lists[i] = kExactEmpty;
    if (tid < QT) { thr[tid] = kExactEmpty; sq_s[tid] = __uint_as_float(0x7f800000u); }
    if (tid < 4) pend_cnt[tid] = 0;
    // the tile's queries as halves (past the last query a slot shadows it; its pairs are masked in the epilogue), n_q, e_q
    for (int qi = wave; qi < QT; qi += kExactThreads / 64) {
        const float *s = a.queries + (size_t)(q0 + (qi < nqt ? qi : nqt - 1)) * dim;
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
        if (lane == 0) { nq_s[qi] = n; eq_s[qi] = exact_pf_e(ss, all_finite); }
    }
    __syncthreads();

    unsigned kept = 0; // pairs this lane's masks sent to the drain
    int buf = 0;
    for (long long base = lo; base < hi; base += kExactIterRows, buf ^= 1) {
        // ---- the tile: this lane's row against the 64 queries ----
        long long idx = base + wave * 32 + rl;
        if (idx >= hi) idx = hi - 1; // past the chunk's end a lane shadows its last row; the pairs are masked below
        const int rid = a.ids ? a.ids[idx] : (int)idx;
        const float *rp = a.rows + (size_t)rid * (size_t)rw;
        pf_float16 acc0 = {}, acc1 = {};
        float nx = 0.0f;
        [[maybe_unused]] double ss = 0.0;
        bool finite = true;
        const _Float16 *qb = qh + (size_t)rl * KP + 8 * hh;
        // operand loads run two MFMA steps (32 elements; dim % 32 == 0) ahead of their use
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
        for (int s = 0; s < nsteps; s += 2) {
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
        // the row's two lanes join their halves of n_x and of the error sum
        nx += __shfl_xor(nx, 32, 64);
        float ex = 0.0f;
        const bool row_finite = finite && __shfl_xor((int)finite, 32, 64) != 0;
        if constexpr (F16) ex = row_finite ? 0.0f : __uint_as_float(0x7f800000u);
        else { ss += __shfl_xor(ss, 32, 64); ex = exact_pf_e(ss, row_finite); }
        if (hh == 0) { nx_s[wave * 32 + rl] = nx; ex_s[wave * 32 + rl] = ex; }
        wave_lds_sync();
        // ---- the epilogue: 16 + 16 pairs of this lane -> two survivor masks ----
        const long long rows_left = hi - base - wave * 32; // rows of this wave's 32 that exist
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qs = 32 * t + rl;
            const float nq = nq_s[qs], sq = sq_s[qs];
            unsigned mask = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = 8 * (v >> 2) + 4 * hh + (v & 3);
                const float dot = t ? acc1[v] : acc0[v];
                const float N = nx_s[wave * 32 + r] + nq;
                const float D = N - 2.0f * dot;
                const float R = fmaxf(D - eps * N, 0.0f);
                const float tt = sq + ex_s[wave * 32 + r];
                const float T = tt * tt * 1.000003814697265625f;
                if (!(R > T) && r < rows_left) mask |= 1u << v;
            }
            if (qs >= nqt) mask = 0;
            kept += (unsigned)__popc(mask);
            reinterpret_cast<unsigned short *>(surv + ((size_t)buf * QT + qs) * 4)[2 * wave + hh] = (unsigned short)mask;
        }
        __syncthreads(); // the step's one barrier: every wave's masks are written (and the previous step's were read: two buffers)
        // ---- the drain: this wave's queries ----
        for (int qi = wave; qi < nqt; qi += kExactThreads / 64) {
            const uint4 sm = *reinterpret_cast<const uint4 *>(surv + ((size_t)buf * QT + qi) * 4);
            unsigned long long m0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sm.y) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)sm.x);
            unsigned long long m1 = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sm.w) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)sm.z);
            if (!(m0 | m1)) continue;
            const float *qp = a.queries + (size_t)(q0 + qi) * dim;
            unsigned long long *L = lists + (size_t)qi * k;
            while (m0 | m1) {
                // the next up to 32 survivors, the n-th to group n % 8 as its row n / 8; a group without one shadows the first
                int pos[4];
                bool act[4];
                const int first = m0 ? __builtin_ctzll(m0) : 64 + __builtin_ctzll(m1);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pos[r] = first; act[r] = false;
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
                    const long long pidx = base + 32 * (u >> 1) + 8 * (v >> 2) + 4 * (u & 1) + (v & 3); // < hi: the mask holds existing rows only
                    prid[r] = a.ids ? a.ids[pidx] : (int)pidx;
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
                const unsigned long long t0 = thr[qi];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dist = collapse_l2(pacc[r]); // (all 64 lanes)
                    if (j == 0 && act[r]) {
                        const unsigned long long key = exact_key(dist, prid[r]);
                        if (key < t0) pend[wave * kExactPfPend + atomicAdd(&pend_cnt[wave], 1)] = key;
                    }
                }
                wave_lds_sync();
                const int cnt = pend_cnt[wave];
                if (cnt > 0) {
                    for (int i = 0; i < cnt; ++i) {
                        const unsigned long long x = pend[wave * kExactPfPend + i];
                        if (x < L[k - 1]) exact_list_insert(L, k, x, lane);
                    }
                    wave_lds_sync();
                    if (lane == 0) {
                        const unsigned long long kth = L[k - 1];
                        thr[qi] = kth; pend_cnt[wave] = 0;
                        sq_s[qi] = exact_pf_sq(kth, eq_s[qi], c); // read by every wave's next epilogue: an older value is a looser one
                    }
                    wave_lds_sync();
                }
            }
        }
    }
    __syncthreads();
    if (kept) atomicAdd(ctr + 1, (unsigned long long)kept);
    if (tid == 0) {
        const unsigned long long pairs = (unsigned long long)nqt * (unsigned long long)(hi - lo);
        atomicAdd(ctr, pairs);
        atomicAdd(a.evals, pairs); // a pair counts once, judged or measured
    }
    for (int qi = 0; qi < nqt; ++qi) {
        unsigned long long *dst = a.lists + ((size_t)(q0 + qi) * a.n_chunks + blockIdx.y) * (size_t)k;
        for (int i = tid; i < k; i += kExactThreads) dst[i] = lists[(size_t)qi * k + i];
    }
}

template <int METRIC>
hipError_t exact_scan_pf_launch(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, size_t lds, hipStream_t st)
{
    if constexpr (!exact_pf_metric(METRIC)) return hipErrorInvalidValue; // no kernel is built for this metric
    else {
        if (!exact_pf_dim(a.dim) || a.k < 1 || lds > kExactPfMaxLds || lds < exact_pf_lds(a.dim, a.k)) return hipErrorInvalidValue;
        hipLaunchKernelGGL((exact_scan_pf_kernel<METRIC>), dim3(n_blocks, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, ctr);
        return hipGetLastError();
    }
}

} // namespace hnsw
#endif
