// dk_exact_mfma_ip.h -- the plain top-k flat scan of the cosine family behind an f16 MFMA tile.
//   exact_scan_ip_pf_kernel<M, WAVES>   exact_scan_pf_kernel's sibling (dk_exact_mfma.h) for the metrics whose distance is a
//                             non-increasing function of the library's f32 dot product s: ucosine and ucosine_f16 (1 - s) and cosine
//                             (1 - s / denom).  The same arguments, the same output -- lists[nq][n_chunks][k], followed by the unchanged
//                             exact_merge_kernel -- and the same two counters.  Every (query, row) pair is JUDGED on the tile
//                             v_mfma_f32_32x32x16_f16 computes of h(row) . h(query), h = rounded to binary16, and only a pair whose proven
//                             lower bound on the library's distance is not above the query's current k-th distance is MEASURED, with the
//                             metric's own arithmetic (the eight lane partials, multiply then add, collapse_cos, the epilogue), so that
//                             every key that reaches a list carries exact_scan_kernel's bits.
// Built for cosine, ucosine (f32 rows, rounded on the fly) and ucosine_f16 (the records are the operand as they are); for the other
// metrics no kernel exists and the launcher fails.
//
// The split is 3.34's -- 64 queries staged once per block as halves in LDS at row stride dim + 8, the row operand straight from global
// memory two MFMA steps ahead, wave w on rows [32 w, 32 w + 32) of a step against both 32-query halves, 16-bit survivor masks in LDS in two
// buffers, one barrier per step, the drain by the wave that owns the query's list -- with two things of its own:
//   * LDS beyond 64 KB.  The staged queries take 64 (dim + 8) 2 bytes: 97 KB at dim 768, 129 KB at dim 1024.  exact_ip_pf_lds and
//     exact_ip_pf_max_k work from the limit the device reports (Device::max_lds_), not from a constant: with 160 KB the form serves
//     dim % 32 == 0 in [64, 1024], with 64 KB dim <= 256.
//   * WAVES in {4, 8}.  Where two blocks fit a CU (the plan's LDS is at most half the limit) a block is 4 waves and a step 128 rows.
//     Above that one block owns the CU, and 4 waves would leave every SIMD a single wave whose global loads nothing hides: the block
//     is then 8 waves and a step 256 rows -- the same 64 staged queries over twice the rows, 256 mask bits per query and step, the
//     lists of queries w, w + 8, ... with wave w.
//
// The test (DESIGN.md 3.38 proves it).  u = 2^-24, K = dim, a = h(x), b = h(q), e_x >= |x - a|_2, e_q >= |q - b|_2,
// beta = (2 K + 32) u (3.34's charge for the matrix core), gamma = 1.001 (K / 8 + 4) u (the library's chain: one rounding per product,
// K / 8 - 1 chain additions, three collapse additions).  The library's s obeys
//     s <= dot + A_r P_q + E_r Q_q + (K + 8) 2^-149 = S_ub
//     A_r >= |a|     E_r >= e_x (1 + gamma)     Q_q >= |q|     P_q >= (beta + 8 u) |b| + e_q + gamma |q|
// (the 8 u |b| pays for the roundings of the three operations that form S_ub itself), every term rounded up as exact_pf_e rounds
// up, +inf for a vector with an element that is not finite or does not round to a finite half.  Then
//     ucosine:  turned away  iff  1.0f - S_ub > thr
//     cosine:   turned away  iff  (denom < 1e-30f ? 1.0f : 1.0f - S_ub / denom) > thr,   denom the pair's own, the library's bits
// thr: the distance of the query's current k-th key, +inf while the list is not full or that distance is no number.  Both epilogues
// are non-increasing in s and IEEE rounding is monotone, so the left sides are lower bounds of the library's distance; the compare
// is strict (ties are measured) and IEEE (a NaN anywhere keeps the pair).
#pragma once
#include "dk_exact_mfma.h"

namespace hnsw {

constexpr int kExactIpPfMaxDim = 1024;   // dim % 32 == 0 in [kExactPfMinDim, this], as far as the device's LDS goes

constexpr bool exact_ip_pf_metric(int metric) { return metric == M_COS || metric == M_UCOS || metric == M_UCOSH; }
inline bool exact_ip_pf_dim(int dim) { return dim >= kExactPfMinDim && dim <= kExactIpPfMaxDim && dim % 32 == 0; }
// LDS of one block of `waves` waves: the staged halves, the lists and their k-th keys, P_q / Q_q / thr as floats, the queries' cosine
// norms, the waves' A_r / E_r and their rows' cosine norms, the survivor masks (two buffers of 32 waves bits per query), the waves'
// pending lists and their counts
inline size_t exact_ip_pf_lds(int dim, int k, int waves)
{
    const size_t qt = kExactPfQTile, w = (size_t)waves;
    return qt * (size_t)(dim + 8) * 2 + qt * (size_t)k * 8 + qt * 8 + 3 * qt * 4 + qt * 8 + 2 * 32 * w * 4 + 32 * w * 8 + 2 * qt * w * 4 +
           w * (size_t)kExactPfPend * 8 + w * 4 + 16;
}
// the waves of a block: 4 while two blocks fit a CU, else 8; `forced`: 4 or 8 (diag exact_qtile under exact_prefilter = 2), else the rule
inline int exact_ip_pf_waves(int dim, int k, size_t lds_limit, int forced = 0)
{
    if (forced == 4 || forced == 8) return forced;
    return 2 * exact_ip_pf_lds(dim, k, 4) <= lds_limit ? 4 : 8;
}
// the largest k the form serves at a row length: what is left of the device's limit
inline int exact_ip_pf_max_k(int dim, int waves, size_t lds_limit)
{
    const size_t fixed = exact_ip_pf_lds(dim, 0, waves);
    return fixed >= lds_limit ? 0 : (int)((lds_limit - fixed) / ((size_t)kExactPfQTile * 8));
}

// where the default (diag exact_prefilter = 1) takes the form above 3.34's floors: the metrics and row lengths at which every run of
// DESIGN.md 3.38's A/B beat every run of the plain scan -- all three metrics at every row length it ran at (64 to 1 024 for ucosine,
// 128 to 768 for the other two; between 3.4 and 6.1 times), so every row length the form serves
inline bool exact_ip_pf_picker(int metric, int dim) { return exact_ip_pf_metric(metric) && exact_ip_pf_dim(dim); }

// One launch of exact_scan_ip_pf_kernel<METRIC, waves>: n_blocks x a.n_chunks blocks of 64 waves threads; lds: exact_ip_pf_lds(a.dim, a.k,
// waves), at most lds_limit (the device's).  a.qtile and a.piece are not read.  ctr[0] += the pairs the tile judged, ctr[1] += those of
// them that were then measured; a.evals += the pairs, each once.  A metric the form is not built for: an error.
template <int METRIC>
hipError_t exact_scan_ip_pf_launch(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, int waves, size_t lds, size_t lds_limit, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT

namespace hnsw {

// a bound that is a sum of squares in f32 (n fused additions of non-negative terms: the true sum is at most the computed one times
// (1 + 1.01 n u)) as an upper bound of its root
__device__ __forceinline__ float exact_ip_pf_norm(float n2, int n, bool finite)
{
    return exact_pf_e((double)n2 * (1.0 + 1.01 * (double)n * 0x1p-24), finite);
}
// the distance the tile compares with: +inf while the list is not full, or its k-th distance is no number
__device__ __forceinline__ float exact_ip_pf_thr(unsigned long long kth)
{
    if (kth == kExactEmpty) return __uint_as_float(0x7f800000u);
    const float thr = exact_key_dist(kth);
    return thr != thr ? __uint_as_float(0x7f800000u) : thr;
}

template <int METRIC, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) exact_scan_ip_pf_kernel(const ExactScanArgs a, unsigned long long *__restrict__ ctr)
{
    static_assert(exact_ip_pf_metric(METRIC), "built for cosine, ucosine and ucosine_f16 only");
    static_assert(WAVES == 4 || WAVES == 8, "a block is 4 or 8 waves");
    constexpr int QT = kExactPfQTile, THREADS = 64 * WAVES, STEP = 32 * WAVES, NM = WAVES / 2; // NM: 64-bit words of a query's masks
    constexpr bool F16 = metric_f16(METRIC), COS = METRIC == M_COS;
    extern __shared__ __align__(16) unsigned char exact_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g8 = lane >> 3, j = lane & 7;
    const int rl = lane & 31, hh = lane >> 5;
    const int dim = a.dim, k = a.k, KP = dim + 8, nsteps = dim >> 4;
    _Float16 *qh = reinterpret_cast<_Float16 *>(exact_lds);
    unsigned long long *lists = reinterpret_cast<unsigned long long *>(exact_lds + (size_t)QT * KP * 2);
    unsigned long long *thr = lists + (size_t)QT * k;
    double *qsn_s = reinterpret_cast<double *>(thr + QT);        // [QT]: the queries' cosine norms (cosine)
    double *rsn_s = qsn_s + QT;                                   // [wave][32]: the rows' (cosine); written and read by their wave alone
    float *pq_s = reinterpret_cast<float *>(rsn_s + STEP), *qq_s = pq_s + QT, *tf_s = qq_s + QT;
    float *ar_s = tf_s + QT, *er_s = ar_s + STEP;                 // [wave][32]: likewise
    unsigned *surv = reinterpret_cast<unsigned *>(er_s + STEP);   // [2][QT][WAVES]: bit 16 (2 w + h) + v of a query's 32 WAVES
    unsigned long long *pend = reinterpret_cast<unsigned long long *>(surv + 2 * QT * WAVES); // [wave][kExactPfPend]
    int *pend_cnt = reinterpret_cast<int *>(pend + WAVES * kExactPfPend);
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT;     // queries of the round in this tile (>= 1)
    const int rw = row_words<METRIC>(dim);
    const float inf = __uint_as_float(0x7f800000u);
    const float gam = 1.001f * (float)((dim >> 3) + 4) * 0x1p-24f * 1.0000002f;  // (the roundings of the constant itself)
    const float bet = (float)(2 * dim + 40) * 0x1p-24f;                            // beta + 8 u: exact
    const float tiny = (float)(dim + 8) * 0x1p-149f;                               // exact: a multiple of the smallest float
    const int nsq = (dim >> 1) + 2;                                                // additions behind a lane pair's sum of squares, and one

    for (int i = tid; i < QT * k; i += THREADS) lists[i] = kExactEmpty;
    if (tid < QT) { thr[tid] = kExactEmpty; tf_s[tid] = inf; }
    if (tid < WAVES) pend_cnt[tid] = 0;
    // the tile's queries as halves (past the last query a slot shadows it; its pairs are masked in the epilogue), P_q, Q_q
    for (int qi = wave; qi < QT; qi += WAVES) {
        const long long src = q0 + (qi < nqt ? qi : nqt - 1);
        const float *s = a.queries + (size_t)src * dim;
        float n = 0.0f;
        double ss = 0.0, qq = 0.0;
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
            qq += (double)v * (double)v;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o, 64); ss += __shfl_xor(ss, o, 64); qq += __shfl_xor(qq, o, 64); }
        const bool all_finite = __ballot(!finite) == 0ull;
        if (lane == 0) {
            const float nb = exact_ip_pf_norm(n, (dim >> 6) + 8, all_finite), eq = exact_pf_e(ss, all_finite), nq = exact_pf_e(qq, all_finite);
            pq_s[qi] = (bet * nb + eq + gam * nq) * 1.00000095367431640625f + 1e-37f;
            qq_s[qi] = nq;
            if constexpr (COS) qsn_s[qi] = a.q_sn[src];
        }
    }
    __syncthreads();

    unsigned kept = 0; // pairs this lane's masks sent to the drain
    int buf = 0;
    for (long long base = lo; base < hi; base += STEP, buf ^= 1) {
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
        // the row's two lanes join their halves of |a|^2 and of the error sum: A_r, E_r
        nx += __shfl_xor(nx, 32, 64);
        float er = 0.0f;
        const bool row_finite = finite && __shfl_xor((int)finite, 32, 64) != 0;
        if constexpr (F16) er = row_finite ? 0.0f : inf;
        else { ss += __shfl_xor(ss, 32, 64); er = exact_pf_e(ss, row_finite) * (1.0f + gam) * 1.00000095367431640625f; }
        if (hh == 0) {
            ar_s[wave * 32 + rl] = exact_ip_pf_norm(nx, nsq, row_finite); er_s[wave * 32 + rl] = er;
            if constexpr (COS) rsn_s[wave * 32 + rl] = a.row_sn[rid];
        }
        wave_lds_sync();
        // ---- the epilogue: 16 + 16 pairs of this lane -> two survivor masks ----
        const long long rows_left = hi - base - wave * 32; // rows of this wave's 32 that exist
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qs = 32 * t + rl;
            const float pq = pq_s[qs], qq = qq_s[qs], tf = tf_s[qs];
            [[maybe_unused]] double qsn = 0.0;
            if constexpr (COS) qsn = qsn_s[qs];
            unsigned mask = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = 8 * (v >> 2) + 4 * hh + (v & 3);
                const float dot = t ? acc1[v] : acc0[v];
                const float sub = __builtin_fmaf(ar_s[wave * 32 + r], pq, __builtin_fmaf(er_s[wave * 32 + r], qq, dot)) + tiny;
                float lb;
                if constexpr (COS) {
                    const float denom = (float)(rsn_s[wave * 32 + r] * qsn); // the library's, bit for bit
                    lb = denom < 1e-30f ? 1.0f : 1.0f - sub / denom;
                } else lb = 1.0f - sub;
                if (!(lb > tf) && r < rows_left) mask |= 1u << v;
            }
            if (qs >= nqt) mask = 0;
            kept += (unsigned)__popc(mask);
            reinterpret_cast<unsigned short *>(surv + ((size_t)buf * QT + qs) * WAVES)[2 * wave + hh] = (unsigned short)mask;
        }
        __syncthreads(); // the step's one barrier: every wave's masks are written (and the previous step's were read: two buffers)
        // ---- the drain: this wave's queries ----
        for (int qi = wave; qi < nqt; qi += WAVES) {
            unsigned long long mm[NM];
            unsigned long long any = 0;
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const uint2 sm = *reinterpret_cast<const uint2 *>(surv + ((size_t)buf * QT + qi) * WAVES + 2 * i);
                mm[i] = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sm.y) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)sm.x);
                any |= mm[i];
            }
            if (!any) continue;
            const float *qp = a.queries + (size_t)(q0 + qi) * dim;
            unsigned long long *L = lists + (size_t)qi * k;
            [[maybe_unused]] double qsn = 0.0;
            if constexpr (COS) qsn = qsn_s[qi];
            while (any) {
                // the next up to 32 survivors, the n-th to group n % 8 as its row n / 8; a group without one shadows the first
                int pos[4];
                bool act[4];
                int first = 0;
#pragma unroll
                for (int i = NM - 1; i >= 0; --i)
                    if (mm[i]) first = 64 * i + __builtin_ctzll(mm[i]);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pos[r] = first; act[r] = false;
#pragma unroll
                    for (int gg = 0; gg < 8; ++gg) {
                        int p = -1;
#pragma unroll
                        for (int i = NM - 1; i >= 0; --i)
                            if (mm[i]) p = i;
                        if (p >= 0) {
                            int bit = 0;
#pragma unroll
                            for (int i = 0; i < NM; ++i)
                                if (i == p) { bit = 64 * i + __builtin_ctzll(mm[i]); mm[i] &= mm[i] - 1; }
                            if (gg == g8) { pos[r] = bit; act[r] = true; }
                        }
                    }
                }
                any = 0;
#pragma unroll
                for (int i = 0; i < NM; ++i) any |= mm[i];
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
                        const float m = row_elem<METRIC>(prp[r], 8 * kk + j) * y; // multiply, then add: no fma (CosineMetric.cs:114-115)
                        pacc[r] = pacc[r] + m;
                    }
                }
                const unsigned long long t0 = thr[qi];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = collapse_cos(pacc[r]); // (all 64 lanes)
                    if (j == 0 && act[r]) {
                        float dist;
                        if constexpr (COS) {
                            const float denom = (float)(a.row_sn[prid[r]] * qsn); // CosineMetric.cs:88
                            dist = denom < 1e-30f ? 1.0f : 1.0f - s / denom;      // :89-91
                        } else dist = 1.0f - s;
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
                        tf_s[qi] = exact_ip_pf_thr(kth); // read by every wave's next epilogue: an older value is a looser one
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
        for (int i = tid; i < k; i += THREADS) dst[i] = lists[(size_t)qi * k + i];
    }
}

template <int METRIC, int WAVES>
static hipError_t exact_scan_ip_pf_launch_w(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, size_t lds, size_t lds_limit, hipStream_t st)
{
    // above 64 KB of dynamic LDS the runtime is told once per instantiation how much this kernel may ask for: the device's limit
    static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void *>(&exact_scan_ip_pf_kernel<METRIC, WAVES>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit);
    if (raised != hipSuccess) {
        (void)hipGetLastError(); // (not left for the launch below to report)
        if (lds > 64 * 1024) return raised;
    }
    hipLaunchKernelGGL((exact_scan_ip_pf_kernel<METRIC, WAVES>), dim3(n_blocks, (unsigned)a.n_chunks), dim3(64 * WAVES), lds, st, a, ctr);
    return hipGetLastError();
}

template <int METRIC>
hipError_t exact_scan_ip_pf_launch(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, int waves, size_t lds, size_t lds_limit, hipStream_t st)
{
    if constexpr (!exact_ip_pf_metric(METRIC)) return hipErrorInvalidValue; // no kernel is built for this metric
    else {
        if (!exact_ip_pf_dim(a.dim) || a.k < 1 || (waves != 4 && waves != 8) || lds > lds_limit || lds < exact_ip_pf_lds(a.dim, a.k, waves) ||
            a.chunk < 1 || (METRIC == M_COS && (!a.row_sn || !a.q_sn)))
            return hipErrorInvalidValue;
        return waves == 4 ? exact_scan_ip_pf_launch_w<METRIC, 4>(a, ctr, n_blocks, lds, lds_limit, st)
                          : exact_scan_ip_pf_launch_w<METRIC, 8>(a, ctr, n_blocks, lds, lds_limit, st);
    }
}

} // namespace hnsw
#endif
