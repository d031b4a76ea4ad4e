// dk_span_tree_pf.h -- the Boruvka scan of the two spanning trees behind dk_exact_mfma.h's f16 MFMA tile.
//   span_pf_kernel<M, MREACH>   the launch shape of Device::exact_triangle_scan, as span_scan_kernel (dk_span_tree.h) and
//                               mreach_scan_kernel (dk_mreach_tree.h): the queries are a contiguous ascending piece of the member list,
//                               the candidates the whole list, a pair (self, rid) counts where rid > self and its ends carry different
//                               labels.  Every such pair is JUDGED on the half-precision tile against the lighter edges its two
//                               components already hold, and only a pair that the bound of 3.34 cannot prove to be heavier than both is
//                               MEASURED, with the metric's own arithmetic (the eight lane partials in element order, collapse_l2:
//                               span_scan_kernel's bits), and offered to both ends.  MREACH: the weight is max(K(d), core[a], core[b]).
// The forests, weights, core and info are byte for byte the plain scans'.
//
// The threshold is per component and moves during the scan.  comp_w[label] -- all ones behind span_reset_kernel, the component's
// lightest key behind span_weight_kernel -- is a LIVE bound here: every measured pair does a min of its 32-bit weight key into
// comp_w[label[a]] and comp_w[label[b]] beside its two 64-bit offers to best[], a plain load in front of each atomic.  The tile's
// queries' bounds are staged in LDS and republished by the wave that drains them; each wave loads its rows' label, id, (core key)
// and comp_w[label] once per step of 128 rows, with plain loads.  comp_w only falls during a round: a stale bound is a looser one.
//
// The rule.  W = max(comp_w[label[a]], comp_w[label[b]]) as keys, thr the float whose key is W.  A foreign pair above the diagonal
//   * MREACH: is turned away where core[a] > W or core[b] > W (its weight is at least either core key);
//   * otherwise is turned away iff 3.34's test proves d > thr strictly, with s = the larger of the two ends' s (s is monotone in the
//     bound, so that is s of W):    R > (max(s_a + e_a, s_b + e_a) + e_b)^2 (1 + 2^-18),  a the query.
// exact_key is strictly increasing apart from -0 and +0 sharing a key, and no bound is -0's, so d > thr gives K(d) > W: the pair's
// weight key is above both components' current minima, which only fall.  It cannot be either component's (key, lo, hi) minimum, so
// it changes neither comp_w nor comp_edge; the round kernels that run behind the scans (span_weight_kernel recomputes the same
// minima from best[]) see what they see behind the plain scan in every slot they read.  A pair whose weight TIES the bound is never
// turned away: it is measured and the (a, b) order decides as it does today.  W all ones (no offer yet) has s = +inf and turns
// nothing away; a NaN anywhere in the test keeps the pair (the IEEE compare); a vector that does not round to finite halves has
// e = +inf.
// What differs behind it: best[v] of a single member may lack offers that the plain scan records ABOVE its component's minimum.
// Nothing reads those: span_weight_kernel takes the minimum over a component, span_edge_kernel only the members whose key is that.
//
// The split, the epilogue's masks, the one __syncthreads_or per step and the drain are exact_tri_pf_kernel's (dk_exact_tri.h), and
// the tile is its tri_pf_tile as it stands.  The epilogue masks, before it counts: rid <= self, equal labels (counted as skipped),
// rows past the chunk's end and query slots past the tile's last.  Kept from span_scan_kernel: the early leave below the diagonal
// and the uniform-segment skip through seg_label, counted the same way; from 3.35: a diagonal block begins at the first step above
// its tile's first query.  evals (pairs_measured) += the foreign pairs above the diagonal, each once, judged or measured; skipped +=
// the pairs above the diagonal with one label: info equals the plain form's in every slot.  ctr[0] += the former, ctr[1] += those
// of them that went to the drain.
#pragma once
#include "dk_exact_tri.h"
#include "dk_mreach_tree.h"

namespace hnsw {

constexpr long long kSpanPfChunk = kExactTriPfChunk; // rows of a chunk of this form unless `exact_chunk` forces them
// what the picker asks of a call before it takes this form by itself (diag exact_prefilter = 1): members, per tree (DESIGN.md 3.37
// has the measurement)
constexpr long long kSpanPfMinMembersSpan = 16384;
constexpr long long kSpanPfMinMembersMreach = 16384;

struct SpanPfArgs {
    const int *label;              // [every id of the list]: its component -- the component's smallest id
    unsigned long long *best;      // [every id of the list]: the smallest (weight key << 32 | other id) offered in this round
    const int *seg_label;          // [ceil(m / kExactIterRows)]: span_reset_kernel's
    const unsigned *core;          // MREACH: [every id of the list]: its core distance as a 32-bit distance key; else not read
    unsigned *comp_w;              // [every label]: the live bound -- the lightest weight key the component was offered so far
    long long q_off;               // query q of the launch is entry q_off + q of the id list (ExactScanArgs::ids)
    unsigned long long *skipped;   // out: pairs above the diagonal with both ends in one component, added up over the blocks
    unsigned long long *ctr;       // out: [0] += foreign pairs above the diagonal, [1] += those of them that were measured
};

// LDS of one block: the staged halves; seven words per query (n_q, e_q, s_q + e_q, bound, id, label, core key); two 16-byte
// records per row of the step; the survivor masks (two buffers)
inline size_t span_pf_lds(int dim)
{
    const size_t qt = kExactPfQTile;
    return qt * (size_t)(dim + 8) * 2 + 7 * qt * 4 + 2 * 128 * 16 + 2 * qt * 16;
}

// One launch of span_pf_kernel<METRIC, mreach>: n_blocks x a.n_chunks blocks of kExactThreads threads; lds: span_pf_lds(a.dim).
// a.ids is the member list (never nullptr), a.queries the gathered rows of its entries [s.q_off, s.q_off + a.nq); a.qtile, a.piece,
// a.k and a.lists are not read.  A metric the form is not built for: an error.
template <int METRIC>
hipError_t span_pf_launch(const ExactScanArgs &a, const SpanPfArgs &s, bool mreach, unsigned n_blocks, size_t lds, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT
namespace hnsw {

struct alignas(16) SpanPfRowA { float nx, ex, s; int rid; };         // n_x, e_x, s of the row's component's bound, the id
struct alignas(16) SpanPfRowB { int lab; unsigned w, core, zero; };   // the label, that bound as a key, the core key (MREACH)

// s of a bound: +inf for all ones (no offer yet), else sqrt(max(thr, 1e-30) c) (1 + 2^-20), thr the float whose key is w.  No bound
// is a NaN's key: a NaN distance is no edge.
__device__ __forceinline__ float span_pf_s(unsigned w, float c)
{
    if (w == 0xffffffffu) return __uint_as_float(0x7f800000u);
    return sqrtf(fmaxf(key2f(w), 1e-30f) * c) * 1.00000095367431640625f;
}
// a 32-bit min where a plain load says the value is smaller
__device__ __forceinline__ void span_pf_min(unsigned *dst, unsigned v)
{
    if (v < __hip_atomic_load(dst, GI_RELAXED)) (void)__hip_atomic_fetch_min(dst, v, GI_RELAXED);
}
__device__ __forceinline__ void span_pf_min(unsigned long long *dst, unsigned long long v)
{
    if (v < __hip_atomic_load(dst, GI_RELAXED)) (void)__hip_atomic_fetch_min(dst, v, GI_RELAXED);
}

// Resources (gfx950, profiles/span_prefilter_kernel_resources.json): exact_tri_pf_kernel's split -- 256 threads, 64 queries staged
// once as halves, steps of 128 rows, wave w owning rows [32 w, 32 w + 32) against both 32-query halves, row operands straight from
// global memory two MFMA steps ahead.  The epilogue reads a row's seven words as two 16-byte LDS records.
template <int METRIC, bool MREACH>
__global__ void __launch_bounds__(kExactThreads) span_pf_kernel(const ExactScanArgs a, const SpanPfArgs s)
{
    static_assert(exact_pf_metric(METRIC), "built for sq_euclid and sq_euclid_f16 only");
    constexpr int QT = kExactPfQTile;
    constexpr bool F16 = metric_f16(METRIC);
    extern __shared__ __align__(16) unsigned char span_pf_lds_[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g8 = lane >> 3, j = lane & 7;
    const int rl = lane & 31, hh = lane >> 5;
    const int dim = a.dim, KP = dim + 8, nsteps = dim >> 4;
    _Float16 *qh = reinterpret_cast<_Float16 *>(span_pf_lds_);
    float *nq_s = reinterpret_cast<float *>(span_pf_lds_ + (size_t)QT * KP * 2), *eq_s = nq_s + QT, *sq_s = eq_s + QT; // sq_s: s of the bound + e_q
    unsigned *qw_s = reinterpret_cast<unsigned *>(sq_s + QT);                 // the query's component's bound as a key
    int *self_s = reinterpret_cast<int *>(qw_s + QT), *qlab_s = self_s + QT;
    unsigned *qcore_s = reinterpret_cast<unsigned *>(qlab_s + QT);
    SpanPfRowA *row_a = reinterpret_cast<SpanPfRowA *>(qcore_s + QT);         // [wave][32]: written and read by their wave alone
    SpanPfRowB *row_b = reinterpret_cast<SpanPfRowB *>(row_a + 128);
    unsigned *surv = reinterpret_cast<unsigned *>(row_b + 128);               // [2][QT][4]: bit 16 (2 w + h) + v of a query's 128
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT; // queries of the round in this tile (>= 1)
    const int *self = a.ids + s.q_off;
    // nothing counts where the chunk's last id is not above the tile's first query id (both lists ascend): the whole block leaves, in
    // front of its first barrier; and a block on the diagonal begins at the first step whose last id is above it
    const int self0 = __builtin_amdgcn_readfirstlane(self[q0]);
    if (__builtin_amdgcn_readfirstlane(a.ids[hi - 1]) <= self0) return;
    long long first = lo;
    while (first + kExactIterRows < hi && __builtin_amdgcn_readfirstlane(a.ids[first + kExactIterRows - 1]) <= self0) first += kExactIterRows;
    const int rw = row_words<METRIC>(dim);
    const float g = 1.001f * (float)((dim >> 3) + 16) * 0x1p-24f, c = 1.0f + 1.5f * g;
    const float eps = 1.01f * (float)(3 * dim + 36) * 0x1p-24f * 1.0000002f; // (the two roundings of the constant itself)

    // the tile's queries as halves (past the last query a slot shadows it; its pairs are masked in the epilogue), n_q, e_q, the id, the
    // label, (the core key) and the component's bound as it stands
    for (int qi = wave; qi < QT; qi += kExactThreads / 64) {
        const long long src = q0 + (qi < nqt ? qi : nqt - 1);
        const float *qsrc = a.queries + (size_t)src * dim;
        float n = 0.0f;
        double ss = 0.0;
        bool finite = true;
        for (int o = lane; o < dim; o += 64) {
            const float v = qsrc[o];
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
        if (lane == 0) {
            const int v = self[src], l = s.label[v];
            const unsigned w = __hip_atomic_load(s.comp_w + l, GI_RELAXED);
            const float e = exact_pf_e(ss, all_finite);
            nq_s[qi] = n; eq_s[qi] = e; sq_s[qi] = span_pf_s(w, c) + e; qw_s[qi] = w;
            self_s[qi] = v; qlab_s[qi] = l;
            if constexpr (MREACH) qcore_s[qi] = s.core[v];
        }
    }
    __syncthreads();
    // the tile's one label, -1 where its queries lie in several components (labels are ids: never negative)
    int tlab = qlab_s[0];
    for (int i = 1; i < nqt; ++i) tlab = qlab_s[i] == tlab ? tlab : -1;
    tlab = __builtin_amdgcn_readfirstlane(tlab);

    // this lane's pairs above the diagonal: foreign ones in its masks, those of them it sent to the drain, and the ones with one label
    // (thread q < nqt also: query q's pairs of the skipped steps)
    unsigned seen = 0, kept = 0, skipped = 0;
    int buf = 1; // the mask buffer of the last step that was not skipped: two such steps in a row never share one
    for (long long base = first; base < hi; base += kExactIterRows) {
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
            continue; // (block-uniform: no lane goes on alone; no barrier, so the mask buffers do not turn either)
        }
        buf ^= 1;
        // ---- the tile: this lane's row against the 64 queries ----
        long long idx = base + wave * 32 + rl;
        if (idx >= hi) idx = hi - 1; // past the chunk's end a lane shadows its last row; the pairs are masked below
        const int rid = a.ids[idx];
        const float *rp = a.rows + (size_t)rid * (size_t)rw;
        // the row's label, (core key) and its component's bound: once per step, plain loads
        const int rlab = s.label[rid];
        const unsigned rbound = __hip_atomic_load(s.comp_w + rlab, GI_RELAXED);
        unsigned rcore = 0u;
        if constexpr (MREACH) rcore = s.core[rid];
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
        if (hh == 0) {
            row_a[wave * 32 + rl] = SpanPfRowA{nx, ex, span_pf_s(rbound, c), rid};
            row_b[wave * 32 + rl] = SpanPfRowB{rlab, rbound, rcore, 0u};
        }
        wave_lds_sync();
        // ---- the epilogue: 16 + 16 pairs of this lane -> two survivor masks ----
        const long long rows_left = hi - base - wave * 32; // rows of this wave's 32 that exist
        unsigned any = 0;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qs = 32 * t + rl;
            const float nq = nq_s[qs], eq = eq_s[qs], sq = sq_s[qs];
            const int qself = self_s[qs], qlab = qlab_s[qs];
            [[maybe_unused]] unsigned qw = 0u, qcore = 0u;
            if constexpr (MREACH) { qw = qw_s[qs]; qcore = qcore_s[qs]; }
            unsigned mask = 0, counted = 0, one = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = 8 * (v >> 2) + 4 * hh + (v & 3);
                const SpanPfRowA ra = row_a[wave * 32 + r];
                const SpanPfRowB rb = row_b[wave * 32 + r];
                const float dot = t ? acc1[v] : acc0[v];
                const float N = ra.nx + nq;
                const float D = N - 2.0f * dot;
                const float R = fmaxf(D - eps * N, 0.0f);
                const float tt = fmaxf(sq, ra.s + eq) + ra.ex; // the larger of the two ends' s: a pair is needed if either component could take it
                const float T = tt * tt * 1.000003814697265625f;
                bool keep = !(R > T);
                if constexpr (MREACH) {
                    const unsigned W = qw > rb.w ? qw : rb.w;
                    keep = keep && !(qcore > W || rb.core > W); // exact in key space: the weight is at least either core key
                }
                if (r < rows_left && ra.rid > qself) { // the pair's other half, the query's own row and the shadows: not counted
                    if (rb.lab == qlab) one |= 1u << v;
                    else {
                        counted |= 1u << v;
                        if (keep) mask |= 1u << v;
                    }
                }
            }
            if (qs >= nqt) mask = counted = one = 0;
            seen += (unsigned)__popc(counted);
            kept += (unsigned)__popc(mask);
            skipped += (unsigned)__popc(one);
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
            const int qself = self_s[qi], qlab = qlab_s[qi];
            [[maybe_unused]] unsigned qcore = 0u;
            if constexpr (MREACH) qcore = qcore_s[qi];
            unsigned long long kq = kExactEmpty; // the query side: this lane's lightest offer to best[qself]
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
                    // < hi: the mask holds existing rows only.  (From the list, not from row_a: another wave may be a step ahead and have rewritten its records)
                    prid[r] = a.ids[base + 32 * (u >> 1) + 8 * (v >> 2) + 4 * (u & 1) + (v & 3)];
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
                    if (j == 0 && act[r] && dist == dist) { // a NaN distance is no edge
                        unsigned wk = (unsigned)(exact_key(dist, 0) >> 32);
                        if constexpr (MREACH) {
                            const unsigned pc = s.core[prid[r]];
                            wk = wk > qcore ? wk : qcore;
                            wk = wk > pc ? wk : pc;
                        }
                        const unsigned long long kc = ((unsigned long long)wk << 32) | (unsigned)prid[r];
                        kq = kc < kq ? kc : kq;
                        // the row side: its offer and its component's bound, from the lane that holds the distance
                        span_pf_min(s.best + prid[r], ((unsigned long long)wk << 32) | (unsigned)qself);
                        span_pf_min(s.comp_w + s.label[prid[r]], wk);
                    }
                }
            }
            // the query side: the wave's lightest offer leaves from one lane, and the query's bound is republished from its component's
            // as it stands now (read by every wave's next epilogue: an older value is a looser one)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(kq, o, 64);
                kq = other < kq ? other : kq;
            }
            if (lane == 0) {
                if (kq != kExactEmpty) {
                    span_pf_min(s.best + qself, kq);
                    span_pf_min(s.comp_w + qlab, (unsigned)(kq >> 32));
                }
                const unsigned w = __hip_atomic_load(s.comp_w + qlab, GI_RELAXED);
                if (w < qw_s[qi]) { qw_s[qi] = w; sq_s[qi] = span_pf_s(w, c) + eq_s[qi]; }
            }
        }
    }
    // one wave, one atomic per counter
    unsigned long long wseen = seen, wkept = kept, wskip = skipped;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { wseen += __shfl_xor(wseen, o, 64); wkept += __shfl_xor(wkept, o, 64); wskip += __shfl_xor(wskip, o, 64); }
    if (lane == 0) {
        if (wseen) {
            atomicAdd(s.ctr, wseen);
            atomicAdd(a.evals, wseen); // a pair counts once, turned away or measured
        }
        if (wkept) atomicAdd(s.ctr + 1, wkept);
        if (wskip) atomicAdd(s.skipped, wskip);
    }
}

template <int METRIC>
hipError_t span_pf_launch(const ExactScanArgs &a, const SpanPfArgs &s, bool mreach, unsigned n_blocks, size_t lds, hipStream_t st)
{
    if constexpr (!exact_pf_metric(METRIC)) return hipErrorInvalidValue; // no kernel is built for this metric
    else {
        if (!exact_pf_dim(a.dim) || !a.ids || lds > kExactPfMaxLds || lds < span_pf_lds(a.dim) || (mreach && !s.core)) return hipErrorInvalidValue;
        const dim3 grid(n_blocks, (unsigned)a.n_chunks), block(kExactThreads);
        if (mreach) hipLaunchKernelGGL((span_pf_kernel<METRIC, true>), grid, block, lds, st, a, s);
        else hipLaunchKernelGGL((span_pf_kernel<METRIC, false>), grid, block, lds, st, a, s);
        return hipGetLastError();
    }
}

} // namespace hnsw
#endif
