// dk_exact_mfma_i8.h -- the plain top-k flat scan of the int8 rows with the dot product on the i8 MFMA tile.
//   exact_scan_i8_mfma_kernel   exact_scan_pf_kernel's sibling (dk_exact_mfma.h) for sq_euclid_i8.  The same arguments, the same
//                             output -- lists[nq][n_chunks][k], followed by the unchanged exact_merge_kernel -- and the same two counters.
//                             The int8 distance (dk_metric.h, i8_epilogue) is a fixed sequence of double operations on the two records'
//                             scales and sums of squares and on their EXACT int32 dot product, and v_mfma_i32_32x32x32_i8 accumulates in
//                             int32, exact in any order: the tile does not estimate the library's dot product, it is that dot product.
//                             So the lane that holds the accumulator can compute the pair's very key.  It does so in two stages: a few
//                             f32 FMAs turn away what is provably above the query's k-th distance, and only what passes pays for the
//                             doubles of i8_epilogue and the compare with the k-th KEY.  What survives both goes to the drain, which
//                             measures it with the plain scan's own code (dot4_i8, group_sum_i32, i8_epilogue) and inserts it.
// Built for sq_euclid_i8 alone; for the other metrics no kernel exists and the launcher fails.
//
// The split is 3.34's -- 256 threads, 64 queries staged once per block in LDS, the row operand straight from global memory two MFMA steps
// ahead, wave w on rows [32 w, 32 w + 32) of a step of 128 against both 32-query halves (two 32 x 32 int32 accumulators), 16-bit survivor
// masks in LDS in two buffers, one barrier per step, the drain by the wave that owns the query's list -- with this of its own:
//   * A record is 4 pitch bytes, pitch % 16 == 0: pitch / 8 MFMA steps of 32 bytes, an even number and no tail at any dim.  Lane
//     (r = lane % 32, h = lane / 32) loads the 16 bytes at byte 32 s + 16 h of its row's record for step s; the query operand is the same
//     16 bytes of the staged query record.  Both operands map k to lanes and bytes the same way, so the order in which the instruction
//     pairs the bytes does not matter (the note in dk_exact_mfma.h).  The zero padding of the element words adds zeros.
//   * The record's last two words are the scale and the sum of squares.  The queries are staged with those two words REPLACED BY 0 (row
//     stride 4 pitch + 16 bytes: the 16-byte reads of 32 consecutive queries spread over the banks), so whatever the row holds there
//     is multiplied by 0 and the row operand needs no mask; the queries' scales and sums stand in LDS arrays of their own.  The h == 1
//     lane of a row holds the row's two words in the registers of its last step and publishes them, with the row's id and its f32
//     term of the bound, to its wave.
//   * The drain reads the query's element words from the staged copy (the two zeroed words make its last dot4 add 0).
//
// The test of stage 1 (DESIGN.md 3.39 proves it).  u = 2^-24; A = sa^2 na, B = sb^2 nb, C = sa sb dot as real numbers, D = A + B - 2 C.
//     ra = fl(fl(sa sa) (float)na)   qb = fl(fl(sb sb) (float)nb)   (NaN where not finite)   S = fl(ra + qb)   p = fl(sa (2 sb))
//     est = fma(-p, (float)dot, S)   lb = fl(est - fma(16 u, S, 2^-96))
//     turned away  iff  lb > thr     thr: the distance of the query's current k-th key, +inf while the list is not full or it is no number
// The compare is strict (ties go on) and IEEE (a NaN anywhere keeps the pair).  Stage 2: d = i8_epilogue(sa, na, sb, nb, dot), survives
// iff exact_key(d, id) < the query's k-th key as this lane reads it -- a snapshot: keys only ever fall, an older one is a looser one.
#pragma once
#include "dk_exact_mfma_ip.h" // (and through it dk_exact_mfma.h: the tile's constants, exact_ip_pf_thr)

namespace hnsw {

// the record words the form serves: what 64 KB of LDS hold at k = 1.  Up to here every sum of squares and every |dot| is at most
// 4 (208 - 2) 127^2 < 2^24: their conversions to float are exact
constexpr int kExactI8MaxPitch = 208;

constexpr bool exact_i8_mfma_metric(int metric) { return metric == M_I8; }
inline bool exact_i8_mfma_pitch(int pitch) { return pitch >= 16 && pitch <= kExactI8MaxPitch && pitch % 16 == 0; }
// LDS of one block: the staged records, the lists and their k-th keys, five words per query (qb, 2 sb, thr; sb, nb), four per row of
// a step (ra, sa; na, id), the survivor masks (two buffers), the waves' pending lists and their counts
inline size_t exact_i8_mfma_lds(int pitch, int k)
{
    const size_t qt = kExactPfQTile;
    return qt * ((size_t)pitch * 4 + 16) + qt * (size_t)k * 8 + qt * 8 + 5 * qt * 4 + 4 * 128 * 4 + 2 * qt * 16 + 4 * (size_t)kExactPfPend * 8 + 16;
}
// the largest k the form serves at a pitch: what is left of 64 KB
inline int exact_i8_mfma_max_k(int pitch)
{
    const size_t fixed = exact_i8_mfma_lds(pitch, 0);
    return fixed >= kExactPfMaxLds ? 0 : (int)((kExactPfMaxLds - fixed) / ((size_t)kExactPfQTile * 8));
}
// where the default (diag exact_prefilter = 1) takes the form above 3.34's floors: the pitches at which every run of DESIGN.md 3.39's A/B
// was below every run of the plain scan -- all it ran at, 16 to 144 words (dims 32 to 520; 3.7 to 6.7 times).  Above the largest of
// them nothing was measured: the form is there under exact_prefilter = 2
constexpr int kExactI8PickerMaxPitch = 144;
inline bool exact_i8_mfma_picker(int pitch) { return exact_i8_mfma_pitch(pitch) && pitch <= kExactI8PickerMaxPitch; }

// One launch of exact_scan_i8_mfma_kernel: n_blocks x a.n_chunks blocks of kExactThreads threads; lds: exact_i8_mfma_lds(a.dim, a.k), a.dim
// the record's words.  a.qtile and a.piece are not read.  ctr[0] += the pairs on the tile, ctr[1] += those of them that went to the
// drain; a.evals += the pairs, each once.  A metric the form is not built for: an error.
template <int METRIC>
hipError_t exact_scan_i8_mfma_launch(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, size_t lds, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT

namespace hnsw {

typedef int i8t_int4 __attribute__((ext_vector_type(4)));
typedef int i8t_int16 __attribute__((ext_vector_type(16)));

// a record's f32 term of the bound, fl(fl(s s) (float)n); NaN where that is not finite (an overflow, an inf or NaN scale), so that
// every bound made of it is NaN and keeps its pair
__device__ __forceinline__ float exact_i8_term(float s, int n)
{
    const float t = (s * s) * (float)n;
    return t - t == 0.0f ? t : __uint_as_float(0x7fc00000u);
}

template <int METRIC>
__global__ void __launch_bounds__(kExactThreads) exact_scan_i8_mfma_kernel(const ExactScanArgs a, unsigned long long *__restrict__ ctr)
{
    static_assert(exact_i8_mfma_metric(METRIC), "built for sq_euclid_i8 only");
    constexpr int QT = kExactPfQTile;
    extern __shared__ __align__(16) unsigned char exact_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g8 = lane >> 3, j = lane & 7;
    const int rl = lane & 31, hh = lane >> 5;
    const int pitch = a.dim, k = a.k, QW = pitch + 4, nsteps = pitch >> 3; // QW: words of a staged record's stride; nsteps: even
    int *qrec = reinterpret_cast<int *>(exact_lds);
    unsigned long long *lists = reinterpret_cast<unsigned long long *>(exact_lds + (size_t)QT * QW * 4);
    unsigned long long *thr = lists + (size_t)QT * k;
    float *qb_s = reinterpret_cast<float *>(thr + QT), *sb2_s = qb_s + QT, *tf_s = sb2_s + QT, *sb_s = tf_s + QT;
    int *nb_s = reinterpret_cast<int *>(sb_s + QT);
    float *ra_s = reinterpret_cast<float *>(nb_s + QT), *sa_s = ra_s + 128; // [wave][32]: written and read by their wave alone
    int *na_s = reinterpret_cast<int *>(sa_s + 128), *rid_s = na_s + 128;    // likewise
    unsigned *surv = reinterpret_cast<unsigned *>(rid_s + 128);              // [2][QT][4]: bit 16 (2 w + h) + v of a query's 128
    unsigned long long *pend = reinterpret_cast<unsigned long long *>(surv + 2 * QT * 4); // [wave][kExactPfPend]
    int *pend_cnt = reinterpret_cast<int *>(pend + 4 * kExactPfPend);
    const long long q0 = (long long)blockIdx.x * QT;
    const long long lo = (long long)blockIdx.y * a.chunk, hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    const int nqt = a.nq - q0 < QT ? (int)(a.nq - q0) : QT;     // queries of the round in this tile (>= 1)
    const float inf = __uint_as_float(0x7f800000u);

    for (int i = tid; i < QT * k; i += kExactThreads) lists[i] = kExactEmpty;
    if (tid < QT) { thr[tid] = kExactEmpty; tf_s[tid] = inf; }
    if (tid < 4) pend_cnt[tid] = 0;
    // the tile's query records, their last two words as 0 (past the last query a slot shadows it; its pairs are masked in the epilogue)
    for (int qi = wave; qi < QT; qi += kExactThreads / 64) {
        const int *s = reinterpret_cast<const int *>(a.queries) + (size_t)(q0 + (qi < nqt ? qi : nqt - 1)) * pitch;
        for (int o = lane; o < pitch; o += 64) qrec[(size_t)qi * QW + o] = o < pitch - 2 ? s[o] : 0;
        if (lane == 0) {
            const float sb = __int_as_float(s[pitch - 2]);
            const int nb = s[pitch - 1];
            sb_s[qi] = sb; nb_s[qi] = nb; sb2_s[qi] = 2.0f * sb; qb_s[qi] = exact_i8_term(sb, nb);
        }
    }
    __syncthreads();

    unsigned kept = 0; // pairs this lane's masks sent to the drain
    int buf = 0;
    for (long long base = lo; base < hi; base += kExactIterRows, buf ^= 1) {
        // ---- the tile: this lane's row against the 64 queries ----
        long long idx = base + wave * 32 + rl;
        if (idx >= hi) idx = hi - 1; // past the chunk's end a lane shadows its last row; the pairs are masked below
        const int rid = a.ids ? a.ids[idx] : (int)idx;
        const uint4 *rp = reinterpret_cast<const uint4 *>(a.rows + (size_t)rid * (size_t)pitch) + hh; // 16 bytes of step s: rp[2 s]
        i8t_int16 acc0 = {}, acc1 = {};
        const int *qb = qrec + (size_t)rl * QW + 4 * hh;
        // operand loads run two MFMA steps (64 bytes) ahead of their use
        uint4 cur[2], nxt[2];
        cur[0] = rp[0]; cur[1] = rp[2];
        nxt[0] = cur[0]; nxt[1] = cur[1];
        uint4 last = cur[1];
        for (int s = 0; s < nsteps; s += 2) {
            if (s + 2 < nsteps) { nxt[0] = rp[2 * (s + 2)]; nxt[1] = rp[2 * (s + 3)]; }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const i8t_int4 av = __builtin_bit_cast(i8t_int4, cur[t]);
                const i8t_int4 b0 = *reinterpret_cast<const i8t_int4 *>(qb + 8 * (s + t));
                const i8t_int4 b1 = *reinterpret_cast<const i8t_int4 *>(qb + (size_t)32 * QW + 8 * (s + t));
                acc0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b1, acc1, 0, 0, 0);
            }
            last = cur[1];
            cur[0] = nxt[0]; cur[1] = nxt[1];
        }
        // the row's h == 1 lane holds words pitch - 4 .. pitch - 1 of the record in the registers of the last step: scale and sum
        if (hh == 1) {
            const float sa = __uint_as_float(last.z);
            const int na = (int)last.w;
            ra_s[wave * 32 + rl] = exact_i8_term(sa, na); sa_s[wave * 32 + rl] = sa; na_s[wave * 32 + rl] = na; rid_s[wave * 32 + rl] = rid;
        }
        wave_lds_sync();
        // ---- the epilogue: 16 + 16 pairs of this lane -> two survivor masks ----
        const long long rows_left = hi - base - wave * 32; // rows of this wave's 32 that exist
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int qs = 32 * t + rl;
            const float qbt = qb_s[qs], sb2 = sb2_s[qs], tf = tf_s[qs], sb = sb_s[qs];
            const int nb = nb_s[qs];
            // the k-th key as one 64-bit LDS read (its owner republishes it with one 64-bit write: never half of each)
            const unsigned long long kth = __hip_atomic_load(thr + qs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            unsigned mask = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int r = 8 * (v >> 2) + 4 * hh + (v & 3);
                const int dot = t ? acc1[v] : acc0[v];
                const float sa = sa_s[wave * 32 + r];
                const float S = ra_s[wave * 32 + r] + qbt;
                const float p = sa * sb2;
                const float est = __builtin_fmaf(-p, (float)dot, S);
                const float lb = est - __builtin_fmaf(0x1p-20f, S, 0x1p-96f);
                if (!(lb > tf) && r < rows_left) {
                    const float d = i8_epilogue(sa, na_s[wave * 32 + r], sb, nb, dot); // the library's distance, bit for bit
                    if (exact_key(d, rid_s[wave * 32 + r]) < kth) mask |= 1u << v;
                }
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
            const int *qp = qrec + (size_t)qi * QW + j;
            const float sb = sb_s[qi];
            const int nb = nb_s[qi];
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
                int prid[4], iacc[4], ta[4];
                const int *prp[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int u = pos[r] >> 4, v = pos[r] & 15; // u = 2 w' + h of the lane that judged the pair
                    const long long pidx = base + 32 * (u >> 1) + 8 * (v >> 2) + 4 * (u & 1) + (v & 3); // < hi: the mask holds existing rows only
                    prid[r] = a.ids ? a.ids[pidx] : (int)pidx;
                    prp[r] = reinterpret_cast<const int *>(a.rows + (size_t)prid[r] * (size_t)pitch) + j;
                    iacc[r] = 0; ta[r] = 0;
                }
                for (int kk = 0; kk < nsteps; ++kk) { // the plain scan's lane partial: word 8 kk + j of both records
                    const int wb = qp[8 * kk];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ta[r] = prp[r][8 * kk];                 // (the last block's lanes 6 / 7 end with the row's scale / sumsq,
                        iacc[r] = dot4_i8(ta[r], wb, iacc[r]);  //  which the staged query's zeros keep out of the sum)
                    }
                }
                const unsigned long long t0 = thr[qi];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int dot = group_sum_i32(iacc[r]); // (all 64 lanes)
                    const float sa = __int_as_float(group_lane_to_first<6>(ta[r]));
                    const int na = group_lane_to_first<7>(ta[r]);
                    if (j == 0 && act[r]) {
                        const unsigned long long key = exact_key(i8_epilogue(sa, na, sb, nb, dot), prid[r]);
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
                        __hip_atomic_store(thr + qi, kth, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        pend_cnt[wave] = 0;
                        tf_s[qi] = exact_ip_pf_thr(kth); // both are read by every wave's next epilogue: an older value is a looser one
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
        atomicAdd(a.evals, pairs); // a pair counts once, on the tile or in the drain
    }
    for (int qi = 0; qi < nqt; ++qi) {
        unsigned long long *dst = a.lists + ((size_t)(q0 + qi) * a.n_chunks + blockIdx.y) * (size_t)k;
        for (int i = tid; i < k; i += kExactThreads) dst[i] = lists[(size_t)qi * k + i];
    }
}

template <int METRIC>
hipError_t exact_scan_i8_mfma_launch(const ExactScanArgs &a, unsigned long long *ctr, unsigned n_blocks, size_t lds, hipStream_t st)
{
    if constexpr (!exact_i8_mfma_metric(METRIC)) return hipErrorInvalidValue; // no kernel is built for this metric
    else {
        if (!exact_i8_mfma_pitch(a.dim) || a.k < 1 || a.chunk < 1 || lds > kExactPfMaxLds || lds < exact_i8_mfma_lds(a.dim, a.k)) return hipErrorInvalidValue;
        hipLaunchKernelGGL((exact_scan_i8_mfma_kernel<METRIC>), dim3(n_blocks, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, ctr);
        return hipGetLastError();
    }
}

} // namespace hnsw
#endif
