// dk_base.h -- device code, part of device_kernels.h: includes, launch-shape macros, wave-level synchronisation, half-precision rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_backend.h"

#ifdef EXP_LAT_REGS // experiment: no occupancy target for the traversal kernels (every register the wave can have: no spills)
#define HNSW_WAVES(x) 1
#else
#define HNSW_WAVES(x) (x)
#endif

#ifndef HNSW_I8_WAVES // waves per SIMD of the int8 search kernels with up to two register sets (build experiment: -DHNSW_I8_WAVES=4 / 6)
#define HNSW_I8_WAVES 5
#endif

#ifndef HNSW_PF_WAVES // waves per SIMD of the row-prefilter search kernels whose row length is a run-time value (-DHNSW_PF_WAVES=4 was measured: 128 VGPRs with 40-59 spilled, 19.7 ms per launch where three waves take 16.5.  The spills come from the run-time row length, not from the exact traversal in the same kernel: kFormLeanPFFixed below)
#define HNSW_PF_WAVES 3
#endif
#ifndef HNSW_PF_FIXED_WAVES // waves per SIMD of the fixed-length row-prefilter kernels (kFormLeanPFFixed): 124-128 VGPRs, nothing spilled
#define HNSW_PF_FIXED_WAVES 4
#endif
#ifndef HNSW_PF8_WAVES // waves per SIMD of the 8-bit row-prefilter kernels (kFormLeanPF8Fixed): the shadow pass holds 16 VGPRs of loads where the f16 pass holds 32, and the f32 pass, which only re-reads the shadow pass's survivors, 32 where the lean form holds 64 (HNSW_PF8_PASS_ROWS): 91-96 VGPRs, nothing spilled
#define HNSW_PF8_WAVES 5
#endif
#ifndef HNSW_PF8_PASS_ROWS // rows per f32 pass of every measure_all inside the 8-bit row-prefilter kernels: 8, 16, 24 or 32 (form_measure_cap below)
#define HNSW_PF8_PASS_ROWS 16
#endif
#ifndef HNSW_PF_FIXED_PASS_ROWS // ... and inside the f16 fixed-length row-prefilter kernels (32: the lean form's passes, the bytes these kernels had before the cap existed)
#define HNSW_PF_FIXED_PASS_ROWS 32
#endif

namespace hnsw {

// Every block of the kernels below that stage data through LDS is ONE wavefront working on its own job (the latency
// variants add a second wave with a role of its own, which never meets the first at a barrier): what the phases of
// such a wave need between a write and the reads of other lanes is that its own memory operations have completed and
// that the compiler keeps the order -- what __syncthreads() does in front of its s_barrier, without the barrier.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_s_waitcnt(0); // vmcnt(0) expcnt(0) lgkmcnt(0)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
}

// LDS ordering inside ONE wave (every traversal block is one wave): the wave's LDS instructions execute in order, so
// all a write-then-read by other lanes needs is that the compiler keeps them in order -- not wave_sync(), whose
// s_waitcnt also drains the vector-memory counter and with it every load still in flight.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// ------------------------------------------------------------------------------------
// device code
// ------------------------------------------------------------------------------------
// Forms of the two traversal kernels (their fourth template argument).  PLAIN: every launch flag is read at run time.  LAT: the
// latency variant, two waves per job (dk_team.h, dk_pool_top.h).  LEAN: what a launch without visited sets (flags 9: the
// default wherever every adjacency list has at most 64 entries and a row at most 1 KB) needs and nothing else -- "no visited
// set" and "rows of all listed neighbours in one go" are compile-time facts, the code of the other two ways through an
// expansion is not there, and the arguments that only the start and the end of a job use are read from the kernarg segment
// where they are used (kernarg_load below): 316 -> 105 spilled scalars in the int8 two-set form, HALF the vector instructions
// per launch (the spills' v_readlane / v_writelane sat in the expansion loop).  Measured (round 5, profiles/r5_lean_ab.log):
// int8 records 12 500-query launches 3.73 -> 2.93 ms, 65 536-query launches 12.9 -> 9.2 ms; f32 rows within +-1.5 %.
// LEAN_PF (sq_euclid, f32 rows only): the lean form with the half-precision row prefilter -- the listed neighbours are measured on
// the index's SHADOW rows (half the bytes), the ones that are provably farther than the farthest result are turned away on that
// value, and only the rest is measured from its f32 row by the lean form's own pass (dk_sorted_top.h).
// LEAN_PF_FIXED: LEAN_PF with the row length (in 32-bit words) compiled in -- kPfFixedDim, assigned to `dim` as graph_search_kernel's
// first statement, so the trip counts of the measure passes are constants: four waves per SIMD without a spilled register, where
// the run-time length spills 55-59 at that occupancy.  Launched where the index's row length is kPfFixedDim (place_traversal).
// LEAN_PF8_FIXED: LEAN_PF_FIXED with the shadow pass on 8-bit codes -- 128 code bytes per row, ONE cache line, decoded on one
// index-wide grid as fmaf(step, code, lo) (measure_shadow8, dk_sorted_top.h); the same decision with E8 for E.
constexpr int kFormPlain = 0, kFormLat = 1, kFormLean = 2, kFormLeanPF = 3, kFormLeanPFFixed = 4, kFormLeanPF8Fixed = 5;
constexpr int kPfFixedDim = 128; // the one length built (another one goes in with an A/B of its own)
constexpr __host__ __device__ bool form_is_pf8(int f) { return f == kFormLeanPF8Fixed; }
constexpr __host__ __device__ bool form_is_pf_fixed(int f) { return f == kFormLeanPFFixed || f == kFormLeanPF8Fixed; }
constexpr __host__ __device__ bool form_is_pf(int f) { return f == kFormLeanPF || form_is_pf_fixed(f); }
constexpr __host__ __device__ bool form_is_lean(int f) { return f == kFormLean || form_is_pf(f); }
// The most rows a lane group keeps in flight in one f32 pass (measure_all's NPCAP, 8 rows each) anywhere in a kernel of form f: the
// survivor re-read, the descent and the exact traversal a tied job falls into alike -- one 32-row pass left in the kernel and its 64
// VGPRs of loads set the kernel's register count.  In the 8-bit row-prefilter form the f32 pass re-reads 5.7 survivors per expansion
// on average and more than 16 in one expansion of fourteen: 16 rows per pass, and the kernel fits five waves.
constexpr __host__ __device__ int form_measure_cap(int f) { return f == kFormLeanPF8Fixed ? HNSW_PF8_PASS_ROWS / 8 : f == kFormLeanPFFixed ? HNSW_PF_FIXED_PASS_ROWS / 8 : 4; }

// A kernel argument read again from the kernarg segment at the point of use (a scalar load that hits the constant cache) instead of
// being carried in SGPRs from the kernel's first instruction to its last: the lean search kernel does this for the two dozen
// arguments that only the start and the end of a job look at (result arrays, job list, scratch of the exact traversal), so that the
// registers belong to the expansion loop.  `volatile`: the load stays where it is written (hoisted out of the job loop it would be the
// long live range again).
template <class T>
__device__ __forceinline__ T kernarg_load(unsigned byte_offset)
{
    typedef const char __attribute__((address_space(4))) *cptr;
    typedef const volatile T __attribute__((address_space(4))) *tptr;
    return *(tptr)((cptr)__builtin_amdgcn_kernarg_segment_ptr() + byte_offset);
}
// (the metric ids M_* and their list HNSW_FOR_EACH_METRIC: device_backend.h, which the host-only units can include too)

// ---- half-precision row storage (M_SQH, M_UCOSH) --------------------------------------------------------
// The arithmetic of X_f16 is X's, on stored rows widened from binary16 (exact): metric_is_sq / metric_is_ucos name the
// arithmetic, metric_f16 the storage.  A stored row is a RECORD of row_words(dim) = 8 * ceil(dim / 16) 32-bit words (32 B
// per 16 elements, zero padded): word 8 b + j holds element 16 b + j in its low half and element 16 b + 8 + j in its high
// half -- so lane j of an 8-lane group reads one dword per TWO consecutive steps of its lane partial, and a lane of a pair
// one 16-byte piece for four partials.  Queries (and rows staged in LDS) stay f32 in element order.  For the f32 metrics
// every helper below is the expression it replaces.
constexpr __host__ __device__ bool metric_f16(int m) { return m == M_SQH || m == M_UCOSH; }
constexpr __host__ __device__ bool metric_is_sq(int m) { return m == M_SQ || m == M_SQH; }
constexpr __host__ __device__ bool metric_is_ucos(int m) { return m == M_UCOS || m == M_UCOSH; }
constexpr __host__ __device__ int metric_arith(int m) { return m == M_SQH ? (int)M_SQ : m == M_UCOSH ? (int)M_UCOS : m; }
constexpr __host__ __device__ int f16_row_words(int dim) { return ((dim + 15) >> 4) << 3; }
template <int METRIC>
__host__ __device__ __forceinline__ int row_words(int dim) // `dim` as the kernels get it: elements (float metrics) or record words (int8)
{
    if constexpr (metric_f16(METRIC)) return f16_row_words(dim);
    else return dim;
}
template <int METRIC>
__device__ __forceinline__ const float *row_at(const float *__restrict__ rows, size_t id, int dim)
{
    if constexpr (metric_f16(METRIC)) return rows + id * (size_t)f16_row_words(dim);
    else return rows + id * dim;
}
__host__ __device__ __forceinline__ float half_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__host__ __device__ __forceinline__ float half_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
// element i of a stored row
template <int METRIC>
__device__ __forceinline__ float row_elem(const float *__restrict__ rec, int i)
{
    if constexpr (metric_f16(METRIC)) {
        const unsigned w = reinterpret_cast<const unsigned *>(rec)[((i >> 4) << 3) | (i & 7)];
        return (i & 8) ? half_hi(w) : half_lo(w);
    } else return rec[i];
}
// binary32 -> binary16 bits: round to nearest even, subnormals kept, beyond 65504 + half an ulp -> inf, NaN stays NaN (quiet), -0 stays -0
// (numpy's astype(float16)); integer arithmetic, so host and device agree whatever the float modes.
__host__ __device__ inline unsigned short f32_to_f16_bits(unsigned x)
{
    const unsigned sign = (x >> 16) & 0x8000u, a = x & 0x7fffffffu;
    if (a >= 0x7f800000u) return (unsigned short)(sign | (a > 0x7f800000u ? 0x7e00u | ((a >> 13) & 0x3ffu) : 0x7c00u));
    if (a >= 0x477ff000u) return (unsigned short)(sign | 0x7c00u); // >= 65520: rounds past the largest finite half
    if (a >= 0x38800000u) { // normal half: rebias, round the 13 dropped bits to nearest even (a carry into the exponent is right)
        const unsigned r = a - 0x38000000u;
        return (unsigned short)(sign | ((r + 0xfffu + ((r >> 13) & 1u)) >> 13));
    }
    if (a < 0x33000000u) return (unsigned short)sign; // below 2^-25: to zero (2^-25 itself ties to even = 0)
    const unsigned e = a >> 23, m = (a & 0x7fffffu) | 0x800000u; // subnormal half: m * 2^(e - 150) in units of 2^-24
    const unsigned sh = 126u - e;                                 // 14 .. 24
    const unsigned q = m >> sh, rem = m & ((1u << sh) - 1u), halfway = 1u << (sh - 1u);
    return (unsigned short)(sign | (q + ((rem > halfway || (rem == halfway && (q & 1u))) ? 1u : 0u)));
}

} // namespace hnsw
