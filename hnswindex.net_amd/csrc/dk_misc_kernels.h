// dk_misc_kernels.h -- device code, part of device_kernels.h: pair distances, per-row norms, int8 quantisation, row download, the gather of stored rows by id, the sqrt test kernel.
#pragma once
#include "dk_metric.h"

namespace hnsw {

// Flat id<->id pairs: 8 lanes per pair (hnswdev_dist_pair_batch).  Ids outside the uploaded rows
// give NaN and raise `guard` (see slot_distance_kernel).
template <int METRIC>
__global__ void __launch_bounds__(256)
pair_distance_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, int dim,
                     const int *__restrict__ a_ids, const int *__restrict__ b_ids, float *__restrict__ out, int n,
                     long long n_rows, int *__restrict__ guard)
{
    const int g = (blockIdx.x * 256 + threadIdx.x) >> 3;
    const int j = threadIdx.x & 7;
    const bool act = g < n;
    int a = a_ids[act ? g : 0], b = b_ids[act ? g : 0];
    const bool bad = (unsigned long long)(long long)a >= (unsigned long long)n_rows || (unsigned long long)(long long)b >= (unsigned long long)n_rows;
    if (bad) { a = 0; b = 0; }
    double sa = 0.0, sb = 0.0;
    if (METRIC == M_COS) { sa = row_sn[a]; sb = row_sn[b]; }
    float r = group_metric<METRIC>(row_at<METRIC>(rows, (size_t)a, dim), row_at<METRIC>(rows, (size_t)b, dim), dim, j, sa, sb);
    if (act && j == 0) {
        out[g] = bad ? __uint_as_float(0x7fc00000u) : r;
        if (bad) atomicOr(guard, 1);
    }
}

// sqrt((double)|row|^2) with |row|^2 summed in f32 in the reference's lane order
// (CosineMetric.cs:40-41,47 / :43-44,48 and the tail :83-84): 8 lanes per row.
#ifdef HNSW_HOST_TU // non-template kernels: only the unit that launches them defines them
__global__ void __launch_bounds__(256)
row_sqrtnorm_kernel(const float *__restrict__ rows, int dim, long long first, int n, double *__restrict__ out)
{
    const int g = (blockIdx.x * 256 + threadIdx.x) >> 3;
    const int j = threadIdx.x & 7;
    const bool act = g < n;
    const float *a = rows + (size_t)(first + (act ? g : 0)) * dim;
    float p = lane_chain<M_COS>(a, a, dim, j);
    float s = collapse_cos(p);
    if (dim & 7) s = scalar_tail<M_COS>(s, a, a, dim);
    if (act && j == 0) out[first + g] = sqrt_rn((double)s);
}
#endif

// exposed for tests: sqrt_rn over an array
#ifdef HNSW_HOST_TU
// float rows -> int8 records (see the layout above): one wave per row; lane l owns elements 4l .. 4l+3 of
// each 256-element stretch.  max and the integer sum are exact in any order.
__global__ void __launch_bounds__(256)
quantize_rows_kernel(const float *__restrict__ src, int dim, int n, float *__restrict__ dst, long long first, int pitch)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float *x = src + (size_t)r * dim;
    int *rec = reinterpret_cast<int *>(dst + (size_t)(first + r) * pitch);
    float m = 0.0f;
    for (int i = lane; i < dim; i += 64) m = fmaxf(m, fabsf(x[i]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    const float scale = m / 127.0f;
    int sumsq = 0;
    const int nwords = pitch - 2;
    for (int w = lane; w < nwords; w += 64) {
        unsigned packed = 0u;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * w + t;
            int q = 0;
            if (i < dim && scale > 0.0f) {
                const float v = __builtin_rintf(x[i] / scale);
                q = (int)fminf(fmaxf(v, -127.0f), 127.0f);
            }
            sumsq += q * q;
            packed |= (unsigned)(q & 0xff) << (8 * t);
        }
        rec[w] = (int)packed;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sumsq += __shfl_xor(sumsq, o, 64);
    if (lane == 0) { rec[pitch - 2] = __float_as_int(scale); rec[pitch - 1] = sumsq; }
}
// records -> the dequantised float rows q_i * scale (hnswdev_download_rows on an int8 context)
__global__ void __launch_bounds__(256)
dequantize_rows_kernel(const float *__restrict__ recs, int pitch, long long first, int n, int dim, float *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * dim) return;
    const int r = (int)(t / dim), i = (int)(t % dim);
    const int *rec = reinterpret_cast<const int *>(recs + (size_t)(first + r) * pitch);
    const int q = (int)(signed char)((rec[i >> 2] >> (8 * (i & 3))) & 0xff);
    out[t] = (float)q * __int_as_float(rec[pitch - 2]);
}
#endif
#ifdef HNSW_HOST_TU
// float rows -> half-precision records (dk_base.h): one thread per record word; padding halves are zero
__global__ void __launch_bounds__(256)
pack_f16_rows_kernel(const float *__restrict__ src, int dim, int n, float *__restrict__ dst, long long first)
{
    const int pitch = f16_row_words(dim);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * pitch) return;
    const int r = (int)(t / pitch), w = (int)(t % pitch);
    const int i0 = ((w >> 3) << 4) | (w & 7), i1 = i0 + 8;
    const float *x = src + (size_t)r * dim;
    const unsigned lo = i0 < dim ? f32_to_f16_bits(__float_as_uint(x[i0])) : 0u, hi = i1 < dim ? f32_to_f16_bits(__float_as_uint(x[i1])) : 0u;
    reinterpret_cast<unsigned *>(dst)[(size_t)(first + r) * pitch + w] = lo | (hi << 16);
}
// The row prefilter's shadow (dk_sorted_top.h): rows [first, first + n) of the f32 matrix `src` -> records [first, first + n) of
// `dst`, pack_f16_rows_kernel's layout and rounding, one wave per row -- which also raises *e_bits (the bits of a float >= 0, so
// atomicMax on them orders like the values) to an upper bound of ||x - h(x)||_2: the sum of squares in double (every difference is
// exact there, the sum is off by less than dim * 2^-53 of itself), its root rounded up to float and raised by 2^-20.  An element
// that does not convert to a finite half (or is not finite itself) makes the bound +inf: no row is turned away on such a shadow.
__global__ void __launch_bounds__(256)
pack_shadow_rows_kernel(const float *__restrict__ src, int dim, long long first, long long n, float *__restrict__ dst, unsigned *__restrict__ e_bits)
{
    const int pitch = f16_row_words(dim), lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float *x = src + (size_t)(first + r) * dim;
    unsigned *rec = reinterpret_cast<unsigned *>(dst) + (size_t)(first + r) * pitch;
    double ss = 0.0;
    bool finite = true;
    for (int w = lane; w < pitch; w += 64) {
        const int i0 = ((w >> 3) << 4) | (w & 7), i1 = i0 + 8;
        const float x0 = i0 < dim ? x[i0] : 0.0f, x1 = i1 < dim ? x[i1] : 0.0f;
        const unsigned word = (unsigned)f32_to_f16_bits(__float_as_uint(x0)) | ((unsigned)f32_to_f16_bits(__float_as_uint(x1)) << 16);
        rec[w] = word;
        const float h0 = half_lo(word), h1 = half_hi(word);
        finite = finite && (h0 - h0 == 0.0f) && (h1 - h1 == 0.0f) && (x0 - x0 == 0.0f) && (x1 - x1 == 0.0f);
        const double d0 = (double)x0 - (double)h0, d1 = (double)x1 - (double)h1;
        ss += d0 * d0 + d1 * d1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const bool all_finite = __ballot(!finite) == 0ull;
    if (lane == 0) {
        unsigned bits = 0x7f800000u; // +inf
        if (all_finite && ss < 1e300) {
            const double e = sqrt(ss);
            float f = (float)e;
            if ((double)f < e) f = __uint_as_float(__float_as_uint(f) + 1u); // (f >= 0: the next float up)
            f = f * 1.00000095367431640625f + 1e-37f; // the double sum's own rounding, and away from the subnormals
            bits = __float_as_uint(f);
        }
        atomicMax(e_bits, bits);
    }
}
// ---- the 8-bit shadow of the row prefilter (kFormLeanPF8Fixed; dk_sorted_top.h) ----
// words: [bits of E8, rows on the shadow, rows re-read, smallest key | largest key << 32, .., word kPf8GridWord: lo | step << 32] -- the
// key word as two 32-bit halves (the ordered keys of f2key, so that negative elements order like their values).
// 1. the smallest and the largest FINITE element of src[0 .. n_elems): keys start at {0xffffffff, 0}
__global__ void __launch_bounds__(256)
shadow8_range_kernel(const float *__restrict__ src, long long n_elems, unsigned *__restrict__ keys)
{
    unsigned kmin = 0xffffffffu, kmax = 0u;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n_elems; t += (long long)gridDim.x * 256) {
        const float x = src[t];
        if (x - x == 0.0f) { const unsigned k = f2key(x); kmin = k < kmin ? k : kmin; kmax = k > kmax ? k : kmax; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = (unsigned)__shfl_xor((int)kmin, o, 64), b = (unsigned)__shfl_xor((int)kmax, o, 64);
        kmin = a < kmin ? a : kmin; kmax = b > kmax ? b : kmax;
    }
    if ((threadIdx.x & 63) == 0 && kmin <= kmax) { atomicMin(keys, kmin); atomicMax(keys + 1, kmax); }
}
// 2. the grid of a FULL pack: lo = the smallest element, step = (hi - lo) / 255 rounded up (1 when hi == lo or no element is finite:
// any positive value will do); E8 starts over.  One thread.
__global__ void shadow8_grid_kernel(unsigned long long *__restrict__ words)
{
    const unsigned *keys = reinterpret_cast<const unsigned *>(words + 3);
    float lo = 0.0f, step = 1.0f;
    if (keys[0] <= keys[1]) {
        lo = key2f(keys[0]);
        const double s = ((double)key2f(keys[1]) - (double)lo) / 255.0;
        if (s > 0.0) {
            step = (float)s;
            if ((double)step < s) step = __uint_as_float(__float_as_uint(step) + 1u); // (a range beyond 255 FLT_MAX: +inf, and E8 with it)
        }
    }
    words[kPf8GridWord] = (unsigned long long)__float_as_uint(lo) | ((unsigned long long)__float_as_uint(step) << 32);
    words[0] = 0ull;
}
// 3. rows [first, first + n) -> their code bytes (element i at byte i of record r, kPfFixedDim bytes per record), one wave per row:
// the nearest grid point, clamped to [0, 255] -- rows packed later keep the grid and clamp.  Which point the encoder picks is not
// part of the proof: the bound is taken from the DECODED value h8 = fmaf(step, (float)c, lo), the search kernel's own expression,
// exactly as pack_shadow_rows_kernel takes E from h(x): squares of x - h8 summed in double, the root rounded up to float and raised
// by 2^-20, atomicMax on the bits; an element or a decoded value that is not finite makes E8 = +inf.
__global__ void __launch_bounds__(256)
pack_shadow8_rows_kernel(const float *__restrict__ src, long long first, long long n, unsigned char *__restrict__ dst, unsigned long long *__restrict__ words)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const unsigned long long grid = words[kPf8GridWord];
    const float lo = __uint_as_float((unsigned)grid), step = __uint_as_float((unsigned)(grid >> 32));
    const float *x = src + (size_t)(first + r) * kPfFixedDim;
    unsigned char *rec = dst + (size_t)(first + r) * kPfFixedDim;
    double ss = 0.0;
    bool finite = true;
    for (int i = lane; i < kPfFixedDim; i += 64) {
        const float xi = x[i];
        const double t = ((double)xi - (double)lo) / (double)step; // (in double: a float quotient near 255 is off by 3e-5 of a step, which picks the wrong side of a midpoint)
        const int c = t > 0.0 ? (t < 255.0 ? (int)__builtin_rint(t) : 255) : 0; // (NaN: 0)
        rec[i] = (unsigned char)c;
        const float h = __builtin_fmaf(step, (float)c, lo);
        finite = finite && (h - h == 0.0f) && (xi - xi == 0.0f);
        const double d = (double)xi - (double)h;
        ss += d * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const bool all_finite = __ballot(!finite) == 0ull;
    if (lane == 0) {
        unsigned bits = 0x7f800000u; // +inf
        if (all_finite && ss < 1e300) {
            const double e = sqrt(ss);
            float f = (float)e;
            if ((double)f < e) f = __uint_as_float(__float_as_uint(f) + 1u); // (f >= 0: the next float up)
            f = f * 1.00000095367431640625f + 1e-37f; // the double sum's own rounding, and away from the subnormals
            bits = __float_as_uint(f);
        }
        atomicMax(reinterpret_cast<unsigned *>(words), bits);
    }
}
// records -> the stored rows widened to float (hnswdev_download_rows on a half-precision context)
__global__ void __launch_bounds__(256)
unpack_f16_rows_kernel(const float *__restrict__ recs, long long first, int n, int dim, float *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)n * dim) return;
    const int r = (int)(t / dim), i = (int)(t % dim);
    out[t] = row_elem<M_SQH>(recs + (size_t)(first + r) * f16_row_words(dim), i);
}
#endif
#ifdef HNSW_HOST_TU
constexpr int kGatherBlock = 256;
// Thread per (row, element): out[i][e] = element e of the stored row ids[i], as f32 -- the rows of an id list back out
// (hnswdev_gather_rows) or as a query set on the device (repair_reachability, the by-id calls: DESIGN.md 3.21, 3.27).
// kind 0: f32 rows (a copy); 1: half-precision records widened (unpack_f16_rows_kernel's value); 2: int8 records dequantised,
// q * scale (dequantize_rows_kernel's value).  pitch: words per stored row.  An id outside [0, n_rows) gives a row of zeros.
__global__ void __launch_bounds__(kGatherBlock)
gather_rows_kernel(const float *__restrict__ rows, int pitch, long long n_rows, int kind, const int *__restrict__ ids, long long n_ids, int dim,
                           float *__restrict__ out)
{
    const long long total = n_ids * dim, step = (long long)gridDim.x * kGatherBlock;
    for (long long t = (long long)blockIdx.x * kGatherBlock + threadIdx.x; t < total; t += step) {
        const long long i = t / dim;
        const int e = (int)(t - i * dim);
        const long long id = ids[i];
        float x = 0.0f;
        if ((unsigned long long)id < (unsigned long long)n_rows) {
            const float *rec = rows + (size_t)id * pitch;
            if (kind == 1) x = row_elem<M_SQH>(rec, e);
            else if (kind == 2) {
                const int *r = reinterpret_cast<const int *>(rec);
                x = (float)(int)(signed char)((r[e >> 2] >> (8 * (e & 3))) & 0xff) * __int_as_float(r[pitch - 2]);
            } else x = rec[e];
        }
        out[t] = x;
    }
}
#endif
#ifdef HNSW_HOST_TU
// knn_query_collapsed: the rows of a traversal's answer, still on the device, collapsed in place.  One wave per row
// of `width` entries (ids and distances, ascending as the traversal left them, padded with -1): the row and the labels of its
// entries go to LDS first, then the wave walks the entries in order -- an entry is kept while fewer than m kept entries have its
// label, counted with one ballot per 64 kept entries -- and lane 0 writes the kept entry to the next place of the row's first k
// columns; what is left of those is padded with -1 / NaN.  Padding, and an id without a label (id >= n_labels: a row that was
// handed back holds nothing meaningful), is skipped.  Every loop bound and branch is the same in all lanes of the wave.
// LDS: width x 12 bytes + k x 4 bytes.
__global__ void __launch_bounds__(64) collapse_rows_kernel(int *__restrict__ ids, float *__restrict__ d, int width, int k, const int *__restrict__ labels,
                                                           long long n_labels, int m)
{
    extern __shared__ int collapse_lds[];
    int *r_id = collapse_lds, *r_lab = r_id + width, *kept_lab = r_lab + width;
    float *r_d = reinterpret_cast<float *>(kept_lab + k);
    const int lane = threadIdx.x;
    int *row_ids = ids + (size_t)blockIdx.x * width;
    float *row_d = d + (size_t)blockIdx.x * width;
    for (int i = lane; i < width; i += 64) {
        const int id = row_ids[i];
        const bool real = id >= 0 && id < n_labels;
        r_id[i] = real ? id : -1;
        r_d[i] = row_d[i];
        r_lab[i] = real ? labels[id] : 0;
    }
    wave_lds_sync();
    int kept = 0;
    for (int e = 0; e < width && kept < k; ++e) {
        const int id = r_id[e], g = r_lab[e]; // (the same address in every lane)
        int same = 0;
        for (int base = 0; base < kept; base += 64) same += __popcll(__ballot(base + lane < kept && kept_lab[base + lane] == g));
        const bool keep = id >= 0 && same < m;
        if (keep && lane == 0) { row_ids[kept] = id; row_d[kept] = r_d[e]; kept_lab[kept] = g; }
        wave_lds_sync();
        kept += keep ? 1 : 0;
    }
    for (int i = kept + lane; i < k; i += 64) { row_ids[i] = -1; row_d[i] = __uint_as_float(0x7fc00000u); }
}
#endif
#ifdef HNSW_HOST_TU // non-template kernels: only the unit that launches them defines them
__global__ void sqrt_rn_kernel(const double *in, double *out, int n)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sqrt_rn(in[i]);
}
#endif

} // namespace hnsw
