// dk_tag_lists.h -- device code of the tagged calls' candidate lists (knn_query_tagged / exact_knn_query_tagged).
// Included by device_backend.hip only: these kernels read tag words, not rows, so they have no metric and live in that unit beside
// the small kernels.
//
// row_tags[id] is a word of 32 tag bits; masks[0 .. D) are the distinct query masks of a call.  Id `id` is a candidate of mask m
// when tag_match(row_tags[id], m, all): (w & m) != 0 for "any", (w & m) == m with m != 0 for "all".  Unlike a group label a word can
// match several masks, so the lists overlap and a row is tested against every mask: D x n tests in all.
//
// A block holds kTagRows consecutive rows in registers, kTagRowsPerThread per thread, and walks a tile of kTagMaskTile masks staged
// in LDS.  Per mask every wave ballots its rows' matches, so a mask costs a wave a handful of scalar bit counts:
//   tag_count_kernel  adds the bit counts into per-mask counters in LDS, flushed to counts[] once per block;
//   tag_offsets_kernel turns the counts of one batch of masks into their segments' offsets (and cursors) in one CSR;
//   tag_fill_kernel   takes, per wave and mask, one place range from the mask's cursor and writes the matching ids there -- the
//                     order inside a segment is that of the atomics: unordered, as exact_group_kernel<true> leaves a group's.
// Only the counts go back to the host.  No kernel waits for another wave.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hnsw {

constexpr int kTagBlock = 256;
constexpr int kTagRowsPerThread = 4;
constexpr int kTagRows = kTagBlock * kTagRowsPerThread; // rows of a block
constexpr int kTagMaskTile = 1024;                      // masks a block walks (grid.y tiles the call's masks)

__device__ __forceinline__ bool tag_match(unsigned w, unsigned m, int all)
{
    const unsigned x = w & m;
    return x != 0u && (!all || x == m);
}

// The block's rows: thread t holds rows base + r * kTagBlock + t (coalesced per r); a row past n carries the word 0 and matches nothing.
__device__ __forceinline__ void tag_load_rows(const unsigned *__restrict__ row_tags, long long n, long long base, unsigned (&w)[kTagRowsPerThread])
{
#pragma unroll
    for (int r = 0; r < kTagRowsPerThread; ++r) {
        const long long id = base + (long long)r * kTagBlock + threadIdx.x;
        w[r] = id < n ? row_tags[id] : 0u;
    }
}

// counts[d] += the rows of this block that match masks[d], for the masks of tile blockIdx.y.  counts is zeroed by the launcher.
__global__ void __launch_bounds__(kTagBlock) tag_count_kernel(const unsigned *__restrict__ row_tags, long long n, const unsigned *__restrict__ masks, int n_masks,
                                                              int all, int *__restrict__ counts)
{
    __shared__ unsigned s_mask[kTagMaskTile];
    __shared__ int s_cnt[kTagMaskTile];
    const int lane = threadIdx.x & 63;
    const int d0 = blockIdx.y * kTagMaskTile, nm = min(kTagMaskTile, n_masks - d0);
    for (int i = threadIdx.x; i < nm; i += kTagBlock) { s_mask[i] = masks[d0 + i]; s_cnt[i] = 0; }
    unsigned w[kTagRowsPerThread];
    tag_load_rows(row_tags, n, (long long)blockIdx.x * kTagRows, w);
    __syncthreads();
    for (int i = 0; i < nm; ++i) { // (nm is the same for all threads)
        const unsigned m = s_mask[i];
        int c = 0;
#pragma unroll
        for (int r = 0; r < kTagRowsPerThread; ++r) c += __popcll(__ballot(tag_match(w[r], m, all)));
        if (lane == 0 && c) atomicAdd(&s_cnt[i], c);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nm; i += kTagBlock)
        if (s_cnt[i]) atomicAdd(&counts[d0 + i], s_cnt[i]);
}

// offsets[i] = cursors[i] = the counts in front of entry i, i < n_masks (one batch of masks, whose counts sum to less than 2^31).
// One block walks the counts kTagBlock at a time: a wave prefix by shuffles, the wave totals through LDS, the running total carried
// by every thread.
__global__ void __launch_bounds__(kTagBlock) tag_offsets_kernel(const int *__restrict__ counts, int n_masks, int *__restrict__ offsets, int *__restrict__ cursors)
{
    __shared__ int wave_total[kTagBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n_masks; base += kTagBlock) { // (n_masks is the same for all threads: so is every barrier)
        const int d = base + tid;
        const int c = d < n_masks ? counts[d] : 0;
        int incl = c;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int o = __shfl_up(incl, s, 64);
            if (lane >= s) incl += o;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int pos = carry + incl - c, total = 0;
        for (int i = 0; i < kTagBlock / 64; ++i) {
            if (i < wave) pos += wave_total[i];
            total += wave_total[i];
        }
        if (d < n_masks) { offsets[d] = pos; cursors[d] = pos; }
        carry += total;
        __syncthreads(); // wave_total is written again in the next step
    }
}

// The members of every mask of the batch into its segment of ids[0 .. cap): per mask a wave counts its matches, lane 0 takes that
// many places from the mask's cursor, and the matching lanes write their ids behind one another, row set by row set.  cap: the
// entries the batch's segments hold together -- nothing is written at or past it, whatever the cursors say.
__global__ void __launch_bounds__(kTagBlock) tag_fill_kernel(const unsigned *__restrict__ row_tags, long long n, const unsigned *__restrict__ masks, int n_masks,
                                                             int all, int *__restrict__ cursors, int *__restrict__ ids, long long cap)
{
    __shared__ unsigned s_mask[kTagMaskTile];
    const int lane = threadIdx.x & 63;
    const int d0 = blockIdx.y * kTagMaskTile, nm = min(kTagMaskTile, n_masks - d0);
    for (int i = threadIdx.x; i < nm; i += kTagBlock) s_mask[i] = masks[d0 + i];
    unsigned w[kTagRowsPerThread];
    const long long base = (long long)blockIdx.x * kTagRows;
    tag_load_rows(row_tags, n, base, w);
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int i = 0; i < nm; ++i) {
        const unsigned m = s_mask[i];
        unsigned long long b[kTagRowsPerThread];
        int c = 0;
#pragma unroll
        for (int r = 0; r < kTagRowsPerThread; ++r) { b[r] = __ballot(tag_match(w[r], m, all)); c += __popcll(b[r]); }
        if (c == 0) continue; // (wave-uniform)
        int first = 0;
        if (lane == 0) first = atomicAdd(&cursors[d0 + i], c);
        long long at = (long long)__shfl(first, 0, 64);
#pragma unroll
        for (int r = 0; r < kTagRowsPerThread; ++r) {
            const long long pos = at + __popcll(b[r] & below);
            if (((b[r] >> lane) & 1ull) && pos >= 0 && pos < cap) ids[pos] = (int)(base + (long long)r * kTagBlock + threadIdx.x);
            at += __popcll(b[r]);
        }
    }
}

inline dim3 tag_grid(long long n, int n_masks)
{
    return dim3((unsigned)((n + kTagRows - 1) / kTagRows), (unsigned)((n_masks + kTagMaskTile - 1) / kTagMaskTile));
}

// counts[0 .. n_masks) of row_tags[0 .. n) (n >= 1, n_masks >= 1)
inline hipError_t tag_counts_launch(const unsigned *row_tags, long long n, const unsigned *masks, int n_masks, int all, int *counts, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)n_masks, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tag_count_kernel, tag_grid(n, n_masks), dim3(kTagBlock), 0, st, row_tags, n, masks, n_masks, all, counts);
    return hipGetLastError();
}

// The CSR of one batch of masks: masks / counts / offsets / cursors point at the batch's first entry, ids holds `cap` entries (the
// sum of the batch's counts).
inline hipError_t tag_lists_launch(const unsigned *row_tags, long long n, const unsigned *masks, int n_masks, int all, const int *counts, int *offsets, int *cursors,
                                   int *ids, long long cap, hipStream_t st)
{
    hipLaunchKernelGGL(tag_offsets_kernel, dim3(1), dim3(kTagBlock), 0, st, counts, n_masks, offsets, cursors);
    hipLaunchKernelGGL(tag_fill_kernel, tag_grid(n, n_masks), dim3(kTagBlock), 0, st, row_tags, n, masks, n_masks, all, cursors, ids, cap);
    return hipGetLastError();
}

} // namespace hnsw
