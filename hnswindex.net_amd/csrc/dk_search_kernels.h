// dk_search_kernels.h -- device code, part of device_kernels.h: KnnQuery / MultiLayerKnnQuery / RangeQuery: search_job, graph_search_kernel (persistent, shadows, gated upload), predicate_search with its kernels graph_search_filtered_kernel (allow-sets), graph_search_grouped_kernel (a group per query), graph_search_tagged_kernel (a tag mask per query), graph_search_self_kernel (every id but the query's own), graph_multilayer_kernel (layer chains), graph_range_kernel.
#pragma once
#include "dk_sorted_top.h"
#include "dk_pool_top.h"
#include "dk_traverse_exact.h"

namespace hnsw {

// Sorted-list traversal with NS register sets (k <= 64 * NS); a wave that meets equal distances where the heap layout
// shows starts over with the exact two-heap traversal (out_flag 2, informational).  Launch flag 0x200 (beams beyond 512
// entries, HNSW_MI355X_SORTED_TOP=0): the two-heap traversal only.
// One job on this wave.  `vis` / `spill`: the wave's own scratch (vis all zero on entry; the caller
// clears it afterwards).
// Job words of a launch with SHADOW traversals (graph_search_kernel): bit 0 answered (results written), bit 1 the
// wave that owns the job met a tie, bit 2 a shadow traversal has been started for it.
constexpr int kJobAnswered = 1, kJobTied = 2, kJobShadowed = 4;

// graph_search_kernel's parameter list as a struct (same order, same types: the kernarg segment's layout) -- see kernarg_load
struct SearchKernArgs {
    const float *rows; const double *row_sn; const float *queries; const double *q_sn; int dim; const int *adj0; int stride0;
    const int64_t *upper; const int *pool; int strideU; const SearchJob *jobs; int k, cand_cap; ND *spill; int spill_cap;
    unsigned *visited; long long vis_words; int *vis_tab; int vis_tab_cap, k_out; int *out_ids; float *out_d; int *out_cnt, *out_flag;
    unsigned long long *eval_counter; int nbcap, njobs; int *job_counter; int overlap; const int *ready;
    const float *pf_rows; unsigned long long *pf_words; // the row prefilter (kFormLeanPF, kFormLeanPFFixed): shadow records; [E's bits, rows on the shadow, rows re-read]; kFormLeanPF8Fixed: the code bytes; [E8's bits, on the shadow, re-read, .., word kPf8GridWord: lo | step << 32]
};
static_assert(offsetof(SearchKernArgs, jobs) == 80 && offsetof(SearchKernArgs, out_ids) == 144 && offsetof(SearchKernArgs, ready) == 208 &&
              offsetof(SearchKernArgs, pf_rows) == 216 && offsetof(SearchKernArgs, pf_words) == 224 && sizeof(SearchKernArgs) == 232,
              "SearchKernArgs must mirror graph_search_kernel's parameter list (the explicit arguments start the kernarg segment, each at its natural alignment)");
#define HNSW_KA(field) kernarg_load<decltype(SearchKernArgs::field)>((unsigned)offsetof(SearchKernArgs, field))

// KnnQuery's tail (HNSWIndex.cs:119-123): OrderBy(c => c.Dist) is a STABLE sort over the heap
// array (ToArray(), BinaryHeap.cs:41-44) and only the first k_out survive -- so select the
// k_out smallest (float.CompareTo order: NaN first, -0 == +0) with ties broken by array index:
// exactly the stable sort's prefix.  Key = (order-preserving bits << 32) | index, wave min.
// L.top[0 .. top_n) holds float distances; writes row `row` of out_ids / out_d (k_out entries, padded).
// CHAIN (a step of MultiLayerKnnQuery on layer `row`, graph_multilayer_kernel): rank 0 is not stored -- when there is one it becomes
// *next, the entry of the layer below (wave-uniform) -- and ranks 1 .. k_out - 1 fill row `row` of rows `per` = k_out - 1 entries (the
// caller's own value: it addresses its slab with it); one store point per rank, no `continue`.  One ranking loop, two
// tails that are the kernels' code as it was: a shared step FUNCTION changed graph_search_kernel's instructions.
struct ChainEntry { int node, layer; };
template <bool CHAIN = false>
__device__ __forceinline__ void take_stable(const SearchLds &L, int lane, int top_n, int k_out, int *__restrict__ out_ids, float *__restrict__ out_d, int row,
                                            ChainEntry *next = nullptr, int per = 0)
{
    wave_sync();
    unsigned long long used = 0; // bit t: entry lane + 64*t already emitted
    for (int r = 0; r < k_out; ++r) {
        unsigned long long best = ~0ull;
        for (int t = 0, i = lane; i < top_n; ++t, i += 64) {
            if ((used >> t) & 1ull) continue;
            float d = L.top[i].dist;
            unsigned u;
            if (d != d) u = 0u;                      // NaN sorts first
            else {
                if (d == 0.0f) d = 0.0f;             // -0 and +0 compare equal
                u = __float_as_uint(d);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
                if (u == 0u) u = 1u;                 // keep NaN's key unique (only -NaN-like bit patterns reach 0)
            }
            unsigned long long key = ((unsigned long long)u << 32) | (unsigned)i;
            best = key < best ? key : best;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            unsigned long long o = __shfl_xor(best, off, 64);
            best = o < best ? o : best;
        }
        if constexpr (CHAIN) {
            const bool have = best != ~0ull;
            const int wi = have ? (int)(best & 0xffffffffu) : 0;
            if (have && (wi & 63) == lane) used |= 1ull << (wi >> 6);
            ND w{-1, __uint_as_float(0x7fc00000u)};
            if (have) w = L.top[wi]; // (every lane reads the same entry)
            if (r == 0) {
                if (have) { next->node = __builtin_amdgcn_readfirstlane(w.id); next->layer = row - 1; } // candidates[0] enters the next layer down: no descent
            } else if (lane == 0) {
                out_ids[(size_t)row * per + (r - 1)] = w.id;
                out_d[(size_t)row * per + (r - 1)] = w.dist;
            }
        } else {
            if (best == ~0ull) { // fewer than k_out results: pad (HNSWIndexExports.cs:144)
                if (lane == 0) { out_ids[(size_t)row * k_out + r] = -1; out_d[(size_t)row * k_out + r] = __uint_as_float(0x7fc00000u); }
                continue;
            }
            const int wi = (int)(best & 0xffffffffu);
            if ((wi & 63) == lane) used |= 1ull << (wi >> 6);
            if (lane == 0) { ND w = L.top[wi]; out_ids[(size_t)row * k_out + r] = w.id; out_d[(size_t)row * k_out + r] = w.dist; }
        }
    }
}

template <int METRIC, int NS, bool HASHED, int FORM = kFormPlain>
__device__ __forceinline__ void search_job(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                    const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                    const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU,
                    const SearchJob *__restrict__ jobs, int k, int cand_cap, ND *__restrict__ spill,
                    int spill_cap, VisitedSet<HASHED> &V, int k_out, int *__restrict__ out_ids,
                    float *__restrict__ out_d, int *__restrict__ out_cnt, int *__restrict__ out_flag,
                    unsigned long long *__restrict__ eval_counter, int nbcap, unsigned char *smem, int job, int overlap,
                    int *__restrict__ job_word = nullptr, bool shadow = false, TeamPort *port = nullptr, bool *v_untouched = nullptr)
{
    constexpr bool LAT = FORM == kFormLat, LEAN = form_is_lean(FORM), PF = form_is_pf(FORM);
    if constexpr (LEAN) { // (what only the start and the end of a job need is read where it is needed: kernarg_load)
        cand_cap = HNSW_KA(cand_cap); nbcap = HNSW_KA(nbcap); jobs = HNSW_KA(jobs); queries = HNSW_KA(queries); q_sn = HNSW_KA(q_sn);
    }
    const SearchLds L = carve_lds(smem, k, cand_cap, dim, nbcap);
    const int lane = threadIdx.x & 63;
    if (v_untouched) *v_untouched = false;
    const SearchJob jb = jobs[job];
    const GraphView G{adj0, stride0, upper, pool, strideU};

    const float *q;
    double sb = 0.0;
    if (jb.qref >= 0) {
        q = queries + (size_t)jb.qref * dim;
        if (METRIC == M_COS) sb = q_sn[jb.qref];
    } else {
        q = row_at<METRIC>(rows, (size_t)(~jb.qref), dim);
        if (METRIC == M_COS) sb = row_sn[~jb.qref];
    }
    if constexpr (metric_f16(METRIC)) { // a stored row as the query is unpacked to f32; a query is f32 as it is
        if (jb.qref >= 0) for (int i = lane; i < dim; i += 64) L.qs[i] = q[i];
        else for (int i = lane; i < dim; i += 64) L.qs[i] = row_elem<METRIC>(q, i);
    } else
    for (int i = lane; i < dim; i += 64) L.qs[i] = q[i];
    if constexpr (LAT) { if (lane == 0) port->m->sb = sb; } // (the memory wave reads both after the first request's release)
    unsigned long long evals = 0;
    int top_n = 0;
    bool repeated = shadow;
    ReadLog RL{nullptr, 0, 0};
    // With shadows, whoever sets kJobAnswered first writes the job's results (both traversals compute the same ones).
    auto claim_answer = [&]() -> bool {
        if (!job_word) return true;
        int old = 0;
        if (lane == 0) old = atomicOr(job_word, kJobAnswered);
        return (__builtin_amdgcn_readfirstlane(old) & kJobAnswered) == 0;
    };
    if constexpr (NS > 0) {
        if (jb.aux != -2 && !shadow && !(overlap & 0x200)) { // (0x200: this launch runs the exact two-heap traversal only)
        bool tie = false;
        // OrderBy + Take(k_out) reads k_out entries in order and decides between entries k_out - 1 and k_out
        bool window = false;
        bool ok1;
        if constexpr (LAT) ok1 = traverse_pool<METRIC, NS, HASHED>(rows, row_sn, dim, sb, G, jb, k, k_out + 1, V, L, lane, top_n, tie, evals, RL, nullptr, &window, port);
        else if constexpr (PF) {
            // E is read once per job (a scalar load); the job's two row counts go to the words behind it
            unsigned long long *const words = HNSW_KA(pf_words);
            RowPrefilterIo pf{nullptr, 0.0f, row_prefilter_c(dim), 0u, 0u, (unsigned)offsetof(SearchKernArgs, pf_rows), (unsigned)offsetof(SearchKernArgs, pf_words)};
            if constexpr (!form_is_pf8(FORM)) { pf.rows = HNSW_KA(pf_rows); pf.e = __uint_as_float(*reinterpret_cast<const unsigned *>(words)); }
            ok1 = traverse_sorted<METRIC, NS, HASHED, true, true, form_is_pf8(FORM), form_measure_cap(FORM)>(rows, row_sn, dim, sb, G, jb, k, k_out + 1, V, L, lane, top_n, tie, evals, overlap, RL, nullptr, &window, &pf);
            if (lane == 0) { atomicAdd(words + 1, (unsigned long long)pf.n_shadow); atomicAdd(words + 2, (unsigned long long)pf.n_reread); }
        }
        else ok1 = traverse_sorted<METRIC, NS, HASHED, LEAN>(rows, row_sn, dim, sb, G, jb, k, k_out + 1, V, L, lane, top_n, tie, evals, overlap, RL, nullptr, &window);
        if (!(ok1 && tie)) {
            if (v_untouched) *v_untouched = LEAN || (!LAT && (overlap & 8) != 0); // the sorted traversal ran without a visited set: nothing to clear
            if (!claim_answer()) return;
            if constexpr (LEAN) {
                k_out = HNSW_KA(k_out); out_ids = HNSW_KA(out_ids); out_d = HNSW_KA(out_d); out_cnt = HNSW_KA(out_cnt); out_flag = HNSW_KA(out_flag);
                eval_counter = HNSW_KA(eval_counter);
            }
            // KnnQuery's tail (HNSWIndex.cs:119-123): OrderBy(Dist).Take(k) of distinct distances is the
            // head of the ascending list; missing results are padded (HNSWIndexExports.cs:144)
            for (int r = lane; r < k_out; r += 64) {
                const bool have = r < top_n;
                out_ids[(size_t)job * k_out + r] = have ? L.top[r].id : -1;
                out_d[(size_t)job * k_out + r] = have ? L.top[r].dist : __uint_as_float(0x7fc00000u);
            }
            if (lane == 0) {
                out_cnt[job] = ok1 ? top_n : 0;
                out_flag[job] = ok1 ? (window ? 4 : 0) : 1; // 4: informational (a group window of equal distances closed cleanly)
                atomicAdd(eval_counter, evals);
            }
            return;
        }
        // equal distances where the heap layout shows: the exact traversal answers this job -- the shadow that an
        // idle wave has already started for it (see graph_search_kernel), or this wave, starting over
        if (job_word) {
            int old = 0;
            if (lane == 0) old = atomicOr(job_word, kJobTied);
            if (__builtin_amdgcn_readfirstlane(old) & (kJobShadowed | kJobAnswered)) return;
        }
        if constexpr (!LEAN) V.clear(lane); // (the lean form's sorted traversal has no visited set)
        evals = 0;
        top_n = 0;
        repeated = true;
        }
    }
    bool aborted = false;
    bool ok;
    if constexpr (LEAN) {
        // the lean kernel carries neither its visited set nor its spill area from job to job: both are looked up here, for the one job
        // in several hundred that takes this path, and the set is left clean again
        cand_cap = HNSW_KA(cand_cap);
        const int spill_cap_ = HNSW_KA(spill_cap);
        const long long vis_words = HNSW_KA(vis_words);
        int *const vis_tab = HNSW_KA(vis_tab);
        const int vis_tab_cap = HNSW_KA(vis_tab_cap);
        VisitedSet<HASHED> VE{HNSW_KA(visited) + (size_t)blockIdx.x * (size_t)vis_words, vis_words,
                              vis_tab ? vis_tab + (size_t)blockIdx.x * (size_t)vis_tab_cap : nullptr, (unsigned)(vis_tab_cap - 1), 0, vis_tab_cap / 4 * 3};
        ok = traverse<METRIC, HASHED, false, AllowSet, form_measure_cap(FORM)>(rows, row_sn, dim, sb, G, jb, k, cand_cap, HNSW_KA(spill) + (size_t)blockIdx.x * spill_cap_, spill_cap_, VE, L, lane, top_n, evals, RL,
                                      shadow ? job_word : nullptr, &aborted, true);
        VE.clear(lane);
        if (v_untouched) *v_untouched = true;
        if (!aborted) {
            k_out = HNSW_KA(k_out); out_ids = HNSW_KA(out_ids); out_d = HNSW_KA(out_d); out_cnt = HNSW_KA(out_cnt); out_flag = HNSW_KA(out_flag);
            eval_counter = HNSW_KA(eval_counter);
        }
    } else
    ok = traverse<METRIC, HASHED>(rows, row_sn, dim, sb, G, jb, k, cand_cap, spill, spill_cap, V, L, lane, top_n, evals, RL,
                                             shadow ? job_word : nullptr, &aborted, LAT || (overlap & 1) != 0 || repeated);
    if (aborted || !claim_answer()) return;
    if (jb.aux == -2) { // SearchLayer's own return value: topCandidates.ToArray(), the heap's array (BinaryHeap.cs:41-44)
        wave_sync();
        for (int r = lane; r < k_out; r += 64) {
            const bool have = ok && r < top_n;
            out_ids[(size_t)job * k_out + r] = have ? L.top[r].id : -1;
            out_d[(size_t)job * k_out + r] = have ? L.top[r].dist : __uint_as_float(0x7fc00000u);
        }
        if (lane == 0) {
            out_cnt[job] = ok ? top_n : 0;
            out_flag[job] = ok ? 0 : 1;
            atomicAdd(eval_counter, evals);
        }
        return;
    }
    take_stable(L, lane, top_n, k_out, out_ids, out_d, job);
    if (lane == 0) {
        out_cnt[job] = ok ? top_n : 0;
        out_flag[job] = ok ? (repeated ? 2 : 0) : 1; // 2: informational (answered by the exact traversal)
        atomicAdd(eval_counter, evals);
    }
}

// Persistent launch: one wave per block, as many blocks as stay resident; each takes jobs from a
// shared counter until none are left.  A wave owns one visited bitset and one spill area for the
// whole launch and leaves the bitset clean after every job, so the scratch is sized by the
// resident waves (not by the batch) and nothing is memset between launches.
template <int METRIC, int NS, bool HASHED, int FORM = kFormPlain>
// float rows: 168 VGPRs, three waves per SIMD; int8 records keep 16 registers of rows in flight, not 64: five waves.
// The fixed-length row-prefilter form (kFormLeanPFFixed): 124-128 VGPRs, four waves.
// Its 8-bit variant (kFormLeanPF8Fixed): every f32 pass of the kernel -- survivor re-read, descent, the exact traversal of a tied
// job -- takes 16 rows, not 32 (form_measure_cap: 32 VGPRs of rows in flight, not 64): 91-96 VGPRs, nothing spilled, FIVE waves
// (profiles/pf8_waves_kernel_resources.json).
// LAT (launches that do not fill the chip): no occupancy to buy -- every spilled register is a memory round trip a lone wave
// waits out in full -- so two waves per SIMD at most (256 VGPRs), one with eight register sets
__global__ void __launch_bounds__(FORM == kFormLat ? 128 : 64) __attribute__((amdgpu_waves_per_eu(HNSW_WAVES(FORM == kFormLat ? (NS <= 4 ? 2 : 1) : FORM == kFormLeanPF ? HNSW_PF_WAVES : FORM == kFormLeanPFFixed ? HNSW_PF_FIXED_WAVES : FORM == kFormLeanPF8Fixed ? HNSW_PF8_WAVES : METRIC == M_I8 ? (NS <= 2 ? HNSW_I8_WAVES : 4) : (NS <= 4 ? 3 : 2)))))
graph_search_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                    const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                    const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU,
                    const SearchJob *__restrict__ jobs, int k, int cand_cap, ND *__restrict__ spill,
                    int spill_cap, unsigned *__restrict__ visited, long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap, int k_out,
                    int *__restrict__ out_ids, float *__restrict__ out_d, int *__restrict__ out_cnt, int *__restrict__ out_flag,
                    unsigned long long *__restrict__ eval_counter, int nbcap, int njobs, int *__restrict__ job_counter, int overlap,
                    const int *__restrict__ ready, const float *__restrict__ pf_rows, unsigned long long *__restrict__ pf_words)
{
    constexpr bool LAT = FORM == kFormLat, LEAN = form_is_lean(FORM);
    if constexpr (form_is_pf(FORM) && METRIC != M_SQ) return; // (the row prefilter exists for sq_euclid on f32 rows: never launched elsewhere)
    else {
    if constexpr (form_is_pf_fixed(FORM)) dim = kPfFixedDim; // (the launch site checks that the argument is this value: place_traversal)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    // (the lean form looks its visited set and spill area up when a job takes the exact traversal: search_job)
    VisitedSet<HASHED> V{LEAN ? nullptr : visited + (size_t)blockIdx.x * (size_t)vis_words, LEAN ? 0 : vis_words,
                 !LEAN && vis_tab ? vis_tab + (size_t)blockIdx.x * (size_t)vis_tab_cap : nullptr, LEAN ? 0u : (unsigned)(vis_tab_cap - 1), 0, LEAN ? 0 : vis_tab_cap / 4 * 3};
    ND *my_spill = LEAN ? nullptr : spill + (size_t)blockIdx.x * spill_cap;

    TeamPort port{nullptr, 0, 0};
    if constexpr (LAT) {
        // two waves per block (see TeamMail): wave 1 serves the expansions, wave 0 is the traversal.  The mailbox follows
        // the traversal's LDS; its sequence words are zeroed before the roles part (the one barrier both waves meet at).
        TeamMail *mail = reinterpret_cast<TeamMail *>(smem + ((search_lds_bytes(k, cand_cap, dim, false, nbcap) + 15) & ~(size_t)15));
        if (threadIdx.x == 0) { mail->req_seq = 0; mail->rsp_seq = 0; mail->hint_node = -1; }
        __syncthreads();
        if (threadIdx.x >= 64) {
            const GraphView G{adj0, stride0, upper, pool, strideU};
            const SearchLds L = carve_lds(smem, k, cand_cap, dim, nbcap);
            memory_wave<METRIC, HASHED>(rows, row_sn, dim, G, V, L.qs, mail, lane);
            return;
        }
        port.m = mail;
    }
    // `ready` (hnsw_knn_query on host buffers): the launch started when the first rows of the query set had landed; the
    // rest is still arriving on the copy engine, and *ready (a word in host memory the uploading thread advances) says how
    // many rows are there.  Jobs are taken in order, so a wave almost never has to wait; when it does it sleeps and
    // polls, for a bounded time -- a job whose row has not arrived by then is handed back (flag 1), never waited for.
    // SHADOW traversals (overlap bit 8; job_counter then is [next job, next shadow, -, -, one word per job ...], all zero
    // at launch).  One traversal in 700 meets equal distances where the heap layout shows and starts over in the exact
    // two-heap form, three times as long as the sorted one; whenever that happened to one of the LAST jobs of a launch,
    // the whole launch waited for it -- 7 % of a 65 536-query launch at C2, 17-35 % of the 12 500-query launches
    // (measured with the re-runs compiled out).  So a wave that finds the queue empty does not leave: it starts the
    // exact traversal of a job another wave is still working on, latest job first.  Almost always the owner answers the
    // job soon after and the shadow stops at its next expansion; when the owner meets a tie it finds the exact
    // traversal already under way and leaves it to the shadow.  Results are written by whoever finishes first -- both
    // compute the reference's answer.
    bool shadows = (overlap & 0x100) != 0 && NS > 0 && !(overlap & 0x200);
    int *job_words = job_counter + 4;
    int known_ready = 0;
    bool v_clean = false;
    for (;;) {
        if constexpr (LEAN) { // what the queue needs, read per job instead of carried through the traversal (kernarg_load)
            job_counter = HNSW_KA(job_counter); njobs = HNSW_KA(njobs); ready = HNSW_KA(ready); jobs = HNSW_KA(jobs); overlap = HNSW_KA(overlap);
            out_cnt = HNSW_KA(out_cnt); out_flag = HNSW_KA(out_flag);
            job_words = job_counter + 4;
            shadows = (overlap & 0x100) != 0 && !(overlap & 0x200);
        }
        int job = 0;
        bool shadow = false;
        if (lane == 0) job = atomicAdd(job_counter, 1);
        job = __builtin_amdgcn_readfirstlane(job);
        if (job >= njobs) {
            if (!shadows) break;
            int t = 0;
            if (lane == 0) t = atomicAdd(job_counter + 1, 1);
            t = __builtin_amdgcn_readfirstlane(t);
            if (t >= njobs || t >= (int)gridDim.x) break; // only the last gridDim.x jobs can still be running
            job = njobs - 1 - t;
            if (ready) {
                // a gated launch (query rows still arriving): no shadow for a job whose row has not landed -- its owner is
                // asleep at the gate and search_job would read whatever the previous call left in that row
                const int need = __builtin_amdgcn_readfirstlane(jobs[job].qref);
                if (need >= known_ready) {
                    int r = 0;
                    if (lane == 0) r = __hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    known_ready = __builtin_amdgcn_readfirstlane(r);
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                    if (need >= known_ready) continue;
                }
            }
            int old = 0;
            if (lane == 0) old = atomicOr(job_words + job, kJobShadowed);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old & (kJobAnswered | kJobTied)) continue; // answered, or its owner is already starting over
            shadow = true;
        } else if (ready) {
            const int need = __builtin_amdgcn_readfirstlane(jobs[job].qref);
            if (need >= known_ready) {
                // a read of host memory per poll: few polls, far apart (thousands of waves polling back to back were
                // measured to starve the very copy they wait for) -- 512 x ~0.2 ms at most, then the job is handed back
                for (int spin = 0; spin < 512; ++spin) {
                    int r = 0;
                    if (lane == 0) r = __hip_atomic_load(ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    known_ready = __builtin_amdgcn_readfirstlane(r);
                    if (need < known_ready) break;
                    for (int z = 0; z < 48; ++z) __builtin_amdgcn_s_sleep(127);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); // the rows read next were written by the copy engine
                if (need >= known_ready) {
                    // handed back.  With shadows the job word decides who answers, exactly as for a tie (search_job): a
                    // shadow that started because the row landed meanwhile keeps the job; otherwise this wave claims it.
                    int old = 0;
                    if (shadows && lane == 0) {
                        old = atomicOr(job_words + job, kJobTied);
                        if (!(old & (kJobShadowed | kJobAnswered))) old = atomicOr(job_words + job, kJobAnswered) & kJobAnswered;
                    }
                    old = __builtin_amdgcn_readfirstlane(old);
                    if (old == 0 && lane == 0) {
                        out_cnt[job] = 0;
                        out_flag[job] = 1;
                    }
                    continue;
                }
            }
        }
        search_job<METRIC, NS, HASHED, FORM>(rows, row_sn, queries, q_sn, dim, adj0, stride0, upper, pool, strideU, jobs, k, cand_cap, my_spill, spill_cap,
                               V, k_out, out_ids, out_d, out_cnt, out_flag, eval_counter, nbcap, smem, job, overlap, shadows ? job_words + job : nullptr,
                               shadow, &port, &v_clean);
        if (!v_clean) V.clear(lane);
    }

    if constexpr (LAT) port.post(-1, 0, lane); // the memory wave leaves
    }
}
#define HNSW_SEARCH_SIGNATURE(PREFIX, M, NS, H, LT)                                                                                  \
    PREFIX template __global__ void graph_search_kernel<M, NS, H, LT>(                                                              \
        const float *__restrict__, const double *__restrict__, const float *__restrict__, const double *__restrict__, int,      \
        const int *__restrict__, int, const int64_t *__restrict__, const int *__restrict__, int, const SearchJob *__restrict__,  \
        int, int, ND *__restrict__, int, unsigned *__restrict__, long long, int *__restrict__, int, int, int *__restrict__,      \
        float *__restrict__, int *__restrict__, int *__restrict__, unsigned long long *__restrict__, int, int, int *__restrict__, int, \
        const int *__restrict__, const float *__restrict__, unsigned long long *__restrict__);
#define HNSW_DECLARE_SEARCH(M, NS, H, LT) HNSW_SEARCH_SIGNATURE(extern, M, NS, H, LT)
#define HNSW_DEFINE_SEARCH(M, NS, H, LT) HNSW_SEARCH_SIGNATURE(, M, NS, H, LT)

// KnnQuery with a predicate over ids (HNSWIndex.KnnQuery(query, k, filterFnc, layer), HNSWIndex.cs:107-124): the one body of
// graph_search_filtered_kernel, graph_search_grouped_kernel and graph_search_tagged_kernel.  FindEntryPointQuery
// down to search_layer (exclusive), unfiltered, then SearchLayerQuery with the filter (GraphNavigator.cs:194-256) in the exact
// two-heap traversal -- the sorted-list forms cannot carry it: a disallowed node is a candidate that is never a result, and the
// result list no longer holds the live candidates -- and the stable Take(k_out).  Persistent like graph_range_kernel: one wave per
// job, jobs from a counter; job j is resident query qi from (entry, entry_layer): qi = j, or with ORDERED qi = order[j] (the host
// lists the queries to answer, order entries in 0 .. the launch's queries - 1).  filter_of(qi) builds the query's filter, what
// traverse asks of a FILTER (dk_search_common.h); its per-query state is wave-uniform.  Results and flag go to row qi.  Each wave
// owns one visited set and one spill area of spill_cap entries (filtered traversals keep far more candidates: the result heap
// fills only after ~k / selectivity evaluations) and leaves the set clean after every job.  out_flag: 0 done, 1 handed back
// (candidate heap full, NaN / -0 distance, visited table crowded).
template <int METRIC, bool HASHED, bool ORDERED, class FilterOf>
__device__ __forceinline__ void
predicate_search(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                 const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0, const int64_t *__restrict__ upper,
                 const int *__restrict__ pool, int strideU, int entry, int entry_layer, int search_layer, int k, int cand_cap,
                 ND *__restrict__ spill, int spill_cap, unsigned *__restrict__ visited, long long vis_words, int *__restrict__ vis_tab,
                 int vis_tab_cap, const int *__restrict__ order, int k_out, int *__restrict__ out_ids, float *__restrict__ out_d,
                 int *__restrict__ out_flag, unsigned long long *__restrict__ eval_counter, int nbcap, int njobs, int *__restrict__ job_counter,
                 FilterOf filter_of)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    VisitedSet<HASHED> V = wave_visited<HASHED>(visited, vis_words, vis_tab, vis_tab_cap);
    ND *my_spill = spill + (size_t)blockIdx.x * (size_t)spill_cap;
    const SearchLds L = carve_lds(smem, k, cand_cap, dim, nbcap);
    const GraphView G{adj0, stride0, upper, pool, strideU};
    for (;;) {
        int job;
        if (!claim_job(job_counter, njobs, lane, job)) break;
        int qi = job;
        if constexpr (ORDERED) qi = __builtin_amdgcn_readfirstlane(order[job]);
        const auto filter = filter_of(qi);
        const SearchJob jb{qi, entry, entry_layer, search_layer, -1, 0};
        const double sb = stage_query<METRIC>(queries, q_sn, qi, dim, L, lane);
        unsigned long long evals = 0;
        int top_n = 0;
        ReadLog RL{nullptr, 0, 0};
        const bool ok = traverse<METRIC, HASHED, true, decltype(filter)>(rows, row_sn, dim, sb, G, jb, k, cand_cap, my_spill, spill_cap, V, L, lane, top_n,
                                                                         evals, RL, nullptr, nullptr, true, filter);
        take_stable(L, lane, top_n, k_out, out_ids, out_d, qi);
        if (lane == 0) {
            out_flag[qi] = ok ? 0 : 1;
            atomicAdd(eval_counter, evals);
        }
        V.clear(lane);
    }
}

// An allow-set (AllowSet): a bitset of allow_n bits over ids, the same for every query; job i is resident query i.
template <int METRIC, bool HASHED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HNSW_WAVES(3))))
graph_search_filtered_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                             const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                             const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU, int entry, int entry_layer,
                             int search_layer, int k, int cand_cap, ND *__restrict__ spill, int spill_cap, unsigned *__restrict__ visited,
                             long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap, const unsigned *__restrict__ allow_bits, long long allow_n, int k_out,
                             int *__restrict__ out_ids, float *__restrict__ out_d, int *__restrict__ out_flag,
                             unsigned long long *__restrict__ eval_counter, int nbcap, int njobs, int *__restrict__ job_counter)
{
    predicate_search<METRIC, HASHED, false>(rows, row_sn, queries, q_sn, dim, adj0, stride0, upper, pool, strideU, entry, entry_layer, search_layer, k,
                                            cand_cap, spill, spill_cap, visited, vis_words, vis_tab, vis_tab_cap, nullptr, k_out, out_ids, out_d, out_flag,
                                            eval_counter, nbcap, njobs, job_counter, [=](int) { return AllowSet{allow_bits, allow_n}; });
}
#define HNSW_FILTERED_SIGNATURE(PREFIX, M, H)                                                                                       \
    PREFIX template __global__ void graph_search_filtered_kernel<M, H>(                                                             \
        const float *__restrict__, const double *__restrict__, const float *__restrict__, const double *__restrict__, int,      \
        const int *__restrict__, int, const int64_t *__restrict__, const int *__restrict__, int, int, int, int, int, int, ND *__restrict__, \
        int, unsigned *__restrict__, long long, int *__restrict__, int, const unsigned *__restrict__, long long, int, int *__restrict__, \
        float *__restrict__, int *__restrict__, unsigned long long *__restrict__, int, int, int *__restrict__);
#define HNSW_FOR_EACH_FILTERED(X, M) X(M, false) X(M, true)
#define HNSW_DECLARE_FILTERED(M, H) HNSW_FILTERED_SIGNATURE(extern, M, H)
#define HNSW_DEFINE_FILTERED(M, H) HNSW_FILTERED_SIGNATURE(, M, H)

// A group filter per query (knn_query_grouped; GroupSet): "row_group[id] == query_group[qi]".  row_group has
// n_labels entries (ids beyond have no group).  The host lists in `order` only the queries whose group holds a graph id, longest
// traversal first, and checks before the launch that query_group values lie in 0 .. n_groups - 1.
template <int METRIC, bool HASHED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HNSW_WAVES(3))))
graph_search_grouped_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                            const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                            const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU, int entry, int entry_layer,
                            int search_layer, int k, int cand_cap, ND *__restrict__ spill, int spill_cap, unsigned *__restrict__ visited,
                            long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap, const int *__restrict__ row_group, long long n_labels,
                            const int *__restrict__ query_group, const int *__restrict__ order, int k_out, int *__restrict__ out_ids,
                            float *__restrict__ out_d, int *__restrict__ out_flag, unsigned long long *__restrict__ eval_counter, int nbcap,
                            int njobs, int *__restrict__ job_counter)
{
    predicate_search<METRIC, HASHED, true>(rows, row_sn, queries, q_sn, dim, adj0, stride0, upper, pool, strideU, entry, entry_layer, search_layer, k,
                                           cand_cap, spill, spill_cap, visited, vis_words, vis_tab, vis_tab_cap, order, k_out, out_ids, out_d, out_flag,
                                           eval_counter, nbcap, njobs, job_counter, [=](int qi) {
                                               return GroupSet{row_group, n_labels, __builtin_amdgcn_readfirstlane(query_group[qi])};
                                           });
}
#define HNSW_GROUPED_SIGNATURE(PREFIX, M, H)                                                                                        \
    PREFIX template __global__ void graph_search_grouped_kernel<M, H>(                                                              \
        const float *__restrict__, const double *__restrict__, const float *__restrict__, const double *__restrict__, int,      \
        const int *__restrict__, int, const int64_t *__restrict__, const int *__restrict__, int, int, int, int, int, int, ND *__restrict__, \
        int, unsigned *__restrict__, long long, int *__restrict__, int, const int *__restrict__, long long, const int *__restrict__, \
        const int *__restrict__, int, int *__restrict__, float *__restrict__, int *__restrict__, unsigned long long *__restrict__, int, int, \
        int *__restrict__);
// (the forms of HNSW_FOR_EACH_FILTERED, built in the units of the `filtered` kind: HNSW_UNIT_filtered, device_kernels.h)
#define HNSW_DECLARE_GROUPED(M, H) HNSW_GROUPED_SIGNATURE(extern, M, H)
#define HNSW_DEFINE_GROUPED(M, H) HNSW_GROUPED_SIGNATURE(, M, H)

// A tag mask per query (knn_query_tagged; TagSet): "row_tags[id] shares a tag with query_tags[qi]" (match_all == 0)
// or "carries every tag of it" (match_all != 0).  row_tags has n_tags entries: ids beyond carry no tag.  The host lists in `order`
// only the queries whose mask has a candidate among the graph ids, fewest candidates first, so the mask is never 0.
template <int METRIC, bool HASHED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HNSW_WAVES(3))))
graph_search_tagged_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                           const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                           const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU, int entry, int entry_layer,
                           int search_layer, int k, int cand_cap, ND *__restrict__ spill, int spill_cap, unsigned *__restrict__ visited,
                           long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap, const unsigned *__restrict__ row_tags, long long n_tags,
                           const unsigned *__restrict__ query_tags, int match_all, const int *__restrict__ order, int k_out, int *__restrict__ out_ids,
                           float *__restrict__ out_d, int *__restrict__ out_flag, unsigned long long *__restrict__ eval_counter, int nbcap,
                           int njobs, int *__restrict__ job_counter)
{
    predicate_search<METRIC, HASHED, true>(rows, row_sn, queries, q_sn, dim, adj0, stride0, upper, pool, strideU, entry, entry_layer, search_layer, k,
                                           cand_cap, spill, spill_cap, visited, vis_words, vis_tab, vis_tab_cap, order, k_out, out_ids, out_d, out_flag,
                                           eval_counter, nbcap, njobs, job_counter, [=](int qi) {
                                               return TagSet{row_tags, n_tags, (unsigned)__builtin_amdgcn_readfirstlane((int)query_tags[qi]), match_all};
                                           });
}
#define HNSW_TAGGED_SIGNATURE(PREFIX, M, H)                                                                                         \
    PREFIX template __global__ void graph_search_tagged_kernel<M, H>(                                                               \
        const float *__restrict__, const double *__restrict__, const float *__restrict__, const double *__restrict__, int,      \
        const int *__restrict__, int, const int64_t *__restrict__, const int *__restrict__, int, int, int, int, int, int, ND *__restrict__, \
        int, unsigned *__restrict__, long long, int *__restrict__, int, const unsigned *__restrict__, long long, const unsigned *__restrict__, \
        int, const int *__restrict__, int, int *__restrict__, float *__restrict__, int *__restrict__, unsigned long long *__restrict__, int, int, \
        int *__restrict__);
// (the forms of HNSW_FOR_EACH_FILTERED, built in the units of the `filtered` kind: HNSW_UNIT_filtered, device_kernels.h)
#define HNSW_DECLARE_TAGGED(M, H) HNSW_TAGGED_SIGNATURE(extern, M, H)
#define HNSW_DEFINE_TAGGED(M, H) HNSW_TAGGED_SIGNATURE(, M, H)

// Query by stored id (knn_query_by_id; SelfSet): resident query i is the stored row of id self_ids[i] (gathered on
// the device before the launch), and every id but that one is a candidate -- a duplicate of the row under another id included.
// Job i is resident query i.  The id is read once per job and kept in a scalar register.
template <int METRIC, bool HASHED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HNSW_WAVES(3))))
graph_search_self_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                         const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                         const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU, int entry, int entry_layer,
                         int search_layer, int k, int cand_cap, ND *__restrict__ spill, int spill_cap, unsigned *__restrict__ visited,
                         long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap, const int *__restrict__ self_ids, int k_out,
                         int *__restrict__ out_ids, float *__restrict__ out_d, int *__restrict__ out_flag,
                         unsigned long long *__restrict__ eval_counter, int nbcap, int njobs, int *__restrict__ job_counter)
{
    predicate_search<METRIC, HASHED, false>(rows, row_sn, queries, q_sn, dim, adj0, stride0, upper, pool, strideU, entry, entry_layer, search_layer, k,
                                            cand_cap, spill, spill_cap, visited, vis_words, vis_tab, vis_tab_cap, nullptr, k_out, out_ids, out_d, out_flag,
                                            eval_counter, nbcap, njobs, job_counter, [=](int qi) {
                                                return SelfSet{__builtin_amdgcn_readfirstlane(self_ids[qi])};
                                            });
}
#define HNSW_SELF_SIGNATURE(PREFIX, M, H)                                                                                           \
    PREFIX template __global__ void graph_search_self_kernel<M, H>(                                                                 \
        const float *__restrict__, const double *__restrict__, const float *__restrict__, const double *__restrict__, int,      \
        const int *__restrict__, int, const int64_t *__restrict__, const int *__restrict__, int, int, int, int, int, int, ND *__restrict__, \
        int, unsigned *__restrict__, long long, int *__restrict__, int, const int *__restrict__, int, int *__restrict__,          \
        float *__restrict__, int *__restrict__, unsigned long long *__restrict__, int, int, int *__restrict__);
// (the forms of HNSW_FOR_EACH_FILTERED, built in the units of the `filtered` kind: HNSW_UNIT_filtered, device_kernels.h)
#define HNSW_DECLARE_SELF(M, H) HNSW_SELF_SIGNATURE(extern, M, H)
#define HNSW_DEFINE_SELF(M, H) HNSW_SELF_SIGNATURE(, M, H)

// MultiLayerKnnQuery (HNSWIndex.cs:173-187), one job = one query's whole chain.  The first step is FindEntryPointQuery from
// (entry, entry_layer) down to first_layer = min(top, maxLayer) (exclusive) and SearchLayerQuery there; every later step searches
// the next layer down from the previous step's NEAREST result (entry_layer == search_layer: no descent), to min_layer.  Each step
// has beam k (not max(MinNN, k)), no filter and a fresh visited list: the wave clears its set between steps.  A step's results are
// the heap array in stable distance order (take_stable's rule): rank 0 is the next entry -- read lane-uniformly from LDS -- and
// ranks 1 .. k - 1 go to slot [job][layer][0 .. k - 1) of the output (nslots = first_layer + 1 slots per job, k - 1 >= 1 entries
// each, padded with -1 / NaN; slots below min_layer are padding).  The exact two-heap traversal runs every step: the heap ARRAY
// decides which of two equally near results leads.  Persistent like graph_search_filtered_kernel (one wave per job, jobs from a
// counter, the query staged in LDS once per job).  out_flag: 0 done, 1 the whole job is handed back (a step met a NaN / -0
// distance, a full candidate heap or a crowded visited table; the host redoes it from the start and rewrites its slots).
template <int METRIC, bool HASHED>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HNSW_WAVES(3))))
graph_multilayer_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                        const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                        const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU, int entry, int entry_layer,
                        int first_layer, int min_layer, int k, int cand_cap, ND *__restrict__ spill, int spill_cap,
                        unsigned *__restrict__ visited, long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap,
                        int *__restrict__ out_ids, float *__restrict__ out_d, int *__restrict__ out_flag,
                        unsigned long long *__restrict__ eval_counter, int nbcap, int njobs, int *__restrict__ job_counter)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    VisitedSet<HASHED> V = wave_visited<HASHED>(visited, vis_words, vis_tab, vis_tab_cap);
    ND *my_spill = spill + (size_t)blockIdx.x * (size_t)spill_cap;
    const SearchLds L = carve_lds(smem, k, cand_cap, dim, nbcap);
    const GraphView G{adj0, stride0, upper, pool, strideU};
    const int per = k - 1, nslots = first_layer + 1;
    for (;;) {
        int job;
        if (!claim_job(job_counter, njobs, lane, job)) break;
        const double sb = stage_query<METRIC>(queries, q_sn, job, dim, L, lane);
        unsigned long long evals = 0;
        int *const ids = out_ids + (size_t)job * nslots * per;
        float *const ds = out_d + (size_t)job * nslots * per;
        ChainEntry ent{entry, entry_layer};
        bool ok = true;
        // the chain: a second lane-uniform loop inside the job loop -- no `continue` behind a lane-0 branch, the stores of a step at
        // the end of its body
        for (int layer = nslots - 1; layer >= 0; --layer) {
            int top_n = 0;
            if (ok && layer >= min_layer) {
                const SearchJob jb{job, ent.node, ent.layer, layer, -1, 0};
                ReadLog RL{nullptr, 0, 0};
                ok = traverse<METRIC, HASHED>(rows, row_sn, dim, sb, G, jb, k, cand_cap, my_spill, spill_cap, V, L, lane, top_n, evals, RL,
                                              nullptr, nullptr, true);
                V.clear(lane); // a fresh visited list per SearchLayerQuery; the set is clean again after the job's last step
                if (!ok) top_n = 0;
            }
            // OrderBy(Dist) over the heap array, stable: candidates[0] is the next step's entry, candidates[1 ..] are the slot's results.
            // top_n = 0 (a slot below min_layer, a handed-back job): padding only, the entry stays.
            take_stable<true>(L, lane, top_n, k, ids, ds, layer, &ent, per);
        }
        if (lane == 0) {
            out_flag[job] = ok ? 0 : 1;
            atomicAdd(eval_counter, evals);
        }
        __builtin_amdgcn_wave_barrier();
    }
}
#define HNSW_MULTILAYER_SIGNATURE(PREFIX, M, H)                                                                                     \
    PREFIX template __global__ void graph_multilayer_kernel<M, H>(                                                                  \
        const float *__restrict__, const double *__restrict__, const float *__restrict__, const double *__restrict__, int,      \
        const int *__restrict__, int, const int64_t *__restrict__, const int *__restrict__, int, int, int, int, int, int, int,  \
        ND *__restrict__, int, unsigned *__restrict__, long long, int *__restrict__, int, int *__restrict__, float *__restrict__, \
        int *__restrict__, unsigned long long *__restrict__, int, int, int *__restrict__);
#define HNSW_FOR_EACH_MULTILAYER(X, M) X(M, false) X(M, true)
#define HNSW_DECLARE_MULTILAYER(M, H) HNSW_MULTILAYER_SIGNATURE(extern, M, H)
#define HNSW_DEFINE_MULTILAYER(M, H) HNSW_MULTILAYER_SIGNATURE(, M, H)

#ifdef HNSW_HOST_TU // few variants and launched from one place: defined only in the unit that launches it
// RangeQuery on the device: FindEntryPointQuery + GraphNavigator.SearchLayerRange (GraphNavigator.cs:262-325)
// for one query per wave, on the lists of the job's search_layer (RangeQuery's `layer`; the descent stops above it).  What the reference's two heaps compute there is a closure: a neighbour enters
// `candidates` and `topCandidates` iff its distance is <= range (:302-308), nothing ever leaves topCandidates
// (its root never exceeds range, :310-311), and the stop test (:286-289) can only fire for the entry point, whose
// farthestResultDist is still MaxValue -- so every listed node and the entry point are expanded exactly once,
// whatever the pop order, and the result SET and the evaluation count do not depend on it.  The order shows only
// in RangeQuery's stable OrderBy over the heap array (HNSWIndex.cs:155) between results of EQUAL distance; the
// host sorts what comes back, and for a query that holds such a pair replays the two heaps from the entry point
// with the distances found here (no evaluation: a neighbour that is not among the results is out of range).
// `found` (per wave, found_cap entries) is both the result list and the work queue: entry `head` is the next
// node to expand.  Results are then copied to a launch-wide arena at an offset taken with one atomic.
// out_flag: 0 done; 1 hand back (more than found_cap results, or the visited table filling up); 3 arena full.
constexpr int kRangeFan = 8; // nodes expanded per step; the id / distance scratch holds kRangeFan adjacency lists
// LAYERED: the lists of the job's search_layer (upper layers go through the per-node offset into the pool: eight more scalar
// loads per step and 40 more spilled SGPRs, so layer-0 calls keep the form without them -- the kernel as it was)
template <int METRIC, bool HASHED, bool LAYERED = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) // at most 168 VGPRs: three waves per SIMD
graph_range_kernel(const float *__restrict__ rows, const double *__restrict__ row_sn, const float *__restrict__ queries,
                   const double *__restrict__ q_sn, int dim, const int *__restrict__ adj0, int stride0,
                   const int64_t *__restrict__ upper, const int *__restrict__ pool, int strideU,
                   const SearchJob *__restrict__ jobs, float range, ND *__restrict__ found_all, int found_cap,
                   unsigned *__restrict__ visited, long long vis_words, int *__restrict__ vis_tab, int vis_tab_cap,
                   ND *__restrict__ arena, unsigned long long arena_cap, unsigned long long *__restrict__ arena_used,
                   unsigned long long *__restrict__ out_off, int *__restrict__ out_cnt, int *__restrict__ out_flag,
                   int *__restrict__ out_entry, unsigned long long *__restrict__ eval_counter, int nbcap, int njobs,
                   int *__restrict__ job_counter)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x;
    VisitedSet<HASHED> V = wave_visited<HASHED>(visited, vis_words, vis_tab, vis_tab_cap);
    const SearchLds L = carve_lds(smem, 0, 0, dim, nbcap);
    const GraphView G{adj0, stride0, upper, pool, strideU};
    // the queue is read back through L2 (agent-scope loads): a line of it cached earlier may lack later entries
    unsigned long long *found = reinterpret_cast<unsigned long long *>(found_all + (size_t)blockIdx.x * (size_t)found_cap);
    int *nbuf = L.nbuf;
    float *dbuf = L.dbuf;
    for (;;) {
        int job;
        if (!claim_job(job_counter, njobs, lane, job)) break;
        const SearchJob jb = jobs[job];
        const double sb = stage_query<METRIC>(queries, q_sn, jb.qref, dim, L, lane);
        unsigned long long evals = 0;
        int best;
        float cur;
        ReadLog RL{nullptr, 0, 0};
        descend<METRIC>(rows, row_sn, dim, sb, G, jb, L, lane, best, cur, evals, RL); // FindEntryPointQuery; :268 reuses its distance
        if (lane == 0) (void)V.first_visit(best);                                  // :279
        V.seen += 1;
        int count = 0, head = 0;
        if (cur <= range) { // :271-275
            if (lane == 0) found[0] = ((unsigned long long)__float_as_uint(cur) << 32) | (unsigned)best;
            count = 1;
        }
        // :277 the entry point is a candidate either way; out of range it is still expanded, unless its distance
        // exceeds farthestResultDist's initial MaxValue (+inf): then :286-289 ends the search at once
        bool entry_pending = !(cur <= range) && !(cur > 3.402823466e+38f);
        bool ok = true;
        for (;;) {
            // up to kRangeFan listed nodes are expanded per step (any order gives the same set): a large result set
            // is a long dependent chain on one wave otherwise
            int W, c0 = best;
            if (entry_pending) { W = 1; entry_pending = false; }
            else {
                W = min(kRangeFan, count - head); // :283 no candidates left
                if (W == 0) break;
                unsigned long long e = 0ull;
                if (lane < W) e = __hip_atomic_load(&found[head + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // :285, :290
                c0 = (int)(unsigned)e;
                head += W;
            }
            int n[kRangeFan], nb[kRangeFan];
            const int *lw[kRangeFan];
#pragma unroll
            for (int w = 0; w < kRangeFan; ++w) {
                lw[w] = G.list(__builtin_amdgcn_readlane(c0, w < W ? w : 0), LAYERED ? jb.search_layer : 0);
                n[w] = w < W ? __builtin_amdgcn_readfirstlane(lw[w][0]) : 0;
                nb[w] = lane < n[w] ? lw[w][1 + lane] : 0;
            }
            bool fr[kRangeFan];
#pragma unroll
            for (int w = 0; w < kRangeFan; ++w) fr[w] = lane < n[w] && V.first_visit(nb[w]); // :297 / :318 (a node two lists share is fresh once)
            int m = 0;
            wave_sync();
#pragma unroll
            for (int w = 0; w < kRangeFan; ++w) {
                const unsigned long long mask = __ballot(fr[w]);
                const int posn = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                if (fr[w]) nbuf[m + posn] = nb[w];
                m += __popcll(mask);
                for (int base = 64; base < n[w]; base += 64) { // lists beyond 64 ids (MaxEdges > 32)
                    const int i = base + lane;
                    bool fresh = false;
                    int x = 0;
                    if (i < n[w]) { x = lw[w][1 + i]; fresh = V.first_visit(x); }
                    const unsigned long long mk = __ballot(fresh);
                    const int pp = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0));
                    if (fresh) nbuf[m + pp] = x;
                    m += __popcll(mk);
                }
            }
            wave_sync();
            if (m == 0) continue;
            V.seen += m;
            if (V.crowded()) { ok = false; break; }
            measure_all<METRIC>(rows, row_sn, dim, L.qs, sb, nbuf, dbuf, m, lane); // :299
            wave_sync();
            evals += (unsigned long long)m;
            for (int base = 0; base < m && ok; base += 64) {
                const int i = base + lane;
                const float d = i < m ? dbuf[i] : 0.0f;
                const bool in = i < m && d <= range; // :302
                const unsigned long long mask = __ballot(in);
                const int add = __popcll(mask);
                if (count + add > found_cap) { ok = false; break; }
                const int posn = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
                if (in) found[count + posn] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)nbuf[i]; // :305, :308
                count += add;
            }
            if (!ok) break;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); // the queue entries just written are read above (through L2)
        }
        unsigned long long off = 0;
        int flag = ok ? 0 : 1;
        if (ok && count > 0) {
            if (lane == 0) off = atomicAdd(arena_used, (unsigned long long)count);
            off = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(off >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)off);
            if (off + (unsigned long long)count > arena_cap) flag = 3;
            else
                for (int i = lane; i < count; i += 64) {
                    const unsigned long long e = __hip_atomic_load(&found[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    arena[off + i] = ND{(int)(unsigned)e, __uint_as_float((unsigned)(e >> 32))};
                }
        }
        if (lane == 0) {
            out_off[job] = off;
            out_cnt[job] = flag == 0 ? count : 0;
            out_flag[job] = flag;
            out_entry[job] = best; // FindEntryPointQuery's answer: where a host replay of the heaps starts
            if (flag != 3) atomicAdd(eval_counter, evals); // (a job that found the arena full runs again)
        }
        V.clear(lane);
    }
}
#endif

} // namespace hnsw
