// device_backend.hip -- gfx950 (MI355X / CDNA4) candidate-distance kernels and the device
// context that owns the HBM-resident vector matrix.
//
// What the kernels replace (all citations relative to /root/reference/):
//   SquaredEuclideanMetric.Compute  src/HNSWIndex/Metrics/EuclideanMetric.cs:11-60
//   CosineMetric.UnitCompute        src/HNSWIndex/Metrics/CosineMetric.cs:95-142
//   CosineMetric.Compute            src/HNSWIndex/Metrics/CosineMetric.cs:10-92
// as invoked through GraphData.Distance (src/HNSWIndex/GraphData.cs:255-277) from the
// search / link loops.
//
// Numerical contract: the reference's AVX branch keeps EIGHT partial sums;
// element i feeds partial (i mod 8) in increasing i; L2 uses fma(d,d,acc) with d = a-b;
// dot/norm use acc + (a*b) (two roundings); the eight partials collapse through a fixed
// tree -- L2 ((p0+p4)+(p1+p5))+((p2+p6)+(p3+p7)), cosine family ((p0+p4)+(p2+p6))+((p1+p5)+(p3+p7))
// -- and a scalar mul-then-add tail handles dim % 8.  The kernels reproduce that order
// exactly, so distances are bit-identical to the CPU path and every float compare in the
// traversal branches the same way.  Built with -ffp-contract=off; every fused operation is
// written as __builtin_fmaf.
//
// Mapping to the wavefront: 8 lanes own the 8 partials of one candidate row, so a wave64
// evaluates 8 candidates at a time (up to 4 rows per lane group in one memory round trip); the
// collapse tree is three cross-lane adds.  Wider per-lane loads and lane-ring variants were
// measured no faster (tools/kbench.hip): this mapping gathers random 512-B rows at 4.2-4.9 TB/s.
//
// Contents: (1) slot_distance_kernel / pair_distance_kernel -- batched distances for a host that
// keeps the traversal (the hnswdev_dist_* entry points, the lock-step engine);  (2) the
// graph-resident traversals -- traverse_sorted (one sorted list in registers; the default) and
// traverse (the reference's two heaps in LDS; exact under equal distances), wrapped by the
// persistent graph_search_kernel (KnnQuery) and graph_insert_search_kernel (Add, search half +
// RelativeNeighborPruning);  (3) Add's link half -- link_plan / link_offsets / link_order
// (grouping of the back-edge appends on the device) and graph_link_kernel (appends and
// PruneOverflow with the tested-prefix shortcut);  (4) class Device: HBM matrix, graph mirror,
// per-wave scratch, launches.  DESIGN.md section 3 has the reasoning and the measurements.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "device_backend.h"
#include "diag.h"
#define HNSW_HOST_TU
#include "device_kernels.h"
#include "dk_exact.h"
#include "dk_graph_info.h"
#include "dk_graph_reach.h"
#include "dk_graph_repair.h"
#include "dk_edge_groups.h"
#include "dk_tag_lists.h"
#include "range_replay.h"

namespace hnsw {

// ------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------
static std::mutex g_err_mu;
static std::string g_err;
static thread_local Device *tl_ctx = nullptr;
ErrorScope::ErrorScope(Device *d) : prev(tl_ctx) { tl_ctx = d; }
ErrorScope::~ErrorScope() { tl_ctx = prev; }
void set_dev_error(const std::string &msg)
{
    if (tl_ctx) tl_ctx->set_error(msg);
    std::lock_guard<std::mutex> lk(g_err_mu);
    g_err = msg;
}
std::string get_dev_error()
{
    std::lock_guard<std::mutex> lk(g_err_mu);
    return g_err;
}

#define HIP_OK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            set_dev_error(std::string(#expr) + ": " + hipGetErrorString(_e));                     \
            return false;                                                                         \
        }                                                                                         \
    } while (0)

// What the holders of dev_buf.h sit on: the only places a context's memory, events and streams are allocated and released
// (alloc_step / free_step keep the StepBuffers' own matched pair).
void *dev_mem_alloc(size_t bytes)
{
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) return p;
    set_dev_error("hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    return nullptr;
}
bool dev_mem_free(void *p) { HIP_OK(hipFree(p)); return true; }
void *pin_mem_alloc(size_t bytes, unsigned flags)
{
    void *p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes, flags);
    if (e == hipSuccess) return p;
    set_dev_error("pinned allocation failed: hipHostMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
    return nullptr;
}
bool pin_mem_free(void *p) { HIP_OK(hipHostFree(p)); return true; }
static constexpr unsigned kPinMappedCoherent = hipHostMallocMapped | hipHostMallocCoherent; // h_ready_: host memory the kernel reads
void *dev_event_create(bool timing)
{
    hipEvent_t ev = nullptr;
    const hipError_t e = timing ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess) return ev;
    set_dev_error(std::string("hipEventCreate: ") + hipGetErrorString(e));
    return nullptr;
}
void dev_event_destroy(void *e) { (void)hipEventDestroy((hipEvent_t)e); }
// High priority (copy streams only): the copies a gated kernel waits for must never queue behind that kernel.  HIP multiplexes
// streams onto a few hardware queues, and a copy stream that lands on the queue of a compute stream does exactly that (measured:
// two lanes, every wave slept its full bound).  High-priority streams have hardware queues of their own.
void *dev_stream_create(bool high_priority)
{
    hipStream_t st = nullptr;
    int lo = 0, hi = 0;
    hipError_t e = high_priority ? hipDeviceGetStreamPriorityRange(&lo, &hi) : hipSuccess;
    if (e == hipSuccess) e = high_priority ? hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi) : hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) return st;
    set_dev_error(std::string("hipStreamCreate failed: ") + hipGetErrorString(e));
    return nullptr;
}
void dev_stream_destroy(void *s) { (void)hipStreamDestroy((hipStream_t)s); }

#ifdef EXP_PHASE_CLOCKS
HNSW_PHASE_BIND(backend)
// one bind per kernel unit, metrics x kinds (all seven kinds: the filtered and multilayer kernels run the same traversal code)
#define HNSW_BIND_PROTO(KIND, ID, TAG) hipError_t hnsw_phase_bind_##TAG##_##KIND(unsigned long long *);
#define HNSW_BIND_PROTOS(ID, TAG, NAME) HNSW_FOR_EACH_KIND(HNSW_BIND_PROTO, ID, TAG)
extern "C" {
HNSW_FOR_EACH_METRIC(HNSW_BIND_PROTOS)
}
static unsigned long long *g_phase_buf = nullptr; // one buffer per process (diagnostic builds run one index at a time)
static bool phase_bind_all()
{
    if (g_phase_buf) return true;
    if (hipMalloc(&g_phase_buf, sizeof(unsigned long long) * hnsw::kPhaseWords) != hipSuccess) return false;
    (void)hipMemset(g_phase_buf, 0, sizeof(unsigned long long) * hnsw::kPhaseWords);
    bool ok = hnsw_phase_bind_backend(g_phase_buf) == hipSuccess;
#ifndef HNSW_SINGLE_TU
#define HNSW_BIND_CALL(KIND, ID, TAG) ok = ok && hnsw_phase_bind_##TAG##_##KIND(g_phase_buf) == hipSuccess;
#define HNSW_BIND_CALLS(ID, TAG, NAME) HNSW_FOR_EACH_KIND(HNSW_BIND_CALL, ID, TAG)
    HNSW_FOR_EACH_METRIC(HNSW_BIND_CALLS)
#endif
    return ok;
}
static bool phase_read(unsigned long long *h) { return g_phase_buf && hipMemcpy(h, g_phase_buf, sizeof(unsigned long long) * hnsw::kPhaseWords, hipMemcpyDeviceToHost) == hipSuccess; }
static void phase_zero() { if (g_phase_buf) (void)hipMemset(g_phase_buf, 0, sizeof(unsigned long long) * hnsw::kPhaseWords); }
static void phase_report(const char *when)
{
    unsigned long long w[hnsw::kPhaseWords] = {0};
    if (!phase_read(w)) return;
    const unsigned long long *h = w, *hl = w + 12, *hx = w + 24;
    double tot = 0, tl = 0;
    for (int i = 0; i < 6; ++i) tot += (double)h[i];
    for (int i = 0; i < 5; ++i) tl += (double)hl[i];
    if (hl[7])
        fprintf(stderr, "[phase clocks, link] stage %.1f%% measure %.1f%% sort %.1f%% heuristic %.1f%% rest %.1f%% | appends %llu, prunes %llu, cycles/prune %.0f\n",
                100 * hl[0] / tl, 100 * hl[1] / tl, 100 * hl[2] / tl, 100 * hl[3] / tl, 100 * hl[4] / tl, hl[6], hl[7], tl / (double)std::max(1ull, hl[7]));
    if (h[9]) fprintf(stderr, "[phase clocks, insert] RelativeNeighborPruning %.1f%% of the insert jobs' cycles; heuristic cycles %.0f, job cycles %.0f\n", 100.0 * (double)h[8] / (double)h[9], (double)h[8], (double)h[9]);
    if (!h[7]) return;
    const double e = (double)h[7];
    fprintf(stderr, "[phase clocks, %s] descent %.1f%% pop %.1f%% list %.1f%% visited %.1f%% rows %.1f%% push %.1f%% | expansions %llu, prefetch hits %.1f%%, cycles/expansion %.0f\n", when,
            100 * h[0] / tot, 100 * h[1] / tot, 100 * h[2] / tot, 100 * h[3] / tot, 100 * h[4] / tot, 100 * h[5] / tot, h[7], 100.0 * h[6] / e, tot / e);
    fprintf(stderr, "[phase clocks, per expansion] descent %.0f pop %.0f list %.0f visited %.0f rows %.0f (before %.0f, measure %.0f, after %.0f) push %.0f (checks %.0f, next-pop guess %.0f, merge %.0f, single inserts %.0f) | merges %.2f, single inserts %.2f, candidates passing %.2f\n",
            h[0] / e, h[1] / e, h[2] / e, h[3] / e, h[4] / e, hx[0] / e, hx[1] / e, hx[2] / e, h[5] / e, hx[8] / e, hx[9] / e, hx[10] / e, hx[11] / e, hx[3] / e, hx[4] / e, hx[5] / e);
    if (hx[13]) fprintf(stderr, "[phase clocks, memory wave, per expansion] waiting for a request %.0f, list %.0f, marks + rows + distances %.0f, keys + answer %.0f\n",
                        hx[12] / e, hx[13] / e, hx[14] / e, hx[15] / e);
}
#endif

// Every traversal kernel form, metrics x kinds (device_kernels.h): declared here and defined in the kernel_unit.hip units, or
// (diagnostic builds) defined here, in one translation unit.
#ifdef HNSW_SINGLE_TU
#define HNSW_TRAVERSAL_UNIT(KIND, ID, TAG) HNSW_UNIT_##KIND(DEFINE, ID)
#else
#define HNSW_TRAVERSAL_UNIT(KIND, ID, TAG) HNSW_UNIT_##KIND(DECLARE, ID)
#endif
#define HNSW_TRAVERSAL_UNITS(ID, TAG, NAME) HNSW_FOR_EACH_KIND(HNSW_TRAVERSAL_UNIT, ID, TAG)
HNSW_FOR_EACH_METRIC(HNSW_TRAVERSAL_UNITS)

// ------------------------------------------------------------------------------------
// host side of the context
// ------------------------------------------------------------------------------------
// C-ABI graph staging (hnswdev_graph_*): the host graph flattened layer by layer
struct Device::HostGraphStage {
    int n = 0, M = 0, stride0 = 0, strideU = 0, top = 0;
    std::vector<int> level, adj0, pool;
    std::vector<int64_t> upper;
};

static inline hipStream_t S(void *p) { return (hipStream_t)p; }
static inline hipEvent_t E(void *p) { return (hipEvent_t)p; }

// The one place a context's metric becomes a template argument: f(std::integral_constant<int, M>{}), one case per row of the
// list of metrics.  ucosine's case passes: its turn is with_metric's last line, which also takes every id outside the list (and
// so this unit's kernels keep the order in which they have always been instantiated: its device code is compared byte for byte).
template <int ID, class F>
static bool metric_case(int metric, F &f)
{
    if constexpr (ID != M_UCOS)
        if (metric == ID) { f(std::integral_constant<int, ID>{}); return true; }
    return false;
}
template <class F>
static void with_metric(int metric, F &&f)
{
#define HNSW_METRIC_CASE(ID, TAG, NAME) if (metric_case<ID>(metric, f)) return;
    HNSW_FOR_EACH_METRIC(HNSW_METRIC_CASE)
#undef HNSW_METRIC_CASE
    f(std::integral_constant<int, M_UCOS>{});
}

// The hnswdev_stats counters of one kernel family.
struct LaunchFamily {
    uint64_t hnswdev_stats::*launches, hnswdev_stats::*evals, hnswdev_stats::*timed_launches, hnswdev_stats::*timed_evals;
    double hnswdev_stats::*kernel_ms;
};
static constexpr LaunchFamily kSearchFamily{&hnswdev_stats::search_launches, &hnswdev_stats::search_evals, &hnswdev_stats::search_timed_launches,
                                            &hnswdev_stats::search_timed_evals, &hnswdev_stats::search_kernel_ms};
static constexpr LaunchFamily kInsertFamily{&hnswdev_stats::insert_launches, &hnswdev_stats::insert_evals, &hnswdev_stats::insert_timed_launches,
                                            &hnswdev_stats::insert_timed_evals, &hnswdev_stats::insert_kernel_ms};
static constexpr LaunchFamily kLinkFamily{&hnswdev_stats::link_launches, &hnswdev_stats::link_evals, &hnswdev_stats::link_timed_launches,
                                          &hnswdev_stats::link_timed_evals, &hnswdev_stats::link_kernel_ms};
static constexpr LaunchFamily kRangeFamily{&hnswdev_stats::range_launches, &hnswdev_stats::range_evals, &hnswdev_stats::range_timed_launches,
                                           &hnswdev_stats::range_timed_evals, &hnswdev_stats::range_kernel_ms};

// One finished traversal, link or range launch into the counters: search_* always, `family`'s own besides (nullptr: a KnnQuery
// launch has none), visited_hash_launches when its visited sets were hash tables.  A timed launch (profiling on) adds the kernel
// time between the events t0 and t1.  (link_dry_run and relink_batch count less: see there.)
bool Device::count_launch(const LaunchFamily *family, unsigned long long evals, bool hashed, bool timed, void *t0, void *t1)
{
    for (const LaunchFamily *f : {&kSearchFamily, family})
        if (f) { stats_.*f->launches += 1; stats_.*f->evals += evals; }
    if (hashed) stats_.visited_hash_launches++;
    if (!timed) return true;
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, E(t0), E(t1)));
    for (const LaunchFamily *f : {&kSearchFamily, family})
        if (f) { stats_.*f->kernel_ms += ms; stats_.*f->timed_launches += 1; stats_.*f->timed_evals += evals; }
    return true;
}

bool Device::bind()
{
    HIP_OK(hipSetDevice(device_));
    return true;
}

Device *Device::create(int device, int dim, int metric, long long capacity)
{
    if (dim <= 0 || metric < 0 || metric >= kMetricCount || capacity < 0) {
        set_dev_error("hnswdev_create: bad argument");
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        set_dev_error(std::string("no HIP device available (") + hipGetErrorString(e) +
                      "): this library has no CPU fallback");
        return nullptr;
    }
    if (device < 0 || device >= ndev) {
        set_dev_error("hnswdev_create: device ordinal out of range");
        return nullptr;
    }
    Device *d = new Device();
    d->device_ = device;
    d->dim_ = dim;
    // words per resident query and per stored f32 row: the floats themselves, or the int8 record (data words + scale + sumsq, a
    // multiple of 16 words = 64 B; device_kernels.h "int8 rows")
    d->pitch_ = metric == M_I8 ? (((dim + 3) / 4 + 2 + 15) & ~15) : dim;
    // half-precision rows: the record of dk_base.h (32 B per 16 elements); queries and every LDS size stay those of `dim` floats
    d->row_pitch_ = metric_f16(metric) ? f16_row_words(dim) : d->pitch_;
    d->metric_ = metric;
    if (metric == M_SQ) d->pf_ = std::make_shared<RowPrefilter>(); // (its device memory: the first lean launch, row_prefilter_ready)
    // algorithmic bytes per evaluation: the row's elements, plus the 4-byte scale for int8
    d->stats_.row_bytes = metric == M_I8 ? (uint64_t)dim + 4u : metric_f16(metric) ? (uint64_t)dim * 2u : (uint64_t)dim * sizeof(float);
    auto fail = [&]() -> Device * { delete d; return nullptr; };
    if (hipSetDevice(device) != hipSuccess) { set_dev_error("hipSetDevice failed"); return fail(); }
    if (!d->stream_.create(false)) return fail();
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) d->num_cu_ = cus;
    }
    if (!d->reserve(capacity > 0 ? capacity : 1)) return fail();
#ifdef EXP_PHASE_CLOCKS
    if (!phase_bind_all()) { set_dev_error("phase-clock buffer: bind failed"); return fail(); }
#endif
    return d;
}

Device *Device::create_view(Device *primary)
{
    if (!primary) return nullptr;
    Device *d = new Device();
    d->device_ = primary->device_;
    d->dim_ = primary->dim_;
    d->pitch_ = primary->pitch_;
    d->row_pitch_ = primary->row_pitch_;
    d->metric_ = primary->metric_;
    d->stats_.row_bytes = primary->stats_.row_bytes;
    d->num_cu_ = primary->num_cu_;
    if (hipSetDevice(d->device_) != hipSuccess) { set_dev_error("hipSetDevice failed"); delete d; return nullptr; }
    if (!d->stream_.create(false)) { delete d; return nullptr; }
    d->rebind(primary);
    return d;
}

void Device::rebind(const Device *p)
{
    d_rows_.borrow(p->d_rows_); d_row_sn_.borrow(p->d_row_sn_); capacity_ = p->capacity_; n_rows_hw_ = p->n_rows_hw_;
    g_adj0_.borrow(p->g_adj0_); g_level_.borrow(p->g_level_); g_upper_.borrow(p->g_upper_); g_pool_.borrow(p->g_pool_);
    g_tested0_.borrow(p->g_tested0_); g_testedU_.borrow(p->g_testedU_);
    g_n_ = p->g_n_; g_stride0_ = p->g_stride0_; g_strideU_ = p->g_strideU_;
    pf_ = p->pf_; // (the shadow of the borrowed rows: one per index)
}

// Only what has an order is written out; the holders release everything else after this body.  Should hipSetDevice fail, the
// memory is still freed by pointer (it used to be left behind).
Device::~Device()
{
    (void)hipSetDevice(device_);
    if (stream_) (void)hipStreamSynchronize(S(stream_));
    stream_.reset();
    if (bg_.th.joinable()) bg_.th.join();
#ifdef EXP_PHASE_CLOCKS
    phase_report("teardown");
#endif
    for (StepBuffers *&sb : abi_sb_) { if (sb) free_step(sb); sb = nullptr; }
    delete hg_;
}

bool Device::reserve(long long capacity)
{
    if (capacity <= capacity_) return true;
    if (!bind()) return false;
    DevBuf<float> nr;
    DevBuf<double> nsn;
    if (!nr.grow((size_t)capacity * row_pitch_) || (metric_ == M_COS && !nsn.grow((size_t)capacity))) return false;
    if (d_rows_) {
        HIP_OK(hipMemcpyAsync(nr, d_rows_, (size_t)capacity_ * row_pitch_ * sizeof(float), hipMemcpyDeviceToDevice, S(stream_)));
        if (nsn) HIP_OK(hipMemcpyAsync(nsn, d_row_sn_, (size_t)capacity_ * sizeof(double), hipMemcpyDeviceToDevice, S(stream_)));
        HIP_OK(hipStreamSynchronize(S(stream_)));
    }
    d_rows_ = std::move(nr); // (the old blocks go here)
    d_row_sn_ = std::move(nsn);
    capacity_ = capacity;
    rows_written(0);
    return true;
}

bool Device::upload_rows(int first_id, int n, const float *rows)
{
    if (n <= 0) return true;
    if (first_id < 0 || (long long)first_id + n > capacity_ || !rows) {
        set_dev_error("upload_rows: range outside capacity");
        return false;
    }
    if (!bind()) return false;
    rows_written(first_id);
    {   // pageable -> pinned bounce buffer -> HBM, 64 MiB at a time (int8 and f16 rows: through a float staging area on the
        // device, quantised into records there)
        const size_t row_bytes = (size_t)dim_ * sizeof(float);
        const size_t chunk_rows = std::max<size_t>(1, (64u << 20) / row_bytes);
        char *hs = static_cast<char *>(pinned_stage(std::min<size_t>((size_t)n, chunk_rows) * row_bytes));
        if (!hs) return false;
        if ((metric_ == M_I8 || metric_f16(metric_)) && !q_stage_.grow(std::min<size_t>((size_t)n, chunk_rows) * (size_t)dim_)) return false;
        for (size_t r0 = 0; r0 < (size_t)n; r0 += chunk_rows) {
            const size_t nr = std::min(chunk_rows, (size_t)n - r0);
            memcpy(hs, rows + r0 * dim_, nr * row_bytes);
            if (metric_ == M_I8) {
                HIP_OK(hipMemcpyAsync(q_stage_, hs, nr * row_bytes, hipMemcpyHostToDevice, S(stream_)));
                hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)((nr + 3) / 4)), dim3(256), 0, S(stream_), q_stage_, dim_, (int)nr, d_rows_,
                                   (long long)first_id + (long long)r0, pitch_);
                HIP_OK(hipGetLastError());
            } else if (metric_f16(metric_)) { // floats to the staging area, rounded into the resident records there
                HIP_OK(hipMemcpyAsync(q_stage_, hs, nr * row_bytes, hipMemcpyHostToDevice, S(stream_)));
                hipLaunchKernelGGL(pack_f16_rows_kernel, dim3((unsigned)((nr * (size_t)row_pitch_ + 255) / 256)), dim3(256), 0, S(stream_), q_stage_, dim_, (int)nr,
                                   d_rows_, (long long)first_id + (long long)r0);
                HIP_OK(hipGetLastError());
            } else {
                HIP_OK(hipMemcpyAsync(d_rows_ + ((size_t)first_id + r0) * pitch_, hs, nr * row_bytes, hipMemcpyHostToDevice, S(stream_)));
            }
            HIP_OK(hipStreamSynchronize(S(stream_))); // the bounce buffer is reused
        }
    }
    if (metric_ == M_COS) {
        int blocks = (int)(((long long)n * 8 + 255) / 256);
        hipLaunchKernelGGL(row_sqrtnorm_kernel, dim3(blocks), dim3(256), 0, S(stream_), d_rows_, pitch_, (long long)first_id, n, d_row_sn_);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(S(stream_))); // `rows` is borrowed only for this call
    n_rows_hw_ = std::max(n_rows_hw_, (long long)first_id + n);
    return true;
}

// float rows -> half-precision records on the host (the background upload): the device kernel's layout and rounding
static void pack_f16_rows_host(unsigned *dst, const float *src, size_t n, int dim)
{
    const int pitch = f16_row_words(dim);
    for (size_t r = 0; r < n; ++r) {
        const float *x = src + r * (size_t)dim;
        unsigned *rec = dst + r * (size_t)pitch;
        for (int w = 0; w < pitch; ++w) {
            const int i0 = ((w >> 3) << 4) | (w & 7), i1 = i0 + 8;
            unsigned b0 = 0u, b1 = 0u;
            if (i0 < dim) { memcpy(&b0, x + i0, 4); b0 = f32_to_f16_bits(b0); }
            if (i1 < dim) { memcpy(&b1, x + i1, 4); b1 = f32_to_f16_bits(b1); }
            rec[w] = b0 | (b1 << 16);
        }
    }
}

bool Device::upload_rows_begin(int first_id, int n, const float *rows)
{
    if (n <= 0) return true;
    if (metric_ == M_I8 || bg_.active.load()) { set_dev_error("upload_rows_begin: not available (int8 rows, or an upload already in flight)"); return false; }
    if (first_id < 0 || (long long)first_id + n > capacity_ || !rows) { set_dev_error("upload_rows: range outside capacity"); return false; }
    if (!bind()) return false;
    rows_written(first_id);
    const size_t row_bytes = (size_t)dim_ * sizeof(float);
    const size_t chunk_rows = std::max<size_t>(1, (8u << 20) / row_bytes);
    if (!bg_.stream.create(false) || !bg_.ev[0].create(false) || !bg_.ev[1].create(false)) return false;
    const size_t pin_need = chunk_rows * std::max(row_bytes, (size_t)row_pitch_ * sizeof(float)); // (a half-precision record of a short row is longer than the row)
    if (!bg_.pin[0].grow(pin_need) || !bg_.pin[1].grow(pin_need)) return false;
    bg_.resident.store(first_id);
    bg_.failed.store(false);
    bg_.active.store(true);
    n_rows_hw_ = std::max(n_rows_hw_, (long long)first_id + n); // ids are valid from now on; their rows are awaited per batch
    const bool f16 = metric_f16(metric_); // the copy into the pinned buffer rounds the rows into records (half the bytes over the link)
    bg_.th = std::thread([this, first_id, n, rows, row_bytes, chunk_rows, f16] {
        auto fail = [&](const char *what, hipError_t e) { bg_.err = std::string(what) + ": " + hipGetErrorString(e); bg_.failed.store(true); };
        hipError_t e = hipSetDevice(device_);
        if (e != hipSuccess) { fail("hipSetDevice", e); return; }
        hipStream_t st = S(bg_.stream);
        size_t pending_rows[2] = {0, 0};
        bool in_flight[2] = {false, false};
        int b = 0;
        long long landed = first_id;
        for (size_t r0 = 0; r0 < (size_t)n; r0 += chunk_rows, b ^= 1) {
            const size_t nr = std::min(chunk_rows, (size_t)n - r0);
            if (in_flight[b]) { // this pinned buffer's previous copy must have left it
                if ((e = hipEventSynchronize(E(bg_.ev[b]))) != hipSuccess) { fail("hipEventSynchronize", e); return; }
                landed += (long long)pending_rows[b];
                bg_.resident.store(landed, std::memory_order_release);
                in_flight[b] = false;
            }
            if (f16) pack_f16_rows_host(reinterpret_cast<unsigned *>(bg_.pin[b].get()), rows + r0 * dim_, nr, dim_);
            else memcpy(bg_.pin[b], rows + r0 * dim_, nr * row_bytes);
            if ((e = hipMemcpyAsync(d_rows_ + ((size_t)first_id + r0) * row_pitch_, bg_.pin[b], f16 ? nr * (size_t)row_pitch_ * sizeof(float) : nr * row_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) { fail("hipMemcpyAsync", e); return; }
            if (metric_ == M_COS) {
                const int blocks = (int)(((long long)nr * 8 + 255) / 256);
                hipLaunchKernelGGL(row_sqrtnorm_kernel, dim3(blocks), dim3(256), 0, st, d_rows_, pitch_, (long long)first_id + (long long)r0, (int)nr, d_row_sn_);
            }
            if ((e = hipEventRecord(E(bg_.ev[b]), st)) != hipSuccess) { fail("hipEventRecord", e); return; }
            pending_rows[b] = nr;
            in_flight[b] = true;
        }
        for (int k = 0; k < 2; ++k, b ^= 1) // the two copies still in flight, oldest first
            if (in_flight[b]) {
                if ((e = hipEventSynchronize(E(bg_.ev[b]))) != hipSuccess) { fail("hipEventSynchronize", e); return; }
                landed += (long long)pending_rows[b];
                bg_.resident.store(landed, std::memory_order_release);
            }
    });
    return true;
}

bool Device::upload_rows_wait(long long upto)
{
    if (!bg_.active.load()) return true;
    if (upto >= 0) {
        while (bg_.resident.load(std::memory_order_acquire) < upto && !bg_.failed.load()) std::this_thread::yield();
        if (!bg_.failed.load()) return true;
    }
    if (bg_.th.joinable()) bg_.th.join();
    bg_.active.store(false);
    if (bg_.failed.load()) { set_dev_error("background row upload failed: " + bg_.err); return false; }
    return true;
}

// ---- the row prefilter's shadow (dk_sorted_top.h) ----
// 0: off, and nothing is ever allocated; 1 (default): the library chooses -- the 8-bit form where it is built for the row length
// (pitch_ == kPfFixedDim, diag pf_fixed_dim != 0) until a launch re-reads more than a quarter of its rows, then (and everywhere else)
// the f16 forms until a launch re-reads more than half, then the lean form; 2: the f16 forms regardless (tests: what this value always
// selected); 3: the 8-bit form regardless, where built (tests; other row lengths: as 2)
static int row_prefilter_mode() { return diag("row_prefilter", 1); }
// Whether mode 1 takes the 8-bit form at all: what the A/B on C2 decided (profiles/pf8_ab_c2.json)
constexpr bool kRowPrefilter8ByDefault = true;

// THE one place that learns of a change to the stored rows: upload_rows, upload_rows_begin (the background upload of a large Add),
// reserve (the matrix moves: everything), clone_from (everything: a re-used slot changes a row the replica already holds).
// Deserialize, import and slot re-use upload through the first two.  A stale shadow row would answer wrongly without a sign.
void Device::rows_written(long long first_id)
{
    if (!pf_) return;
    std::lock_guard<std::mutex> lk(pf_->mu);
    pf_->packed = std::min(pf_->packed, std::max(0ll, first_id));
    pf_->lost = false; // the next launch repacks, and with other rows the prefilter may pay again
    pf_->c8.packed = std::min(pf_->c8.packed, std::max(0ll, first_id)); // (a fallback left 0 here: the next try derives a fresh grid)
    pf_->c8.lost = false;
}

// The 8-bit shadow for rows [0, n_rows_hw_): allocated by the first launch that takes it; a FULL pack (watermark 0) derives the grid
// from the rows as they stand, a partial one keeps it (rows outside are clamped, and E8 grows).  pf_->mu is held.
bool Device::row_prefilter8_ready()
{
    RowPrefilter::Codes &C = pf_->c8;
    hipStream_t st = S(stream_);
    if (C.row_cap < capacity_ || !C.bytes) {
        const std::string before = get_dev_error();
        const bool first = !C.words;
        if (!C.bytes.grow((size_t)capacity_ * kPfFixedDim) || !C.words.grow(kPf8GridWord + 1)) { // the next form down, and report nothing
            (void)C.bytes.reset();
            C.row_cap = C.packed = 0;
            C.no_memory = true;
            (void)hipGetLastError();
            set_dev_error(before);
            return false;
        }
        C.row_cap = capacity_;
        C.packed = 0;
        if (first) HIP_OK(hipMemsetAsync(C.words, 0, (kPf8GridWord + 1) * sizeof(unsigned long long), st));
    }
    const long long n = n_rows_hw_;
    if (C.packed < n) {
        if (C.packed == 0) { // a full pack: a fresh grid, and E8 starts over
            static const unsigned key_start[2] = {0xffffffffu, 0u};
            HIP_OK(hipMemcpyAsync(C.words.get() + 3, key_start, sizeof(key_start), hipMemcpyHostToDevice, st));
            const long long elems = n * kPfFixedDim;
            const unsigned blocks = (unsigned)std::min<long long>((elems + 255) / 256, 8192);
            hipLaunchKernelGGL(shadow8_range_kernel, dim3(blocks), dim3(256), 0, st, d_rows_.get(), elems, reinterpret_cast<unsigned *>(C.words.get() + 3));
            HIP_OK(hipGetLastError());
            hipLaunchKernelGGL(shadow8_grid_kernel, dim3(1), dim3(1), 0, st, C.words.get());
            HIP_OK(hipGetLastError());
            C.full_packs++;
        }
        const long long more = n - C.packed;
        hipLaunchKernelGGL(pack_shadow8_rows_kernel, dim3((unsigned)((more + 3) / 4)), dim3(256), 0, st, d_rows_.get(), C.packed, more, C.bytes.get(), C.words.get());
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st)); // (the views launch on streams of their own)
        C.rows_packed += (uint64_t)more;
        C.packed = n;
    }
    return true;
}

int Device::row_prefilter_ready()
{
    const int mode = row_prefilter_mode();
    if (!pf_ || metric_ != M_SQ || mode == 0 || bg_.active.load() || n_rows_hw_ <= 0) return 0;
    RowPrefilter &P = *pf_;
    std::lock_guard<std::mutex> lk(P.mu);
    if (pitch_ == kPfFixedDim && !P.c8.no_memory && (mode == 3 || (mode == 1 && kRowPrefilter8ByDefault && diag("pf_fixed_dim", 1) != 0 && !P.c8.lost))) {
        if (row_prefilter8_ready()) return 2;
        if (!P.c8.no_memory) return 0; // (a HIP error, reported)
    }
    if (P.no_memory || (P.lost && mode != 2 && mode != 3)) return 0;
    hipStream_t st = S(stream_);
    const size_t words = (size_t)f16_row_words(dim_);
    if (P.row_cap < capacity_ || !P.rows) {
        const std::string before = get_dev_error();
        const bool first = !P.words;
        if (!P.rows.grow((size_t)capacity_ * words) || !P.words.grow(4)) { // run without it, and report nothing
            (void)P.rows.reset();
            P.row_cap = P.packed = 0;
            P.no_memory = true;
            (void)hipGetLastError();
            set_dev_error(before);
            return 0;
        }
        P.row_cap = capacity_;
        P.packed = 0;
        if (first) HIP_OK(hipMemsetAsync(P.words, 0, 4 * sizeof(unsigned long long), st));
    }
    const long long n = n_rows_hw_;
    if (P.packed < n) {
        if (P.packed == 0) HIP_OK(hipMemsetAsync(P.words, 0, sizeof(unsigned long long), st)); // a full repack: E starts over
        const long long more = n - P.packed;
        hipLaunchKernelGGL(pack_shadow_rows_kernel, dim3((unsigned)((more + 3) / 4)), dim3(256), 0, st, d_rows_.get(), dim_, P.packed, more, P.rows.get(),
                           reinterpret_cast<unsigned *>(P.words.get()));
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st)); // (the views launch on streams of their own)
        P.rows_packed += (uint64_t)more;
        P.packed = n;
    }
    return 1;
}

void Device::row_prefilter_stats(uint64_t out[4])
{
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!pf_) return;
    std::lock_guard<std::mutex> lk(pf_->mu);
    const RowPrefilter::Codes &C = pf_->c8; // (totals over both widths)
    out[0] = pf_->launches + C.launches; out[1] = pf_->on_shadow + C.on_shadow; out[2] = pf_->reread + C.reread; out[3] = pf_->rows_packed + C.rows_packed;
}

void Device::row_prefilter8_stats(uint64_t out[6])
{
    std::fill_n(out, 6, (uint64_t)0);
    if (!pf_) return;
    std::lock_guard<std::mutex> lk(pf_->mu);
    const RowPrefilter::Codes &C = pf_->c8;
    out[0] = C.launches; out[1] = C.rows_packed; out[2] = C.on_shadow; out[3] = C.reread; out[4] = C.full_packs; out[5] = C.fallbacks;
}

bool Device::row_prefilter8_peek(long long first_id, int count, uint64_t out[4], unsigned char *codes)
{
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!pf_ || !pf_->c8.bytes || !pf_->c8.words) {
        if (count > 0) set_dev_error("row_prefilter8_peek: the index has no 8-bit shadow rows");
        return count <= 0;
    }
    if (!bind()) return false;
    std::lock_guard<std::mutex> lk(pf_->mu); // (a pack runs under it, and waits for its kernel)
    RowPrefilter::Codes &C = pf_->c8;
    unsigned long long w[kPf8GridWord + 1] = {};
    HIP_OK(hipMemcpy(w, C.words.get(), sizeof(w), hipMemcpyDeviceToHost));
    out[0] = (uint64_t)C.packed;
    out[1] = (uint64_t)(w[kPf8GridWord] & 0xffffffffull);
    out[2] = (uint64_t)(w[kPf8GridWord] >> 32);
    out[3] = (uint64_t)(w[0] & 0xffffffffull);
    if (count <= 0) return true;
    if (first_id < 0 || first_id + count > C.packed || !codes) {
        set_dev_error("row_prefilter8_peek: range outside the packed shadow rows");
        return false;
    }
    HIP_OK(hipMemcpy(codes, C.bytes.get() + (size_t)first_id * kPfFixedDim, (size_t)count * kPfFixedDim, hipMemcpyDeviceToHost));
    return true;
}

void Device::row_prefilter_form_stats(uint64_t out[2])
{
    out[0] = out[1] = 0;
    if (!pf_) return;
    std::lock_guard<std::mutex> lk(pf_->mu);
    out[0] = pf_->form_launches[0]; out[1] = pf_->form_launches[1];
}

bool Device::row_prefilter_peek(long long first_id, int count, uint64_t out[2], float *rows)
{
    out[0] = out[1] = 0;
    if (!pf_ || !pf_->rows || !pf_->words) {
        if (count > 0) set_dev_error("row_prefilter_peek: the index has no shadow rows");
        return count <= 0;
    }
    if (!bind()) return false;
    RowPrefilter &P = *pf_;
    std::lock_guard<std::mutex> lk(P.mu); // (a pack runs under it, and waits for its kernel)
    unsigned long long e_word = 0;
    HIP_OK(hipMemcpy(&e_word, P.words.get(), sizeof(e_word), hipMemcpyDeviceToHost));
    out[0] = (uint64_t)P.packed;
    out[1] = (uint64_t)(e_word & 0xffffffffull);
    if (count <= 0) return true;
    if (first_id < 0 || first_id + count > P.packed || !rows) {
        set_dev_error("row_prefilter_peek: range outside the packed shadow rows");
        return false;
    }
    // the records cross in pieces of a fixed buffer and are widened here, by the kernels' accessors (pack_f16_rows_kernel's layout)
    const size_t words = (size_t)f16_row_words(dim_), total = (size_t)count * words;
    const unsigned *src = reinterpret_cast<const unsigned *>(P.rows.get()) + (size_t)first_id * words;
    unsigned buf[2048];
    for (size_t w0 = 0; w0 < total; w0 += 2048) {
        const size_t nw = std::min<size_t>(2048, total - w0);
        HIP_OK(hipMemcpy(buf, src + w0, nw * sizeof(unsigned), hipMemcpyDeviceToHost));
        for (size_t j = 0; j < nw; ++j) {
            const size_t r = (w0 + j) / words;
            const int w = (int)((w0 + j) % words), i0 = ((w >> 3) << 4) | (w & 7), i1 = i0 + 8;
            if (i0 < dim_) rows[r * (size_t)dim_ + i0] = half_lo(buf[j]);
            if (i1 < dim_) rows[r * (size_t)dim_ + i1] = half_hi(buf[j]);
        }
    }
    return true;
}

bool Device::download_rows(int first_id, int n, float *rows)
{
    if (n <= 0) return true;
    if (first_id < 0 || (long long)first_id + n > capacity_ || !rows) {
        set_dev_error("download_rows: range outside capacity");
        return false;
    }
    if (!bind()) return false;
    if (metric_ == M_I8) { // the dequantised rows q_i * scale
        if (!q_stage_.grow((size_t)n * (size_t)dim_)) return false;
        hipLaunchKernelGGL(dequantize_rows_kernel, dim3((unsigned)(((long long)n * dim_ + 255) / 256)), dim3(256), 0, S(stream_), d_rows_, pitch_,
                           (long long)first_id, n, dim_, q_stage_);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(rows, q_stage_, (size_t)n * dim_ * sizeof(float), hipMemcpyDeviceToHost, S(stream_)));
    } else if (metric_f16(metric_)) { // the stored rows widened to float: h(x), 64 MiB of floats at a time (Serialize downloads the whole
        // index: a staging area of the whole f32 matrix would undo the halving)
        const size_t chunk_rows = std::max<size_t>(1, (64u << 20) / ((size_t)dim_ * sizeof(float)));
        if (!q_stage_.grow(std::min<size_t>((size_t)n, chunk_rows) * (size_t)dim_)) return false;
        for (size_t r0 = 0; r0 < (size_t)n; r0 += chunk_rows) {
            const size_t nr = std::min(chunk_rows, (size_t)n - r0);
            hipLaunchKernelGGL(unpack_f16_rows_kernel, dim3((unsigned)((nr * (size_t)dim_ + 255) / 256)), dim3(256), 0, S(stream_), d_rows_,
                               (long long)first_id + (long long)r0, (int)nr, dim_, q_stage_);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(rows + r0 * (size_t)dim_, q_stage_, nr * (size_t)dim_ * sizeof(float), hipMemcpyDeviceToHost, S(stream_)));
            HIP_OK(hipStreamSynchronize(S(stream_))); // (pageable destination: the copy has left the staging area when this returns)
        }
    } else {
        HIP_OK(hipMemcpyAsync(rows, d_rows_ + (size_t)first_id * pitch_, (size_t)n * dim_ * sizeof(float), hipMemcpyDeviceToHost, S(stream_)));
    }
    HIP_OK(hipStreamSynchronize(S(stream_)));
    return true;
}

// Pageable host memory -> HBM for the large per-call inputs (a 65 536 x 128 query set is 33 MB): four host
// threads copy their quarter of the source through two pinned 2-MB buffers each while the DMA engine drains the
// buffers filled before -- the copy into pinned memory (3 ms on one thread) was most of what the boundary call
// hnsw_knn_query cost beyond the resident-query step.  Everything is enqueued on the context's stream; returns
// when the SOURCE has been read (the caller's buffer is borrowed only for the call), not when the DMA is done.
bool Device::staged_upload(float *dst, const float *src, size_t bytes)
{
    constexpr int T = 4;
    constexpr size_t kChunk = 2u << 20;
    for (int i = 0; i < 2 * T; ++i) {
        if (!up_pin_[i].grow(kChunk) || !up_ev_[i].create(false)) return false;
    }
    std::atomic<int> failed{0};
    const size_t slice = (((bytes + T - 1) / T) + 255) & ~(size_t)255;
    auto work = [&](int t) {
        if (hipSetDevice(device_) != hipSuccess) { failed.store(1); return; }
        const size_t lo = std::min(bytes, slice * (size_t)t), hi = std::min(bytes, slice * (size_t)(t + 1));
        int b = 0;
        for (size_t off = lo; off < hi; off += kChunk, b ^= 1) {
            const int slot = 2 * t + b;
            const size_t nb = std::min(kChunk, hi - off);
            if (up_busy_[slot] && hipEventSynchronize(E(up_ev_[slot])) != hipSuccess) { failed.store(1); return; }
            memcpy(up_pin_[slot], reinterpret_cast<const char *>(src) + off, nb);
            if (hipMemcpyAsync(reinterpret_cast<char *>(dst) + off, up_pin_[slot], nb, hipMemcpyHostToDevice, S(stream_)) != hipSuccess ||
                hipEventRecord(E(up_ev_[slot]), S(stream_)) != hipSuccess) { failed.store(1); return; }
            up_busy_[slot] = true;
        }
    };
    std::thread th[T - 1];
    for (int t = 1; t < T; ++t) th[t - 1] = std::thread(work, t);
    work(0);
    for (int t = 1; t < T; ++t) th[t - 1].join();
    if (failed.load()) { set_dev_error("staged_upload: a HIP call failed"); return false; }
    return true;
}

// Room for a resident set of nq queries.  Nothing is kept: the old set goes first; the new one becomes the member once it is whole.
bool Device::query_room(int nq)
{
    if (nq <= q_capacity()) return true;
    if (!reset_all(d_queries_, d_q_sn_)) return false;
    const size_t cap = (size_t)std::max<long long>(nq, 1024);
    DevBuf<float> nqbuf;
    DevBuf<double> nsn;
    if (!nqbuf.grow(cap * pitch_) || (metric_ == M_COS && !nsn.grow(cap))) return false;
    d_queries_ = std::move(nqbuf);
    d_q_sn_ = std::move(nsn);
    return true;
}

bool Device::set_queries(const float *queries, int nq)
{
    if (nq < 0 || (nq > 0 && !queries)) { set_dev_error("set_queries: bad argument"); return false; }
    if (!bind() || !query_room(nq)) return false;
    n_queries_ = nq;
    q_by_id_ = false;
    if (nq == 0) return true;
    {
        const size_t bytes = (size_t)nq * dim_ * sizeof(float);
        void *hs = bytes < (4u << 20) ? pinned_stage(bytes) : nullptr;
        float *dst = d_queries_;
        if (metric_ == M_I8) { // floats to the staging area, quantised into the resident records
            if (!q_stage_.grow((size_t)nq * (size_t)dim_)) return false;
            dst = q_stage_;
        }
        if (bytes >= (4u << 20)) { if (!staged_upload(dst, queries, bytes)) return false; }
        else if (hs) { memcpy(hs, queries, bytes); HIP_OK(hipMemcpyAsync(dst, hs, bytes, hipMemcpyHostToDevice, S(stream_))); }
        else HIP_OK(hipMemcpyAsync(dst, queries, bytes, hipMemcpyHostToDevice, S(stream_)));
        if (metric_ == M_I8) {
            hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, S(stream_), q_stage_, dim_, nq, d_queries_, 0LL, pitch_);
            HIP_OK(hipGetLastError());
        }
    }
    if (metric_ == M_COS) {
        int blocks = (int)(((long long)nq * 8 + 255) / 256);
        hipLaunchKernelGGL(row_sqrtnorm_kernel, dim3(blocks), dim3(256), 0, S(stream_), d_queries_, pitch_, 0LL, nq, d_q_sn_);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(S(stream_)));
    return true;
}

StepBuffers *Device::alloc_step(int nslots, int stride)
{
    if (nslots <= 0 || stride <= 0) { set_dev_error("alloc_step: bad argument"); return nullptr; }
    if (!bind()) return nullptr;
    StepBuffers *sb = new StepBuffers();
    sb->nslots = nslots;
    sb->stride = stride;
    sb->rec_stride = stride + 2;
    const size_t rec_bytes = sizeof(int) * (size_t)nslots * sb->rec_stride;
    const size_t dist_bytes = sizeof(float) * ((size_t)nslots * stride + StepBuffers::kHeader);
    float *h_dist = nullptr;
    bool ok = hipHostMalloc((void **)&sb->rec, rec_bytes, hipHostMallocDefault) == hipSuccess &&
              hipHostMalloc((void **)&h_dist, dist_bytes, hipHostMallocDefault) == hipSuccess &&
              hipMalloc((void **)&sb->d_rec, rec_bytes) == hipSuccess &&
              hipMalloc((void **)&sb->d_dist, dist_bytes) == hipSuccess;
    if (ok) {
        memset(sb->rec, 0, rec_bytes);
        memset(h_dist, 0, dist_bytes);
        ok = hipMemsetAsync(sb->d_dist, 0, dist_bytes, S(stream_)) == hipSuccess && hipStreamSynchronize(S(stream_)) == hipSuccess;
    }
    if (h_dist) sb->dist = h_dist + StepBuffers::kHeader;
    hipEvent_t ev = nullptr, t0 = nullptr, t1 = nullptr;
    ok = ok && hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess &&
         hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess;
    sb->done = ev; sb->t0 = t0; sb->t1 = t1;
    if (!ok) {
        set_dev_error("alloc_step: allocation failed");
        free_step(sb);
        return nullptr;
    }
    return sb;
}

// hnsw_knn_query hands over host buffers every call, and a 65 536 x 128 query set is 33 MB: uploaded in front of
// the traversal it was 4 % of the call.  Here only the first `head` rows are uploaded before the launch; the rest
// follows on the copy stream WHILE the traversal kernel runs (search_batch -> upload_tail), chunk by chunk, and a word
// in host memory tells the kernel how many rows have landed (graph_search_kernel's `ready`).  Chunks are whole 128-byte
// lines of the query matrix, so no line of it is ever read half-arrived.  Plain float metrics only (nothing to
// compute per query row on arrival).
bool Device::set_queries_streamed(const float *queries, int nq, int head)
{
    if (metric_ == M_COS || metric_ == M_I8 || nq <= 0 || head <= 0 || head >= nq) return set_queries(queries, nq);
    head = std::min(nq, (head + 31) & ~31);
    if (head >= nq) return set_queries(queries, nq);
    if (!bind()) return false;
    if (!copy_stream_) {
        if (!h_ready_) {
            h_ready_ = PinBuf<int>(kPinMappedCoherent);
            if (!h_ready_.grow(16)) return false;
        }
        HIP_OK(hipHostGetDevicePointer((void **)&d_ready_, h_ready_, 0));
        if (!copy_stream_.create(true)) return false; // (high priority: only copy streams are, dev_stream_create)
    }
    if (!set_queries(queries, head)) return false; // allocates for `head` rows at least ...
    if (nq > q_capacity()) {                        // ... and for the whole set, keeping the head
        DevBuf<float> nqbuf;
        const long long cap = std::max<long long>(nq, 1024);
        if (!nqbuf.grow((size_t)cap * pitch_)) return false;
        HIP_OK(hipMemcpyAsync(nqbuf, d_queries_, (size_t)head * pitch_ * sizeof(float), hipMemcpyDeviceToDevice, S(stream_)));
        HIP_OK(hipStreamSynchronize(S(stream_)));
        d_queries_ = std::move(nqbuf);
    }
    n_queries_ = nq;
    __atomic_store_n(h_ready_.get(), head, __ATOMIC_RELEASE);
    tail_.src = queries;
    tail_.first = head;
    tail_.n = nq - head;
    return true;
}

bool Device::upload_tail()
{
    const long long first = tail_.first, n = tail_.n;
    const float *src = tail_.src;
    tail_.n = 0;
    if (n <= 0) return true;
    constexpr size_t kChunk = 2u << 20;
    for (int i = 0; i < 2; ++i) {
        if (!up_pin_[i].grow(kChunk) || !up_ev_[i].create(false)) return false;
    }
    const size_t row_bytes = (size_t)dim_ * sizeof(float);
    const long long rows_per_chunk = std::max<long long>(32, (long long)(kChunk / row_bytes) & ~31LL); // whole 128-B lines
    hipStream_t cs = S(copy_stream_);
    long long sent = 0, confirmed = 0;
    int b = 0;
    long long in_slot[2] = {0, 0};
    while (confirmed < n) {
        if (sent < n && in_slot[b] == 0) {
            const long long r = std::min(rows_per_chunk, n - sent);
            memcpy(up_pin_[b], src + (size_t)(first + sent) * dim_, (size_t)r * row_bytes);
            HIP_OK(hipMemcpyAsync(d_queries_ + (size_t)(first + sent) * pitch_, up_pin_[b], (size_t)r * row_bytes, hipMemcpyHostToDevice, cs));
            HIP_OK(hipEventRecord(E(up_ev_[b]), cs));
            in_slot[b] = r;
            sent += r;
            b ^= 1;
            continue;
        }
        // the older of the two copies in flight
        const int o = in_slot[b] != 0 ? b : b ^ 1;
        HIP_OK(hipEventSynchronize(E(up_ev_[o])));
        confirmed += in_slot[o];
        in_slot[o] = 0;
        b = o;
        __atomic_store_n(h_ready_.get(), (int)(first + confirmed), __ATOMIC_RELEASE);
    }
    up_busy_[0] = up_busy_[1] = false;
    return true;
}

// Peer access between two devices, asked for once per ordered pair.  hipMemcpyPeerAsync works either way -- without peer
// access the runtime stages the copy through host memory -- so a refusal is not an error; it is COUNTED, because "replicas
// are copied device to device over xGMI" is a claim about the machine, not about this code (hnswdev_stats.peer_direct_copies
// / .peer_staged_copies).  Same device on both sides: a plain device-to-device copy, counted as direct.
static bool peer_direct(int dst, int src)
{
    if (dst == src) return true;
    static std::mutex mu;
    static std::map<std::pair<int, int>, bool> known;
    std::lock_guard<std::mutex> lk(mu);
    auto it = known.find({dst, src});
    if (it != known.end()) return it->second;
    int can = 0;
    bool ok = hipDeviceCanAccessPeer(&can, dst, src) == hipSuccess && can != 0;
    if (ok) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        ok = hipSetDevice(dst) == hipSuccess;
        if (ok) {
            const hipError_t e = hipDeviceEnablePeerAccess(src, 0);
            ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            (void)hipGetLastError(); // (already enabled is not an error to keep)
        }
        (void)hipSetDevice(cur);
    }
    known[{dst, src}] = ok;
    return ok;
}

bool Device::clone_from(Device *src, long long pool_len)
{
    if (!src || src == this || src->dim_ != dim_ || src->metric_ != metric_ || src->pitch_ != pitch_ || src->row_pitch_ != row_pitch_) { set_dev_error("clone_from: contexts differ in shape"); return false; }
    if (pool_len < 0 || pool_len > src->g_pool_cap()) { set_dev_error("clone_from: bad pool length"); return false; }
    if (!src->sync()) return false; // what is copied must have landed
    if (!reserve(src->capacity_)) return false;
    const bool direct = peer_direct(device_, src->device_);
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const long long have = std::min(n_rows_hw_, src->n_rows_hw_); // rows never change once uploaded (slot reuse re-clones: see HnswIndex)
    const long long more = src->n_rows_hw_ - have;
    rows_written(0);
    if (more > 0) {
        HIP_OK(hipMemcpyPeerAsync(d_rows_ + (size_t)have * row_pitch_, device_, src->d_rows_ + (size_t)have * row_pitch_, src->device_, (size_t)more * row_pitch_ * sizeof(float), st));
        if (metric_ == M_COS) HIP_OK(hipMemcpyPeerAsync(d_row_sn_ + have, device_, src->d_row_sn_ + have, src->device_, (size_t)more * sizeof(double), st));
    }
    const long long n = src->g_n_;
    if (!graph_room(n, std::max<long long>(src->g_cap_n(), std::max<long long>(n, 1024)), src->g_stride0_, pool_len)) return false;
    g_n_ = n; g_stride0_ = src->g_stride0_; g_strideU_ = src->g_strideU_;
    if (n > 0) {
        HIP_OK(hipMemcpyPeerAsync(g_adj0_, device_, src->g_adj0_, src->device_, sizeof(int) * (size_t)n * g_stride0_, st));
        HIP_OK(hipMemcpyPeerAsync(g_level_, device_, src->g_level_, src->device_, sizeof(int) * (size_t)n, st));
        HIP_OK(hipMemcpyPeerAsync(g_upper_, device_, src->g_upper_, src->device_, sizeof(int64_t) * (size_t)n, st));
    }
    if (pool_len > 0) HIP_OK(hipMemcpyPeerAsync(g_pool_, device_, src->g_pool_, src->device_, sizeof(int) * (size_t)pool_len, st));
    // a replica only answers queries: the link kernel's pruning history is not carried over
    if (g_tested0_) HIP_OK(hipMemsetAsync(g_tested0_, 0, sizeof(int) * g_tested0_.cap(), st));
    if (g_testedU_) HIP_OK(hipMemsetAsync(g_testedU_, 0, sizeof(int) * g_testedU_.cap(), st));
    HIP_OK(hipStreamSynchronize(st));
    n_rows_hw_ = src->n_rows_hw_;
    stats_.replica_bytes += (uint64_t)more * row_pitch_ * sizeof(float) + sizeof(int) * ((uint64_t)n * g_stride0_ + (uint64_t)n * 3 + (uint64_t)pool_len);
    (direct ? stats_.peer_direct_copies : stats_.peer_staged_copies) += 1;
    return true;
}

bool Device::adopt_queries(Device *src, long long first, long long n, long long at, long long total)
{
    if (!src || src->dim_ != dim_ || src->metric_ != metric_ || first < 0 || n < 0 || first + n > src->n_queries_ || at < 0 || at + n > total) {
        set_dev_error("adopt_queries: bad argument");
        return false;
    }
    if (!src->sync()) return false;
    (peer_direct(device_, src->device_) ? stats_.peer_direct_copies : stats_.peer_staged_copies) += 1;
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (total > q_capacity()) { // grow, keeping what is resident
        DevBuf<float> nq;
        DevBuf<double> nsn;
        const long long cap = std::max<long long>(total, 1024);
        if (!nq.grow((size_t)cap * pitch_) || (metric_ == M_COS && !nsn.grow((size_t)cap))) return false;
        if (d_queries_ && n_queries_ > 0) {
            HIP_OK(hipMemcpyAsync(nq, d_queries_, (size_t)n_queries_ * pitch_ * sizeof(float), hipMemcpyDeviceToDevice, st));
            if (nsn) HIP_OK(hipMemcpyAsync(nsn, d_q_sn_, (size_t)n_queries_ * sizeof(double), hipMemcpyDeviceToDevice, st));
            HIP_OK(hipStreamSynchronize(st));
        }
        d_queries_ = std::move(nq);
        d_q_sn_ = std::move(nsn);
    }
    if (n > 0 && src != this) {
        HIP_OK(hipMemcpyPeerAsync(d_queries_ + (size_t)at * pitch_, device_, src->d_queries_ + (size_t)first * pitch_, src->device_, (size_t)n * pitch_ * sizeof(float), st));
        if (metric_ == M_COS) HIP_OK(hipMemcpyPeerAsync(d_q_sn_ + at, device_, src->d_q_sn_ + first, src->device_, (size_t)n * sizeof(double), st));
        HIP_OK(hipStreamSynchronize(st));
    }
    n_queries_ = total;
    q_by_id_ = false; // (the ids of a by-id set stay with the context that gathered it)
    return true;
}

void Device::free_step(StepBuffers *sb)
{
    if (!sb) return;
    (void)hipSetDevice(device_);
    if (sb->rec) (void)hipHostFree(sb->rec);
    if (sb->dist) (void)hipHostFree(sb->dist - StepBuffers::kHeader);
    if (sb->d_rec) (void)hipFree(sb->d_rec);
    if (sb->d_dist) (void)hipFree(sb->d_dist);
    if (sb->done) (void)hipEventDestroy(E(sb->done));
    if (sb->t0) (void)hipEventDestroy(E(sb->t0));
    if (sb->t1) (void)hipEventDestroy(E(sb->t1));
    delete sb;
}

bool Device::launch_step(StepBuffers *sb, int nslots_used, uint64_t evals)
{
    sb->in_flight = false;
    if (nslots_used <= 0 || evals == 0) { sb->evals = 0; sb->timed = false; return true; }
    if (nslots_used > sb->nslots) { set_dev_error("launch_step: too many slots"); return false; }
    hipStream_t st = S(stream_);
    sb->timed = profiling_;
    sb->evals = evals;
    HIP_OK(hipMemcpyAsync(sb->d_rec, sb->rec, sizeof(int) * (size_t)nslots_used * sb->rec_stride, hipMemcpyHostToDevice, st));
    if (sb->timed) HIP_OK(hipEventRecord(E(sb->t0), st));
    dim3 grid((nslots_used + 3) / 4), block(256);
    with_metric(metric_, [&](auto m) {
        hipLaunchKernelGGL(slot_distance_kernel<m>, grid, block, 0, st, d_rows_, d_row_sn_, d_queries_, d_q_sn_, pitch_, sb->d_rec,
                           sb->d_dist + StepBuffers::kHeader, sb->stride, sb->rec_stride, nslots_used, n_rows_hw_, n_queries_,
                           reinterpret_cast<int *>(sb->d_dist));
    });
    HIP_OK(hipGetLastError());
    if (sb->timed) HIP_OK(hipEventRecord(E(sb->t1), st));
    // guard word + distances of the used slots: one copy
    HIP_OK(hipMemcpyAsync(sb->dist - StepBuffers::kHeader, sb->d_dist, sizeof(float) * ((size_t)nslots_used * sb->stride + StepBuffers::kHeader),
                          hipMemcpyDeviceToHost, st));
    HIP_OK(hipEventRecord(E(sb->done), st));
    sb->in_flight = true;
    stats_.launches++;
    stats_.evals += evals;
    return true;
}

bool Device::wait_step(StepBuffers *sb)
{
    if (!sb->in_flight) return true;
    HIP_OK(hipEventSynchronize(E(sb->done)));
    sb->in_flight = false;
    if (sb->timed) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, E(sb->t0), E(sb->t1)));
        stats_.kernel_ms += ms;
        stats_.timed_launches++;
        stats_.timed_evals += sb->evals;
        sb->timed = false;
    }
    sb->evals = 0;
    int *guard = reinterpret_cast<int *>(sb->dist - StepBuffers::kHeader);
    if (*guard != 0) { // the kernel refused a record: clear the flag, report
        *guard = 0;
        HIP_OK(hipMemsetAsync(sb->d_dist, 0, sizeof(int), S(stream_)));
        set_dev_error("distance step: a record names a row / query outside the uploaded data, or more ids than a slot holds (those distances are NaN)");
        return false;
    }
    return true;
}

// ---- step buffers of the C ABI ---------------------------------------------------------------
bool Device::step_buffers(int set, int nslots, int stride, int **rec, float **dist, bool internal)
{
    if (set < 0 || set > (internal ? 3 : 1) || nslots <= 0 || stride <= 0 || !rec || !dist) { set_dev_error("step_buffers: bad argument"); return false; }
    StepBuffers *&sb = abi_sb_[set];
    if (sb && sb->in_flight) { set_dev_error("step_buffers: the set is in flight (call hnswdev_step_wait first)"); return false; }
    if (!sb || sb->nslots < nslots || sb->stride != stride) {
        if (sb) { if (!sync()) return false; free_step(sb); sb = nullptr; }
        sb = alloc_step(nslots, stride);
        if (!sb) return false;
    }
    *rec = sb->rec;
    *dist = sb->dist;
    return true;
}

bool Device::step_submit(int set, int nslots_used)
{
    if (set < 0 || set > 1 || !abi_sb_[set]) { set_dev_error("step_submit: no such buffer set (call hnswdev_step_buffers first)"); return false; }
    StepBuffers *sb = abi_sb_[set];
    if (sb->in_flight) { set_dev_error("step_submit: the set is already in flight"); return false; }
    if (nslots_used < 0 || nslots_used > sb->nslots) { set_dev_error("step_submit: more slots than the set holds"); return false; }
    uint64_t evals = 0; // ids are guarded on the device; the counts are summed here for the counters
    for (int s = 0; s < nslots_used; ++s) {
        const int c = sb->rec[(size_t)s * sb->rec_stride];
        if (c > 0) evals += (uint64_t)c;
    }
    if (!bind()) return false;
    return launch_step(sb, nslots_used, evals);
}

bool Device::step_wait(int set)
{
    if (set < 0 || set > 1 || !abi_sb_[set]) { set_dev_error("step_wait: no such buffer set"); return false; }
    if (!bind()) return false;
    return wait_step(abi_sb_[set]);
}

bool Device::sync()
{
    if (!bind()) return false;
    HIP_OK(hipStreamSynchronize(S(stream_)));
    return true;
}

void Device::get_stats(hnswdev_stats *out) { *out = stats_; }
void Device::reset_stats()
{
    uint64_t rb = stats_.row_bytes;
    stats_ = hnswdev_stats{};
    stats_.row_bytes = rb;
    memset(counters_, 0, sizeof(counters_));
    xg_list_ms_ = 0.0;
    xt_list_ms_ = 0.0;
#ifdef EXP_PHASE_CLOCKS
    (void)hipDeviceSynchronize();
    phase_report("reset_stats");
    phase_zero();
#endif
}


// ---- graph mirror + graph-resident search -------------------------------------------------
// Room in the mirror for n nodes of stride0 and pool_len pool ints.  The four node arrays are replaced together, node_cap nodes
// each, when n outgrows them or the stride changes; the pool pair when pool_len outgrows it, doubled, 4096 ints at least.  (The
// caller sets g_stride0_ afterwards: after a failure here the arrays are empty, and the next call allocates whatever the stride.)
bool Device::graph_room(long long n, long long node_cap, int stride0, long long pool_len)
{
    if (n > g_cap_n() || stride0 != g_stride0_) {
        if (!reset_all(g_adj0_, g_level_, g_upper_, g_tested0_)) return false;
        if (!g_adj0_.grow((size_t)node_cap * stride0) || !g_level_.grow((size_t)node_cap) || !g_upper_.grow((size_t)node_cap) ||
            !g_tested0_.grow((size_t)node_cap))
            return false;
    }
    if (pool_len > g_pool_cap()) {
        if (!reset_all(g_pool_, g_testedU_)) return false;
        const size_t cap = (size_t)std::max<long long>(pool_len * 2, 4096);
        if (!g_pool_.grow(cap) || !g_testedU_.grow(cap)) return false; // (g_testedU_ is indexed by list offset / strideU: never more than cap)
    }
    return true;
}

bool Device::set_graph(const int *adj0, long long n, int stride0, const int *level, const int64_t *upper, const int *pool,
                       long long pool_len, int strideU)
{
    if (n < 0 || (n > 0 && (!adj0 || !level || !upper))) { set_dev_error("set_graph: bad argument"); return false; }
    if (stride0 - 1 > 128 || strideU - 1 > 128) { set_dev_error("set_graph: MaxEdges > 63 is not supported by the graph-resident kernels (use hnsw_mi355x_set_device_traversal(0))"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (!graph_room(n, std::max<long long>(n, std::max<long long>(capacity_, 1024)), stride0, pool_len)) return false;
    g_n_ = n; g_stride0_ = stride0; g_strideU_ = strideU;
    if (n > 0) {
        HIP_OK(hipMemcpyAsync(g_adj0_, adj0, sizeof(int) * (size_t)n * stride0, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(g_level_, level, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(g_upper_, upper, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    }
    if (pool_len > 0) HIP_OK(hipMemcpyAsync(g_pool_, pool, sizeof(int) * (size_t)pool_len, hipMemcpyHostToDevice, st));
    // lists that arrive from the host carry no pruning history
    if (g_tested0_) HIP_OK(hipMemsetAsync(g_tested0_, 0, sizeof(int) * g_tested0_.cap(), st));
    if (g_testedU_) HIP_OK(hipMemsetAsync(g_testedU_, 0, sizeof(int) * g_testedU_.cap(), st));
    HIP_OK(hipStreamSynchronize(st)); // host arrays are borrowed only for this call
    return true;
}

// LDS part of the candidate heap: sized for the common case (4 x beam width; C2 queries peak
// near 500 entries at ef = 128), the rest spills to HBM (SpillHeap).  A smaller LDS footprint means
// more resident waves to hide memory latency: 7.6 -> 6.1 ms per 10k-query launch going from 1024
// to 512 entries.  Beyond LDS + spill capacity the traversal is flagged for the lock-step path.
// Register sets of the sorted-list traversal (SortedTop<NS>: k <= 64 * NS); 0 = two-heap traversal
// only.  Diag sorted_top=0 forces the latter (the tests run both).
static int sorted_top_sets(int k)
{
    if (diag("sorted_top", 1) == 0) return 0;
    return k <= 128 ? 2 : k <= 256 ? 4 : k <= 512 ? 8 : 0; // (a beam of up to 64 entries runs in the two-set form as well)
}
constexpr long long kSortedTopMaxNodes = 1LL << 30; // the sorted list keeps two mark bits in the id word

int Device::max_waves_per_cu()
{
    // 20 = five per SIMD: what the int8 kernels' 92 VGPRs allow (10M x 96 int8, 12 500-query calls: 2.19 M queries/s at
    // 16, 2.31 M at 20); the float kernels (168 VGPRs) keep 12 resident whatever this says
    return 20;
}

// Blocks (= waves) of a persistent traversal launch: what stays resident on the chip.
template <class K>
static int resident_blocks(K kernel, size_t lds, int num_cu, int threads = 64)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds) != hipSuccess || per_cu < 1) per_cu = threads > 64 ? 4 : 8;
    return per_cu * std::max(1, num_cu);
}

static int cand_lds_cap(int k, int dim, bool heur, int nbcap)
{
    int cap = std::min(std::max(4 * k, 256), 4096);
    if (const int c = diag("cand_cap", 0)) cap = std::max(1, c); // tests: force spill / hand-back
    while (cap > 64 && search_lds_bytes(k, cap, dim, heur, nbcap) > 64 * 1024) cap /= 2;
    return cap;
}
// The LDS of a link launch (link_lds_bytes, dk_search_common.h), or 0 with the error set where it exceeds the budget: that launch
// is not made.  (Device::traversal_fits keeps Add away from such shapes; this is the guard of the launch itself.)
static size_t link_lds_or_error(const char *who, int pitch, int nbcap)
{
    const size_t lds = link_lds_bytes(pitch, nbcap);
    if (lds > 64 * 1024) { set_dev_error(std::string(who) + ": row length / list length exceed the LDS budget of the link launch"); return 0; }
    return lds;
}
static int spill_cap_for_tests()
{
    const int c = diag("spill_cap", -1);
    return c < 0 ? kSpillCap : std::min(kSpillCap, c);
}
// Filtered searches (graph_search_filtered_kernel): a candidate heap of cand_lds_cap() entries in LDS, as the unfiltered launches
// have, plus kFilterSpillCap in HBM per resident wave -- 256 KB each, 0.75 GB for the 3 072 waves of the float kernels (164 VGPRs,
// three per SIMD), 1.25 GB for the 5 120 of int8 (82 VGPRs) -- allocated by the first filtered call.  A selective filter keeps the
// result heap short of k for about k / selectivity evaluations, and every fresh neighbour is pushed meanwhile: at 1 % and a beam
// of 128 the heap was estimated to peak near 12 000 entries.  More LDS per wave would cost resident waves (the float kernel's
// LDS at C2 is 5.6 KB against VGPRs that allow three waves per SIMD, so LDS is not what limits it).  A job that outgrows the
// heap is handed back.  Diag spill_cap forces a smaller area (tests).
constexpr int kFilterSpillCap = 32768;
static int filter_spill_cap()
{
    const int c = diag("spill_cap", -1);
    return c < 0 ? kFilterSpillCap : std::min(kFilterSpillCap, c);
}
// ... and their visited tables (graphs whose sets are hash tables, above ~4M nodes): at least this many entries per wave (512 KB;
// 2.5 GB for the 5 120 waves the per-wave scratch is sized for), a table of their own (visited_scratch), crowded -- the job handed
// back -- beyond 98 304 visited ids.
// Each job clears its whole table, as every hashed launch does.  None of this is measured.
constexpr int kFilterVisCap = 1 << 17;


// Row loads overlapped with the visited atomics in launches that do not fill the chip, and in every launch on a
// graph large enough for the visited hash tables: there the traversal is bound by rows in flight, not by bytes
// (10M x 96 int8: 2.19 -> 2.43 M queries/s, 1.03 -> 1.12 M adds/s; 10M x 128 f32: +3 % / +5 %), while a full
// launch at 1M nodes is bandwidth-bound and gains nothing.  Diag overlap=0 disables, =2 forces it for
// every launch (tests).
// Shadow traversals in the search launches (graph_search_kernel): idle waves of a draining launch start the exact
// traversal of the jobs still running.  Diag shadow=0 disables (tests run both).
static bool shadow_mode()
{
    return diag("shadow", 1) != 0;
}
static int overlap_mode()
{
    return diag("overlap", 1);
}
// The latency variants of the traversal kernels (device_kernels.h, LAT) for launches that do not fill the chip -- B = 1
// Add, the exact window's rounds, small query calls: 0 never, 1 (default) when the jobs fit the variant's resident waves,
// 2 whenever the graph allows it (adjacency lists of at most 64 entries; tests).
// KnnQuery launches run WITHOUT a visited set (traverse_sorted, oflags bit 3): every listed neighbour's row is requested as
// soon as the list is known, and a neighbour seen before is recognised by what the set was standing in for -- it is still in
// the result list, or the push test turns it away again.  Diag novis=0 keeps the sets, =1 drops them only on the
// graphs whose sets are hash tables (A/B runs; same answers either way).  Measured, same box: C2 (1M x 128, bitsets) 2.46-2.56
// -> 3.07 M queries/s (25-26 -> 20.7 ms per 65 536-query launch, +2.5 % rows measured), 12 500-query calls 2.0 -> 2.39 M; C4-size
// 1.68 -> 2.03 M, C5-size 2.26 -> 2.70 M.
static bool lean_mode() { return diag("lean", 1) != 0; } // launches with flags 9 on the lean kernel forms (0: the plain forms read the flags)
static int novis_mode() // 0 never, 1 hash-table graphs only, 2 (default) every graph
{
    return diag("novis", 2);
}
static constexpr size_t kTeamLds = ((sizeof(TeamMail) + 15) & ~(size_t)15) + 16; // the latency variants' mailbox, behind the traversal's LDS
static int lat_mode()
{
    return diag("lat", 1);
}

// The MFMA Gram-block prefilter of RelativeNeighborPruning (device_kernels.h): on by default where it applies
// (cosine family, dim % 8 == 0); diag mfma=0 keeps the exact-only forms (the tests run both).
static bool mfma_heuristic()
{
    return diag("mfma", 1) != 0;
}

// The visited set of a traversal launch: a bitset of `words` words per wave (s_visited_), or per-wave hash tables of tab_cap
// entries (tab != nullptr), whose launches never touch the bitset arena -- bytes_per_job is what ensure_search_scratch sizes it by.
struct VisitedScratch {
    long long words = 0;
    size_t bytes_per_job = 0;
    int *tab = nullptr;
    int tab_cap = 0;
};

// The per-wave visited-id hash tables (VisitedSet): capacity a power of two, >= 16384 and >= 64 per
// beam entry (a traversal visits roughly 35 ids per beam entry), all entries -1 between jobs.
// Diag vis_hash=1/0 forces / forbids them; vis_hash_cap overrides the capacity (tests).
// filtered: the tables of the filtered search launches (far larger: kFilterVisCap), kept apart so that calls alternating between
// filtered and unfiltered searches never reallocate either.
bool Device::visited_scratch(int k, int min_cap, bool allow_hash, VisitedScratch *v, bool filtered)
{
    *v = VisitedScratch{};
    v->words = ((g_n_ + 31) / 32 + 3) & ~3LL;
    v->bytes_per_job = sizeof(unsigned) * (size_t)v->words;
    if (!allow_hash) return true; // (the eight-set kernels have no hash-table form: their launches keep bitsets whatever the graph's size)
    const int e = diag("vis_hash", -1);
    // measured: at 1M nodes (125-KB bitsets) the bitset is faster (2.5 M vs 1.9 M queries/s on C2); at
    // 10M (1.25 MB) the table wins (1.48 M vs 1.28 M with the log-cleared bitset, 0.98 M streaming it)
    const bool want = e >= 0 ? e != 0 : v->bytes_per_job > (512u << 10);
    if (!want) return true;
    int cap = 16384;
    while (cap < 64 * k && cap < (1 << 22)) cap <<= 1;
    if (const int c = diag("vis_hash_cap", 0)) { cap = 64; while (cap < c && cap < (1 << 22)) cap <<= 1; }
    // a traversal step inserts up to min_cap / 4 ids between two looks at crowded() (limit: 3/4 of the table)
    while (cap < min_cap) cap <<= 1;
    const size_t need = (size_t)max_slots() * (size_t)cap;
    DevBuf<int> &tab = filtered ? s_fvistab_ : s_vistab_;
    int &tab_each = filtered ? s_fvistab_each_ : s_vistab_each_;
    if (need > tab.cap() || cap != tab_each) { // (another capacity per wave: a new table even where the total fits)
        HIP_OK(hipStreamSynchronize(S(stream_)));
        if (!tab.reset() || !tab.grow(need)) return false;
        HIP_OK(hipMemsetAsync(tab, 0xff, sizeof(int) * need, S(stream_)));
        tab_each = cap;
    }
    v->tab = tab;
    v->tab_cap = cap;
    v->words = 0;          // the hashed kernels never touch the bitset arena: do not allocate one
    v->bytes_per_job = 16;
    return true;
}

// ---- traversal launches: which form of graph_search_kernel / graph_insert_search_kernel, on how many waves, with which flags ----
// Device::plan_traversal decides what holds for a whole call (register sets, visited set, novis), place_traversal what holds for
// one launch (form, waves, flags), traversal_kernel names the instantiation.
struct TraversalLaunch {
    int metric, max_slots, num_cu;
    size_t lds;          // the traversal's LDS (search_lds_bytes)
    int ns;              // sorted-top register sets: 2, 4, 8 (beams up to 128 / 256 / 512)
    bool exact_only;     // the exact two-heap traversal alone: the two-set form with launch flag 0x200
    VisitedScratch vis;
    bool novis;          // no visited set at all: flags 9 (bit 3 with the overlap bit)
    bool lat_ok;         // the latency form may run: sorted top, lists of at most 64 ids, room for its mailbox
    bool filtered;       // graph_search_filtered_kernel (an allow-set): exact traversal, visited sets kept, no latency form
    // per launch
    bool prefilter;      // the lean form's row prefilter may run: the index's shadow rows are current (search_batch_impl says so)
    bool pf_fixed;       // ... in its fixed-length form: the row length is kPfFixedDim words (diag pf_fixed_dim=0: the run-time form)
    bool pf8;            // ... on the 8-bit shadow (row_prefilter_ready() == 2; the row length then is kPfFixedDim words)
    int form;            // kFormLat, kFormLean, kFormLeanPF, kFormLeanPFFixed, kFormLeanPF8Fixed, kFormPlain
    int slots, grid;     // the form's resident waves; grid = min(jobs, slots)
    unsigned block;      // 128 threads for the latency form (logic wave + memory wave), else 64
    size_t lds_total;    // lds, plus kTeamLds of mailbox for the latency form
    int flags;           // 0x200 (exact only) | 9 (novis) or 1 (overlap); the launch site adds 0x100 (shadow, search) / 2 (mfma, insert)
};

bool Device::plan_traversal(bool insert, int k, bool two_heap, size_t lds, TraversalLaunch *t, bool filtered)
{
    const int ns = g_n_ < kSortedTopMaxNodes && !two_heap && !filtered ? sorted_top_sets(k) : 0;
    t->metric = metric_;
    t->max_slots = max_slots();
    t->num_cu = num_cu_;
    t->lds = lds;
    t->filtered = filtered;
    t->prefilter = t->pf8 = false;
    t->pf_fixed = pitch_ == kPfFixedDim && diag("pf_fixed_dim", 1) != 0; // (pitch_: the kernels' `dim` argument)
    t->exact_only = ns == 0; // two_heap callers, beams beyond 512 entries, diag sorted_top=0, filtered searches
    t->ns = t->exact_only ? 2 : ns;
    if (!visited_scratch(k, filtered ? kFilterVisCap : 512, t->ns != 8, &t->vis, filtered)) return false;
    if (filtered) { // the visited set stays (a disallowed node that was expanded and left the heap would be pushed again: DESIGN.md 3.9)
        t->novis = false;
        t->lat_ok = false;
        return true;
    }
    // (rows of more than 1 KB keep the sets: their traffic is small beside the rows', and the rows of re-seen neighbours are what
    //  costs -- C3's 3-KB rows: 282.7 k queries/s with the sets against 273.6 k without, build 69.5 k against 61.3 k adds/s.
    //  Add's searches run without a set as well; diag novis_insert=0 keeps the sets there)
    const int novis = novis_mode();
    t->novis = (!insert || diag("novis_insert", 1) != 0) && g_stride0_ - 2 <= 64 && overlap_mode() != 0 && (size_t)pitch_ * sizeof(float) <= 1024 &&
               (novis == 2 || (novis == 1 && t->vis.tab != nullptr));
    t->lat_ok = !t->exact_only && g_stride0_ - 2 <= 64 && lds + kTeamLds <= 64 * 1024;
    return true;
}

// The traversal kernel instantiation of (metric, NS, hashed, form).  This names exactly the forms device_kernels.h instantiates
// (HNSW_FOR_EACH_TRAVERSAL, HNSW_FOR_EACH_TRAVERSAL_LAT, HNSW_FOR_EACH_TRAVERSAL_LEAN): NS = 8 has no hashed form (visited_scratch() is
// told so), lean forms exist for graph_search_kernel with NS <= 4 only, graph_insert_search_kernel has none.  The forms of one kernel
// share a type: one function pointer serves the occupancy query and the launch.
template <bool Insert, int M, int NS, bool H>
static auto traversal_form(int form)
{
    if constexpr (Insert)
        return form == kFormLat ? &graph_insert_search_kernel<M, NS, H, kFormLat> : &graph_insert_search_kernel<M, NS, H, kFormPlain>;
    else if constexpr (NS <= 4)
        return form == kFormLat ? &graph_search_kernel<M, NS, H, kFormLat>
               : form == kFormLean ? &graph_search_kernel<M, NS, H, kFormLean>
               : form == kFormLeanPF ? &graph_search_kernel<M, NS, H, kFormLeanPF>
               : form == kFormLeanPFFixed ? &graph_search_kernel<M, NS, H, kFormLeanPFFixed>
               : form == kFormLeanPF8Fixed ? &graph_search_kernel<M, NS, H, kFormLeanPF8Fixed> : &graph_search_kernel<M, NS, H, kFormPlain>;
    else
        return form == kFormLat ? &graph_search_kernel<M, NS, H, kFormLat> : &graph_search_kernel<M, NS, H, kFormPlain>;
}
template <bool Insert>
static auto traversal_kernel(const TraversalLaunch &t, int form)
{
    const bool hashed = t.vis.tab != nullptr;
    decltype(traversal_form<Insert, M_SQ, 2, false>(0)) kernel = nullptr;
    with_metric(t.metric, [&](auto m) {
        if (t.ns == 2) kernel = hashed ? traversal_form<Insert, m, 2, true>(form) : traversal_form<Insert, m, 2, false>(form);
        else if (t.ns == 4) kernel = hashed ? traversal_form<Insert, m, 4, true>(form) : traversal_form<Insert, m, 4, false>(form);
        else kernel = traversal_form<Insert, m, 8, false>(form);
    });
    return kernel;
}

// The single-form persistent kernels (graph_search_filtered_kernel, graph_multilayer_kernel, graph_range_kernel; each with its own
// parameter list): the instantiation of (metric, hashed), named by of(m, h): [](auto m, auto h) { return &graph_multilayer_kernel<m, h>; }.
template <class Of>
static auto persistent_kernel(int metric, bool hashed, Of of)
{
    decltype(of(std::integral_constant<int, M_SQ>{}, std::false_type{})) kernel = nullptr;
    with_metric(metric, [&](auto m) { kernel = hashed ? of(m, std::true_type{}) : of(m, std::false_type{}); });
    return kernel;
}
// A launch of nj jobs of one of them: the plain persistent form on what stays resident, no flags.
template <class K>
static void place_persistent(K kernel, TraversalLaunch &t, int nj)
{
    t.form = kFormPlain;
    t.slots = std::min(t.max_slots, resident_blocks(kernel, t.lds, t.num_cu));
    t.grid = std::min(nj, t.slots);
    t.block = 64;
    t.lds_total = t.lds;
    t.flags = 0;
}

// One launch of nj jobs: the latency form when the jobs fit its resident waves (diag lat=2: whenever lat_ok), else the lean form for a
// search without visited sets (diag lean=0: the plain form, which reads flags 9 itself), else the plain form.  (No lean form of the
// insert kernel: measured, the f32 insert search LOSES 6 % with it -- profiles/r5_lean_ab.log.)  One occupancy query per form weighed.
template <bool Insert>
static auto place_traversal(TraversalLaunch &t, int nj)
{
    const bool hashed = t.vis.tab != nullptr;
    const int lat = lat_mode();
    t.form = kFormPlain;
    if (t.lat_ok && lat != 0) {
        const int slots = std::min(t.max_slots, resident_blocks(traversal_kernel<Insert>(t, kFormLat), t.lds + kTeamLds, t.num_cu, 128));
        if (slots > 0 && (lat == 2 || nj <= slots)) { t.form = kFormLat; t.slots = slots; }
    }
    if (!Insert && t.form == kFormPlain && t.novis && !t.exact_only && lean_mode() && t.ns <= 4) t.form = !t.prefilter ? kFormLean : t.pf8 ? kFormLeanPF8Fixed : t.pf_fixed ? kFormLeanPFFixed : kFormLeanPF;
    const auto kernel = traversal_kernel<Insert>(t, t.form);
    if (t.form != kFormLat) t.slots = std::min(t.max_slots, resident_blocks(kernel, t.lds, t.num_cu));
    t.grid = std::min(nj, t.slots);
    t.block = t.form == kFormLat ? 128 : 64;
    t.lds_total = t.lds + (t.form == kFormLat ? kTeamLds : 0);
    const int overlap = overlap_mode();
    t.flags = (t.exact_only ? 0x200 : 0) | (t.novis ? 9 : overlap == 2 || (overlap == 1 && (nj <= t.slots || hashed)) ? 1 : 0);
    return kernel;
}

// chunk: jobs per launch (job / result buffers); slots: waves of a persistent launch (visited
// bitsets, spill areas).  The visited arena is all zero between launches: zeroed when allocated,
// and every wave clears its bitset after each job.
bool Device::ensure_search_scratch(long long chunk, long long slots, int k, size_t vis_bytes_per_job)
{
    const size_t vis_words = vis_bytes_per_job * (size_t)slots / sizeof(unsigned); // (bytes_per_job is whole words)
    if (vis_words > s_visited_.cap()) {
        if (!s_visited_.grow(vis_words)) return false;
        HIP_OK(hipMemsetAsync(s_visited_, 0, sizeof(unsigned) * vis_words, S(stream_)));
    }
    const size_t jobs_cap = s_flag_.cap();
    // [next job, next shadow, -, -, one word per job] (graph_search_kernel): as many words as s_jobs_ has jobs, so it grows when s_jobs_ does
    if (!s_jobctr_.grow(4 + std::max<size_t>((size_t)chunk, jobs_cap))) return false;
    if ((size_t)chunk > jobs_cap) {
        uj_len_ = 0;
        if (!reset_all(s_jobs_, s_cnt_, s_flag_)) return false;
        if (!s_jobs_.grow((size_t)chunk) || !s_cnt_.grow((size_t)chunk) || !s_flag_.grow((size_t)chunk)) return false;
    }
    if (k > 0 && !s_hits_.grow((size_t)chunk * k + ((size_t)chunk + 1) / 2)) return false; // ids, distances, and (single-launch calls) the flags behind them
    if (!s_spill_.grow((size_t)slots * kSpillCap + 8)) return false; // +8: get2 may read one entry past a heap
    if (!s_evals_.grow(1)) return false;
    return ev0_.create(true) && ev1_.create(true) && ev2_.create(false);
}

static bool jobs_valid(const SearchJob *jobs, int njobs, long long g_n, long long n_queries, long long n_rows)
{
    for (int i = 0; i < njobs; ++i) {
        const SearchJob &j = jobs[i];
        bool ok = j.entry >= 0 && j.entry < g_n && j.search_layer >= 0 && j.entry_layer >= j.search_layer &&
                  (j.qref >= 0 ? j.qref < n_queries : (~j.qref) < n_rows);
        if (!ok) return false;
    }
    return true;
}

bool Device::insert_search_batch(const SearchJob *jobs, int njobs, int k, int max_edges0, int n_upper, InsertResults *res, WindowExtras *win)
{
    if (njobs <= 0) return true;
    const bool windowed = win != nullptr; // exact-window Add: read logs, selections and dry-run flags come back with the job flags, one wait
    const int read_log_cap = windowed ? win->read_log_cap : 0;
    if (windowed && (read_log_cap < 8 || njobs > (1 << 16) || (n_upper > 0 && !win->upper_owner))) { set_dev_error("insert_search_batch: bad window request"); return false; }
    if (!jobs || !res || k < 1 || n_upper < 0 || max_edges0 < 2) { set_dev_error("insert_search_batch: bad argument"); return false; }
    if (g_n_ <= 0) { set_dev_error("insert_search_batch: no graph uploaded"); return false; }
    for (int i = 0; i < njobs; ++i) {
        const SearchJob &j = jobs[i];
        if (j.qref >= 0) { set_dev_error("insert_search_batch: qref must name a stored row"); return false; }
        if (j.search_layer > 0 && (j.aux < 0 || j.aux + j.search_layer > n_upper)) { set_dev_error("insert_search_batch: upper-layer slot out of range"); return false; }
        if (j.stop_layer < 0 || j.stop_layer > j.search_layer || (!windowed && j.stop_layer != 0)) { set_dev_error("insert_search_batch: bad stop layer"); return false; }
    }
    if (!jobs_valid(jobs, njobs, g_n_, n_queries_, n_rows_hw_)) { set_dev_error("insert_search_batch: job outside the uploaded graph / rows"); return false; }
    const int cand_cap = cand_lds_cap(k, pitch_, true, nbcap());
    const size_t lds = search_lds_bytes(k, cand_cap, pitch_, true, nbcap());
    if (lds > 64 * 1024) { set_dev_error("insert_search_batch: beam width / dimension exceed the LDS budget"); return false; }
    const size_t lds_link = windowed ? link_lds_or_error("insert_search_batch", pitch_, nbcap()) : 0; // the window's dry-run link launch
    if (windowed && !lds_link) return false;
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const int sel_stride = max_edges0;
    const long long chunk = std::min<long long>(njobs, 1 << 20);
    TraversalLaunch tl;
    if (!plan_traversal(true, k, false, lds, &tl)) return false;
    if (!ensure_search_scratch(chunk, max_slots(), 0, tl.vis.bytes_per_job)) return false;
    const size_t nU = (size_t)std::max(n_upper, 1);
    if (!s_sel_.grow((size_t)njobs * sel_stride) || !s_lcnt_.grow((size_t)njobs) || !s_selU_.grow(nU * sel_stride) || !s_cntU_.grow(nU) || !s_iflag_.grow((size_t)njobs))
        return false;
    if (windowed && !s_rlog_.grow((size_t)njobs * (size_t)read_log_cap)) return false;
    // pinned results: [sel0 | cnt0 | selU | cntU | flag | evals | read logs | dry0 | dryU]
    const size_t b_sel0 = 4u * (size_t)njobs * sel_stride, b_cnt0 = 4u * (size_t)njobs, b_selU = 4u * nU * sel_stride, b_cntU = 4u * nU, b_flag = 4u * (size_t)njobs;
    const size_t b_log = windowed ? 4u * (size_t)njobs * (size_t)read_log_cap : 0;
    const size_t b_dry = windowed ? b_sel0 + b_selU : 0;
    const size_t b_drop = windowed ? 3u * b_sel0 : 0;          // three ids per layer-0 selection entry
    const size_t b_rep = windowed ? b_flag : 0;                // the jobs' "repeated" flags (the job flags themselves are folded to 0 / 1 below)
    if (windowed && !s_wdry_.grow(nU)) return false; // (upper_owner)
    const size_t need = b_sel0 + b_cnt0 + b_selU + b_cntU + b_flag + 16 + b_log + b_dry + b_drop + b_rep;
    // windowed: everything the kernels write lives in ONE device block laid out like the pinned results below, so that it comes
    // back in one copy (a round of the exact window is ~2 ms: a dozen 4-microsecond copies and their launch overhead showed)
    if (windowed && !s_win_.grow((need - b_rep + 3) / 4u + 64)) return false;
    if (!h_res_.grow(need, need + need / 2)) return false;
    char *hb = h_res_;
    int *h_sel0 = reinterpret_cast<int *>(hb), *h_cnt0 = reinterpret_cast<int *>(hb + b_sel0);
    int *h_selU = reinterpret_cast<int *>(hb + b_sel0 + b_cnt0), *h_cntU = reinterpret_cast<int *>(hb + b_sel0 + b_cnt0 + b_selU);
    int *h_flag = reinterpret_cast<int *>(hb + b_sel0 + b_cnt0 + b_selU + b_cntU);
    unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hb + ((b_sel0 + b_cnt0 + b_selU + b_cntU + b_flag + 7) & ~(size_t)7));
    int *h_log = reinterpret_cast<int *>(reinterpret_cast<char *>(h_ev) + 8);
    // where the kernels write: the members, or (windowed) the same offsets inside s_win_
    char *db = reinterpret_cast<char *>(s_win_.get());
    int *p_sel0 = windowed ? reinterpret_cast<int *>(db) : s_sel_, *p_cnt0 = windowed ? reinterpret_cast<int *>(db + b_sel0) : s_lcnt_;
    int *p_selU = windowed ? reinterpret_cast<int *>(db + b_sel0 + b_cnt0) : s_selU_, *p_cntU = windowed ? reinterpret_cast<int *>(db + b_sel0 + b_cnt0 + b_selU) : s_cntU_;
    int *p_flag = windowed ? reinterpret_cast<int *>(db + b_sel0 + b_cnt0 + b_selU + b_cntU) : s_iflag_;
    const size_t off_ev = (b_sel0 + b_cnt0 + b_selU + b_cntU + b_flag + 7) & ~(size_t)7;
    unsigned long long *p_evals = windowed ? reinterpret_cast<unsigned long long *>(db + off_ev) : s_evals_;
    int *p_log = windowed ? reinterpret_cast<int *>(db + off_ev + 8) : s_rlog_;
    // staging: [jobs | processing order]
    SearchJob *h_jobs = static_cast<SearchJob *>(pinned_stage((sizeof(SearchJob) + sizeof(int)) * (size_t)chunk));
    if (!h_jobs) return false;
    int *h_order = reinterpret_cast<int *>(h_jobs + chunk);
    if (!s_order_.grow((size_t)chunk)) return false;
    for (long long off = 0; off < njobs; off += chunk) {
        const int nj = (int)std::min<long long>(chunk, njobs - off);
        memcpy(h_jobs, jobs + off, sizeof(SearchJob) * (size_t)nj);
        HIP_OK(hipMemcpyAsync(s_jobs_, h_jobs, sizeof(SearchJob) * (size_t)nj, hipMemcpyHostToDevice, st));
        uj_len_ = 0; // search_queries' jobs are gone from s_jobs_
        // items that search several layers first (counting sort by first layer, descending; stable)
        const int *d_order = nullptr;
        {
            int hist[64] = {0}, maxl = 0;
            for (int i = 0; i < nj; ++i) { const int l = std::min(h_jobs[i].search_layer, 63); hist[l]++; maxl = std::max(maxl, l); }
            if (maxl > 0 && nj > 1) {
                int start[64], acc = 0;
                for (int l = maxl; l >= 0; --l) { start[l] = acc; acc += hist[l]; }
                for (int i = 0; i < nj; ++i) h_order[start[std::min(h_jobs[i].search_layer, 63)]++] = i;
                HIP_OK(hipMemcpyAsync(s_order_, h_order, sizeof(int) * (size_t)nj, hipMemcpyHostToDevice, st));
                d_order = s_order_;
            }
        }
        HIP_OK(hipMemsetAsync(s_jobctr_, 0, sizeof(int), st));
        HIP_OK(hipMemsetAsync(p_evals, 0, sizeof(unsigned long long), st));
        const bool timed = profiling_;
        if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
        const auto kernel = place_traversal<true>(tl, nj);
        hipLaunchKernelGGL(kernel, dim3(tl.grid), dim3(tl.block), tl.lds_total, st, d_rows_, d_row_sn_, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_,
                           g_strideU_, s_jobs_, k, cand_cap, reinterpret_cast<ND *>(s_spill_.get()), spill_cap_for_tests(), max_edges0, s_visited_, tl.vis.words,
                           tl.vis.tab, tl.vis.tab_cap, p_sel0 + (size_t)off * sel_stride, p_cnt0 + off, p_selU, p_cntU, sel_stride, p_flag + off, p_evals,
                           nbcap(), nj, s_jobctr_, tl.flags | (mfma_heuristic() ? 2 : 0), d_order, windowed ? p_log : (int *)nullptr, read_log_cap);
        if (tl.form == kFormLat) stats_.lat_launches++;
        HIP_OK(hipGetLastError());
        if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
        if (!windowed) HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (windowed) { // one launch (njobs <= chunk): everything the host validates with rides on the same wait
            int *d_owner = s_wdry_, *d_dry0 = p_log + b_log / 4u, *d_dryU = d_dry0 + (size_t)njobs * sel_stride, *d_drop0 = d_dry0 + b_dry / 4u;
            if (n_upper > 0) {
                memcpy(h_log + b_log / 4u, win->upper_owner, 4u * (size_t)n_upper); // staged behind the logs (the dry flags land there afterwards)
                HIP_OK(hipMemcpyAsync(d_owner, h_log + b_log / 4u, 4u * (size_t)n_upper, hipMemcpyHostToDevice, st));
            }
            HIP_OK(hipMemsetAsync(d_dry0, 0xff, b_dry, st)); // every code "changed, set of lost ids unknown" unless the kernel says otherwise
            const int k_cap = nbcap();
            const int grid = (njobs + n_upper) * sel_stride;
            with_metric(metric_, [&](auto m) {
                hipLaunchKernelGGL(graph_link_dry_sel_kernel<m>, dim3(grid), dim3(64), lds_link, st, d_rows_, d_row_sn_, pitch_, g_adj0_, g_stride0_,
                                   g_upper_, g_pool_, g_strideU_, s_jobs_, p_flag, p_sel0, p_cnt0, p_selU, p_cntU, sel_stride, d_owner, njobs, max_edges0,
                                   k_cap, d_dry0, d_dryU, p_evals, nbcap(), g_tested0_, g_testedU_, g_n_, d_drop0);
            });
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(hb, db, need - b_rep, hipMemcpyDeviceToHost, st)); // selections, counts, flags, evaluations, read logs, dry-run codes, lost ids
        }
        const bool last_chunk = off + nj >= njobs;
        if (!windowed && last_chunk) HIP_OK(hipMemcpyAsync(h_flag, s_iflag_, b_flag, hipMemcpyDeviceToHost, st)); // the flags ride on the same wait
        HIP_OK(hipStreamSynchronize(st)); // the job staging buffer is reused by the next chunk
        if (!count_launch(&kInsertFamily, *h_ev, tl.vis.tab != nullptr, timed, ev0_, ev1_)) return false;
    }
    // Only the flags come back (with the last launch's wait): the selections stay on the device, where the link half reads
    // them (link_batch_planned); a caller that links on the host fetches them (fetch_insert_selections).
    int *h_rep = windowed ? h_log + (b_log + b_dry + b_drop) / 4u : nullptr;
    for (int i = 0; i < njobs; ++i) {
        if (h_rep) h_rep[i] = h_flag[i] == 2;
        if (h_flag[i] == 2) { stats_.search_repeats++; stats_.insert_tie_reruns++; h_flag[i] = 0; }
        stats_.search_overflows += (uint64_t)(h_flag[i] != 0);
    }
    last_insert_jobs_ = (njobs <= chunk && !windowed) ? njobs : 0; // a single launch left everything in place (windowed: in its own block)
    last_insert_upper_ = n_upper;
    last_insert_stride_ = sel_stride;
    fetch_njobs_ = windowed ? 0 : njobs;
    fetch_nupper_ = n_upper;
    *res = InsertResults{h_sel0, h_cnt0, h_selU, h_cntU, h_flag, sel_stride};
    if (windowed) {
        win->read_log = h_log; win->dry0 = h_log + b_log / 4u; win->dryU = win->dry0 + (size_t)njobs * sel_stride;
        win->drop0 = win->dry0 + b_dry / 4u; win->repeated = h_rep;
    }
    return true;
}

// The selected ids of the last insert_search_batch, into the pinned arrays its InsertResults name.
bool Device::fetch_insert_selections(const InsertResults *res)
{
    if (!res || fetch_njobs_ <= 0) return true;
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const int njobs = fetch_njobs_, n_upper = fetch_nupper_, sel_stride = res->sel_stride;
    HIP_OK(hipMemcpyAsync(const_cast<int *>(res->sel0), s_sel_, 4u * (size_t)njobs * sel_stride, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(const_cast<int *>(res->cnt0), s_lcnt_, 4u * (size_t)njobs, hipMemcpyDeviceToHost, st));
    if (n_upper > 0) {
        HIP_OK(hipMemcpyAsync(const_cast<int *>(res->selU), s_selU_, 4u * (size_t)n_upper * sel_stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(const_cast<int *>(res->cntU), s_cntU_, 4u * (size_t)n_upper, hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));
    fetch_njobs_ = 0;
    return true;
}

bool Device::traversal_fits(int k, bool with_heuristic, int max_edges) const
{
    if (k < 1 || 2 * max_edges + 1 > 128) return false;
    const int nb = std::max(8, (2 * max_edges + 1 + 7) & ~7);
    const int cap = cand_lds_cap(k, pitch_, with_heuristic, nb);
    // with_heuristic: Add, whose selections the link launches apply -- their LDS is the relink's plus the shortcut's scratch
    const bool link_ok = !with_heuristic || link_lds_bytes(pitch_, nb) <= 64 * 1024;
    return search_lds_bytes(k, cap, pitch_, with_heuristic, nb) <= 64 * 1024 && search_lds_bytes(nb, 0, pitch_, true, nb) <= 64 * 1024 && link_ok;
}

bool Device::graph_append_nodes(long long first, long long n, const int *level, const int64_t *upper, const int *pool,
                                long long pool_from, long long pool_len, bool *need_full_sync)
{
    *need_full_sync = false;
    if (n <= 0) return true;
    if (!g_adj0_ || first != g_n_ || first + n > g_cap_n() || pool_len > g_pool_cap()) { *need_full_sync = true; return true; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    HIP_OK(hipMemcpyAsync(g_level_ + first, level + first, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(g_upper_ + first, upper + first, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, st));
    // new nodes start with empty lists (GraphData.NewNode :224-242)
    HIP_OK(hipMemsetAsync(g_adj0_ + (size_t)first * g_stride0_, 0, sizeof(int) * (size_t)n * g_stride0_, st));
    HIP_OK(hipMemsetAsync(g_tested0_ + first, 0, sizeof(int) * (size_t)n, st));
    if (pool_len > pool_from) HIP_OK(hipMemsetAsync(g_testedU_ + pool_from / std::max(1, g_strideU_), 0, sizeof(int) * (size_t)((pool_len - pool_from) / std::max(1, g_strideU_) + 1), st));
    if (pool_len > pool_from) HIP_OK(hipMemcpyAsync(g_pool_ + pool_from, pool + pool_from, sizeof(int) * (size_t)(pool_len - pool_from), hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
    g_n_ = first + n;
    return true;
}

bool Device::link_batch(const int *rows, int nrows, int row_stride, const int *g_node, const int *g_layer, const int *g_off,
                        const int *g_items, int ngroups, int max_edges0, int *out_lists, int list_stride)
{
    if (ngroups > 0 && !out_lists) { set_dev_error("link_batch: bad argument"); return false; }
    const int *res = nullptr;
    if (!link_batch_begin(0, rows, nrows, row_stride, g_node, g_layer, g_off, g_items, ngroups, max_edges0, list_stride)) return false;
    if (!link_batch_finish(0, &res)) return false;
    if (ngroups > 0) memcpy(out_lists, res, sizeof(int) * (size_t)ngroups * list_stride);
    return true;
}

bool Device::link_batch_begin(int set, const int *rows, int nrows, int row_stride, const int *g_node, const int *g_layer, const int *g_off,
                              const int *g_items, int ngroups, int max_edges0, int list_stride, bool want_lists)
{
    if (set < 0 || set > 1 || nrows < 0 || ngroups < 0 || (nrows > 0 && !rows) || (ngroups > 0 && (!g_node || !g_layer || !g_off || !g_items))) {
        set_dev_error("link_batch: bad argument");
        return false;
    }
    LinkSet &ls = lset_[set];
    if (ls.busy) { set_dev_error("link_batch: staging set still in flight"); return false; }
    if (g_n_ <= 0) { set_dev_error("link_batch: no graph uploaded"); return false; }
    // host-side validation: a bad id must be an error return, never a GPU fault
    for (int r = 0; r < nrows; ++r) {
        const int *x = rows + (size_t)r * row_stride;
        bool ok = x[0] >= 0 && x[0] < g_n_ && x[1] >= 0 && x[2] >= 0 && x[2] <= row_stride - 3 &&
                  x[2] <= (x[1] == 0 ? max_edges0 : max_edges0 / 2);
        for (int i = 0; ok && i < x[2]; ++i) ok = x[3 + i] >= 0 && x[3 + i] < g_n_;
        if (!ok) { set_dev_error("link_batch: row record outside the graph"); return false; }
    }
    const int total = ngroups > 0 ? g_off[ngroups] : 0;
    for (int g = 0; g < ngroups; ++g)
        if (g_node[g] < 0 || g_node[g] >= g_n_ || g_layer[g] < 0 || g_off[g + 1] < g_off[g]) { set_dev_error("link_batch: group outside the graph"); return false; }
    for (int t = 0; t < total; ++t)
        if (g_items[t] < 0 || g_items[t] >= g_n_) { set_dev_error("link_batch: item outside the graph"); return false; }
    if (list_stride < max_edges0 + 1 || max_edges0 + 1 > nbcap()) { set_dev_error("link_batch: list stride too small"); return false; }
    const size_t lds = ngroups > 0 ? link_lds_or_error("link_batch", pitch_, nbcap()) : 0;
    if (ngroups > 0 && !lds) return false;
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (!ensure_search_scratch(1, 1, 0, 16)) return false;
    const size_t need[5] = {(size_t)nrows * row_stride, (size_t)ngroups * 2, (size_t)ngroups + 1, (size_t)std::max(total, 1), (size_t)ngroups * list_stride};
    // device buffers are shared by both sets: the stream orders one sub-batch after the other.
    // Growing one frees the old allocation, which must not be in use any more.
    for (int i = 0; i < 5; ++i) {
        if (std::max<size_t>(need[i], 1) > s_lk_[i].cap()) {
            HIP_OK(hipStreamSynchronize(st));
            if (!s_lk_[i].grow(std::max<size_t>(need[i], 1), std::max<size_t>(need[i], 1) * 2)) return false;
        }
    }
    // pinned staging of this set: [rows | node | layer | off | items], results, evaluation count
    const size_t in_ints = need[0] + need[1] + need[2] + need[3];
    if (!ls.h_in.grow(in_ints, in_ints * 2) || !ls.h_out.grow(std::max<size_t>(need[4], 1), std::max<size_t>(need[4], 1) * 2) || !ls.h_ev.grow(2)) return false;
    if (!ls.ev_start.create(true) || !ls.ev_stop.create(true) || !ls.ev_done.create(true)) return false;
    int *h_rows = ls.h_in, *h_node = h_rows + need[0], *h_off = h_node + need[1], *h_items = h_off + need[2];
    if (nrows > 0) memcpy(h_rows, rows, sizeof(int) * need[0]);
    if (ngroups > 0) {
        memcpy(h_node, g_node, sizeof(int) * (size_t)ngroups);
        memcpy(h_node + ngroups, g_layer, sizeof(int) * (size_t)ngroups);
        memcpy(h_off, g_off, sizeof(int) * ((size_t)ngroups + 1));
        memcpy(h_items, g_items, sizeof(int) * (size_t)total);
    }
    *ls.h_ev = 0;
    ls.ngroups = ngroups;
    ls.timed = false;
    if (nrows > 0) {
        HIP_OK(hipMemcpyAsync(s_lk_[0], h_rows, sizeof(int) * need[0], hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(graph_write_rows_kernel, dim3(nrows), dim3(64), 0, st, g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, s_lk_[0], row_stride,
                           g_tested0_, g_testedU_, max_edges0);
        HIP_OK(hipGetLastError());
    }
    if (ngroups > 0) {
        HIP_OK(hipMemcpyAsync(s_lk_[1], h_node, sizeof(int) * (size_t)ngroups * 2, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s_lk_[2], h_off, sizeof(int) * ((size_t)ngroups + 1), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemcpyAsync(s_lk_[3], h_items, sizeof(int) * (size_t)total, hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
        ls.timed = profiling_;
        if (ls.timed) HIP_OK(hipEventRecord(E(ls.ev_start), st));
        const int k_cap = nbcap();
        with_metric(metric_, [&](auto m) {
            hipLaunchKernelGGL(graph_link_kernel<m>, dim3(ngroups), dim3(64), lds, st, d_rows_, d_row_sn_, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_,
                               g_strideU_, s_lk_[1], s_lk_[1] + ngroups, s_lk_[2], (const int *)nullptr, s_lk_[3], max_edges0, k_cap, s_lk_[4], list_stride,
                               s_evals_, nbcap(), g_tested0_, g_testedU_, (const int *)nullptr);
        });
        HIP_OK(hipGetLastError());
        if (ls.timed) HIP_OK(hipEventRecord(E(ls.ev_stop), st));
        if (want_lists) HIP_OK(hipMemcpyAsync(ls.h_out, s_lk_[4], sizeof(int) * (size_t)ngroups * list_stride, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(ls.h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipEventRecord(E(ls.ev_done), st));
    ls.busy = true;
    return true;
}

bool Device::link_dry_run(const int *jobs3, int n, int max_edges0, int *changed)
{
    if (n <= 0) return true;
    if (!jobs3 || !changed || max_edges0 + 1 > nbcap()) { set_dev_error("link_dry_run: bad argument"); return false; }
    if (g_n_ <= 0) { set_dev_error("link_dry_run: no graph uploaded"); return false; }
    const size_t lds = link_lds_or_error("link_dry_run", pitch_, nbcap());
    if (!lds) return false;
    for (int i = 0; i < n; ++i) { // a bad id must be an error return, never a GPU fault
        const int nb = jobs3[3 * i], layer = jobs3[3 * i + 1], item = jobs3[3 * i + 2];
        if (nb < 0 || nb >= g_n_ || item < 0 || item >= g_n_ || layer < 0) { set_dev_error("link_dry_run: job outside the graph"); return false; }
    }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (!ensure_search_scratch(1, 1, 0, 16)) return false;
    if (!s_dry_.grow((size_t)n * 4)) return false;
    int *h = static_cast<int *>(pinned_stage(sizeof(int) * (size_t)n * 4 + 16));
    if (!h) return false;
    unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(h + (((size_t)n * 4 + 1) & ~(size_t)1));
    memcpy(h, jobs3, sizeof(int) * (size_t)n * 3);
    HIP_OK(hipMemcpyAsync(s_dry_, h, sizeof(int) * (size_t)n * 3, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
    const int k_cap = nbcap();
    with_metric(metric_, [&](auto m) {
        hipLaunchKernelGGL(graph_link_dry_kernel<m>, dim3(n), dim3(64), lds, st, d_rows_, d_row_sn_, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_,
                           g_strideU_, s_dry_, max_edges0, k_cap, s_dry_ + (size_t)n * 3, s_evals_, nbcap(), g_tested0_, g_testedU_);
    });
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h + (size_t)n * 3, s_dry_ + (size_t)n * 3, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    memcpy(changed, h + (size_t)n * 3, sizeof(int) * (size_t)n);
    stats_.search_launches++; // a search launch whose evaluations are link work -- but not a link launch
    stats_.search_evals += *h_ev;
    stats_.link_evals += *h_ev;
    return true;
}

bool Device::link_batch_planned(int njobs, int n_upper, int max_edges0)
{
    if (njobs <= 0) return true;
    if (njobs != last_insert_jobs_ || n_upper != last_insert_upper_ || max_edges0 != last_insert_stride_ || max_edges0 + 1 > nbcap()) {
        set_dev_error("link_batch_planned: no matching insert_search_batch results on the device");
        return false;
    }
    const size_t lds = link_lds_or_error("link_batch_planned", pitch_, nbcap());
    if (!lds) return false;
    last_insert_jobs_ = 0;
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (!ensure_search_scratch(1, 1, 0, 16)) return false;
    // per-slot counters: all zero between batches (the link kernel resets what it used)
    const long long slots = g_cap_n() + g_pool_cap() / std::max(1, g_strideU_) + 2;
    if ((size_t)slots != lp_slot_[2].cap()) { // (the mirror was resized: the last of the three says for how many slots they stand)
        HIP_OK(hipStreamSynchronize(st));
        for (int i = 0; i < 3; ++i) {
            if (!lp_slot_[i].reset() || !lp_slot_[i].grow((size_t)slots)) return false;
            HIP_OK(hipMemsetAsync(lp_slot_[i], 0, sizeof(int) * (size_t)slots, st));
        }
    }
    const size_t max_appends = (size_t)(njobs + n_upper) * (size_t)max_edges0 + 1;
    for (int i = 0; i < 6; ++i) {
        if (max_appends > lp_grp_[i].cap()) {
            HIP_OK(hipStreamSynchronize(st));
            if (!lp_grp_[i].grow(max_appends, max_appends * 2)) return false;
        }
    }
    if (!lp_counters_.grow(4)) return false;
    HIP_OK(hipMemsetAsync(lp_counters_, 0, sizeof(int) * 4, st));
    HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
    size_t g_cap = lp_grp_[0].cap();
    for (int i = 1; i < 6; ++i) g_cap = std::min(g_cap, lp_grp_[i].cap());
    LinkPlan P{lp_slot_[0], lp_slot_[1], lp_slot_[2], lp_grp_[0], lp_grp_[1], lp_grp_[2], lp_grp_[3], lp_grp_[4], lp_counters_, g_cap_n(),
               slots, g_n_, (int)std::min<size_t>(g_cap, 0x7fffffff), njobs};
    const bool timed = profiling_;
    if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
    hipLaunchKernelGGL(link_plan_kernel<true>, dim3(njobs), dim3(64), 0, st, s_jobs_, s_sel_, s_lcnt_, s_selU_, s_cntU_, last_insert_stride_,
                       g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, g_tested0_, g_testedU_, max_edges0, P);
    hipLaunchKernelGGL(link_offsets_kernel, dim3(512), dim3(256), 0, st, g_upper_, g_strideU_, P);
    hipLaunchKernelGGL(link_plan_kernel<false>, dim3(njobs), dim3(64), 0, st, s_jobs_, s_sel_, s_lcnt_, s_selU_, s_cntU_, last_insert_stride_,
                       g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, g_tested0_, g_testedU_, max_edges0, P);
    HIP_OK(hipGetLastError());
    // the number of groups comes back to size the last two launches (16 bytes, one short wait) -- except for small batches
    // (bounded-concurrency Add: a few hundred items per batch, a batch every 1-3 ms), which launch the upper bound
    // instead and let the surplus blocks leave at once
    unsigned long long *h_ev = static_cast<unsigned long long *>(pinned_stage(32));
    if (!h_ev) return false;
    int *h_ctr = reinterpret_cast<int *>(h_ev + 1);
    const bool bounded = njobs <= 4096;
    int G = (int)std::min<size_t>(max_appends - 1, g_cap);
    if (!bounded) {
        HIP_OK(hipMemcpyAsync(h_ctr, lp_counters_, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        G = h_ctr[0];
        if (h_ctr[3] != 0 || G < 0 || (size_t)G > g_cap) {
            set_dev_error("link_batch_planned: inconsistent selection data on the device (guard " + std::to_string(h_ctr[3]) + ")");
            return false;
        }
    }
    if (G > 0) {
        hipLaunchKernelGGL(link_order_kernel, dim3(G), dim3(64), 0, st, s_jobs_, g_upper_, g_strideU_, lp_grp_[5], P, bounded ? 1 : 0);
        HIP_OK(hipGetLastError());
        const int k_cap = nbcap();
        with_metric(metric_, [&](auto m) {
            hipLaunchKernelGGL(graph_link_kernel<m>, dim3(G), dim3(64), lds, st, d_rows_, d_row_sn_, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_,
                               g_strideU_, lp_grp_[0], lp_grp_[1], lp_grp_[2], lp_grp_[3], lp_grp_[5], max_edges0, k_cap, (int *)nullptr, 0, s_evals_,
                               nbcap(), g_tested0_, g_testedU_, bounded ? (const int *)lp_counters_ : (const int *)nullptr);
        });
        HIP_OK(hipGetLastError());
    }
    if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
    HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_ctr, lp_counters_, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (h_ctr[3] != 0 || h_ctr[0] < 0 || (size_t)h_ctr[0] > g_cap) {
        set_dev_error("link_batch_planned: inconsistent selection data on the device (guard " + std::to_string(h_ctr[3]) + ")");
        return false;
    }
    return count_launch(&kLinkFamily, *h_ev, false, timed, ev0_, ev1_);
}

bool Device::download_graph(int *adj0, long long n, int *pool, long long pool_len)
{
    if (n < 0 || n > g_n_ || pool_len < 0 || pool_len > g_pool_cap() || (n > 0 && !adj0) || (pool_len > 0 && !pool)) { set_dev_error("download_graph: bad argument"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (n > 0) HIP_OK(hipMemcpyAsync(adj0, g_adj0_, sizeof(int) * (size_t)n * g_stride0_, hipMemcpyDeviceToHost, st));
    if (pool_len > 0) HIP_OK(hipMemcpyAsync(pool, g_pool_, sizeof(int) * (size_t)pool_len, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    return true;
}

bool Device::link_batch_finish(int set, const int **out_lists)
{
    if (set < 0 || set > 1 || !lset_[set].busy) { set_dev_error("link_batch_finish: nothing in flight"); return false; }
    LinkSet &ls = lset_[set];
    if (!bind()) return false;
    HIP_OK(hipEventSynchronize(E(ls.ev_done)));
    ls.busy = false;
    if (out_lists) *out_lists = ls.h_out;
    if (ls.ngroups > 0 && !count_launch(&kLinkFamily, *ls.h_ev, false, ls.timed, ls.ev_start, ls.ev_stop)) return false;
    return true;
}


// Pinned host staging (grown on demand): DMA to/from pageable user memory runs at ~2 GB/s,
// through a pinned bounce buffer at PCIe rate.
void *Device::pinned_stage(size_t bytes)
{
    return h_stage_.grow(bytes, std::max<size_t>(bytes, 1u << 20)) ? h_stage_.get() : nullptr;
}

// KnnQuery on the device: descent + layer-0 beam search (width k) + the stable top-k_out tail.
// out_ids / out_d: njobs x k_out, final (padded with -1 / NaN); out_flag: 1 = not run to
// completion (candidate heap beyond LDS + spill), caller re-runs that job on the lock-step path.
bool Device::search_batch(const SearchJob *jobs, int njobs, int k, int k_out, int *out_ids, float *out_d, int *out_flag, bool keep_repeat_flag,
                          bool two_heap)
{
    if (njobs <= 0) return true;
    if (!jobs) { set_dev_error("search_batch: bad argument"); return false; }
    return search_batch_impl(jobs, njobs, k, k_out, out_ids, out_d, out_flag, keep_repeat_flag, two_heap, -1, -1);
}

bool Device::search_queries(int nq, int entry, int entry_layer, int k, int k_out, int *out_ids, float *out_d, int *out_flag)
{
    if (nq <= 0) return true;
    if (nq > (1 << 20)) { // more than one launch: the plain path
        std::vector<SearchJob> jobs((size_t)nq);
        for (int i = 0; i < nq; ++i) jobs[(size_t)i] = SearchJob{i, entry, entry_layer, 0, -1, 0};
        return search_batch(jobs.data(), nq, k, k_out, out_ids, out_d, out_flag);
    }
    return search_batch_impl(nullptr, nq, k, k_out, out_ids, out_d, out_flag, false, false, entry, entry_layer);
}

// jobs == nullptr: search_queries' jobs {i, u_entry, u_layer, 0, -1, 0}, i < njobs <= 2^20
bool Device::search_batch_impl(const SearchJob *jobs, int njobs, int k, int k_out, int *out_ids, float *out_d, int *out_flag, bool keep_repeat_flag,
                               bool two_heap, int u_entry, int u_layer)
{
    if (!out_ids || !out_d || !out_flag || k < 1 || k_out < 1) { set_dev_error("search_batch: bad argument"); return false; }
    if (g_n_ <= 0) { set_dev_error("search_batch: no graph uploaded"); return false; }
    if (jobs ? !jobs_valid(jobs, njobs, g_n_, n_queries_, n_rows_hw_) : !(u_entry >= 0 && u_entry < g_n_ && u_layer >= 0 && njobs <= n_queries_)) {
        set_dev_error("search_batch: job outside the uploaded graph / rows / queries");
        return false;
    }
    const int cand_cap = cand_lds_cap(k, pitch_, false, nbcap());
    const size_t lds = search_lds_bytes(k, cand_cap, pitch_, false, nbcap());
    if (lds > 64 * 1024) { set_dev_error("search_batch: beam width / dimension exceed the LDS budget"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const long long chunk = std::min<long long>(njobs, 1 << 20);
    TraversalLaunch tl;
    if (!plan_traversal(false, k, two_heap, lds, &tl)) return false;
    if (!ensure_search_scratch(chunk, max_slots(), k_out, tl.vis.bytes_per_job)) return false;
    // pinned layout: [evals (16 B) | jobs | ids | dists | flags]
    const size_t b_jobs = sizeof(SearchJob) * (size_t)chunk, b_res = 4u * (size_t)chunk * k_out;
    const size_t off_pf = (16 + b_jobs + 2 * b_res + 4u * (size_t)chunk + 7) & ~(size_t)7; // the row prefilter's two counters land behind the flags
    char *hs = static_cast<char *>(pinned_stage(off_pf + 16));
    if (!hs) return false;
    unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs), *h_pf = reinterpret_cast<unsigned long long *>(hs + off_pf);
    SearchJob *h_jobs = reinterpret_cast<SearchJob *>(hs + 16);
    int *h_ids = reinterpret_cast<int *>(hs + 16 + b_jobs);
    float *h_d = reinterpret_cast<float *>(hs + 16 + b_jobs + b_res);
    int *h_flag = reinterpret_cast<int *>(hs + 16 + b_jobs + 2 * b_res);
    int *d_ids = reinterpret_cast<int *>(s_hits_.get());
    float *d_d = reinterpret_cast<float *>(s_hits_.get()) + (size_t)chunk * k_out;
    // A call answered by ONE launch of modest size is mostly API calls around a latency-bound kernel (a single query: 0.37 ms
    // of kernel in a 0.45-ms call, eleven HIP calls): ids, distances and flags then sit in one device slab and come back in
    // one copy into the pinned staging (laid out alike), the evaluation counter lives in the job counter's spare words and
    // is zeroed with it -- five HIP calls.  (A large call keeps the separate copies: its ids are handed to the caller while
    // the distances are still crossing the link.)
    const bool compact = !row_collapse_ && njobs == chunk && 2 * b_res + 4u * (size_t)chunk <= (size_t)1 << 20;
    const size_t w_out = row_collapse_ ? (size_t)row_collapse_->k : (size_t)k_out; // entries per row that leave the device
    int *d_flag = compact ? reinterpret_cast<int *>(d_d + (size_t)chunk * k_out) : s_flag_;
    unsigned long long *d_ev = compact ? reinterpret_cast<unsigned long long *>(s_jobctr_.get() + 2) : s_evals_;
    // a query set whose tail is still on the host (set_queries_streamed): the launch is gated on the rows' arrival
    const int *gate = tail_.n > 0 ? d_ready_ : nullptr;
    // whatever happens below, nothing stays pending -- and a tail that never went up (an error between the launch and
    // upload_tail) leaves no resident query set behind: hnsw_mi355x_knn_query_resident must not answer from rows that
    // were never uploaded
    struct TailGuard { Device *d; ~TailGuard() { if (d->tail_.n > 0) d->n_queries_ = 0; d->tail_.n = 0; } } tail_guard{this};
    for (long long off = 0; off < njobs; off += chunk) {
        const int nj = (int)std::min<long long>(chunk, njobs - off);
        if (jobs) {
            memcpy(h_jobs, jobs + off, sizeof(SearchJob) * (size_t)nj);
            HIP_OK(hipMemcpyAsync(s_jobs_, h_jobs, sizeof(SearchJob) * (size_t)nj, hipMemcpyHostToDevice, st));
            uj_len_ = 0;
        } else if (!(uj_len_ >= nj && uj_entry_ == u_entry && uj_layer_ == u_layer)) {
            for (int i = 0; i < nj; ++i) h_jobs[i] = SearchJob{i, u_entry, u_layer, 0, -1, 0};
            HIP_OK(hipMemcpyAsync(s_jobs_, h_jobs, sizeof(SearchJob) * (size_t)nj, hipMemcpyHostToDevice, st));
            uj_len_ = nj; uj_entry_ = u_entry; uj_layer_ = u_layer;
        }
        // a launch that would take the lean form takes its row-prefilter variant where the index has current shadow rows (the
        // first such launch allocates and packs them, a launch after an Add packs what is new)
        auto kernel = place_traversal<false>(tl, nj);
        if (tl.form == kFormLean) {
            const int shadow = row_prefilter_ready(); // 1: the f16 shadow, 2: the 8-bit one
            if (shadow != 0) {
                tl.prefilter = true;
                tl.pf8 = shadow == 2;
                kernel = place_traversal<false>(tl, nj);
            }
        }
        const bool prefiltered = form_is_pf(tl.form), pf8 = form_is_pf8(tl.form);
        unsigned long long *const pf_words = !prefiltered ? nullptr : pf8 ? pf_->c8.words.get() : pf_->words.get();
        HIP_OK(hipMemsetAsync(s_jobctr_, 0, sizeof(int) * (4 + (size_t)nj), st));
        if (!compact) HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
        const bool timed = profiling_;
        if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
        hipLaunchKernelGGL(kernel, dim3(tl.grid), dim3(tl.block), tl.lds_total, st, d_rows_, d_row_sn_, d_queries_, d_q_sn_, pitch_, g_adj0_, g_stride0_,
                           g_upper_, g_pool_, g_strideU_, s_jobs_, k, cand_cap, reinterpret_cast<ND *>(s_spill_.get()), spill_cap_for_tests(), s_visited_,
                           tl.vis.words, tl.vis.tab, tl.vis.tab_cap, k_out, d_ids, d_d, s_cnt_, d_flag, d_ev, nbcap(), nj, s_jobctr_,
                           tl.flags | (shadow_mode() && shadows_allowed_ ? 0x100 : 0), gate,
                           !prefiltered ? (const float *)nullptr : pf8 ? reinterpret_cast<const float *>(pf_->c8.bytes.get()) : pf_->rows.get(), pf_words);
        if (tl.form == kFormLat) stats_.lat_launches++;
        if (form_is_lean(tl.form)) stats_.lean_launches++;
        HIP_OK(hipGetLastError());
        if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
        if (prefiltered) HIP_OK(hipMemcpyAsync(h_pf, pf_words + 1, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        if (tail_.n > 0 && !upload_tail()) return false; // the rest of the query set, while the launch above is running
        if (compact) { // [ids | distances | flags] in one piece (nj == chunk: the device slab and the staging are laid out alike)
            HIP_OK(hipMemcpyAsync(h_ids, d_ids, 2 * b_res + sizeof(int) * (size_t)nj, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(h_ev, d_ev, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            memcpy(out_ids + (size_t)off * k_out, h_ids, 4u * (size_t)nj * k_out);
        } else if (row_collapse_) { // search_collapsed: the rows are collapsed where they are, and k columns of them come back
            if (!collapse_and_fetch(d_ids, d_d, nj, (size_t)k_out, h_ids, h_d)) return false;
            HIP_OK(hipMemcpyAsync(h_flag, s_flag_, sizeof(int) * (size_t)nj, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            memcpy(out_ids + (size_t)off * w_out, h_ids, 4u * (size_t)nj * w_out);
        } else {
        // the ids are copied out to the caller's array while the distances are still crossing the link
        HIP_OK(hipMemcpyAsync(h_ids, d_ids, 4u * (size_t)nj * k_out, hipMemcpyDeviceToHost, st));
        HIP_OK(hipEventRecord(E(ev2_), st));
        HIP_OK(hipMemcpyAsync(h_d, d_d, 4u * (size_t)nj * k_out, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_flag, s_flag_, sizeof(int) * (size_t)nj, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_OK(hipEventSynchronize(E(ev2_)));
        memcpy(out_ids + (size_t)off * k_out, h_ids, 4u * (size_t)nj * k_out);
        HIP_OK(hipStreamSynchronize(st));
        }
        memcpy(out_d + (size_t)off * w_out, h_d, 4u * (size_t)nj * w_out);
        for (int i = 0; i < nj; ++i) {
            if (h_flag[i] == 2) { stats_.search_repeats++; if (!keep_repeat_flag) h_flag[i] = 0; }
            else if (h_flag[i] == 4) { stats_.tie_windows++; h_flag[i] = 0; } // informational: a group window closed cleanly
        }
        memcpy(out_flag + off, h_flag, sizeof(int) * (size_t)nj);
        if (pf8) { // 128 + p * 512 B against the f16 shadow's 256 B breaks even at p = 1/4: from there the f16 prefilter, and a fresh grid next time
            std::lock_guard<std::mutex> lk(pf_->mu);
            RowPrefilter::Codes &C = pf_->c8;
            const uint64_t d_shadow = h_pf[0] > C.on_shadow ? h_pf[0] - C.on_shadow : 0, d_reread = h_pf[1] > C.reread ? h_pf[1] - C.reread : 0;
            C.launches++;
            C.on_shadow += d_shadow;
            C.reread += d_reread;
            if (4 * d_reread > d_shadow && row_prefilter_mode() == 1 && !C.lost) { C.lost = true; C.packed = 0; C.fallbacks++; }
        } else
        if (prefiltered) { // the device words are cumulative; a launch that re-read more than half of its rows cost more than it saved
            std::lock_guard<std::mutex> lk(pf_->mu);
            const uint64_t d_shadow = h_pf[0] > pf_->on_shadow ? h_pf[0] - pf_->on_shadow : 0, d_reread = h_pf[1] > pf_->reread ? h_pf[1] - pf_->reread : 0;
            pf_->launches++;
            pf_->form_launches[tl.form == kFormLeanPFFixed]++;
            pf_->on_shadow += d_shadow;
            pf_->reread += d_reread;
            if (2 * d_reread > d_shadow && row_prefilter_mode() != 2) pf_->lost = true;
        }
        tl.prefilter = tl.pf8 = false; // (decided per launch)
        if (!count_launch(nullptr, *h_ev, tl.vis.tab != nullptr, timed, ev0_, ev1_)) return false;
    }
    for (int i = 0; i < njobs; ++i) stats_.search_overflows += (uint64_t)(out_flag[i] == 1);
    return true;
}

// search_collapsed's part of a launch's copy-out (row_collapse_ is set): the nj rows of `width` entries at d_ids / d_d are collapsed
// in place by collapse_rows_kernel and their first k columns enqueued to h_ids / h_d as rows of k.
bool Device::collapse_and_fetch(int *d_ids, float *d_d, int nj, size_t width, int *h_ids, float *h_d)
{
    hipStream_t st = S(stream_);
    const RowCollapse &rc = *row_collapse_;
    const size_t lds = 12 * width + 4 * (size_t)rc.k, w = (size_t)rc.k;
    if (lds > 64 * 1024) { set_dev_error("search_collapsed: the beam exceeds the LDS budget of the collapse"); return false; }
    hipLaunchKernelGGL(collapse_rows_kernel, dim3((unsigned)nj), dim3(64), lds, st, d_ids, d_d, (int)width, rc.k, rc.d_labels, rc.n_labels, rc.per_group);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy2DAsync(h_ids, 4 * w, d_ids, 4 * width, 4 * w, (size_t)nj, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpy2DAsync(h_d, 4 * w, d_d, 4 * width, 4 * w, (size_t)nj, hipMemcpyDeviceToHost, st));
    return true;
}

// ---- the resident-query kernels (graph_search_filtered_kernel, graph_multilayer_kernel): job i is resident query i, all from one
// entry point.  One call over nq of them, in launches of up to `chunk` jobs with result rows of `row` entries: the pinned staging
// [evals (16 B) | ids | dists | flags | `extra` bytes], upload(those bytes) once before the first launch (what the caller sends up
// from pinned memory), then per launch the counters zeroed, launch(off, nj, d_ids, d_d) -- the kernel for queries off .. off + nj,
// flags to s_flag_, evaluations to s_evals_, jobs from s_jobctr_ -- and rows and flags copied to the caller's arrays.  The callers
// keep their own checks, scratch and counters.  (search_batch_impl is not built on this: job upload, the compact copy, the gated tail.)
template <class Upload, class Launch>
bool Device::run_resident(size_t row, long long chunk, size_t extra, bool hashed, int nq, int *out_ids, float *out_d, int *out_flag, Upload &&upload,
                          Launch &&launch)
{
    hipStream_t st = S(stream_);
    const size_t b_res = 4u * (size_t)chunk * row;
    char *hs = static_cast<char *>(pinned_stage(16 + 2 * b_res + 4u * (size_t)chunk + extra));
    if (!hs) return false;
    unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs);
    int *h_ids = reinterpret_cast<int *>(hs + 16);
    float *h_d = reinterpret_cast<float *>(hs + 16 + b_res);
    int *h_flag = reinterpret_cast<int *>(hs + 16 + 2 * b_res);
    if (!upload(hs + 16 + 2 * b_res + 4u * (size_t)chunk)) return false;
    int *d_ids = reinterpret_cast<int *>(s_hits_.get());
    float *d_d = reinterpret_cast<float *>(s_hits_.get()) + (size_t)chunk * row;
    for (long long off = 0; off < nq; off += chunk) {
        const int nj = (int)std::min<long long>(chunk, nq - off);
        HIP_OK(hipMemsetAsync(s_jobctr_, 0, sizeof(int) * 4, st));
        HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
        const bool timed = profiling_;
        if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
        launch(off, nj, d_ids, d_d);
        HIP_OK(hipGetLastError());
        if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
        const size_t w = row_collapse_ ? (size_t)row_collapse_->k : row; // entries per row that leave the device
        if (row_collapse_) { if (!collapse_and_fetch(d_ids, d_d, nj, row, h_ids, h_d)) return false; }
        else {
            HIP_OK(hipMemcpyAsync(h_ids, d_ids, 4u * (size_t)nj * row, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(h_d, d_d, 4u * (size_t)nj * row, hipMemcpyDeviceToHost, st));
        }
        HIP_OK(hipMemcpyAsync(h_flag, s_flag_, sizeof(int) * (size_t)nj, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        memcpy(out_ids + (size_t)off * w, h_ids, 4u * (size_t)nj * w);
        memcpy(out_d + (size_t)off * w, h_d, 4u * (size_t)nj * w);
        memcpy(out_flag + off, h_flag, sizeof(int) * (size_t)nj);
        if (!count_launch(nullptr, *h_ev, hashed, timed, ev0_, ev1_)) return false;
    }
    return true;
}

// ---- KnnQuery with a predicate over ids (search_filtered, search_grouped, search_tagged; predicate_search in dk_search_kernels.h):
// what the three calls share.  Each keeps its own argument rules, its upload layout and its counters.
struct PredicateCall {
    std::string who; // the caller's name, the prefix of every message
    int nq, entry, entry_layer, search_layer, k, k_out;
    int *out_ids;
    float *out_d;
    int *out_flag;
};
// What a launch needs beyond the call's own arguments (plan_predicate_search); ok: everything below it is set.
template <class K>
struct PredicatePlan {
    bool ok;
    K kernel;
    TraversalLaunch tl;
    int cand_cap, fspill;
    long long chunk; // queries per launch
};

// The entry checks, in the order of their messages: the outputs and beams, the caller's own argument rules (own_rules(): the message
// of the first one broken, empty when none is), the graph, the search layer, the entry point and the resident queries.
template <class OwnRules>
bool Device::predicate_call_ok(const PredicateCall &c, OwnRules &&own_rules)
{
    const std::string &who = c.who;
    if (!c.out_ids || !c.out_d || !c.out_flag || c.k < 1 || c.k_out < 1) { set_dev_error(who + ": bad argument"); return false; }
    if (const std::string why = own_rules(); !why.empty()) { set_dev_error(why); return false; }
    if (g_n_ <= 0) { set_dev_error(who + ": no graph uploaded"); return false; }
    if (c.search_layer < 0 || c.search_layer > c.entry_layer) { set_dev_error(who + ": the search layer must lie between 0 and the entry point's top layer"); return false; }
    if (!(c.entry >= 0 && c.entry < g_n_ && c.entry_layer >= 0 && c.nq <= n_queries_) || tail_.n > 0) {
        set_dev_error(who + ": entry point outside the graph, or fewer resident queries than asked for");
        return false;
    }
    return true;
}

// The planning step: the candidate heap and its LDS, the traversal plan, the kernel of (metric, hashed) named by `of` (as
// persistent_kernel takes it) placed on the device, the spill areas, and the scratch grown for launches of `chunk` queries.
template <class Of>
auto Device::plan_predicate_search(const PredicateCall &c, Of of)
{
    PredicatePlan<decltype(persistent_kernel(0, false, of))> p{};
    const std::string &who = c.who;
    p.chunk = std::min<long long>(c.nq, 1 << 20);
    p.cand_cap = cand_lds_cap(c.k, pitch_, false, nbcap());
    const size_t lds = search_lds_bytes(c.k, p.cand_cap, pitch_, false, nbcap());
    if (lds > 64 * 1024) { set_dev_error(who + ": beam width / dimension exceed the LDS budget"); return p; }
    if (!bind() || !plan_traversal(false, c.k, true, lds, &p.tl, true)) return p;
    p.kernel = persistent_kernel(metric_, p.tl.vis.tab != nullptr, of);
    place_persistent(p.kernel, p.tl, (int)p.chunk);
    if (p.tl.slots < 1) { set_dev_error(who + ": the kernel does not fit the device"); return p; }
    p.fspill = filter_spill_cap();
    if (!ensure_search_scratch(p.chunk, max_slots(), c.k_out, p.tl.vis.bytes_per_job)) return p;
    p.ok = s_fspill_.grow((size_t)p.tl.slots * (size_t)std::max(p.fspill, 1) + 8); // +8: get2 may read one entry past a heap
    return p;
}

// The launches (run_resident): `extra` pinned bytes for upload(h); the launch for the queries from `off` has jobs_of(off, nj) jobs
// (0: one wave finds the counter past the jobs and leaves) and, between the arguments that every predicate kernel begins and
// ends with, the tuple predicate(off).
template <class K, class Upload, class JobsOf, class Predicate>
bool Device::run_predicate_search(const PredicateCall &c, const PredicatePlan<K> &p, size_t extra, Upload &&upload, JobsOf &&jobs_of, Predicate &&predicate)
{
    hipStream_t st = S(stream_);
    const TraversalLaunch &tl = p.tl;
    const auto launch = [&](long long off, int nj, int *d_ids, float *d_d) {
        const int n = jobs_of(off, nj);
        std::apply([&](auto... filter) {
            hipLaunchKernelGGL(p.kernel, dim3(std::max(1, std::min(n, tl.slots))), dim3(tl.block), tl.lds_total, st, d_rows_, d_row_sn_,
                               d_queries_ + (size_t)off * pitch_, d_q_sn_ ? d_q_sn_ + off : nullptr, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_,
                               c.entry, c.entry_layer, c.search_layer, c.k, p.cand_cap, reinterpret_cast<ND *>(s_fspill_.get()), p.fspill, s_visited_,
                               tl.vis.words, tl.vis.tab, tl.vis.tab_cap, filter..., c.k_out, d_ids, d_d, s_flag_, s_evals_, nbcap(), n, s_jobctr_);
        }, predicate(off));
    };
    return run_resident((size_t)c.k_out, p.chunk, extra, tl.vis.tab != nullptr, c.nq, c.out_ids, c.out_d, c.out_flag, upload, launch);
}

// The queries handed back (out_flag 1), counted once every row has its flag.
uint64_t Device::count_search_overflows(const PredicateCall &c)
{
    uint64_t n = 0;
    for (int i = 0; i < c.nq; ++i) n += (uint64_t)(c.out_flag[i] == 1);
    stats_.search_overflows += n;
    return n;
}

// The skip-and-order step of the calls with a predicate per query.  members(i): the graph ids that pass query i's predicate.  A
// query with none is padded without a job; the others are listed per launch (chunk) in its order table -- the chunk's own query
// indices -- longest traversal first: a traversal's length grows with 1 / selectivity and a persistent launch ends
// with its longest job, so ascending by members, queries of equal counts in query order.
struct LaunchOrder {
    std::vector<int> order, jobs_of; // the tables, launch after launch ([nq]); the jobs of every launch
    long long launched = 0;
};
template <class Members>
static LaunchOrder order_by_members(int nq, long long chunk, Members &&members)
{
    LaunchOrder lo;
    lo.order.resize((size_t)nq);
    for (long long off = 0; off < nq; off += chunk) {
        const int nj = (int)std::min<long long>(chunk, nq - off);
        int *o = lo.order.data() + off;
        int n = 0;
        for (int i = 0; i < nj; ++i)
            if (members(off + i) > 0) o[n++] = i;
        std::stable_sort(o, o + n, [&](int a, int b) { return members(off + a) < members(off + b); });
        for (int i = n; i < nj; ++i) o[i] = 0; // (never read: the launch has n jobs)
        lo.jobs_of.push_back(n);
        lo.launched += n;
    }
    return lo;
}
// ... and the rows no job writes: padding, flag 0 (after the launches' rows have been copied over the caller's arrays)
template <class Members>
static void pad_skipped(const PredicateCall &c, Members &&members)
{
    for (int i = 0; i < c.nq; ++i)
        if (members(i) == 0) {
            pad_results(c.out_ids + (size_t)i * c.k_out, c.out_d + (size_t)i * c.k_out, (size_t)c.k_out);
            c.out_flag[i] = 0;
        }
}

// KnnQuery with an allow-set (graph_search_filtered_kernel): resident query i from (entry, entry_layer), i < nq.  Only the words that
// cover graph ids travel: bits of ids >= min(nbits, graph nodes) are never read.  A set that allows no graph id pads every
// row without a launch (the result is empty whatever the order).
bool Device::search_filtered(int nq, int entry, int entry_layer, int k, int k_out, const uint32_t *allow_bits, long long nbits, int *out_ids,
                             float *out_d, int *out_flag, int search_layer)
{
    if (nq <= 0) return true;
    const PredicateCall c{"search_filtered", nq, entry, entry_layer, search_layer, k, k_out, out_ids, out_d, out_flag};
    const auto own_rules = [&] { return std::string(nbits < 0 || (!allow_bits && nbits > 0) ? "search_filtered: bad argument" : ""); };
    if (!predicate_call_ok(c, own_rules)) return false;
    if (!allows_any(allow_bits, nbits, g_n_)) {
        pad_results(out_ids, out_d, (size_t)nq * (size_t)k_out);
        for (int i = 0; i < nq; ++i) out_flag[i] = 0;
        return true;
    }
    const long long n_allow = std::min<long long>(nbits, g_n_);
    const size_t words = (size_t)((n_allow + 31) / 32);
    const auto p = plan_predicate_search(c, [](auto m, auto h) { return &graph_search_filtered_kernel<m, h>; });
    if (!p.ok || !s_allow_.grow(std::max<size_t>(words, 1))) return false;
    hipStream_t st = S(stream_);
    const auto upload = [&](char *h_allow) { // the allow words go up from pinned memory
        memcpy(h_allow, allow_bits, 4u * words);
        HIP_OK(hipMemcpyAsync(s_allow_, h_allow, 4u * words, hipMemcpyHostToDevice, st));
        return true;
    };
    const auto every_query = [](long long, int nj) { return nj; };
    const auto filter = [&](long long) { return std::make_tuple(reinterpret_cast<const unsigned *>(s_allow_.get()), n_allow); };
    if (!run_predicate_search(c, p, 4u * words, upload, every_query, filter)) return false;
    count_search_overflows(c);
    return true;
}

// The argument rules the grouped calls share (group_args_error, device_backend.h), filed as the context's error.
static bool group_args_ok(const char *who, const int *query_group, int nq, int n_groups)
{
    const std::string why = group_args_error(who, query_group, nq, n_groups);
    if (!why.empty()) set_dev_error(why);
    return why.empty();
}

// KnnQuery with a group filter per query (graph_search_grouped_kernel): the labels in the allow words' place.  Only
// the labels of graph ids travel.  The graph ids of every group are counted here, on the host, for order_by_members.
bool Device::search_grouped(int nq, int entry, int entry_layer, int k, int k_out, const int *row_group, long long n_row_group, const int *query_group,
                            int n_groups, int *out_ids, float *out_d, int *out_flag, int search_layer)
{
    if (nq <= 0) return true;
    const PredicateCall c{"search_grouped", nq, entry, entry_layer, search_layer, k, k_out, out_ids, out_d, out_flag};
    const auto own_rules = [&]() -> std::string {
        if (!row_group || n_row_group < 0) return "search_grouped: row_group must not be NULL and n_row_group must be >= 0";
        if (!query_group) return "search_grouped: query_group must not be NULL";
        return group_args_error("search_grouped", query_group, nq, n_groups);
    };
    if (!predicate_call_ok(c, own_rules)) return false;
    const long long n_lab = std::min<long long>(n_row_group, g_n_);
    std::vector<long long> group_ids((size_t)n_groups, 0);
    for (long long id = 0; id < n_lab; ++id) {
        const int g = row_group[id];
        if (g >= 0 && g < n_groups) group_ids[(size_t)g] += 1;
    }
    const auto members = [&](long long i) { return group_ids[(size_t)query_group[i]]; };
    const LaunchOrder lo = order_by_members(nq, std::min<long long>(nq, 1 << 20), members);
    if (lo.launched > 0) { // (else nothing to traverse: no launch, as a set that allows nothing)
        const auto p = plan_predicate_search(c, [](auto m, auto h) { return &graph_search_grouped_kernel<m, h>; });
        if (!p.ok || !s_glabel_.grow((size_t)n_lab) || !s_gquery_.grow(2 * (size_t)nq)) return false;
        hipStream_t st = S(stream_);
        const size_t b_lab = 4u * (size_t)n_lab, b_q = 4u * (size_t)nq;
        const auto upload = [&](char *h) { // labels, groups and order tables go up from pinned memory: [row_group | query_group | order]
            memcpy(h, row_group, b_lab);
            memcpy(h + b_lab, query_group, b_q);
            memcpy(h + b_lab + b_q, lo.order.data(), b_q);
            HIP_OK(hipMemcpyAsync(s_glabel_, h, b_lab, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(s_gquery_, h + b_lab, 2 * b_q, hipMemcpyHostToDevice, st));
            return true;
        };
        const auto listed = [&](long long off, int) { return lo.jobs_of[(size_t)(off / p.chunk)]; };
        const auto filter = [&](long long off) { return std::make_tuple(s_glabel_.get(), n_lab, s_gquery_.get() + off, s_gquery_.get() + (size_t)nq + off); };
        if (!run_predicate_search(c, p, b_lab + 2 * b_q, upload, listed, filter)) return false;
    }
    pad_skipped(c, members); // (every row when nothing was launched: no flag is set then)
    using Slot = slot::knn_grouped_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::calls] += 1;
    ctr[Slot::launched] += (uint64_t)lo.launched;
    ctr[Slot::skipped] += (uint64_t)(nq - lo.launched);
    ctr[Slot::handbacks] += count_search_overflows(c);
    return true;
}

// The tagged calls' argument rules (tag_args_error, device_backend.h), filed as the context's error.
static bool tag_args_ok(const char *who, const uint32_t *query_tags, int nq, int match, TagCall *tc)
{
    const std::string why = tag_args_error(who, query_tags, nq, match, tc);
    if (!why.empty()) set_dev_error(why);
    return why.empty();
}

// What both tagged calls begin with (dk_tag_lists.h): row_tags[0, n) (n >= 1) and the call's distinct masks go up
// to buffers of their own, tag_count_kernel counts every mask's candidates, and the counts come back in one copy -- cnt[d]: the ids
// below n whose word matches masks[d].  The words and the masks stay on the device for the call (s_ttags_, s_tmask_; s_tcnt_ holds
// [counts | offsets | cursors]).  The stream is idle and the pinned stage free when this returns.
bool Device::tag_counts(const unsigned *row_tags, long long n, const std::vector<uint32_t> &masks, int match, std::vector<int> &cnt)
{
    hipStream_t st = S(stream_);
    const size_t D = masks.size(), b_tags = 4 * (size_t)n, b_masks = 4 * D;
    if (!s_ttags_.grow((size_t)n) || !s_tmask_.grow(D) || !s_tcnt_.grow(3 * D)) return false;
    cnt.assign(D, 0);
    const size_t staged = b_tags < (4u << 20) ? b_tags : 0; // larger arrays go up in pieces, as query sets do
    char *hs = static_cast<char *>(pinned_stage(staged + 2 * b_masks));
    if (!hs) return false;
    if (staged) { memcpy(hs, row_tags, b_tags); HIP_OK(hipMemcpyAsync(s_ttags_, hs, b_tags, hipMemcpyHostToDevice, st)); }
    else if (!staged_upload(reinterpret_cast<float *>(s_ttags_.get()), reinterpret_cast<const float *>(row_tags), b_tags)) return false;
    memcpy(hs + staged, masks.data(), b_masks);
    HIP_OK(hipMemcpyAsync(s_tmask_, hs + staged, b_masks, hipMemcpyHostToDevice, st));
    const bool timed = profiling_; // the list-building kernels have an event pair of their own (tag_list_ms)
    if (timed && (!ev0_.create(true) || !ev1_.create(true))) return false;
    if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
    HIP_OK(tag_counts_launch(s_ttags_, n, s_tmask_, (int)D, match, s_tcnt_, st));
    if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
    HIP_OK(hipMemcpyAsync(hs + staged + b_masks, s_tcnt_, b_masks, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (timed) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, E(ev0_), E(ev1_)));
        xt_list_ms_ += ms;
    }
    memcpy(cnt.data(), hs + staged + b_masks, b_masks); // (the stage is used again by the caller)
    for (size_t d = 0; d < D; ++d)
        if (cnt[d] < 0 || cnt[d] > n) { set_dev_error("tag_counts: a mask's count is outside 0 .. the ids"); return false; }
    return true;
}

bool Device::tag_candidates(const uint32_t *row_tags, long long n, const std::vector<uint32_t> &masks, int match, std::vector<int> &cnt)
{
    cnt.assign(masks.size(), 0);
    if (n <= 0 || masks.empty()) return true;
    return bind() && tag_counts(row_tags, n, masks, match, cnt);
}

// KnnQuery with a tag mask per query (graph_search_tagged_kernel): the tag words in the labels' place.  Only the
// words of graph ids travel.  The candidates of every distinct mask are counted on the device (tag_counts) for order_by_members.
bool Device::search_tagged(int nq, int entry, int entry_layer, int k, int k_out, const uint32_t *row_tags, long long n_row_tags, const uint32_t *query_tags,
                           int match, int *out_ids, float *out_d, int *out_flag, int search_layer)
{
    if (nq <= 0) return true;
    const PredicateCall c{"search_tagged", nq, entry, entry_layer, search_layer, k, k_out, out_ids, out_d, out_flag};
    TagCall tc;
    const auto own_rules = [&]() -> std::string {
        if (!row_tags || n_row_tags < 0) return "search_tagged: row_tags must not be NULL and n_row_tags must be >= 0";
        if (!query_tags) return "search_tagged: query_tags must not be NULL";
        return tag_args_error("search_tagged", query_tags, nq, match, &tc);
    };
    if (!predicate_call_ok(c, own_rules)) return false;
    const long long n_lab = std::min<long long>(n_row_tags, g_n_);
    std::vector<int> cnt(tc.masks.size(), 0);
    if (n_lab > 0 && (!bind() || !tag_counts(row_tags, n_lab, tc.masks, match, cnt))) return false; // (no word of a graph id: no candidate, nothing goes up)
    const auto members = [&](long long i) { return cnt[(size_t)tc.of[(size_t)i]]; };
    const LaunchOrder lo = order_by_members(nq, std::min<long long>(nq, 1 << 20), members);
    if (lo.launched > 0) { // (else nothing to traverse: no launch, as a set that allows nothing)
        const auto p = plan_predicate_search(c, [](auto m, auto h) { return &graph_search_tagged_kernel<m, h>; });
        if (!p.ok || !s_tquery_.grow(2 * (size_t)nq)) return false;
        hipStream_t st = S(stream_);
        const size_t b_q = 4u * (size_t)nq;
        const auto upload = [&](char *h) { // masks and order tables go up from pinned memory, behind the words tag_counts sent: [query_tags | order]
            memcpy(h, query_tags, b_q);
            memcpy(h + b_q, lo.order.data(), b_q);
            HIP_OK(hipMemcpyAsync(s_tquery_, h, 2 * b_q, hipMemcpyHostToDevice, st));
            return true;
        };
        const auto listed = [&](long long off, int) { return lo.jobs_of[(size_t)(off / p.chunk)]; };
        const auto filter = [&](long long off) {
            return std::make_tuple(s_ttags_.get(), n_lab, reinterpret_cast<const unsigned *>(s_tquery_.get()) + off, match, s_tquery_.get() + (size_t)nq + off);
        };
        if (!run_predicate_search(c, p, 2 * b_q, upload, listed, filter)) return false;
    }
    pad_skipped(c, members); // (every row when nothing was launched: no flag is set then)
    using Slot = slot::knn_tagged_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::calls] += 1;
    ctr[Slot::masks] += (uint64_t)tc.masks.size();
    ctr[Slot::launched] += (uint64_t)lo.launched;
    ctr[Slot::skipped] += (uint64_t)(nq - lo.launched);
    ctr[Slot::handbacks] += count_search_overflows(c);
    return true;
}

// MultiLayerKnnQuery's chains (graph_multilayer_kernel): resident query i from (entry, entry_layer), searched on every layer from
// first_layer down to min_layer with beam k, each step entering at the one before's nearest result.  out_ids / out_d:
// [nq][first_layer + 1][k - 1], slots below min_layer padded; out_flag[i] = 1: the job is handed back (the caller redoes it).
bool Device::multilayer_search(int nq, int entry, int entry_layer, int first_layer, int min_layer, int k, int *out_ids, float *out_d, int *out_flag)
{
    if (nq <= 0) return true;
    if (!out_ids || !out_d || !out_flag || k < 2) { set_dev_error("multilayer_search: bad argument"); return false; }
    if (g_n_ <= 0) { set_dev_error("multilayer_search: no graph uploaded"); return false; }
    if (!(entry >= 0 && entry < g_n_ && nq <= n_queries_) || tail_.n > 0) {
        set_dev_error("multilayer_search: entry point outside the graph, or fewer resident queries than asked for");
        return false;
    }
    if (!(min_layer >= 0 && min_layer <= first_layer && first_layer <= entry_layer && entry_layer < 0x4000)) {
        set_dev_error("multilayer_search: layers must satisfy 0 <= min_layer <= first_layer <= the entry point's top layer");
        return false;
    }
    const size_t row = (size_t)(first_layer + 1) * (size_t)(k - 1); // results of one job
    const int cand_cap = cand_lds_cap(k, pitch_, false, nbcap());
    const size_t lds = search_lds_bytes(k, cand_cap, pitch_, false, nbcap());
    if (lds > 64 * 1024) { set_dev_error("multilayer_search: beam width / dimension exceed the LDS budget"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const long long chunk = std::max<long long>(1, std::min<long long>(nq, (long long)((size_t)(1 << 24) / row)));
    TraversalLaunch tl;
    if (!plan_traversal(false, k, true, lds, &tl)) return false;
    const auto kernel = persistent_kernel(metric_, tl.vis.tab != nullptr, [](auto m, auto h) { return &graph_multilayer_kernel<m, h>; });
    place_persistent(kernel, tl, (int)chunk);
    if (tl.slots < 1) { set_dev_error("multilayer_search: the kernel does not fit the device"); return false; }
    if (!ensure_search_scratch(chunk, max_slots(), (int)row, tl.vis.bytes_per_job)) return false;
    const int spill_cap = spill_cap_for_tests();
    const auto launch = [&](long long off, int nj, int *d_ids, float *d_d) {
        hipLaunchKernelGGL(kernel, dim3(std::min(nj, tl.slots)), dim3(tl.block), tl.lds_total, st, d_rows_, d_row_sn_, d_queries_ + (size_t)off * pitch_,
                           d_q_sn_ ? d_q_sn_ + off : nullptr, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, entry, entry_layer, first_layer,
                           min_layer, k, cand_cap, reinterpret_cast<ND *>(s_spill_.get()), spill_cap, s_visited_, tl.vis.words, tl.vis.tab, tl.vis.tab_cap, d_ids,
                           d_d, s_flag_, s_evals_, nbcap(), nj, s_jobctr_);
        stats_.multilayer_launches += 1; // counted as made, so a call that fails part-way keeps the launches before the failure
    };
    if (!run_resident(row, chunk, 0, tl.vis.tab != nullptr, nq, out_ids, out_d, out_flag, [](char *) { return true; }, launch)) return false;
    stats_.multilayer_jobs += (uint64_t)nq;
    for (int i = 0; i < nq; ++i) stats_.multilayer_handbacks += (uint64_t)(out_flag[i] != 0);
    return true;
}

bool Device::relink_batch(const int *affected, const int *layer, const int *removed, const int *step, int n, const int *cands, const int *cand_off,
                          const int *cand_cnt, int nsteps, int max_edges0, int *out_sel, int *out_cnt, int *out_flag, int sel_stride, bool heap_order)
{
    if (n <= 0) return true;
    if (!affected || !layer || !removed || !step || !cand_off || !cand_cnt || !out_sel || !out_cnt || !out_flag || nsteps < 1 || max_edges0 < 2 ||
        sel_stride < max_edges0) {
        set_dev_error("relink_batch: bad argument");
        return false;
    }
    if (g_n_ <= 0) { set_dev_error("relink_batch: no graph uploaded"); return false; }
    int total_c = 0, max_c = 0;
    for (int s = 0; s < nsteps; ++s) {
        if (cand_cnt[s] < 0 || cand_off[s] != total_c) { set_dev_error("relink_batch: candidate ranges must be packed in step order"); return false; }
        total_c += cand_cnt[s];
        max_c = std::max(max_c, cand_cnt[s]);
    }
    if (total_c > 0 && !cands) { set_dev_error("relink_batch: bad argument"); return false; }
    for (int i = 0; i < total_c; ++i)
        if (cands[i] < 0 || cands[i] >= g_n_ || cands[i] >= n_rows_hw_) { set_dev_error("relink_batch: candidate outside the graph / rows"); return false; }
    for (int i = 0; i < n; ++i)
        if (affected[i] < 0 || affected[i] >= g_n_ || affected[i] >= n_rows_hw_ || removed[i] < 0 || removed[i] >= g_n_ || layer[i] < 0 || layer[i] > 200 ||
            step[i] < 0 || step[i] >= nsteps) {
            set_dev_error("relink_batch: job outside the graph / rows");
            return false;
        }
    const int kcap = (g_stride0_ - 2) + max_c + 1, nb = (kcap + 7) & ~7;
    const size_t lds = search_lds_bytes(kcap, 0, pitch_, true, nb);
    if (lds > 64 * 1024) { set_dev_error("relink_batch: candidate count / dimension exceed the LDS budget"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (!ensure_search_scratch(1, 1, 0, 16)) return false;
    // device staging: [jobs (4 n) | cand_off | cand_cnt | cands | sel | cnt | flag]
    const size_t o_off = 4u * (size_t)n, o_cnt = o_off + (size_t)nsteps, o_c = o_cnt + (size_t)nsteps, o_s = o_c + (size_t)std::max(total_c, 1),
                 o_n = o_s + (size_t)n * sel_stride, o_f = o_n + (size_t)n, total = o_f + (size_t)n;
    if (!s_rl_.grow(total + 4)) return false; // (+4: the int4 view of the jobs starts aligned, as a device allocation does)
    int *hs = static_cast<int *>(pinned_stage(sizeof(int) * total + 16));
    if (!hs) return false;
    for (int i = 0; i < n; ++i) { hs[4 * i] = affected[i]; hs[4 * i + 1] = layer[i]; hs[4 * i + 2] = removed[i]; hs[4 * i + 3] = step[i]; }
    memcpy(hs + o_off, cand_off, sizeof(int) * (size_t)nsteps);
    memcpy(hs + o_cnt, cand_cnt, sizeof(int) * (size_t)nsteps);
    if (total_c > 0) memcpy(hs + o_c, cands, sizeof(int) * (size_t)total_c);
    HIP_OK(hipMemcpyAsync(s_rl_, hs, sizeof(int) * o_s, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
    with_metric(metric_, [&](auto m) {
        hipLaunchKernelGGL(graph_relink_kernel<m>, dim3(n), dim3(64), lds, st, d_rows_, d_row_sn_, pitch_, g_adj0_, g_stride0_, g_upper_, g_pool_,
                           g_strideU_, reinterpret_cast<const int4 *>(s_rl_.get()), s_rl_ + o_c, s_rl_ + o_off, s_rl_ + o_cnt, max_edges0, kcap, nb, s_rl_ + o_s,
                           s_rl_ + o_n, s_rl_ + o_f, sel_stride, s_evals_, heap_order ? 1 : 0);
    });
    HIP_OK(hipGetLastError());
    unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs + ((total + 1) & ~(size_t)1));
    HIP_OK(hipMemcpyAsync(hs + o_s, s_rl_ + o_s, sizeof(int) * (total - o_s), hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_ev, s_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    memcpy(out_sel, hs + o_s, sizeof(int) * (size_t)n * sel_stride);
    memcpy(out_cnt, hs + o_n, sizeof(int) * (size_t)n);
    memcpy(out_flag, hs + o_f, sizeof(int) * (size_t)n);
    stats_.search_evals += *h_ev; // (evaluations only: no launch is counted for Remove's re-link)
    return true;
}

bool Device::patch_lists(const int *recs, int nrows, int row_stride)
{
    if (nrows <= 0) return true;
    if (!recs || row_stride < 4) { set_dev_error("patch_lists: bad argument"); return false; }
    if (g_n_ <= 0) { set_dev_error("patch_lists: no graph uploaded"); return false; }
    std::vector<int> tagged(recs, recs + (size_t)nrows * row_stride);
    for (int r = 0; r < nrows; ++r) { // a bad record must be an error return, never a GPU fault
        int *x = tagged.data() + (size_t)r * row_stride;
        const int cap = (x[1] == 0 ? g_stride0_ : g_strideU_) - 2;
        bool ok = x[0] >= 0 && x[0] < g_n_ && x[1] >= 0 && x[1] < 0x4000 && x[2] >= 0 && x[2] <= row_stride - 3 && x[2] <= cap &&
                  (x[1] == 0 || (hg_ ? hg_->level[(size_t)x[0]] >= x[1] : true));
        for (int i = 0; ok && i < x[2]; ++i) ok = x[3 + i] >= 0 && x[3 + i] < g_n_;
        if (!ok) { set_dev_error("patch_lists: record outside the graph"); return false; }
        x[1] |= 1 << 30; // not a heuristic's ordered output
    }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const size_t total = (size_t)nrows * row_stride;
    if (!s_rl_.grow(total)) return false;
    int *hs = static_cast<int *>(pinned_stage(sizeof(int) * total));
    if (!hs) return false;
    memcpy(hs, tagged.data(), sizeof(int) * total);
    HIP_OK(hipMemcpyAsync(s_rl_, hs, sizeof(int) * total, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(graph_write_rows_kernel, dim3(nrows), dim3(64), 0, st, g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, s_rl_, row_stride,
                       g_tested0_, g_testedU_, g_stride0_ - 2);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(st)); // the staging buffers are reused
    return true;
}

// RangeQuery on the device (graph_range_kernel).  A launch packs its results into an arena sized from the last
// call's results per query (at least 1M entries); the jobs that did not fit run once more in an arena of exactly
// the size they asked for.  Jobs whose result set outgrew a wave's list (kSpillCap entries) run again, few at a
// time, with lists as long as the graph.
// Room for `entries` results in the pinned host buffer, the first `keep` of which survive a reallocation.
bool Device::range_host_room(size_t entries, size_t keep)
{
    if (entries <= h_range_.cap()) return true;
    PinBuf<SearchHit> p;
    if (!p.grow(entries, std::max(entries + entries / 2, (size_t)1 << 20))) return false;
    if (h_range_ && keep) memcpy(p, h_range_, sizeof(SearchHit) * keep);
    h_range_ = std::move(p);
    return true;
}

bool Device::range_batch(const SearchJob *jobs, int njobs, float range, RangeResults *res, const RangeFilter &f)
{
    const bool filtered = f.kind != RangeFilter::kNone; // (labels, tags: the bit set's ranking, replay and packing, on their predicate)
    const bool keyed = f.per_query();
    // The counter blocks of the two per-query kinds, range_tagged_info and range_grouped_info: the same quantities under each block's
    // own slot (-1: the grouped block keeps no such counter); the other kinds keep none.
    using Tagged = slot::range_tagged_info;
    using Grouped = slot::range_grouped_info;
    struct What { int tagged, grouped; };
    constexpr What kCalls{Tagged::calls, Grouped::calls}, kMasks{Tagged::masks, -1}, kLaunched{Tagged::launched, Grouped::launched},
        kSkipped{Tagged::skipped, Grouped::skipped}, kHostFinished{Tagged::host_finished, Grouped::host_finished}, kLongFinished{Tagged::long_finished, -1};
    const auto count = [&](What what, uint64_t by) {
        if (f.kind == RangeFilter::kTags) counter_block(Tagged::kBlock)[what.tagged] += by;
        else if (f.kind == RangeFilter::kLabels && what.grouped >= 0) counter_block(Grouped::kBlock)[what.grouped] += by;
    };
    if (keyed) {
        if (f.n < 0 || (f.match != 0 && f.match != 1) || (njobs > 0 && (!f.per_id || !f.keys))) { set_dev_error("range_batch: bad argument"); return false; }
        count(kCalls, 1);
        count(kMasks, (uint64_t)f.n_masks);
        count(kLaunched, (uint64_t)std::max(njobs, 0));
        count(kSkipped, (uint64_t)std::max<long long>(f.skipped, 0));
    }
    res->off.assign((size_t)std::max(njobs, 0), 0ull);
    res->cnt.assign((size_t)std::max(njobs, 0), 0);
    res->flag.assign((size_t)std::max(njobs, 0), 0);
    res->entry.assign((size_t)std::max(njobs, 0), -1);
    res->state.assign((size_t)std::max(njobs, 0), kRangeHostSort);
    res->found = nullptr;
    res->found_n = 0;
    if (njobs <= 0) return true;
    if (!jobs) { set_dev_error("range_batch: bad argument"); return false; }
    if (g_n_ <= 0) { set_dev_error("range_batch: no graph uploaded"); return false; }
    if (!jobs_valid(jobs, njobs, g_n_, n_queries_, n_rows_hw_)) { set_dev_error("range_batch: job outside the uploaded graph / rows / queries"); return false; }
    if (filtered && f.n < 0) { set_dev_error("range_batch: bad argument"); return false; }
    const int layer = jobs[0].search_layer; // RangeQuery's `layer`: one per call (the replay kernels walk that layer's lists)
    for (int i = 0; i < njobs; ++i)
        if (jobs[i].qref < 0 || jobs[i].search_layer != layer) { set_dev_error("range_batch: jobs must name a resident query and one search layer"); return false; }
    if (layer >= 0x4000) { set_dev_error("range_batch: bad argument"); return false; }
    const int nbcap_r = kRangeFan * nbcap(); // the kernel expands kRangeFan lists per step
    const size_t lds = search_lds_bytes(0, 0, pitch_, false, nbcap_r);
    if (lds > 64 * 1024) { set_dev_error("range_batch: dimension exceeds the LDS budget"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    VisitedScratch vis; // 32 768 hash slots: 24 576 visited ids before a hand-back; a step inserts up to kRangeFan lists of 128 ids
    if (!visited_scratch(512, 4 * kRangeFan * 128, true, &vis)) return false;
    const long long chunk = std::min<long long>(njobs, 1 << 20);
    if (!ensure_search_scratch(chunk, max_slots(), 0, vis.bytes_per_job)) return false; // also the per-wave result lists (s_spill_)
    if ((size_t)chunk > s_roff_.cap()) { // the per-job arrays grow together; s_roff_ says for how many jobs they stand, so it is let go when one of the others fails
        const size_t c = (size_t)chunk;
        const bool ok = reset_all(s_roff_, s_rentry_) && s_roff_.grow(c) && s_rentry_.grow(c) && reset_all(s_rstate_, s_rtied_) && s_rstate_.grow(c) &&
                        s_rtied_.grow(c + 1) && reset_all(s_rres_, s_rdst_); // (those two: allocated by the first filtered call)
        if (!ok) { (void)s_roff_.reset(); return false; }
    }
    // the call's per-id array -- the words of the bit set that cover graph ids, the labels or the tag words of graph ids -- on this
    // context, as the KnnQuery forms have it; the per-query kinds besides need room for a launch's key table
    const long long n_ids = filtered ? std::min<long long>(f.n, g_n_) : 0;
    const auto make_resident = [&](auto &buf, size_t words, bool held) -> bool {
        if (held && words <= buf.cap()) return true;
        if (!buf.grow(std::max<size_t>(words, 1))) return false;
        if (words) {
            HIP_OK(hipMemcpyAsync(buf, f.per_id, 4u * words, hipMemcpyHostToDevice, st));
            HIP_OK(hipStreamSynchronize(st)); // (pageable source: the caller's buffer)
        }
        return true;
    };
    if (filtered && (!s_rres_.grow(s_roff_.cap()) || !s_rdst_.grow(s_roff_.cap()))) return false;
    if (keyed && !s_gquery_.grow((size_t)chunk)) return false;
    switch (f.kind) {
    case RangeFilter::kNone: break;
    case RangeFilter::kBits: if (!make_resident(s_allow_, (size_t)((n_ids + 31) / 32), false)) return false; break;
    case RangeFilter::kLabels: if (!make_resident(s_glabel_, (size_t)n_ids, false)) return false; break;
    case RangeFilter::kTags: if (!make_resident(s_ttags_, (size_t)n_ids, f.resident)) return false; break;
    }
    unsigned long long closure_total = 0; // entries the traversals found (sizes the next call's arena)
    if (!s_arena_used_.grow(1) || !s_rfin_ctr_.grow(2)) return false;
    constexpr size_t kArenaMax = (size_t)1 << 27; // 1 GB of results per launch; what does not fit then is handed back

    // One launch over the jobs listed in `todo` (at most `chunk`): results appended to res->found; jobs that found
    // the arena full are listed in `again` and *need = the entries they asked for; handed-back jobs in `handed`.
    auto launch = [&](const int *todo, int nj, ND *lists, int list_cap, int grid_cap, size_t arena_cap, std::vector<int> &again,
                      unsigned long long *need, std::vector<int> &handed) -> bool {
        if (!s_arena_.grow(arena_cap)) return false;
        // pinned layout: [evals, used (16 B) | jobs | offsets | counts | flags | entries | states]; then reused for the results
        // (filtered: [... | allowed counts | packed offsets] besides)
        const size_t b_jobs = sizeof(SearchJob) * (size_t)nj, b_off = 8u * (size_t)nj, b_i = 4u * (size_t)nj;
        // (a key per query: [... | the jobs' groups, or their masks] behind those)
        char *hs = static_cast<char *>(pinned_stage(16 + b_jobs + b_off + 4 * b_i + (filtered ? b_i + b_off : 0) + (keyed ? b_i : 0)));
        if (!hs) return false;
        SearchJob *h_jobs = reinterpret_cast<SearchJob *>(hs + 16);
        for (int i = 0; i < nj; ++i) h_jobs[i] = jobs[todo[i]];
        HIP_OK(hipMemcpyAsync(s_jobs_, h_jobs, b_jobs, hipMemcpyHostToDevice, st));
        if (keyed) { // the sort kernel's table: job -> the key of the query it names (its group, its mask)
            uint32_t *h_key = reinterpret_cast<uint32_t *>(hs + 16 + b_jobs + b_off + 5 * b_i + b_off);
            for (int i = 0; i < nj; ++i) h_key[i] = f.keys[h_jobs[i].qref];
            HIP_OK(hipMemcpyAsync(s_gquery_, h_key, b_i, hipMemcpyHostToDevice, st));
        }
        uj_len_ = 0;
        HIP_OK(hipMemsetAsync(s_jobctr_, 0, sizeof(int), st));
        HIP_OK(hipMemsetAsync(s_evals_, 0, sizeof(unsigned long long), st));
        HIP_OK(hipMemsetAsync(s_arena_used_, 0, sizeof(unsigned long long), st));
        const bool timed = profiling_;
        if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
        const auto kernel = persistent_kernel(metric_, vis.tab != nullptr, [&](auto m, auto h) {
            return layer != 0 ? &graph_range_kernel<m, h, true> : &graph_range_kernel<m, h>;
        });
        const int slots = std::min(std::min(max_slots(), grid_cap), resident_blocks(kernel, lds, num_cu_));
        hipLaunchKernelGGL(kernel, dim3(std::min<int>(nj, slots)), dim3(64), lds, st, d_rows_, d_row_sn_, d_queries_, d_q_sn_, pitch_, g_adj0_,
                           g_stride0_, g_upper_, g_pool_, g_strideU_, s_jobs_, range, lists, list_cap, s_visited_, vis.words, vis.tab, vis.tab_cap,
                           reinterpret_cast<ND *>(s_arena_.get()), (unsigned long long)arena_cap, s_arena_used_, s_roff_, s_cnt_, s_flag_, s_rentry_, s_evals_,
                           nbcap_r, nj, s_jobctr_);
        HIP_OK(hipGetLastError());
        // the ORDER, still on the device (dk_range_finish.h): every finished list ranked ascending in place; the lists that hold equal
        // distances replayed -- the reference's two heaps on the distances just found -- and ranked in heap-array order.  What these
        // hand back (lists beyond kRangeSortMax entries, -0 distances) the callers sort and replay on the host as before.
        // Filtered calls always rank (the partition by the filter is what makes the copy-back small); range_finish=0 and range < 0
        // then only count and leave every list to the host.
        const int finish = diag("range_finish", 2); // 0: order left to the host (as until round 5), 1: ranking only, 2: ranking and replays
        HIP_OK(hipMemsetAsync(s_rfin_ctr_, 0, sizeof(int) * 2, st));
        HIP_OK(hipMemsetAsync(s_rtied_, 0, sizeof(int), st));
        HIP_OK(hipMemsetAsync(s_rstate_, 0, sizeof(int) * (size_t)nj, st));
        const dim3 sort_grid(std::min(nj, 8 * std::max(1, num_cu_))), replay_grid(std::min(nj, 2 * std::max(1, num_cu_)));
        ND *arena = reinterpret_cast<ND *>(s_arena_.get());
        const int host_all = (int)(finish == 0 || range < 0.0f);
        switch (f.kind) {
        case RangeFilter::kTags:
            hipLaunchKernelGGL(range_sort_tagged_kernel, sort_grid, dim3(64), 0, st, arena, s_roff_, s_cnt_, s_flag_, nj, s_rstate_, s_rtied_, s_rfin_ctr_,
                               s_ttags_.get(), n_ids, reinterpret_cast<const unsigned *>(s_gquery_.get()), f.match, s_rres_, host_all,
                               (int)(diag("range_sort_long", 1) != 0));
            break;
        case RangeFilter::kLabels:
            hipLaunchKernelGGL(range_sort_grouped_kernel, sort_grid, dim3(64), 0, st, arena, s_roff_, s_cnt_, s_flag_, nj, s_rstate_, s_rtied_, s_rfin_ctr_,
                               s_glabel_.get(), n_ids, s_gquery_.get(), s_rres_, host_all);
            break;
        case RangeFilter::kBits:
            hipLaunchKernelGGL(range_sort_filtered_kernel, sort_grid, dim3(64), 0, st, arena, s_roff_, s_cnt_, s_flag_, nj, s_rstate_, s_rtied_, s_rfin_ctr_,
                               reinterpret_cast<const unsigned *>(s_allow_.get()), n_ids, s_rres_, host_all);
            break;
        case RangeFilter::kNone:
            if (finish >= 1)
                hipLaunchKernelGGL(range_sort_kernel, sort_grid, dim3(64), 0, st, arena, s_roff_, s_cnt_, s_flag_, nj, s_rstate_, s_rtied_, s_rfin_ctr_);
            break;
        }
        HIP_OK(hipGetLastError());
        if (finish >= 2) {
            if (filtered)
                hipLaunchKernelGGL(range_replay_filtered_kernel, replay_grid, dim3(64), sizeof(RangeReplayLds) + 64, st, reinterpret_cast<ND *>(s_arena_.get()), s_roff_,
                                   s_cnt_, s_rentry_, g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, layer, g_n_, range, s_rstate_, s_rtied_, s_rfin_ctr_ + 1, s_rres_);
            else
                hipLaunchKernelGGL(range_replay_kernel, replay_grid, dim3(64), sizeof(RangeReplayLds) + 64, st, reinterpret_cast<ND *>(s_arena_.get()), s_roff_,
                                   s_cnt_, s_rentry_, g_adj0_, g_stride0_, g_upper_, g_pool_, g_strideU_, layer, g_n_, range, s_rstate_, s_rtied_, s_rfin_ctr_ + 1);
            HIP_OK(hipGetLastError());
        }
        if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
        unsigned long long *h_hdr = reinterpret_cast<unsigned long long *>(hs);
        unsigned long long *h_off = reinterpret_cast<unsigned long long *>(hs + 16 + b_jobs);
        int *h_cnt = reinterpret_cast<int *>(hs + 16 + b_jobs + b_off);
        int *h_flag = h_cnt + nj, *h_entry = h_flag + nj, *h_state = h_entry + nj, *h_res = h_state + nj;
        unsigned long long *h_dst = reinterpret_cast<unsigned long long *>(h_res + nj);
        HIP_OK(hipMemcpyAsync(h_state, s_rstate_, b_i, hipMemcpyDeviceToHost, st));
        if (filtered) HIP_OK(hipMemcpyAsync(h_res, s_rres_, b_i, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_hdr, s_evals_, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_hdr + 1, s_arena_used_, 8, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_off, s_roff_, b_off, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_cnt, s_cnt_, b_i, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_flag, s_flag_, b_i, hipMemcpyDeviceToHost, st));
        HIP_OK(hipMemcpyAsync(h_entry, s_rentry_, b_i, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        const unsigned long long ev = h_hdr[0], used = h_hdr[1];
        // entries claimed beyond arena_cap belong to the jobs flagged 3 and were never written; the claims of the
        // finished jobs all lie below it, though not contiguously: the span they cover is copied back
        unsigned long long span = 0, finished = 0;
        const size_t base = res->found_n;
        for (int i = 0; i < nj; ++i) {
            const int j = todo[i];
            res->entry[(size_t)j] = h_entry[i];
            res->flag[(size_t)j] = 0;
            if (h_flag[i] == 0) {
                res->off[(size_t)j] = base + h_off[i];
                res->cnt[(size_t)j] = h_cnt[i];
                res->state[(size_t)j] = finish >= 1 || filtered ? h_state[i] : kRangeHostSort;
                const int results = filtered ? h_res[i] : h_cnt[i]; // (filtered, handed to the host: the allowed members of its closure)
                if (results >= 2) { if (res->state[(size_t)j] == kRangeFinal) stats_.range_device_ordered++; else stats_.range_host_ordered++; }
                if (h_cnt[i] > 0 && h_state[i] != kRangeFinal) count(kHostFinished, 1); // a closure the host finishes
                if (keyed && h_cnt[i] > kRangeSortMax && h_state[i] == kRangeFinal && h_res[i] >= 2) count(kLongFinished, 1); // rank_long's
                finished += (unsigned long long)h_cnt[i];
                if (h_cnt[i] > 0) span = std::max(span, h_off[i] + (unsigned long long)h_cnt[i]);
            } else if (h_flag[i] == 3) again.push_back(j);
            else { res->flag[(size_t)j] = 1; handed.push_back(j); }
        }
        *need = used - finished;
        closure_total += finished;
        if (filtered) { // only what the host needs crosses: final lists' results, other lists' closures -- packed in job order
            unsigned long long packed = 0;
            for (int i = 0; i < nj; ++i) {
                h_dst[i] = packed;
                if (h_flag[i] != 0) continue;
                const int j = todo[i];
                const int held = h_state[i] == kRangeFinal ? h_res[i] : h_cnt[i]; // (range_pack_kernel's own rule)
                res->off[(size_t)j] = base + packed;
                res->cnt[(size_t)j] = held;
                packed += (unsigned long long)held;
            }
            if (packed > 0) {
                if (!s_rpack_.grow((size_t)packed)) return false;
                HIP_OK(hipMemcpyAsync(s_rdst_, h_dst, b_off, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(range_pack_kernel, dim3(std::min((nj + 3) / 4, 8 * std::max(1, num_cu_))), dim3(256), 0, st, reinterpret_cast<const ND *>(s_arena_.get()),
                                   s_roff_, s_cnt_, s_flag_, s_rstate_, s_rres_, s_rdst_, nj, reinterpret_cast<ND *>(s_rpack_.get()));
                HIP_OK(hipGetLastError());
                if (!range_host_room(base + (size_t)packed, base)) return false;
                HIP_OK(hipMemcpyAsync(h_range_ + base, s_rpack_, sizeof(SearchHit) * (size_t)packed, hipMemcpyDeviceToHost, st));
                HIP_OK(hipStreamSynchronize(st));
                res->found_n = base + (size_t)packed;
            }
            span = 0;
        }
        if (span > 0) { // one copy, straight into the context's pinned result buffer (no staging hop, nothing zero-filled first)
            if (!range_host_room(base + (size_t)span, base)) return false;
            HIP_OK(hipMemcpyAsync(h_range_ + base, s_arena_, sizeof(SearchHit) * (size_t)span, hipMemcpyDeviceToHost, st));
            HIP_OK(hipStreamSynchronize(st));
            res->found_n = base + (size_t)span;
        }
        res->found = h_range_;
        return count_launch(&kRangeFamily, ev, vis.tab != nullptr, timed, ev0_, ev1_);
    };
    // `todo` through `launch`, with one more pass for the jobs that found the arena full
    auto run = [&](std::vector<int> todo, ND *lists, int list_cap, int grid_cap, size_t arena_cap, std::vector<int> &handed) -> bool {
        for (int pass = 0; pass < 2 && !todo.empty(); ++pass) {
            std::vector<int> again;
            unsigned long long need_total = 0;
            for (size_t off = 0; off < todo.size(); off += (size_t)chunk) {
                const int nj = (int)std::min<size_t>((size_t)chunk, todo.size() - off);
                unsigned long long need = 0;
                if (!launch(todo.data() + off, nj, lists, list_cap, grid_cap, arena_cap, again, &need, handed)) return false;
                need_total = std::max(need_total, need);
            }
            todo.swap(again);
            arena_cap = (size_t)std::min<unsigned long long>(std::max<unsigned long long>(need_total, 1ull << 20), kArenaMax);
        }
        for (int j : todo) { res->flag[(size_t)j] = 1; handed.push_back(j); } // more than kArenaMax results in one launch
        return true;
    };

    std::vector<int> all((size_t)njobs), handed, still;
    for (int i = 0; i < njobs; ++i) all[(size_t)i] = i;
    const size_t guess = (size_t)((range_hint_ * 1.25 + 16.0) * (double)std::min<long long>(chunk, njobs));
    if (!run(std::move(all), reinterpret_cast<ND *>(s_spill_.get()), kSpillCap, max_slots(), std::min(std::max<size_t>((size_t)1 << 20, guess), kArenaMax), handed)) return false;
    // result sets beyond a wave's list: again, with lists as long as the graph (at most 1 GB of them at a time);
    // a visited table filling up (graphs above 4M nodes) is not helped by that and stays handed back
    if (!handed.empty() && !vis.tab && g_n_ > kSpillCap) {
        const size_t list_cap = (size_t)std::min<long long>(g_n_, 1 << 24);
        const int waves = (int)std::max<size_t>(1, std::min<size_t>(handed.size(), ((size_t)1 << 27) / list_cap));
        if (!s_rlists_.grow(list_cap * (size_t)waves)) return false;
        if (!run(handed, reinterpret_cast<ND *>(s_rlists_.get()), (int)list_cap, waves, std::min(std::max<size_t>((size_t)1 << 20, list_cap), kArenaMax), still)) return false;
        handed.swap(still);
    }
    stats_.range_handbacks += handed.size();
    count(kHostFinished, handed.size());
    range_hint_ = (double)closure_total / (double)njobs; // (filtered calls too: the arena holds closures)
    return true;
}

// float.CompareTo order on distances that are never NaN here (d <= range held)
static inline bool range_hit_less(const SearchHit &a, const SearchHit &b) { return a.dist < b.dist; }

bool Device::range_search(const float *queries, int nq, int entry_point, float range, int *out_counts, int *out_flags)
{
    return range_search_filtered(queries, nq, entry_point, range, nullptr, 0, out_counts, out_flags);
}

// What the C ABI's searches begin with: a committed graph, an entry point in it, *top = its top layer ...  args_ok is the shim's own
// argument test: it fails with the entry point's "<who>: bad argument", after "no graph committed", as each shim had it.
bool Device::abi_entry(const char *who, int entry_point, int *top, bool args_ok)
{
    if (!hg_ || g_n_ <= 0) { set_dev_error(std::string(who) + ": no graph committed"); return false; }
    if (entry_point < 0 || entry_point >= hg_->n || !args_ok) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    *top = hg_->level[(size_t)entry_point];
    return true;
}
// ... a layer the entry point has (the reference indexes OutEdges[layer] of nodes reached from it), and the queries made resident.
bool Device::abi_begin(const char *who, const float *queries, int nq, int entry_point, int layer, int *top, bool args_ok)
{
    if (!abi_entry(who, entry_point, top, args_ok)) return false;
    if (layer < 0 || layer > *top) {
        set_dev_error(std::string(who) + ": layer " + std::to_string(layer) + " outside 0 .. " + std::to_string(*top) + " (the entry point's top layer)");
        return false;
    }
    return set_queries(queries, nq);
}

// The committed host graph's list of `id` on `layer`: what the range replays walk.
auto Device::host_list_of(int layer) const
{
    return [this, layer](int id) {
        return layer == 0 ? hg_->adj0.data() + (size_t)id * (size_t)hg_->stride0
                          : hg_->pool.data() + hg_->upper[(size_t)id] + (size_t)(layer - 1) * (size_t)hg_->strideU;
    };
}
// A closure of m entries finished on the host -- partitioned by `allow`, sorted, replayed where the allowed results tie
// (finish_filtered_range) -- and appended to abi_range_, *count its length.  An empty heap there fails the whole call, as the
// reference's exception does: no list, out_counts[0, nq) zero, kHeapEmptyError.
bool Device::finish_closure(int layer, int entry, float range, SearchHit *b, int m, const AllowPred &allow, int nq, int *out_counts, int *count)
{
    std::vector<NodeDist> ordered;
    if (finish_filtered_range(host_list_of(layer), 2 * hg_->M, entry, range, b, m, allow, ordered) == kRangeHeapEmpty) {
        abi_range_.clear();
        for (int j = 0; j < nq; ++j) out_counts[j] = 0;
        set_dev_error(kHeapEmptyError);
        return false;
    }
    *count = (int)ordered.size();
    for (const NodeDist &nd : ordered) abi_range_.push_back(SearchHit{nd.id, nd.dist});
    return true;
}

// What the three range_search forms run once their arguments stand and the queries are resident: a job for every query that
// has_candidate(i) -- or any query at all when range < 0: below zero the filtered call can throw on an empty set too
// (range_replay.h), so those queries run -- the launch, and the lists collected into abi_range_ in query order, as range_results
// hands them out.  A query without a job keeps the count and flag its caller gave it.  With a filter a list comes back final or as
// a closure to finish with the query's own predicate; without one it comes back ranked, or to sort, and tied distances are replayed.
template <class HasCandidate>
bool Device::range_search_run(int nq, int entry_point, int top, float range, RangeFilter f, HasCandidate &&has_candidate, int *out_counts, int *out_flags,
                              int layer)
{
    std::vector<SearchJob> jobs;
    for (int i = 0; i < nq; ++i)
        if (has_candidate(i) || !(range >= 0.0f)) jobs.push_back(SearchJob{i, entry_point, top, layer, -1});
    const int nj = (int)jobs.size();
    f.skipped = nq - nj;
    RangeResults r;
    if (!range_batch(jobs.data(), nj, range, &r, f)) return false;
    for (int j = 0; j < nj; ++j) {
        const int i = jobs[(size_t)j].qref;
        out_counts[i] = 0;
        out_flags[i] = r.flag[(size_t)j];
        if (out_flags[i]) continue;
        SearchHit *b = r.found + r.off[(size_t)j], *e = b + r.cnt[(size_t)j];
        if (f.kind != RangeFilter::kNone && r.state[(size_t)j] != kRangeFinal) { // a closure: partition, sort, replay where the allowed results tie
            if (!finish_closure(layer, r.entry[(size_t)j], range, b, r.cnt[(size_t)j], f.of(i), nq, out_counts, &out_counts[i])) return false;
            continue;
        }
        out_counts[i] = r.cnt[(size_t)j];
        if (f.kind == RangeFilter::kNone) {
            bool tie = r.state[(size_t)j] == kRangeTied; // (the device replays what it can: this is what it handed back)
            if (r.state[(size_t)j] == kRangeHostSort) {
                std::sort(b, e, range_hit_less);
                for (SearchHit *p = b; p + 1 < e; ++p) tie |= p[0].dist == p[1].dist; // also -0 next to +0
            }
            if (tie) { // OrderBy keeps the heap array's order there (HNSWIndex.cs:155): replay the heaps on the committed graph
                std::vector<NodeDist> ordered;
                replay_range_heaps(host_list_of(layer), 2 * hg_->M, r.entry[(size_t)j], range, b, r.cnt[(size_t)j], ordered);
                for (const NodeDist &nd : ordered) abi_range_.push_back(SearchHit{nd.id, nd.dist});
                continue;
            }
        }
        abi_range_.insert(abi_range_.end(), b, e); // the results, in the reference's order
    }
    return true;
}

// allow_bits == nullptr: no filter (range_search)
bool Device::range_search_filtered(const float *queries, int nq, int entry_point, float range, const uint32_t *allow_bits, long long nbits,
                                   int *out_counts, int *out_flags, int layer)
{
    abi_range_.clear();
    if (nq <= 0) return true;
    if (!out_counts || !out_flags) { set_dev_error("range_search: null argument"); return false; }
    int top;
    const bool args_ok = !(allow_bits && nbits < 0); // (false: "range_search: bad argument", in abi_entry's place for it)
    if (!abi_begin("range_search", queries, nq, entry_point, layer, &top, args_ok)) return false;
    return range_search_run(nq, entry_point, top, range, AllowBits{allow_bits, nbits}, [](int) { return true; }, out_counts, out_flags, layer);
}

// range_search_filtered with a group filter per query: query i is answered as with the allow-set
// { id : row_group[id] == query_group[i] }, every group in one traversal launch.  Only the labels of graph ids count.  A query whose
// group holds no graph id gets an empty list without a job (when range >= 0: range_search_run).
bool Device::range_search_grouped(const float *queries, int nq, int entry_point, float range, const int *row_group, long long n_row_group,
                                  const int *query_group, int n_groups, int *out_counts, int *out_flags, int layer)
{
    abi_range_.clear();
    if (nq <= 0) return true;
    if (!out_counts || !out_flags) { set_dev_error("range_search_grouped: null argument"); return false; }
    for (int i = 0; i < nq; ++i) { out_counts[i] = 0; out_flags[i] = 0; }
    if (!row_group || n_row_group < 0) { set_dev_error("range_search_grouped: row_group must not be NULL and n_row_group must be >= 0"); return false; }
    if (!query_group) { set_dev_error("range_search_grouped: query_group must not be NULL"); return false; }
    if (!group_args_ok("range_search_grouped", query_group, nq, n_groups)) return false;
    int top;
    if (!abi_begin("range_search_grouped", queries, nq, entry_point, layer, &top, true)) return false;
    const long long n_lab = std::min<long long>(n_row_group, g_n_);
    std::vector<char> has_id((size_t)n_groups, 0);
    for (long long id = 0; id < n_lab; ++id)
        if (row_group[id] >= 0 && row_group[id] < n_groups) has_id[(size_t)row_group[id]] = 1;
    return range_search_run(nq, entry_point, top, range, RangeFilter::labels(row_group, n_lab, query_group),
                            [&](int i) { return has_id[(size_t)query_group[i]] != 0; }, out_counts, out_flags, layer);
}

// range_search_grouped with a tag mask per query: query i is answered as with the allow-set
// { id : row_tags[id] matches query_tags[i] }, every mask in one traversal launch.  Only the words of graph ids count; which masks
// have a candidate among them the device counts (tag_counts) -- no host pass over the words -- and the words stay there for the
// sort kernel.  A query whose mask has none gets an empty list without a job, as for a group without ids.
bool Device::range_search_tagged(const float *queries, int nq, int entry_point, float range, const uint32_t *row_tags, long long n_row_tags,
                                 const uint32_t *query_tags, int match, int *out_counts, int *out_flags, int layer)
{
    abi_range_.clear();
    if (nq <= 0) return true;
    if (!out_counts || !out_flags) { set_dev_error("range_search_tagged: null argument"); return false; }
    for (int i = 0; i < nq; ++i) { out_counts[i] = 0; out_flags[i] = 0; }
    if (!row_tags || n_row_tags < 0) { set_dev_error("range_search_tagged: row_tags must not be NULL and n_row_tags must be >= 0"); return false; }
    if (!query_tags) { set_dev_error("range_search_tagged: query_tags must not be NULL"); return false; }
    TagCall tc;
    if (!tag_args_ok("range_search_tagged", query_tags, nq, match, &tc)) return false;
    int top;
    if (!abi_begin("range_search_tagged", queries, nq, entry_point, layer, &top, true)) return false;
    const long long n_lab = std::min<long long>(n_row_tags, g_n_);
    std::vector<int> cnt;
    if (!tag_candidates(row_tags, n_lab, tc.masks, match, cnt)) return false;
    RangeFilter f = RangeFilter::tags(row_tags, n_lab, query_tags, match, tc.masks.size());
    f.resident = n_lab > 0;
    return range_search_run(nq, entry_point, top, range, f, [&](int i) { return cnt[(size_t)tc.of[(size_t)i]] > 0; }, out_counts, out_flags, layer);
}

bool Device::range_results(int *out_ids, float *out_d)
{
    if (abi_range_.empty()) return true;
    if (!out_ids || !out_d) { set_dev_error("range_results: null argument"); return false; }
    for (size_t i = 0; i < abi_range_.size(); ++i) { out_ids[i] = abi_range_[i].id; out_d[i] = abi_range_[i].dist; }
    return true;
}

// ---- C-ABI graph staging (layer by layer) -------------------------------------------------
bool Device::graph_begin(int n, int max_edges, const int *levels)
{
    if (n <= 0 || max_edges < 1 || !levels) { set_dev_error("graph_begin: bad argument"); return false; }
    delete hg_;
    hg_ = new HostGraphStage();
    HostGraphStage &g = *hg_;
    g.n = n; g.M = max_edges; g.stride0 = 2 * max_edges + 2; g.strideU = max_edges + 2;
    g.level.assign(levels, levels + n);
    g.adj0.assign((size_t)n * g.stride0, 0);
    g.upper.assign((size_t)n, -1);
    size_t pool_len = 0;
    for (int i = 0; i < n; ++i) {
        if (levels[i] < 0 || levels[i] > 200) { set_dev_error("graph_begin: level out of range"); return false; }
        g.top = std::max(g.top, levels[i]);
        if (levels[i] > 0) { g.upper[(size_t)i] = (int64_t)pool_len; pool_len += (size_t)levels[i] * g.strideU; }
    }
    g.pool.assign(pool_len, 0);
    return true;
}

bool Device::graph_set_layer(int layer, const int *counts, const int *edges, int stride)
{
    if (!hg_) { set_dev_error("graph_set_layer: call hnswdev_graph_begin first"); return false; }
    HostGraphStage &g = *hg_;
    if (layer < 0 || !counts || !edges || stride < 1) { set_dev_error("graph_set_layer: bad argument"); return false; }
    const int cap = layer == 0 ? 2 * g.M + 1 : g.M + 1;
    // diag graph_unchecked=1 (tests of the graph-info / graph-reach kernels only: no traversal may run on such a graph): the count
    // word and the entries are staged as given -- at most the list's capacity of them -- so that a test can hand the kernels lists
    // that no build writes
    const bool unchecked = diag("graph_unchecked", 0) != 0;
    for (int i = 0; i < g.n; ++i) {
        if (g.level[(size_t)i] < layer) continue;
        const int c = counts[i];
        if (!unchecked && (c < 0 || c > cap || c > stride)) { set_dev_error("graph_set_layer: edge count exceeds MaxEdges(layer) + 1"); return false; }
        int *l = layer == 0 ? g.adj0.data() + (size_t)i * g.stride0 : g.pool.data() + g.upper[(size_t)i] + (size_t)(layer - 1) * g.strideU;
        l[0] = c;
        for (int j = 0; j < c && j < cap && j < stride; ++j) {
            const int e = edges[(size_t)i * stride + j];
            if (!unchecked && (e < 0 || e >= g.n || g.level[(size_t)e] < layer)) { set_dev_error("graph_set_layer: edge to a node outside the layer"); return false; }
            l[1 + j] = e;
        }
    }
    return true;
}

bool Device::graph_commit()
{
    if (!hg_) { set_dev_error("graph_commit: nothing staged"); return false; }
    HostGraphStage &g = *hg_;
    if (g.n > n_rows_hw_) { set_dev_error("graph_commit: graph has more nodes than uploaded rows"); return false; }
    return set_graph(g.adj0.data(), g.n, g.stride0, g.level.data(), g.upper.data(), g.pool.data(), (long long)g.pool.size(), g.strideU);
}

bool Device::knn_search(const float *queries, int nq, int entry_point, int k_beam, int k_out, int *out_ids, float *out_d, int *out_flag, int layer)
{
    if (nq <= 0) return true;
    int top;
    const bool args_ok = k_out >= 1 && k_beam >= k_out; // (false: "knn_search: bad argument", in abi_entry's place for it)
    if (!abi_begin("knn_search", queries, nq, entry_point, layer, &top, args_ok)) return false;
    std::vector<SearchJob> jobs((size_t)nq);
    for (int i = 0; i < nq; ++i) jobs[(size_t)i] = SearchJob{i, entry_point, top, layer, -1};
    return search_batch(jobs.data(), nq, k_beam, k_out, out_ids, out_d, out_flag);
}

int Device::multilayer_search_abi(const float *queries, int nq, int entry_point, int k, int max_layer, int min_layer, int layers_cap, int *out_ids,
                                  float *out_d, int *out_flag)
{
    if (max_layer < -1 || min_layer < 0) { set_dev_error("multilayer_search: max_layer must be >= -1 and min_layer >= 0"); return -1; }
    if (nq <= 0 || k < 1 || max_layer == -1) return 0;
    int top; // (no abi_begin: the layers are this call's own to check, and the queries go up only once something will be searched)
    if (!abi_entry("multilayer_search", entry_point, &top)) return -1;
    const int first = std::min(top, max_layer), nslots = first + 1;
    if (layers_cap < nslots) { set_dev_error("multilayer_search: layers_cap " + std::to_string(layers_cap) + " is too small, " + std::to_string(nslots) + " layer slots are needed"); return -1; }
    if (k == 1) return nslots;
    if (!out_ids || !out_d || !out_flag) { set_dev_error("multilayer_search: null argument"); return -1; }
    const size_t per = (size_t)(k - 1);
    for (int i = 0; i < nq; ++i) {
        out_flag[i] = 0;
        pad_results(out_ids + (size_t)i * layers_cap * per, out_d + (size_t)i * layers_cap * per, (size_t)nslots * per);
    }
    if (min_layer > first) return nslots;
    if (!set_queries(queries, nq)) return -1;
    if (layers_cap == nslots) return multilayer_search(nq, entry_point, top, first, min_layer, k, out_ids, out_d, out_flag) ? nslots : -1;
    std::vector<int> ids((size_t)nq * nslots * per);
    std::vector<float> ds(ids.size());
    if (!multilayer_search(nq, entry_point, top, first, min_layer, k, ids.data(), ds.data(), out_flag)) return -1;
    widen_rows(out_ids, out_d, ids.data(), ds.data(), (size_t)nq, (size_t)nslots * per, (size_t)layers_cap * per);
    return nslots;
}

bool Device::knn_search_filtered(const float *queries, int nq, int entry_point, int k_beam, int k_out, const uint32_t *allow_bits, long long nbits,
                                 int *out_ids, float *out_d, int *out_flag, int layer)
{
    if (!allow_bits || nbits < 0) { set_dev_error("knn_search_filtered: allow_bits must not be NULL and nbits must be >= 0"); return false; }
    if (nq <= 0) return true;
    int top;
    const bool args_ok = k_out >= 1 && k_beam >= k_out; // (false: "knn_search_filtered: bad argument", in abi_entry's place for it)
    if (!abi_begin("knn_search_filtered", queries, nq, entry_point, layer, &top, args_ok)) return false;
    return search_filtered(nq, entry_point, top, k_beam, k_out, allow_bits, nbits, out_ids, out_d, out_flag, layer);
}

bool Device::knn_search_grouped(const float *queries, int nq, int entry_point, int k_beam, int k_out, const int *row_group, long long n_row_group,
                                const int *query_group, int n_groups, int *out_ids, float *out_d, int *out_flag, int layer)
{
    if (!row_group || n_row_group < 0) { set_dev_error("knn_search_grouped: row_group must not be NULL and n_row_group must be >= 0"); return false; }
    if (nq <= 0) return true;
    if (!query_group) { set_dev_error("knn_search_grouped: query_group must not be NULL"); return false; }
    if (!queries || !out_ids || !out_d || !out_flag) { set_dev_error("knn_search_grouped: null argument"); return false; }
    if (!group_args_ok("knn_search_grouped", query_group, nq, n_groups)) return false;
    int top;
    const bool args_ok = k_out >= 1 && k_beam >= k_out; // (false: "knn_search_grouped: bad argument", in abi_entry's place for it)
    if (!abi_begin("knn_search_grouped", queries, nq, entry_point, layer, &top, args_ok)) return false;
    return search_grouped(nq, entry_point, top, k_beam, k_out, row_group, n_row_group, query_group, n_groups, out_ids, out_d, out_flag, layer);
}

bool Device::knn_search_tagged(const float *queries, int nq, int entry_point, int k_beam, int k_out, const uint32_t *row_tags, long long n_row_tags,
                               const uint32_t *query_tags, int match, int *out_ids, float *out_d, int *out_flag, int layer)
{
    if (!row_tags || n_row_tags < 0) { set_dev_error("knn_search_tagged: row_tags must not be NULL and n_row_tags must be >= 0"); return false; }
    if (match != 0 && match != 1) { set_dev_error("knn_search_tagged: match = " + std::to_string(match) + " is neither 0 (any) nor 1 (all)"); return false; }
    if (nq <= 0) return true;
    if (!query_tags) { set_dev_error("knn_search_tagged: query_tags must not be NULL"); return false; }
    if (!queries || !out_ids || !out_d || !out_flag) { set_dev_error("knn_search_tagged: null argument"); return false; }
    TagCall tc;
    if (!tag_args_ok("knn_search_tagged", query_tags, nq, match, &tc)) return false;
    int top;
    const bool args_ok = k_out >= 1 && k_beam >= k_out; // (false: "knn_search_tagged: bad argument", in abi_entry's place for it)
    if (!abi_begin("knn_search_tagged", queries, nq, entry_point, layer, &top, args_ok)) return false;
    return search_tagged(nq, entry_point, top, k_beam, k_out, row_tags, n_row_tags, query_tags, match, out_ids, out_d, out_flag, layer);
}

// ---- the flat scan (hnswdev_exact_knn; device code in dk_exact.h) --------------------------------------
// Tile and chunk of a call.  The query tile: as many queries as 16 KB of staged query words and 32 KB of k-entry lists hold, at
// most 32 and no more than the call has; `exact_qtile` forces it.  The chunk: enough chunks that the tiles x chunks fill the chip
// about twice over, none shorter than 1 024 rows; `exact_chunk` forces it.  At most 4 096 chunks either way (the merge walks them).
struct ExactPlan {
    int qtile, piece, n_chunks;
    long long chunk, round; // rows per chunk, queries per round
    size_t lds;
};
static ExactPlan exact_plan(int nq, long long m, int k, int pitch, int num_cu, int entry_bytes = kExactKeyBytes)
{
    ExactPlan p;
    const int forced_q = diag("exact_qtile", 0);
    const long long forced_c = diag("exact_chunk", 0);
    int qt = forced_q > 0 ? std::min(forced_q, kExactMaxQTile) : kExactMaxQTile;
    const auto tile_rows = [](int q) { return (size_t)((q + kExactRQ - 1) / kExactRQ * kExactRQ); };
    while (qt > kExactRQ && (tile_rows(qt) * (size_t)k * (size_t)entry_bytes > 32768 || (forced_q <= 0 && ((size_t)qt * pitch * 4 > 16384 || qt / 2 >= nq)))) qt >>= 1;
    p.qtile = qt;
    const size_t qtr = tile_rows(qt);
    // (entries of 12 bytes can leave the smallest tile's lists above 32 KB -- k = 1024: 48 KB -- and the staged words take what is left)
    const size_t fixed = exact_scan_lds(qt, 0, pitch, k, entry_bytes), q_room = std::min<size_t>(16384, (64 * 1024 - fixed) & ~(size_t)255); // (fixed <= 55 KB)
    p.piece = qtr * (size_t)pitch * 4 <= q_room ? pitch : std::max(16, (int)(q_room / 4 / qtr) & ~15);
    p.lds = exact_scan_lds(qt, p.piece, pitch, k, entry_bytes);
    const long long tiles = (std::min<long long>(nq, 65536) + qt - 1) / qt;
    long long chunks = forced_c > 0 ? (m + forced_c - 1) / forced_c
                                    : std::max<long long>(1, std::min<long long>((2LL * num_cu + tiles - 1) / tiles, m / 1024));
    chunks = std::min<long long>(chunks, 4096);
    p.chunk = (m + chunks - 1) / chunks;
    if (forced_c <= 0) p.chunk = (p.chunk + kExactIterRows - 1) / kExactIterRows * kExactIterRows;
    p.n_chunks = (int)((m + p.chunk - 1) / p.chunk);
    // the lists of a round: at most 1 GiB; its results: at most 2^24 entries through the pinned stage
    const long long by_lists = (1LL << 30) / ((long long)p.n_chunks * k * 8), by_out = (1LL << 24) / k;
    p.round = std::max<long long>(1, std::min<long long>({(long long)nq, by_lists, by_out}));
    return p;
}

// The queries of a flat scan: the resident set, or the scan's own -- uploaded by set_queries (the one staging path: pinned copy,
// int8 quantisation, cosine norms) while the scan's buffers stand in for the resident set's, which is then put back untouched.
bool Device::exact_queries(const char *who, const float *queries, int nq, const float **d_q, const double **d_qsn)
{
    *d_q = d_queries_;
    *d_qsn = d_q_sn_;
    if (queries) {
        if (tail_.n > 0) { set_dev_error(std::string(who) + ": a streamed query set is still being uploaded"); return false; }
        std::swap(d_queries_, x_queries_); std::swap(d_q_sn_, x_q_sn_);
        const long long kept = n_queries_;
        const bool kept_by_id = q_by_id_;
        const bool ok = set_queries(queries, nq);
        std::swap(d_queries_, x_queries_); std::swap(d_q_sn_, x_q_sn_);
        n_queries_ = kept;
        q_by_id_ = kept_by_id;
        if (!ok) return false;
        *d_q = x_queries_; *d_qsn = x_q_sn_;
    } else if (nq > n_queries_ || tail_.n > 0) {
        set_dev_error(std::string(who) + ": queries == NULL needs a resident query set of at least nq rows (hnswdev_set_queries)");
        return false;
    }
    return true;
}

// The id list of a flat scan in x_ids_, *m entries: the identity without a bitset (x_ids_ is not used: *m = n_allow); otherwise
// the masked words go up from pinned memory with the bit counts in front of each block of them (counted while they are copied),
// and exact_compact_kernel writes the ascending ids.  The stream is idle and the pinned stage free when this returns.
bool Device::exact_id_list(const uint32_t *allow_bits, long long n_allow, long long *m_out)
{
    *m_out = n_allow;
    if (!allow_bits) return true;
    hipStream_t st = S(stream_);
    const size_t words = (size_t)((n_allow + 31) / 32), blocks = (words + kExactCompactWords - 1) / kExactCompactWords;
    char *hs = static_cast<char *>(pinned_stage(8 * blocks + 4 * words));
    if (!hs) return false;
    long long *h_off = reinterpret_cast<long long *>(hs);
    unsigned *h_words = reinterpret_cast<unsigned *>(hs + 8 * blocks);
    long long m = 0;
    for (size_t w = 0; w < words; ++w) {
        if (w % kExactCompactWords == 0) h_off[w / kExactCompactWords] = m;
        const unsigned v = allow_bits[w] & ((long long)(w + 1) * 32 <= n_allow ? ~0u : (1u << (n_allow & 31)) - 1u);
        h_words[w] = v;
        m += __builtin_popcount(v);
    }
    if (!s_allow_.grow(words) || !x_boff_.grow(blocks) || !x_ids_.grow((size_t)m)) return false;
    HIP_OK(hipMemcpyAsync(x_boff_, h_off, 8 * blocks, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(s_allow_, h_words, 4 * words, hipMemcpyHostToDevice, st));
    HIP_OK(exact_compact_launch(s_allow_, (long long)words, x_boff_, x_ids_, st));
    HIP_OK(hipStreamSynchronize(st)); // the pinned stage is used again by the caller
    *m_out = m;
    return true;
}

// How a flat-scan call begins (exact_scan_begin, exact_grouped_begin): with an error; with nothing to measure -- no query has a
// candidate, so the caller writes its padding or leaves its lists empty and succeeds without a launch; or ready to scan.
enum class ExactStart { failed, nothing, ready };

// What an ungrouped flat scan measures: the queries on the device (pitch_ words each; d_qsn their cosine norms or nullptr) and the
// m entries of the id list `ids` (nullptr: the identity).
struct ExactScanInput {
    const float *d_q;
    const double *d_qsn;
    const int *ids;
    long long m;
};

// The candidates and queries of an ungrouped flat scan, after the caller's own argument checks: the rows that exist and are
// allowed (none: nothing to measure), then the queries, the device and the id list as exact_queries and exact_id_list leave them.
ExactStart Device::exact_scan_begin(const char *who, const float *queries, int nq, long long n_rows, const uint32_t *allow_bits, long long nbits, ExactScanInput *in)
{
    if (!allow_bits) nbits = 0; // no filter: nbits means nothing, whatever the caller left in it
    // rows that exist: a row beyond what was uploaded is never dereferenced, whatever n_rows and the bitset say
    const long long n = std::min(n_rows, n_rows_hw_), n_allow = allow_bits ? std::min(nbits, n) : n;
    if (n_allow <= 0 || (allow_bits && !allows_any(allow_bits, nbits, n))) return ExactStart::nothing;
    if (!exact_queries(who, queries, nq, &in->d_q, &in->d_qsn) || !bind() || !exact_id_list(allow_bits, n_allow, &in->m)) return ExactStart::failed;
    in->ids = allow_bits ? x_ids_.get() : nullptr;
    return ExactStart::ready;
}

// The scan's arguments for one round: `nr` queries from query `off` of d_q on, the tile `qt` and `piece`, the pairs counted in
// x_evals_ (allocated here).  The rest is left at nothing -- what a grouped range sink reads: the caller sets ids / m / chunk /
// n_chunks where its blocks are not work items, and k / lists where its sink keeps lists.
bool Device::exact_scan_args(const float *d_q, const double *d_qsn, long long off, int nr, int qt, int piece, ExactScanArgs *a)
{
    if (!x_evals_.grow(1)) return false;
    *a = ExactScanArgs{};
    a->rows = d_rows_; a->row_sn = d_row_sn_;
    a->queries = d_q + (size_t)off * pitch_;
    a->q_sn = d_qsn ? d_qsn + off : nullptr;
    a->dim = pitch_; a->nq = nr; a->qtile = qt; a->piece = piece; a->evals = x_evals_;
    return true;
}

// One launch of the flat scan, timed and counted -- the only place the exact_* statistics are written.  x_evals_ is zeroed;
// `enqueue` launches the scan, and whatever else belongs inside the timed window (the top-k calls' merge; a range call's sort is
// outside it), between the event pair when profiling is on; `fetch` enqueues the caller's own copies out; then the kernel's count
// goes to the pinned word h_ev and the stream is synchronised, so what `fetch` asked for is on the host when this returns.
// The flat scan is no traversal: it counts in its own family only, not in the search_* totals, and the evaluations are the kernel's
// own count of the pairs it turned into keys -- shadows excluded -- not queries x rows worked out here.  Every sink counts here, so
// a repeated pass counts its pairs again, the unwanted queries of its tiles included.
template <class Enqueue, class Fetch>
bool Device::exact_timed_scan(unsigned long long *h_ev, Enqueue &&enqueue, Fetch &&fetch)
{
    hipStream_t st = S(stream_);
    if (!ev0_.create(true) || !ev1_.create(true)) return false;
    const bool timed = profiling_;
    HIP_OK(hipMemsetAsync(x_evals_, 0, sizeof(unsigned long long), st));
    if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
    if (!enqueue()) return false;
    if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
    if (!fetch()) return false;
    HIP_OK(hipMemcpyAsync(h_ev, x_evals_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    stats_.exact_launches += 1; stats_.exact_evals += *h_ev;
    if (timed) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, E(ev0_), E(ev1_)));
        stats_.exact_kernel_ms += ms; stats_.exact_timed_launches += 1; stats_.exact_timed_evals += *h_ev;
    }
    return true;
}

bool Device::exact_knn(const float *queries, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d)
{
    if (nq <= 0) return true;
    if (!out_ids || !out_d || k < 1 || n_rows < 0 || (allow_bits && nbits < 0)) { set_dev_error("exact_knn: bad argument"); return false; }
    if (k > kExactMaxK) { set_dev_error("exact_knn: k = " + std::to_string(k) + " is above the limit of " + std::to_string(kExactMaxK)); return false; }
    ExactScanInput in;
    const ExactStart s = exact_scan_begin("exact_knn", queries, nq, n_rows, allow_bits, nbits, &in);
    if (s == ExactStart::nothing) pad_results(out_ids, out_d, (size_t)nq * (size_t)k); // padding, no launch
    if (s != ExactStart::ready) return s == ExactStart::nothing;
    return exact_knn_rounds(in.d_q, in.d_qsn, nq, in.ids, in.m, k, out_ids, out_d, nullptr);
}

// What exact_knn_rounds needs for the collapsed sink (ExactTopKCollapse): row_group on the device, the cap, the two device counters.
struct ExactCollapseArgs {
    const int *d_row_group;
    int per_group;
    unsigned long long *d_info;
};

// The rounds of a top-k flat scan: nq queries on the device (d_q, pitch_ words each; d_qsn their cosine norms or nullptr) against the
// m entries of the id list d_ids (nullptr: the identity).  out_d may be nullptr; d_keep_ids: nullptr, or nq x k ints on the device
// that receive the ids as well (graph_repair_round's candidates stay there for the proposal kernel).
// d_self: nullptr, or nq ids on the device -- query i is the stored row d_self[i], which is no candidate of it (ExactTopKSelf).
// collapse: nullptr, or the collapsed sink's arguments -- scan and merge are then ExactTopKCollapse's, the tile planned for its entries.
bool Device::exact_knn_rounds(const float *d_q, const double *d_qsn, int nq, const int *d_idlist, long long m, int k, int *out_ids, float *out_d, int *d_keep_ids,
                              const int *d_self, const ExactCollapseArgs *collapse)
{
    hipStream_t st = S(stream_);
    const ExactPlan p = exact_plan(nq, m, k, pitch_, num_cu_, collapse ? kExactCollapseEntryBytes : kExactKeyBytes);
    if (p.lds > 64 * 1024) { set_dev_error("exact_knn: tile exceeds the LDS budget"); return false; }
    if (!x_lists_.grow((size_t)p.round * p.n_chunks * k) || !x_out_.grow(2 * (size_t)p.round * k)) return false;
    char *hs = static_cast<char *>(pinned_stage(8 * (size_t)p.round * k + 8));
    if (!hs) return false;
    unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs + 8 * (size_t)p.round * k);
    for (long long off = 0; off < nq; off += p.round) {
        const int nr = (int)std::min<long long>(p.round, nq - off);
        ExactScanArgs a;
        if (!exact_scan_args(d_q, d_qsn, off, nr, p.qtile, p.piece, &a)) return false;
        a.ids = d_idlist; a.m = m; a.chunk = p.chunk; a.n_chunks = p.n_chunks; a.k = k; a.lists = x_lists_;
        const unsigned tiles = (unsigned)((nr + p.qtile - 1) / p.qtile);
        const size_t res = 4u * (size_t)nr * k;
        int *d_ids = x_out_;
        float *d_d = reinterpret_cast<float *>(x_out_.get() + (size_t)p.round * k);
        const auto enqueue = [&]() -> bool {
            hipError_t e = hipSuccess;
            if (collapse) {
                const ExactTopKCollapse sink{collapse->d_row_group, collapse->per_group, collapse->d_info};
                with_metric(metric_, [&](auto mt) { e = exact_collapsed_scan_launch<mt>(a, sink, tiles, p.lds, st); });
                HIP_OK(e);
                HIP_OK(exact_merge_collapsed_launch(x_lists_, p.n_chunks, k, nr, sink.row_group, sink.per_group, sink.info, d_ids, d_d, st));
                return true;
            }
            if (d_self) with_metric(metric_, [&](auto mt) { e = exact_self_scan_launch<mt>(a, ExactTopKSelf{d_self + off}, tiles, p.lds, st); });
            else with_metric(metric_, [&](auto mt) { e = exact_scan_launch<mt>(a, tiles, p.lds, st); });
            HIP_OK(e);
            HIP_OK(exact_merge_launch(x_lists_, p.n_chunks, k, nr, d_ids, d_d, st));
            return true;
        };
        const auto fetch = [&]() -> bool {
            HIP_OK(hipMemcpyAsync(hs, d_ids, res, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(hs + 4u * (size_t)p.round * k, d_d, res, hipMemcpyDeviceToHost, st));
            if (d_keep_ids) HIP_OK(hipMemcpyAsync(d_keep_ids + (size_t)off * k, d_ids, res, hipMemcpyDeviceToDevice, st));
            return true;
        };
        if (!exact_timed_scan(h_ev, enqueue, fetch)) return false;
        memcpy(out_ids + (size_t)off * k, hs, res);
        if (out_d) memcpy(out_d + (size_t)off * k, hs + 4u * (size_t)p.round * k, res);
    }
    return true;
}

// ---- hnswdev_exact_knn_collapsed: at most per_group results per label ------------------------------------------
// exact_knn with another sink: the same queries, id list, rounds and statistics; the labels of ids [0, min(n_rows, uploaded)) go up
// once, before the rounds, into a buffer of the call's own, and two device counters come back after them.
bool Device::exact_knn_collapsed(const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group, int per_group,
                                 const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d)
{
    if (nq <= 0) return true;
    const char *who = "exact_knn_collapsed";
    const auto fail = [&](const std::string &what) { set_dev_error(std::string(who) + ": " + what); return false; };
    if (!out_ids || !out_d || k < 1 || n_rows < 0 || (allow_bits && nbits < 0)) return fail("bad argument");
    if (k > kExactMaxK) return fail("k = " + std::to_string(k) + " is above the limit of " + std::to_string(kExactMaxK));
    if (per_group < 1 || per_group > k) return fail("per_group = " + std::to_string(per_group) + " is outside [1, k = " + std::to_string(k) + "]");
    if (!row_group || n_row_group < 0) return fail("row_group must not be NULL and n_row_group must be >= 0");
    const long long n = std::min(n_rows, n_rows_hw_); // the ids that can be candidates: every one of them needs a label
    if (n_row_group < n) return fail("row_group has " + std::to_string(n_row_group) + " entries, the scan's " + std::to_string(n) + " ids need one each");
    ExactScanInput in;
    const ExactStart s = exact_scan_begin(who, queries, nq, n_rows, allow_bits, nbits, &in);
    if (s == ExactStart::nothing) pad_results(out_ids, out_d, (size_t)nq * (size_t)k); // padding, no launch
    if (s != ExactStart::ready) return s == ExactStart::nothing;
    hipStream_t st = S(stream_);
    if (!x_clabels_.grow((size_t)n) || !x_cinfo_.grow(2)) return false;
    if (!staged_upload(reinterpret_cast<float *>(x_clabels_.get()), reinterpret_cast<const float *>(row_group), 4 * (size_t)n)) return false;
    HIP_OK(hipMemsetAsync(x_cinfo_, 0, 2 * sizeof(unsigned long long), st));
    const ExactCollapseArgs ca{x_clabels_, per_group, x_cinfo_};
    if (!exact_knn_rounds(in.d_q, in.d_qsn, nq, in.ids, in.m, k, out_ids, out_d, nullptr, nullptr, &ca)) return false;
    unsigned long long *h = static_cast<unsigned long long *>(pinned_stage(2 * sizeof(unsigned long long)));
    if (!h) return false;
    HIP_OK(hipMemcpyAsync(h, x_cinfo_, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    using Slot = slot::exact_collapsed_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::calls] += 1; ctr[Slot::queries] += (uint64_t)nq; ctr[Slot::dropped] += h[0]; ctr[Slot::evicted] += h[1];
    return true;
}

// knn_query_collapsed on this context: the labels of the graph's ids go up, then the traversal the plain calls run
// -- search_filtered with a bitset, search_batch without -- with row_collapse_ set, so that its launches collapse their rows on the
// device and copy k columns out.
bool Device::search_collapsed(int nq, int entry, int entry_layer, int ef, int beam, int k, const int *row_group, long long n_row_group, int per_group,
                              const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d, int *out_flag, int search_layer)
{
    if (nq <= 0) return true;
    const auto fail = [&](const std::string &what) { set_dev_error("search_collapsed: " + what); return false; };
    if (!out_ids || !out_d || !out_flag || !row_group || k < 1 || beam < k || per_group < 1 || per_group > k || (allow_bits && nbits < 0)) return fail("bad argument");
    if (n_row_group < g_n_) return fail("row_group has " + std::to_string(n_row_group) + " entries, the graph has " + std::to_string(g_n_) + " ids");
    if (allow_bits && !allows_any(allow_bits, nbits, g_n_)) { // no candidate: padding in rows of k, no launch
        pad_results(out_ids, out_d, (size_t)nq * (size_t)k);
        for (int i = 0; i < nq; ++i) out_flag[i] = 0;
        return true;
    }
    if (!bind() || !x_clabels_.grow((size_t)std::max<long long>(g_n_, 1))) return false;
    if (g_n_ > 0 && !staged_upload(reinterpret_cast<float *>(x_clabels_.get()), reinterpret_cast<const float *>(row_group), 4 * (size_t)g_n_)) return false;
    const RowCollapse rc{x_clabels_, g_n_, per_group, k};
    struct Scope { Device *d; ~Scope() { d->row_collapse_ = nullptr; } } scope{this};
    row_collapse_ = &rc;
    if (allow_bits) return search_filtered(nq, entry, entry_layer, ef, beam, allow_bits, nbits, out_ids, out_d, out_flag, search_layer);
    std::vector<SearchJob> jobs((size_t)nq);
    for (int i = 0; i < nq; ++i) jobs[(size_t)i] = SearchJob{i, entry, entry_layer, search_layer, -1, 0};
    return search_batch(jobs.data(), nq, ef, beam, out_ids, out_d, out_flag);
}

// The group lists of a grouped flat scan: row_group[0, n) up, counts | offsets | cursors and the members on the device (a CSR in
// x_ids_, built by exact_group_lists_launch), the counts back in one copy.  cnt[g]: members of group g; goff[g]: where its segment
// starts in x_ids_; *listed: ids that are in a group.  The stream is idle and the pinned stage free when this returns.
bool Device::exact_group_lists(const char *who, const int *row_group, long long n, int n_groups, std::vector<int> &cnt, std::vector<int> &goff, uint64_t *listed)
{
    hipStream_t st = S(stream_);
    const size_t G = (size_t)n_groups, rg_bytes = 4 * (size_t)n;
    if (!x_grow_.grow((size_t)n) || !x_gcnt_.grow(3 * G) || !x_ids_.grow((size_t)n)) return false;
    cnt.assign(G, 0);
    goff.assign(G, 0);
    const size_t staged = rg_bytes < (4u << 20) ? rg_bytes : 0; // larger arrays go up in pieces, as query sets do
    char *hs = static_cast<char *>(pinned_stage(staged + 4 * G));
    if (!hs) return false;
    if (staged) { memcpy(hs, row_group, rg_bytes); HIP_OK(hipMemcpyAsync(x_grow_, hs, rg_bytes, hipMemcpyHostToDevice, st)); }
    else if (!staged_upload(reinterpret_cast<float *>(x_grow_.get()), reinterpret_cast<const float *>(row_group), rg_bytes)) return false;
    const bool timed = profiling_; // the list-building kernels have an event pair of their own (exact_grouped_list_ms)
    if (timed && (!ev0_.create(true) || !ev1_.create(true))) return false;
    if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
    HIP_OK(exact_group_lists_launch(x_grow_, n, n_groups, x_gcnt_, x_gcnt_.get() + G, x_gcnt_.get() + 2 * G, x_ids_, st));
    if (timed) HIP_OK(hipEventRecord(E(ev1_), st));
    HIP_OK(hipMemcpyAsync(hs + staged, x_gcnt_, 4 * G, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (timed) {
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, E(ev0_), E(ev1_)));
        xg_list_ms_ += ms;
    }
    memcpy(cnt.data(), hs + staged, 4 * G); // (the stage is used again by the caller)
    long long at = 0;
    for (size_t g = 0; g < G; ++g) { goff[g] = (int)at; at += cnt[g]; }
    if (at > n) { set_dev_error(std::string(who) + ": the group counts exceed the ids"); return false; }
    *listed = (uint64_t)at;
    return true;
}

// The queries of a grouped flat scan in the order `order` (sorted position -> the caller's index): uploaded through set_queries'
// path, or (queries == nullptr) gathered from the resident set on the device -- the caller's query i is resident query resident[i]
// (nullptr: i).  The stream is idle and the pinned stage free when this returns.
bool Device::exact_sorted_queries(const char *who, const float *queries, int nq, const std::vector<int> &order, const float **d_q, const double **d_qsn,
                                  const int *resident)
{
    hipStream_t st = S(stream_);
    if (queries) {
        std::vector<float> sorted((size_t)nq * (size_t)dim_);
        for (int p = 0; p < nq; ++p) memcpy(&sorted[(size_t)p * dim_], queries + (size_t)order[(size_t)p] * dim_, sizeof(float) * (size_t)dim_);
        return exact_queries(who, sorted.data(), nq, d_q, d_qsn);
    }
    if (!x_queries_.grow((size_t)nq * pitch_, (size_t)std::max(nq, 1024) * pitch_) || (metric_ == M_COS && !x_q_sn_.grow((size_t)nq, (size_t)std::max(nq, 1024)))) return false;
    if (!x_gperm_.grow((size_t)nq)) return false;
    int *hp = static_cast<int *>(pinned_stage(4 * (size_t)nq));
    if (!hp) return false;
    if (resident) for (int p = 0; p < nq; ++p) hp[p] = resident[order[(size_t)p]];
    else memcpy(hp, order.data(), 4 * (size_t)nq);
    HIP_OK(hipMemcpyAsync(x_gperm_, hp, 4 * (size_t)nq, hipMemcpyHostToDevice, st));
    HIP_OK(exact_gather_queries_launch(d_queries_, metric_ == M_COS ? d_q_sn_.get() : nullptr, x_gperm_, nq, pitch_, x_queries_, x_q_sn_, st));
    HIP_OK(hipStreamSynchronize(st)); // the pinned stage is used again by the caller
    *d_q = x_queries_; *d_qsn = metric_ == M_COS ? x_q_sn_.get() : nullptr;
    return true;
}

// Each scanned group's chunks (a group is scanned when it has a query and a member): the (tile, row) work of the call spread over
// about two blocks per CU, no chunk shorter than 1 024 rows, at most kExactMaxChunks per group; `exact_chunk` forces the rows per
// chunk.  gchunk[g]: rows per chunk; gnch[g]: chunks, 0 where the group is not scanned.
static void exact_group_chunks(const std::vector<int> &gq, const std::vector<int> &cnt, int qt, int num_cu, std::vector<int> &gchunk, std::vector<int> &gnch)
{
    const size_t G = gq.size();
    const long long forced_c = diag("exact_chunk", 0);
    long long work = 0; // (tile, row) pairs of the call
    for (size_t g = 0; g < G; ++g)
        if (gq[g] > 0 && cnt[g] > 0) work += (long long)((gq[g] + qt - 1) / qt) * cnt[g];
    const long long target = std::max<long long>(1024, (work + 2LL * num_cu - 1) / (2LL * num_cu));
    gchunk.assign(G, 0);
    gnch.assign(G, 0);
    for (size_t g = 0; g < G; ++g) {
        if (gq[g] <= 0 || cnt[g] <= 0) continue;
        const long long m = cnt[g];
        long long chunks = forced_c > 0 ? (m + forced_c - 1) / forced_c : std::max<long long>(1, std::min<long long>((m + target - 1) / target, m / 1024));
        chunks = std::min<long long>(chunks, kExactMaxChunks);
        long long chunk = (m + chunks - 1) / chunks;
        if (forced_c <= 0) chunk = (chunk + kExactIterRows - 1) / kExactIterRows * kExactIterRows;
        gchunk[g] = (int)chunk;
        gnch[g] = (int)((m + chunk - 1) / chunk);
    }
}

// The queries of each round (round_end: one past the last query of each, in the caller's order) sorted by group -- a counting sort,
// stable.  order[sorted position] = the caller's index.
static std::vector<int> exact_group_order(const int *query_group, int n_groups, const std::vector<int> &round_end)
{
    const size_t G = (size_t)n_groups;
    std::vector<int> order((size_t)(round_end.empty() ? 0 : round_end.back())), at(G + 1);
    int r0 = 0;
    for (const int r1 : round_end) {
        std::fill(at.begin(), at.end(), 0);
        for (int i = r0; i < r1; ++i) at[(size_t)query_group[i] + 1] += 1;
        for (size_t g = 0; g < G; ++g) at[g + 1] += at[g];
        for (int i = r0; i < r1; ++i) order[(size_t)r0 + (size_t)at[(size_t)query_group[i]]++] = i;
        r0 = r1;
    }
    return order;
}

// What a grouped flat scan knows once exact_grouped_begin is through.  A group is scanned when it has a query and a member.
struct ExactGroupedCall {
    std::vector<int> gq, cnt, goff;   // per group: queries of the call, members, where its segment starts in x_ids_
    long long n = 0;                  // ids that exist and have a group
    int max_gq = 0;                   // the most queries of a scanned group
    uint64_t scanned = 0, listed = 0; // scanned groups; ids that are in a group
    ExactPlan tp{};                   // the tile (one for the call: the LDS layout is the launch's); chunks are planned per group
};

// The arguments, group lists and tile of a grouped flat scan.  args_ok: the caller's check of the arguments that are its own; k: the
// keys a list keeps (0: the sink keeps none, and the tile is planned as for lists of one key).  Nothing to measure: no id exists
// and has a group (before anything touches the device), or no group has both a query and a member.  The stream is idle and the
// pinned stage free when this returns.
ExactStart Device::exact_grouped_begin(const char *who, bool args_ok, const float *queries, int nq, long long n_rows, int k, const int *row_group,
                                       long long n_row_group, const int *query_group, int n_groups, ExactGroupedCall *gc)
{
    const auto fail = [&](const std::string &what) { set_dev_error(std::string(who) + ": " + what); return ExactStart::failed; };
    if (!args_ok) return fail("bad argument");
    if (!row_group || n_row_group < 0) return fail("row_group must not be NULL and n_row_group must be >= 0");
    if (!query_group) return fail("query_group must not be NULL");
    if (k > kExactMaxK) return fail("k = " + std::to_string(k) + " is above the limit of " + std::to_string(kExactMaxK));
    if (!group_args_ok(who, query_group, nq, n_groups)) return ExactStart::failed;
    gc->gq.assign((size_t)n_groups, 0);
    for (int i = 0; i < nq; ++i) gc->gq[(size_t)query_group[i]] += 1;
    // ids that exist and have a group: a row beyond what was uploaded is never dereferenced, whatever n_rows and n_row_group say
    gc->n = std::min({n_rows, n_rows_hw_, n_row_group});
    if (gc->n <= 0) return ExactStart::nothing;
    if (!queries && (nq > n_queries_ || tail_.n > 0)) return fail("queries == NULL needs a resident query set of at least nq rows (hnswdev_set_queries)");
    if (!bind() || !exact_group_lists(who, row_group, gc->n, n_groups, gc->cnt, gc->goff, &gc->listed)) return ExactStart::failed;
    if (!exact_grouped_plan(who, k, gc)) return ExactStart::failed;
    return gc->scanned == 0 ? ExactStart::nothing : ExactStart::ready;
}

// The groups a grouped flat scan measures -- those with a query (gq) and a member (cnt) -- counted in gc->scanned, and the call's
// tile planned for the most queries any of them has.  false: the tile does not fit LDS.
bool Device::exact_grouped_plan(const char *who, int k, ExactGroupedCall *gc)
{
    gc->max_gq = 0;
    gc->scanned = 0;
    for (size_t g = 0; g < gc->gq.size(); ++g)
        if (gc->gq[g] > 0 && gc->cnt[g] > 0) { gc->max_gq = std::max(gc->max_gq, gc->gq[g]); gc->scanned += 1; }
    if (gc->scanned == 0) return true;
    gc->tp = exact_plan(gc->max_gq, 1, std::max(k, 1), pitch_, num_cu_);
    gc->tp.lds = exact_scan_lds(gc->tp.qtile, gc->tp.piece, pitch_, k);
    if (gc->tp.lds > 64 * 1024) { set_dev_error(std::string(who) + ": tile exceeds the LDS budget"); return false; }
    return true;
}

// The queries of the round at sorted positions [off, off + nr) of `order`, a run of one group's queries at a time, each run cut
// into tiles of qt: f(g, t, tn) for the tile of queries [t, t + tn) of the round, all of group g, in ascending t.
template <class F>
static void exact_for_each_tile(const int *query_group, const std::vector<int> &order, int off, int nr, int qt, F &&f)
{
    for (int p = 0; p < nr;) {
        const int g = query_group[order[(size_t)(off + p)]];
        int e = p + 1;
        while (e < nr && query_group[order[(size_t)(off + e)]] == g) ++e;
        for (int t = p; t < e; t += qt) f(g, t, std::min(qt, e - t));
        p = e;
    }
}

// A tile x each of the nch chunks of its group's list (m entries from entry `first` of x_ids_ on, `chunk` per chunk) is an
// ExactWorkItem; list0: the tile's first list (top-k sinks).
static void exact_tile_items(std::vector<ExactWorkItem> &wi, int t, int tn, int first, int m, int chunk, int nch, long long list0)
{
    for (int c = 0; c < nch; ++c) {
        const int lo = c * chunk; // (chunk * nch < m + chunk: no overflow of int while m is one)
        wi.push_back(ExactWorkItem{t, tn, first + lo, std::min(chunk, m - lo), list0, nch, c});
    }
}

// ---- hnswdev_exact_knn_grouped: a candidate group per query, every group scanned in one launch --------
// The groups' id lists are a CSR in x_ids_, built on the device from row_group; the counts come back in one copy.  The queries are
// uploaded sorted by group (stable), so a group's queries are a run that is cut into tiles, and its list into chunks: a scan block
// is one (tile, chunk) pair read from a table.  Chunks: the (tile, row) work of the call spread over about two blocks per CU, no
// chunk shorter than 1 024 rows, at most 4 096 per group -- a large group gets more chunks than a small one; `exact_chunk` forces
// the rows per chunk and `exact_qtile` the tile for every group.  Rounds are ranges of the CALLER's order (at most 1 GiB of lists
// and 2^24 output entries each); the sort is inside a round, so a round's results are rows [off, off + nr) of the output.
bool Device::exact_knn_grouped(const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group, const int *query_group,
                               int n_groups, int *out_ids, float *out_d)
{
    if (nq <= 0) return true;
    ExactGroupedCall gc;
    const ExactStart s = exact_grouped_begin("exact_knn_grouped", out_ids && out_d && k >= 1 && n_rows >= 0, queries, nq, n_rows, k, row_group, n_row_group,
                                             query_group, n_groups, &gc);
    if (s == ExactStart::nothing) pad_results(out_ids, out_d, (size_t)nq * (size_t)k); // no query has a candidate: padding, no scan
    if (s != ExactStart::ready) return s == ExactStart::nothing;
    uint64_t blocks = 0;
    if (!exact_knn_grouped_scan("exact_knn_grouped", queries, nullptr, nq, k, query_group, n_groups, gc, out_ids, out_d, &blocks)) return false;
    using Slot = slot::exact_grouped_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    if (blocks) { ctr[Slot::calls] += 1; ctr[Slot::groups_scanned] += gc.scanned; ctr[Slot::scan_blocks] += blocks; ctr[Slot::ids_listed] += gc.listed; } // (a call that scans nothing counts nowhere)
    return true;
}

// A grouped top-k scan once the groups' lists stand in x_ids_ (gc: per group its queries, members and segment; the tile): chunks,
// rounds, the sorted upload, work items, scan and merge -- what exact_knn_grouped and every batch of exact_knn_tagged run.  The nq
// queries are `queries`, or (nullptr) the resident queries resident[0 .. nq) (nullptr: 0 .. nq - 1); query_group[i] names query i's
// list.  *blocks: the scan blocks launched, 0 when no query has a candidate (every row is padded).
bool Device::exact_knn_grouped_scan(const char *who, const float *queries, const int *resident, int nq, int k, const int *query_group, int n_groups,
                                    const ExactGroupedCall &gc, int *out_ids, float *out_d, uint64_t *blocks)
{
    hipStream_t st = S(stream_);
    const ExactPlan &tp = gc.tp;
    const int qt = tp.qtile;
    std::vector<int> gchunk, gnch; // each scanned group's chunks: rows per chunk, chunks (0: not scanned)
    exact_group_chunks(gc.gq, gc.cnt, qt, num_cu_, gchunk, gnch);

    // rounds: ranges of the caller's order within both budgets; inside each the queries sorted by group (counting sort: stable)
    const long long lists_cap = (1LL << 30) / ((long long)k * 8), out_cap = std::max<long long>(1, (1LL << 24) / k);
    std::vector<int> round_end; // one past the last query of each round
    {
        long long lists = 0, rows = 0;
        for (int i = 0; i < nq; ++i) {
            const long long c = gnch[(size_t)query_group[i]];
            if (rows > 0 && (lists + c > lists_cap || rows + 1 > out_cap)) { round_end.push_back(i); lists = 0; rows = 0; }
            lists += c; rows += 1;
        }
        round_end.push_back(nq);
    }
    const std::vector<int> order = exact_group_order(query_group, n_groups, round_end);

    const float *d_q;
    const double *d_qsn;
    if (!exact_sorted_queries(who, queries, nq, order, &d_q, &d_qsn, resident)) return false;

    std::vector<ExactMergeItem> mi;
    std::vector<ExactWorkItem> wi;
    *blocks = 0;
    int off = 0;
    for (const int r1 : round_end) {
        const int nr = r1 - off;
        // the round's tables: a query's lists follow those of the queries before it in the sorted order
        mi.resize((size_t)nr);
        wi.clear();
        long long lists = 0;
        exact_for_each_tile(query_group, order, off, nr, qt, [&](int g, int t, int tn) {
            const int nch = gnch[(size_t)g];
            for (int j = t; j < t + tn; ++j) mi[(size_t)j] = ExactMergeItem{lists + (long long)(j - t) * nch, nch, order[(size_t)(off + j)] - off};
            exact_tile_items(wi, t, tn, gc.goff[(size_t)g], gc.cnt[(size_t)g], gchunk[(size_t)g], nch, lists);
            lists += (long long)tn * nch;
        });
        const size_t res = 4u * (size_t)nr * k, b_mi = sizeof(ExactMergeItem) * (size_t)nr, b_wi = sizeof(ExactWorkItem) * wi.size();
        if (wi.empty()) { // no query of this round has a candidate
            pad_results(out_ids + (size_t)off * k, out_d + (size_t)off * k, (size_t)nr * (size_t)k);
            off = r1;
            continue;
        }
        char *hs = static_cast<char *>(pinned_stage(2 * res + 8 + b_mi + b_wi));
        if (!hs || !x_out_.grow(2 * (size_t)nr * k) || !x_lists_.grow((size_t)lists * k) || !x_gwork_.grow(b_mi + b_wi)) return false;
        int *d_ids = x_out_;
        float *d_d = reinterpret_cast<float *>(x_out_.get() + (size_t)nr * k);
        unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs + 2 * res);
        char *h_tab = hs + 2 * res + 8;
        memcpy(h_tab, mi.data(), b_mi);
        memcpy(h_tab + b_mi, wi.data(), b_wi);
        HIP_OK(hipMemcpyAsync(x_gwork_, h_tab, b_mi + b_wi, hipMemcpyHostToDevice, st));
        ExactScanArgs a;
        if (!exact_scan_args(d_q, d_qsn, off, nr, qt, tp.piece, &a)) return false;
        a.ids = x_ids_; a.k = k; a.lists = x_lists_;
        ExactTopKGrouped sink;
        sink.items = reinterpret_cast<const ExactWorkItem *>(x_gwork_.get() + b_mi);
        const auto enqueue = [&]() -> bool {
            hipError_t e = hipSuccess;
            with_metric(metric_, [&](auto mt) { e = exact_grouped_scan_launch<mt>(a, sink, (unsigned)wi.size(), tp.lds, st); });
            HIP_OK(e);
            HIP_OK(exact_merge_grouped_launch(x_lists_, reinterpret_cast<const ExactMergeItem *>(x_gwork_.get()), k, nr, d_ids, d_d, st));
            return true;
        };
        const auto fetch = [&]() -> bool {
            HIP_OK(hipMemcpyAsync(hs, d_ids, res, hipMemcpyDeviceToHost, st));
            HIP_OK(hipMemcpyAsync(hs + res, d_d, res, hipMemcpyDeviceToHost, st));
            return true;
        };
        if (!exact_timed_scan(h_ev, enqueue, fetch)) return false;
        memcpy(out_ids + (size_t)off * k, hs, res);
        memcpy(out_d + (size_t)off * k, hs + res, res);
        *blocks += wi.size();
        off = r1;
    }
    return true;
}

// ---- hnswdev_exact_knn_tagged: a tag mask per query, every distinct mask a candidate list ------------------
// The lists overlap -- a row is in the list of every mask it matches -- so together they can hold D x n ids, and an ExactWorkItem
// addresses x_ids_ with an int.  The distinct masks are therefore taken in batches, in the order they first appear, whose counts
// (tag_counts) sum to at most kTagListEntries (`tag_list_cap` lowers it); a mask with more is a batch alone, and fits because
// n < 2^31.  Per batch dk_tag_lists.h builds the CSR in x_ids_ and exact_knn_grouped_scan answers the queries of the batch's masks;
// with more than one batch their rows go through arrays of the batch's size and are scattered to the caller's order.
//
// The batches of masks of a tagged flat scan, walked: the candidates of every distinct mask counted (tag_counts, into cnt); then, for
// each batch of masks that holds a candidate, the ExactGroupedCall of its lists (k: the keys a list keeps, as exact_grouped_plan
// takes it), the lists built in x_ids_ (timed into xt_list_ms_ while profiling is on), and on_batch(gc, bq, resident, sel, qg) for
// the batch's queries -- those of its masks that have a candidate, sel[j] their places in the caller's order and qg[j] their
// lists: bq / resident name them as the grouped scans take queries, the caller's own when the batch is the whole call, a gathered
// copy otherwise.  info: the caller's counter block, exact_tagged_info or exact_range_tagged_info -- the six slots a tagged scan
// leads with are added to when every batch went through.
template <class OnBatch>
bool Device::exact_tag_batches(const char *who, const float *queries, int nq, long long n, int k, const uint32_t *row_tags, const TagCall &tc, int match,
                               std::vector<int> &cnt, uint64_t *info, OnBatch &&on_batch)
{
    if (!queries && (nq > n_queries_ || tail_.n > 0)) {
        set_dev_error(std::string(who) + ": queries == NULL needs a resident query set of at least nq rows (hnswdev_set_queries)");
        return false;
    }
    const int D = (int)tc.masks.size();
    if (!bind() || !tag_counts(row_tags, n, tc.masks, match, cnt)) return false;
    hipStream_t st = S(stream_);
    const long long forced = diag("tag_list_cap", 0), cap = forced > 0 ? forced : kTagListEntries;
    std::vector<int> gq((size_t)D, 0);
    for (int i = 0; i < nq; ++i) gq[(size_t)tc.of[(size_t)i]] += 1;
    uint64_t scanned_q = 0, listed = 0, batches = 0;
    std::vector<int> sel, qg;
    std::vector<float> t_q;
    for (int d0 = 0; d0 < D;) {
        // the batch: masks d0 .. d1 - 1, `sum` entries
        long long sum = cnt[(size_t)d0];
        int d1 = d0 + 1;
        while (d1 < D && sum + cnt[(size_t)d1] <= cap) sum += cnt[(size_t)d1++];
        if (sum == 0) { d0 = d1; continue; } // (no mask of it has a candidate: its queries are left to the caller)
        ExactGroupedCall gc;
        gc.gq.assign((size_t)D, 0);
        gc.cnt.assign((size_t)D, 0);
        gc.goff.assign((size_t)D, 0);
        gc.n = n;
        gc.listed = (uint64_t)sum;
        long long at = 0;
        for (int d = d0; d < d1; ++d) { gc.gq[(size_t)d] = gq[(size_t)d]; gc.cnt[(size_t)d] = cnt[(size_t)d]; gc.goff[(size_t)d] = (int)at; at += cnt[(size_t)d]; }
        if (!exact_grouped_plan(who, k, &gc)) return false;
        if (!x_ids_.grow((size_t)sum)) return false;
        const bool timed = profiling_;
        if (timed && (!ev0_.create(true) || !ev1_.create(true))) return false;
        if (timed) HIP_OK(hipEventRecord(E(ev0_), st));
        HIP_OK(tag_lists_launch(s_ttags_, n, s_tmask_.get() + d0, d1 - d0, match, s_tcnt_.get() + d0, s_tcnt_.get() + D + d0, s_tcnt_.get() + 2 * (size_t)D + d0,
                                x_ids_, sum, st));
        if (timed) {
            HIP_OK(hipEventRecord(E(ev1_), st));
            HIP_OK(hipStreamSynchronize(st)); // (the scan records the same pair of events)
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, E(ev0_), E(ev1_)));
            xt_list_ms_ += ms;
        }
        // the batch's queries: those of its masks that have a candidate, in the caller's order
        sel.clear();
        qg.clear();
        for (int i = 0; i < nq; ++i) {
            const int d = tc.of[(size_t)i];
            if (d >= d0 && d < d1 && cnt[(size_t)d] > 0) { sel.push_back(i); qg.push_back(d); }
        }
        const int nb = (int)sel.size();
        const bool gathered = nb != nq && queries; // (resident queries are named by sel instead)
        if (gathered) {
            t_q.resize((size_t)nb * (size_t)dim_);
            for (int j = 0; j < nb; ++j) memcpy(&t_q[(size_t)j * dim_], queries + (size_t)sel[(size_t)j] * dim_, sizeof(float) * (size_t)dim_);
        }
        if (!on_batch(gc, gathered ? t_q.data() : queries, nb == nq || queries ? nullptr : sel.data(), sel, qg.data())) return false;
        scanned_q += (uint64_t)nb;
        listed += (uint64_t)sum;
        batches += 1;
        d0 = d1;
    }
    using Slot = slot::exact_tagged_info; // (exact_range_tagged_info leads with the same six: counter_blocks.h asserts it)
    info[Slot::calls] += 1; info[Slot::masks] += (uint64_t)D; info[Slot::scanned] += scanned_q; info[Slot::skipped] += (uint64_t)nq - scanned_q;
    info[Slot::ids_listed] += listed; info[Slot::batches] += batches;
    return true;
}

// exact_knn_tagged: every batch one grouped top-k scan.
bool Device::exact_knn_tagged(const float *queries, int nq, long long n_rows, int k, const uint32_t *row_tags, long long n_row_tags, const uint32_t *query_tags,
                              int match, int *out_ids, float *out_d)
{
    if (nq <= 0) return true;
    const char *who = "exact_knn_tagged";
    const auto fail = [&](const std::string &what) { set_dev_error(std::string(who) + ": " + what); return false; };
    if (!(out_ids && out_d && k >= 1 && n_rows >= 0)) return fail("bad argument");
    if (!row_tags || n_row_tags < 0) return fail("row_tags must not be NULL and n_row_tags must be >= 0");
    if (!query_tags) return fail("query_tags must not be NULL");
    if (k > kExactMaxK) return fail("k = " + std::to_string(k) + " is above the limit of " + std::to_string(kExactMaxK));
    TagCall tc;
    if (!tag_args_ok(who, query_tags, nq, match, &tc)) return false;
    // ids that exist and have a word: a row beyond what was uploaded is never dereferenced, whatever n_rows and n_row_tags say
    const long long n = std::min({n_rows, n_rows_hw_, n_row_tags});
    if (n <= 0) { pad_results(out_ids, out_d, (size_t)nq * (size_t)k); return true; }
    const int D = (int)tc.masks.size();
    std::vector<int> cnt, t_ids;
    std::vector<float> t_d;
    const bool ok = exact_tag_batches(who, queries, nq, n, k, row_tags, tc, match, cnt, counter_block(CounterBlock::exact_tagged_info), [&](const ExactGroupedCall &gc, const float *bq, const int *resident, const std::vector<int> &sel, const int *qg) {
        const int nb = (int)sel.size();
        uint64_t blocks = 0;
        if (nb == nq) return exact_knn_grouped_scan(who, bq, resident, nq, k, qg, D, gc, out_ids, out_d, &blocks); // straight into the caller's arrays
        t_ids.resize((size_t)nb * k);
        t_d.resize((size_t)nb * k);
        if (!exact_knn_grouped_scan(who, bq, resident, nb, k, qg, D, gc, t_ids.data(), t_d.data(), &blocks)) return false;
        for (int j = 0; j < nb; ++j) {
            memcpy(out_ids + (size_t)sel[(size_t)j] * k, &t_ids[(size_t)j * k], 4u * (size_t)k);
            memcpy(out_d + (size_t)sel[(size_t)j] * k, &t_d[(size_t)j * k], 4u * (size_t)k);
        }
        return true;
    });
    if (!ok) return false;
    for (int i = 0; i < nq; ++i) // a mask without a candidate: padding, no scan
        if (cnt[(size_t)tc.of[(size_t)i]] == 0) pad_results(out_ids + (size_t)i * k, out_d + (size_t)i * k, (size_t)k);
    return true;
}

// ---- hnswdev_exact_range: the same scan with the range sink -------------------------------------------
// Pass A scans a round of queries with one capacity for each (the arena's entries / the round's queries, or less: the picker
// stops at kExactRangePickCap, `exact_range_cap` forces it).  The counts come back exact; where one exceeds its capacity the round
// is cut into pieces whose counts fit the arena and each piece is scanned again with segments of exactly its counts (pass B).
// Lists of up to `exact_range_sort` (4096) keys are ordered by exact_range_sort_kernel, longer ones cross as keys and are ordered
// here: the keys are unique, so the order is the same.
constexpr long long kExactRangeArena = 1LL << 27;  // keys: 1 GiB
constexpr long long kExactRangePickCap = 8192;     // pass A's capacity per query unless forced (unmeasured: DESIGN.md 3.16)
constexpr size_t kExactRangePiece = 1u << 21;      // entries per copy through the pinned stage

static inline float exact_host_key_dist(unsigned long long key) // exact_key_dist (dk_exact.h) on the host
{
    const uint32_t dk = (uint32_t)(key >> 32), u = dk == 0xffffffffu ? 0x7fc00000u : (dk & 0x80000000u) ? (dk & 0x7fffffffu) : ~dk;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// device -> host through the pinned stage, in pieces
bool Device::exact_copy_out(void *dst, const void *src, size_t bytes)
{
    hipStream_t st = S(stream_);
    const size_t piece = kExactRangePiece * 8;
    for (size_t o = 0; o < bytes; o += piece) {
        const size_t n = std::min(piece, bytes - o);
        void *hs = pinned_stage(n);
        if (!hs) return false;
        HIP_OK(hipMemcpyAsync(hs, static_cast<const char *>(src) + o, n, hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        memcpy(static_cast<char *>(dst) + o, hs, n);
    }
    return true;
}

// What both range calls bring to their lists: the three knobs, read here and nowhere else, and exact_range_finish's scratch.
struct ExactRangeWork {
    long long arena_max; // keys of a round's arena (`exact_range_arena` forces it)
    long long pick;      // pass A's capacity per query, where the candidates and the arena allow as much (`exact_range_cap` forces it)
    int sort_max;        // the longest list exact_range_sort_kernel orders (`exact_range_sort` lowers it)
    std::vector<long long> ooff; // per segment: where its list goes among those ordered on the device
    std::vector<unsigned long long> keys;
    std::vector<int> t_ids;
    std::vector<float> t_d;
    ExactRangeWork()
    {
        const int d_arena = diag("exact_range_arena", 0), d_cap = diag("exact_range_cap", 0), d_sort = diag("exact_range_sort", 0);
        arena_max = d_arena > 0 ? d_arena : kExactRangeArena;
        pick = d_cap > 0 ? (long long)d_cap : kExactRangePickCap;
        sort_max = d_sort > 0 ? std::min(d_sort, kExactRangeSortMax) : kExactRangeSortMax;
    }
};

// A range call around its `body`: the results of the call before are dropped first, and a failed call keeps nothing -- no
// results, every count 0 where the caller gave counts.
bool Device::exact_range_call(int nq, int *out_counts, const std::function<bool()> &body)
{
    xr_ids_.clear();
    xr_d_.clear();
    if (body()) return true;
    xr_ids_.clear();
    xr_d_.clear();
    for (int i = 0; out_counts && i < nq; ++i) out_counts[i] = 0;
    return false;
}

// The lists of segments [0, ns) of the arena, c[s] keys each (0: nothing to do for that segment), every one inside its segment,
// which starts at seg[s]: ordered and written to the call's results, which have room for them.  Segment s is query sq[s] of the
// round (nullptr: s itself), and that query's list starts at xr_ids_[base + obase[query]].  counts_on_device: x_rcnt_ holds c[]
// as the scan left it; otherwise c[] goes up first -- the kernel orders what counts[] says, so the segments that are not to be
// read get 0.  *by_device: lists of two or more keys that exact_range_sort_kernel ordered; *by_host: lists ordered here.  The
// stream is idle and the pinned stage free when this returns.
bool Device::exact_range_finish(ExactRangeWork &w, int ns, const unsigned *c, const long long *seg, const int *sq, const long long *obase, size_t base,
                                bool counts_on_device, uint64_t *by_device, uint64_t *by_host)
{
    hipStream_t st = S(stream_);
    size_t on_dev = 0;
    int n_dev = 0;
    w.ooff.resize((size_t)ns);
    for (int s = 0; s < ns; ++s) {
        w.ooff[(size_t)s] = (long long)on_dev;
        if (c[s] > 0 && c[s] <= (unsigned)w.sort_max) { on_dev += c[s]; ++n_dev; }
    }
    if (n_dev > 0) {
        if (!x_rout_.grow(2 * on_dev)) return false;
        char *hs = static_cast<char *>(pinned_stage(12 * (size_t)ns));
        if (!hs) return false;
        memcpy(hs, w.ooff.data(), 8 * (size_t)ns);
        HIP_OK(hipMemcpyAsync(x_rooff_, hs, 8 * (size_t)ns, hipMemcpyHostToDevice, st));
        if (!counts_on_device) {
            memcpy(hs + 8 * (size_t)ns, c, 4 * (size_t)ns);
            HIP_OK(hipMemcpyAsync(x_rcnt_, hs + 8 * (size_t)ns, 4 * (size_t)ns, hipMemcpyHostToDevice, st));
        }
        ExactRangeSortArgs sa;
        sa.arena = x_rarena_; sa.seg_off = x_rseg_; sa.counts = x_rcnt_; sa.out_off = x_rooff_;
        sa.out_ids = x_rout_; sa.out_d = reinterpret_cast<float *>(x_rout_.get() + on_dev); sa.sort_max = w.sort_max;
        HIP_OK(exact_range_sort_launch(sa, ns, st));
        HIP_OK(hipStreamSynchronize(st)); // (the pinned stage is used again by the copies)
        w.t_ids.resize(on_dev);
        w.t_d.resize(on_dev);
        if (!exact_copy_out(w.t_ids.data(), sa.out_ids, 4 * on_dev) || !exact_copy_out(w.t_d.data(), sa.out_d, 4 * on_dev)) return false;
    }
    for (int s = 0; s < ns; ++s) {
        const size_t cs = c[s], at = base + (size_t)obase[(size_t)(sq ? sq[s] : s)];
        if (cs > 0 && cs <= (size_t)w.sort_max) {
            memcpy(xr_ids_.data() + at, w.t_ids.data() + w.ooff[(size_t)s], 4 * cs);
            memcpy(xr_d_.data() + at, w.t_d.data() + w.ooff[(size_t)s], 4 * cs);
            if (cs >= 2) *by_device += 1;
        } else if (cs > 0) { // longer than the kernel orders: the keys cross and are ordered here (they are unique: the same order)
            w.keys.resize(cs);
            if (!exact_copy_out(w.keys.data(), x_rarena_.get() + seg[(size_t)s], 8 * cs)) return false;
            std::sort(w.keys.begin(), w.keys.end());
            for (size_t j = 0; j < cs; ++j) { xr_ids_[at + j] = (int)(uint32_t)w.keys[j]; xr_d_[at + j] = exact_host_key_dist(w.keys[j]); }
            *by_host += 1;
        }
    }
    return true;
}

// Pass B's next piece: as many of the counts c[s0 .. n) -- exact: pass A's -- as fit the arena together, with segments of
// exactly those counts in seg[0 .. *s1 - s0].  A count that the arena cannot hold alone fails the call.
static bool exact_range_piece(const char *who, const unsigned *c, size_t n, size_t s0, long long arena_max, std::vector<long long> &seg, size_t *s1)
{
    size_t s = s0;
    seg[0] = 0;
    for (; s < n && seg[s - s0] + (long long)c[s] <= arena_max; ++s) seg[s - s0 + 1] = seg[s - s0] + (long long)c[s];
    *s1 = s;
    if (s > s0) return true;
    set_dev_error(std::string(who) + ": a query has " + std::to_string(c[s0]) + " results within the range, above the arena's limit of " +
                  std::to_string(arena_max) + " entries per call round");
    return false;
}

// ... and what its scan counted against pass A's counts of the same n segments: the segments were cut to these, so they must agree
static bool exact_range_recount_ok(const char *who, const unsigned *again, const unsigned *first, size_t n)
{
    if (std::equal(again, again + n, first)) return true;
    set_dev_error(std::string(who) + ": the repeated scan counted differently");
    return false;
}

bool Device::exact_range(const float *queries, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_counts)
{
    return exact_range_call(nq, out_counts, [&]() -> bool {
        if (nq <= 0) return true;
        if (!out_counts || n_rows < 0 || (allow_bits && nbits < 0)) { set_dev_error("exact_range: bad argument"); return false; }
        for (int i = 0; i < nq; ++i) out_counts[i] = 0;
        ExactScanInput in;
        const ExactStart s = exact_scan_begin("exact_range", queries, nq, n_rows, allow_bits, nbits, &in);
        if (s != ExactStart::ready) return s == ExactStart::nothing; // (nothing to measure: empty lists, no launch)
        return exact_range_rounds("exact_range", in, nq, range, nullptr, out_counts);
    });
}

// The rounds of a range scan over the queries and the id list of `in`: pass A, the finish and pass B, the lists appended to the
// call's results in query order and counted in exact_range_info.  d_self: nullptr, or the nq ids on the device whose stored rows
// the queries are (exact_range_by_id) -- the sink is then ExactRangeSelf, and every launch gets the ids of ITS queries: a repeated
// pass scans queries [q0, q0 + ns) of the call and reads d_self + q0, as it reads the queries from q0 on.  Runs inside
// exact_range_call's body.
bool Device::exact_range_rounds(const char *who, const ExactScanInput &in, int nq, float range, const int *d_self, int *out_counts)
{
    hipStream_t st = S(stream_);
    ExactPlan p = exact_plan(std::min(nq, 65536), in.m, 1, pitch_, num_cu_); // tile and chunks as for lists of one key: this sink keeps none
    p.lds = exact_scan_lds(p.qtile, p.piece, pitch_, 0);
    if (p.lds > 64 * 1024) { set_dev_error(std::string(who) + ": tile exceeds the LDS budget"); return false; }
    ExactRangeWork w;
    const long long cap = std::min<long long>({w.pick, in.m, w.arena_max});
    const long long round = std::max<long long>(1, std::min<long long>({(long long)nq, 65536LL, w.arena_max / cap}));
    if (!x_rcnt_.grow((size_t)round) || !x_rseg_.grow((size_t)round + 1) || !x_rooff_.grow((size_t)round)) return false;
    std::vector<long long> seg((size_t)round + 1), obase((size_t)round);
    std::vector<unsigned> cnt((size_t)round), cnt_b;

    // one scan of queries [q0, q0 + nr) with the segments seg[0 .. nr]: the counts into c[0 .. nr)
    const auto scan = [&](long long q0, int nr, unsigned *c) -> bool {
        if (!x_rarena_.grow((size_t)std::max<long long>(seg[(size_t)nr], 1))) return false;
        char *hs = static_cast<char *>(pinned_stage(8 * ((size_t)nr + 1) + 4 * (size_t)nr + 8));
        if (!hs) return false;
        unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs);
        long long *h_seg = reinterpret_cast<long long *>(hs + 8);
        unsigned *h_cnt = reinterpret_cast<unsigned *>(hs + 8 + 8 * ((size_t)nr + 1));
        memcpy(h_seg, seg.data(), 8 * ((size_t)nr + 1));
        ExactScanArgs a;
        if (!exact_scan_args(in.d_q, in.d_qsn, q0, nr, p.qtile, p.piece, &a)) return false;
        a.ids = in.ids; a.m = in.m; a.chunk = p.chunk; a.n_chunks = p.n_chunks;
        ExactRange sink;
        sink.range = range; sink.counts = x_rcnt_; sink.seg_off = x_rseg_; sink.arena = x_rarena_;
        const unsigned tiles = (unsigned)((nr + p.qtile - 1) / p.qtile);
        HIP_OK(hipMemcpyAsync(x_rseg_, h_seg, 8 * ((size_t)nr + 1), hipMemcpyHostToDevice, st));
        HIP_OK(hipMemsetAsync(x_rcnt_, 0, 4 * (size_t)nr, st));
        const auto enqueue = [&]() -> bool {
            hipError_t e = hipSuccess;
            if (d_self) {
                const ExactRangeSelf own{range, sink.counts, sink.seg_off, sink.arena, d_self + q0};
                with_metric(metric_, [&](auto mt) { e = exact_range_self_scan_launch<mt>(a, own, tiles, p.lds, st); });
            } else with_metric(metric_, [&](auto mt) { e = exact_range_scan_launch<mt>(a, sink, tiles, p.lds, st); });
            HIP_OK(e);
            return true;
        };
        const auto fetch = [&]() -> bool { HIP_OK(hipMemcpyAsync(h_cnt, x_rcnt_, 4 * (size_t)nr, hipMemcpyDeviceToHost, st)); return true; };
        if (!exact_timed_scan(h_ev, enqueue, fetch)) return false;
        memcpy(c, h_cnt, 4 * (size_t)nr);
        return true;
    };

    // the lists of queries [q0, q0 + nr), every one inside its segment seg[i] .. : ordered and appended to the call's results
    using Slot = slot::exact_range_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    const auto finish = [&](long long q0, int nr, const unsigned *c) -> bool {
        size_t total = 0;
        for (int i = 0; i < nr; ++i) {
            obase[(size_t)i] = (long long)total;
            total += c[i];
            out_counts[q0 + i] = (int)c[i];
        }
        const size_t base = xr_ids_.size();
        xr_ids_.resize(base + total);
        xr_d_.resize(base + total);
        if (!exact_range_finish(w, nr, c, seg.data(), nullptr, obase.data(), base, true, &ctr[Slot::device_sorted], &ctr[Slot::host_sorted])) return false;
        ctr[Slot::results] += total;
        return true;
    };

    for (long long off = 0; off < nq; off += round) {
        const int nr = (int)std::min<long long>(round, nq - off);
        for (int i = 0; i <= nr; ++i) seg[(size_t)i] = (long long)i * cap;
        if (!scan(off, nr, cnt.data())) return false;
        bool fits = true;
        for (int i = 0; i < nr; ++i) fits = fits && cnt[(size_t)i] <= (unsigned long long)cap;
        if (fits) {
            if (!finish(off, nr, cnt.data())) return false;
            continue;
        }
        // pass B: pieces of the round whose exact counts fit the arena, each with segments of exactly its counts
        cnt_b.resize((size_t)nr);
        for (size_t s0 = 0, s1; s0 < (size_t)nr; s0 = s1) {
            if (!exact_range_piece(who, cnt.data(), (size_t)nr, s0, w.arena_max, seg, &s1)) return false;
            ctr[Slot::repeated_rounds] += 1;
            const int ns = (int)(s1 - s0);
            if (!scan(off + (long long)s0, ns, cnt_b.data()) || !exact_range_recount_ok(who, cnt_b.data(), cnt.data() + s0, (size_t)ns)) return false;
            if (!finish(off + (long long)s0, ns, cnt_b.data())) return false;
        }
    }
    return true;
}

// ---- hnswdev_exact_range_grouped: the range sink behind exact_knn_grouped's work items ------------------
// Group lists, tile, chunks and the sorted upload are exact_knn_grouped's; capacities, the two passes, the sort limit and the host
// sort are exact_range's.  The scan writes to segments in the CALLER's order (ExactRangeGrouped::dest), so counts, segments and
// exact_range_sort_kernel's output need no permutation.  A query's pass-A capacity is min(the picker's, its group's members, the
// arena): a round is a range of the caller's order whose capacities fit the arena.  The counts of pass A are exact, so a round's
// output places are known after it; the lists that fitted are finished from pass A's arena and only the tiles that hold a query
// whose count exceeded its capacity are scanned again (pass B), in pieces whose exact counts fit the arena.
bool Device::exact_range_grouped(const float *queries, int nq, long long n_rows, float range, const int *row_group, long long n_row_group,
                                 const int *query_group, int n_groups, int *out_counts)
{
    return exact_range_call(nq, out_counts, [&]() -> bool {
        if (nq <= 0) return true;
        ExactGroupedCall gc;
        const ExactStart s = exact_grouped_begin("exact_range_grouped", out_counts && n_rows >= 0, queries, nq, n_rows, 0, row_group, n_row_group,
                                                 query_group, n_groups, &gc);
        if (s == ExactStart::failed) return false;
        for (int i = 0; i < nq; ++i) out_counts[i] = 0;
        if (s == ExactStart::nothing) return true; // no query has a candidate: empty lists, no scan
        return exact_range_grouped_scan("exact_range_grouped", queries, nullptr, nq, range, query_group, n_groups, gc, out_counts, counter_block(CounterBlock::exact_range_grouped_info));
    });
}

// A grouped range scan once the groups' lists stand in x_ids_ (gc: per group its queries, members and segment; the tile): rounds,
// the sorted upload, work items, pass A, the finish and pass B -- what exact_range_grouped and every batch of exact_range_tagged
// run.  The nq queries are `queries`, or (nullptr) the resident queries resident[0 .. nq) (nullptr: 0 .. nq - 1); query_group[i]
// names query i's list.  out_counts[0, nq) are written (zeroed by the caller) and the lists APPENDED to xr_ids_ / xr_d_ in the order
// of the nq queries.  info: a block of exact_range_grouped_info's slots, added to -- the context's own, or exact_range_tagged's
// scratch of that shape.
bool Device::exact_range_grouped_scan(const char *who, const float *queries, const int *resident, int nq, float range, const int *query_group, int n_groups,
                                      const ExactGroupedCall &gc, int *out_counts, uint64_t *info)
{
    using Slot = slot::exact_range_grouped_info;
    {
        hipStream_t st = S(stream_);
        const std::vector<int> &cnt = gc.cnt;
        const ExactPlan &tp = gc.tp;
        const int qt = tp.qtile;
        std::vector<int> gchunk((size_t)n_groups, 0), gnch((size_t)n_groups, 0); // each scan's chunks: rows per chunk, chunks per group (planned by `items` below)

        ExactRangeWork w;
        const auto cap_of = [&](int i) { return std::min<long long>({w.pick, (long long)cnt[(size_t)query_group[i]], w.arena_max}); };

        // rounds: ranges of the caller's order whose pass-A capacities fit the arena, at most 65 536 queries each
        std::vector<int> round_end;
        int max_round = 0;
        {
            long long keys = 0;
            int r0 = 0;
            for (int i = 0; i < nq; ++i) {
                const long long c = cap_of(i);
                if (i > r0 && (keys + c > w.arena_max || i - r0 >= 65536)) { round_end.push_back(i); max_round = std::max(max_round, i - r0); keys = 0; r0 = i; }
                keys += c;
            }
            round_end.push_back(nq);
            max_round = std::max(max_round, nq - r0);
        }
        const std::vector<int> order = exact_group_order(query_group, n_groups, round_end);
        const float *d_q;
        const double *d_qsn;
        if (!exact_sorted_queries(who, queries, nq, order, &d_q, &d_qsn, resident)) return false;

        if (!x_rcnt_.grow((size_t)max_round) || !x_rseg_.grow((size_t)max_round + 1) || !x_rooff_.grow((size_t)max_round)) return false;
        std::vector<long long> seg((size_t)max_round + 1), obase((size_t)max_round);
        std::vector<unsigned> cnt_a((size_t)max_round), cnt_b, cnt_fit, cnt_ov;
        std::vector<int> dest((size_t)max_round), slot_q, ov;
        std::vector<ExactWorkItem> wi;
        bool launched = false;

        // the work items of the round at [off, off + nr): every (tile, chunk) of every scanned group whose tile holds a query with a
        // segment in dest.  The chunks are planned for the tiles that are scanned (first the queries of those tiles are counted per
        // group): a repeated pass of a few tiles is cut into many chunks, not left to a few blocks that each walk a whole group.
        const auto tile_wanted = [&](int t, int tn) {
            for (int j = t; j < t + tn; ++j)
                if (dest[(size_t)j] >= 0) return true;
            return false;
        };
        const auto items = [&](int off, int nr) {
            wi.clear();
            std::vector<int> wq(gc.gq.size(), 0); // per group the queries of the wanted tiles (a count of its own: gc.gq stays the call's)
            exact_for_each_tile(query_group, order, off, nr, qt, [&](int g, int t, int tn) {
                if (cnt[(size_t)g] > 0 && tile_wanted(t, tn)) wq[(size_t)g] += tn;
            });
            exact_group_chunks(wq, cnt, qt, num_cu_, gchunk, gnch);
            exact_for_each_tile(query_group, order, off, nr, qt, [&](int g, int t, int tn) {
                if (cnt[(size_t)g] > 0 && tile_wanted(t, tn)) exact_tile_items(wi, t, tn, gc.goff[(size_t)g], cnt[(size_t)g], gchunk[(size_t)g], gnch[(size_t)g], 0);
            });
        };

        // one scan of the round at [off, off + nr) with `ns` segments seg[0 .. ns], dest[0 .. nr) and the work items wi: the counts of
        // the segments into c[0 .. ns)
        const auto scan = [&](int off, int nr, int ns, unsigned *c) -> bool {
            if (!x_rarena_.grow((size_t)std::max<long long>(seg[(size_t)ns], 1))) return false;
            const size_t b_wi = sizeof(ExactWorkItem) * wi.size(), b_dest = 4 * (size_t)nr, b_seg = 8 * ((size_t)ns + 1), b_cnt = 4 * (size_t)ns;
            char *hs = static_cast<char *>(pinned_stage(8 + b_seg + b_wi + b_dest + b_cnt));
            if (!hs || !x_gwork_.grow(b_wi + b_dest)) return false;
            unsigned long long *h_ev = reinterpret_cast<unsigned long long *>(hs);
            char *h_seg = hs + 8, *h_tab = h_seg + b_seg, *h_cnt = h_tab + b_wi + b_dest;
            memcpy(h_seg, seg.data(), b_seg);
            memcpy(h_tab, wi.data(), b_wi);
            memcpy(h_tab + b_wi, dest.data(), b_dest);
            ExactScanArgs a;
            if (!exact_scan_args(d_q, d_qsn, off, nr, qt, tp.piece, &a)) return false;
            a.ids = x_ids_;
            ExactRangeGrouped sink;
            sink.range = range; sink.counts = x_rcnt_; sink.seg_off = x_rseg_; sink.arena = x_rarena_;
            sink.items = reinterpret_cast<const ExactWorkItem *>(x_gwork_.get());
            sink.dest = reinterpret_cast<const int *>(x_gwork_.get() + b_wi);
            HIP_OK(hipMemcpyAsync(x_rseg_, h_seg, b_seg, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemcpyAsync(x_gwork_, h_tab, b_wi + b_dest, hipMemcpyHostToDevice, st));
            HIP_OK(hipMemsetAsync(x_rcnt_, 0, b_cnt, st));
            const auto enqueue = [&]() -> bool {
                hipError_t e = hipSuccess;
                with_metric(metric_, [&](auto mt) { e = exact_range_grouped_scan_launch<mt>(a, sink, (unsigned)wi.size(), tp.lds, st); });
                HIP_OK(e);
                return true;
            };
            const auto fetch = [&]() -> bool { HIP_OK(hipMemcpyAsync(h_cnt, x_rcnt_, b_cnt, hipMemcpyDeviceToHost, st)); return true; };
            if (!exact_timed_scan(h_ev, enqueue, fetch)) return false;
            memcpy(c, h_cnt, b_cnt);
            launched = true;
            return true;
        };

        int off = 0;
        for (const int r1 : round_end) {
            const int nr = r1 - off;
            // pass A: a segment per query at its place in the caller's order
            seg[0] = 0;
            for (int i = 0; i < nr; ++i) seg[(size_t)i + 1] = seg[(size_t)i] + cap_of(off + i);
            for (int p = 0; p < nr; ++p) dest[(size_t)p] = order[(size_t)(off + p)] - off;
            items(off, nr);
            if (wi.empty()) { off = r1; continue; } // no query of this round has a candidate
            if (!scan(off, nr, nr, cnt_a.data())) return false;
            const size_t base = xr_ids_.size();
            size_t total = 0;
            ov.clear();
            cnt_ov.clear();
            cnt_fit.assign(cnt_a.begin(), cnt_a.begin() + nr);
            for (int i = 0; i < nr; ++i) {
                obase[(size_t)i] = (long long)total;
                total += cnt_a[(size_t)i];
                out_counts[off + i] = (int)cnt_a[(size_t)i];
                if ((long long)cnt_a[(size_t)i] > seg[(size_t)i + 1] - seg[(size_t)i]) { ov.push_back(i); cnt_ov.push_back(cnt_a[(size_t)i]); cnt_fit[(size_t)i] = 0; }
            }
            xr_ids_.resize(base + total);
            xr_d_.resize(base + total);
            if (!exact_range_finish(w, nr, cnt_fit.data(), seg.data(), nullptr, obase.data(), base, ov.empty(), &info[Slot::device_sorted], &info[Slot::host_sorted])) return false;
            // pass B: the queries whose count exceeded its capacity (ov, their counts in cnt_ov), in pieces whose exact counts fit the
            // arena, each with segments of exactly its counts; the other queries of their tiles are measured again and their keys dropped
            for (size_t s0 = 0, s1; s0 < ov.size(); s0 = s1) {
                if (!exact_range_piece(who, cnt_ov.data(), ov.size(), s0, w.arena_max, seg, &s1)) return false;
                const int ns = (int)(s1 - s0);
                slot_q.assign((size_t)nr, -1); // query of the round -> its segment in this piece
                for (int s = 0; s < ns; ++s) slot_q[(size_t)ov[s0 + (size_t)s]] = s;
                for (int p = 0; p < nr; ++p) dest[(size_t)p] = slot_q[(size_t)(order[(size_t)(off + p)] - off)];
                items(off, nr);
                info[Slot::repeated_pieces] += 1;
                cnt_b.resize((size_t)ns);
                if (!scan(off, nr, ns, cnt_b.data()) || !exact_range_recount_ok(who, cnt_b.data(), cnt_ov.data() + s0, (size_t)ns)) return false;
                if (!exact_range_finish(w, ns, cnt_b.data(), seg.data(), ov.data() + s0, obase.data(), base, true, &info[Slot::device_sorted], &info[Slot::host_sorted])) return false;
            }
            off = r1;
        }
        if (launched) info[Slot::calls] += 1;
        return true;
    }
}

// ---- hnswdev_exact_range_tagged: a tag mask per query, every distinct mask a candidate list, the range sink ----
// exact_knn_tagged's counts, batches of masks and lists (dk_tag_lists.h); per batch exact_range_grouped_scan answers the queries of
// the batch's masks that have a candidate, in the caller's order among themselves.  A batch appends its lists to xr_ids_ / xr_d_;
// with more than one batch the lists are moved into the caller's query order afterwards (exact_range_results hands them out so).
bool Device::exact_range_tagged(const float *queries, int nq, long long n_rows, float range, const uint32_t *row_tags, long long n_row_tags,
                                const uint32_t *query_tags, int match, int *out_counts)
{
    return exact_range_call(nq, out_counts, [&]() -> bool {
        if (nq <= 0) return true;
        const char *who = "exact_range_tagged";
        const auto fail = [&](const std::string &what) { set_dev_error(std::string(who) + ": " + what); return false; };
        if (!(out_counts && n_rows >= 0)) return fail("bad argument");
        if (!row_tags || n_row_tags < 0) return fail("row_tags must not be NULL and n_row_tags must be >= 0");
        if (!query_tags) return fail("query_tags must not be NULL");
        TagCall tc;
        if (!tag_args_ok(who, query_tags, nq, match, &tc)) return false;
        for (int i = 0; i < nq; ++i) out_counts[i] = 0;
        // ids that exist and have a word: a row beyond what was uploaded is never dereferenced, whatever n_rows and n_row_tags say
        const long long n = std::min({n_rows, n_rows_hw_, n_row_tags});
        if (n <= 0) return true; // no candidate: empty lists, nothing launched
        const int D = (int)tc.masks.size();
        using Slot = slot::exact_range_tagged_info;
        using Scan = slot::exact_range_grouped_info;
        uint64_t *ctr = counter_block(Slot::kBlock);
        uint64_t scan_info[Scan::kCount] = {}; // what the batches' scans count, folded into the call's block below
        int batches = 0;
        std::vector<int> cnt, t_cnt;
        std::vector<size_t> at_of((size_t)nq, 0); // where query i's list starts in xr_ids_ as the batches left it
        const bool ok = exact_tag_batches(who, queries, nq, n, 0, row_tags, tc, match, cnt, ctr, [&](const ExactGroupedCall &gc, const float *bq, const int *resident, const std::vector<int> &sel, const int *qg) {
            const int nb = (int)sel.size();
            size_t o = xr_ids_.size();
            if (nb == nq) { // every query of the call: straight into the caller's counts
                if (!exact_range_grouped_scan(who, bq, resident, nq, range, qg, D, gc, out_counts, scan_info)) return false;
            } else if (nb > 0) {
                t_cnt.assign((size_t)nb, 0);
                if (!exact_range_grouped_scan(who, bq, resident, nb, range, qg, D, gc, t_cnt.data(), scan_info)) return false;
                for (int j = 0; j < nb; ++j) out_counts[sel[(size_t)j]] = t_cnt[(size_t)j];
            }
            for (int j = 0; j < nb; ++j) { at_of[(size_t)sel[(size_t)j]] = o; o += (size_t)out_counts[sel[(size_t)j]]; }
            batches += 1;
            return true;
        });
        if (!ok) return false;
        if (batches > 1) { // the batches' lists, moved into the caller's query order
            std::vector<int> ids(xr_ids_.size());
            std::vector<float> d(xr_d_.size());
            size_t o = 0;
            for (int i = 0; i < nq; ++i) {
                const size_t c = (size_t)out_counts[i];
                if (c) { memcpy(ids.data() + o, xr_ids_.data() + at_of[(size_t)i], 4 * c); memcpy(d.data() + o, xr_d_.data() + at_of[(size_t)i], 4 * c); }
                o += c;
            }
            xr_ids_.swap(ids);
            xr_d_.swap(d);
        }
        ctr[Slot::device_sorted] += scan_info[Scan::device_sorted];
        ctr[Slot::host_sorted] += scan_info[Scan::host_sorted];
        ctr[Slot::repeated_pieces] += scan_info[Scan::repeated_pieces];
        return true;
    });
}

bool Device::exact_range_results(int *out_ids, float *out_d)
{
    if (xr_ids_.empty()) return true;
    if (!out_ids || !out_d) { set_dev_error("exact_range_results: null argument"); return false; }
    memcpy(out_ids, xr_ids_.data(), 4 * xr_ids_.size());
    memcpy(out_d, xr_d_.data(), 4 * xr_d_.size());
    return true;
}

// ---- GetInfo / GetConnectedComponentCounts on the mirror (device code in dk_graph_info.h) ----------------
// Grid-stride launches: enough blocks for the items, at most eight per CU.
static unsigned graph_info_blocks(long long items, int num_cu)
{
    const long long want = (items + kGraphInfoBlock - 1) / kGraphInfoBlock;
    return (unsigned)std::max<long long>(1, std::min<long long>(want, (long long)num_cu * 8));
}

// What both calls begin with: the arguments, the view of the mirror for `layer` with the live set uploaded (its words travel in the
// pinned stage behind the GraphAcc that comes back, so the stage is asked for once), and the accumulators zeroed.
bool Device::graph_info_begin(const char *who, int layer, const uint32_t *live_bits, long long nbits, LayerView *g)
{
    if (g_n_ <= 0 || !g_adj0_) { set_dev_error(std::string(who) + ": no graph committed"); return false; }
    if (layer < 0 || (live_bits && nbits < 0)) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    if (g_stride0_ > kGraphInfoMaxStride || g_strideU_ > kGraphInfoMaxStride) { set_dev_error(std::string(who) + ": adjacency lists too long"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const long long nb = live_bits ? std::min(nbits, g_n_) : 0;
    const size_t words = (size_t)((nb + 31) / 32);
    char *hs = static_cast<char *>(pinned_stage(sizeof(GraphAcc) + 4 * words));
    if (!hs || !gi_acc_.grow((sizeof(GraphAcc) + 7) / 8)) return false;
    if (live_bits) {
        if (!gi_live_.grow(std::max<size_t>(words, 1))) return false;
        memcpy(hs + sizeof(GraphAcc), live_bits, 4 * words);
        if (words) HIP_OK(hipMemcpyAsync(gi_live_, hs + sizeof(GraphAcc), 4 * words, hipMemcpyHostToDevice, st));
    }
    g->adj0 = g_adj0_; g->level = g_level_; g->pool = g_pool_; g->upper = g_upper_;
    g->n = g_n_; g->pool_cap = g_pool_ ? g_pool_cap() : 0;
    g->stride0 = g_stride0_; g->strideU = g_strideU_; g->layer = layer;
    g->live = live_bits ? gi_live_.get() : nullptr;
    g->nbits = nb;
    HIP_OK(hipMemsetAsync(gi_acc_, 0, sizeof(GraphAcc), st));
    return true;
}
// ... and end with: the accumulators on the host (valid until the pinned stage is used again)
bool Device::graph_info_fetch(const GraphAcc **acc)
{
    hipStream_t st = S(stream_);
    HIP_OK(hipMemcpyAsync(h_stage_.get(), gi_acc_, sizeof(GraphAcc), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    *acc = reinterpret_cast<const GraphAcc *>(h_stage_.get());
    return true;
}

// The value of rank r (0-based, ascending) among sum(hist) values, hist[d] of them equal to d
static long long hist_rank(const int *hist, long long bins, long long r)
{
    long long seen = 0;
    for (long long d = 0; d < bins; ++d) {
        seen += hist[d];
        if (seen > r) return d;
    }
    return bins - 1;
}
// HNSWInfo.LayerInfo.Median (HNSWInfo.cs:45-51) of such values: sorted[n / 2], for an even n the integer mean of the two middle ones
static int hist_median(const int *hist, long long bins, long long n)
{
    if (n % 2) return (int)hist_rank(hist, bins, n / 2);
    return (int)((hist_rank(hist, bins, n / 2 - 1) + hist_rank(hist, bins, n / 2)) / 2);
}

bool Device::graph_info(int layer, const uint32_t *live_bits, long long nbits, bool with_in_edges, hnsw_mi355x_layer_info *out)
{
    if (!out) { set_dev_error("graph_info: null argument"); return false; }
    LayerView g;
    if (!graph_info_begin("graph_info", layer, live_bits, nbits, &g)) return false;
    hipStream_t st = S(stream_);
    GraphAcc *d_acc = reinterpret_cast<GraphAcc *>(gi_acc_.get());
    uint64_t launches = 0;
    if (with_in_edges) {
        if (!gi_indeg_.grow((size_t)g_n_, (size_t)std::max<long long>(g_n_, g_cap_n()))) return false;
        HIP_OK(hipMemsetAsync(gi_indeg_, 0, sizeof(int) * (size_t)g_n_, st));
    }
    const unsigned edge_blocks = graph_info_blocks(g_n_ * (layer == 0 ? g_stride0_ : g_strideU_), num_cu_), node_blocks = graph_info_blocks(g_n_, num_cu_);
    hipLaunchKernelGGL(graph_edge_pass_kernel<false>, dim3(edge_blocks), dim3(kGraphInfoBlock), 0, st, g, with_in_edges ? gi_indeg_.get() : nullptr, d_acc);
    HIP_OK(hipGetLastError());
    ++launches;
    if (with_in_edges) {
        hipLaunchKernelGGL(graph_indeg_reduce_kernel, dim3(node_blocks), dim3(kGraphInfoBlock), 0, st, g, gi_indeg_.get(), d_acc);
        HIP_OK(hipGetLastError());
        ++launches;
    }
    const GraphAcc *h;
    if (!graph_info_fetch(&h)) return false;
    const GraphAcc a = *h; // (the stage is used again below)
    *out = hnsw_mi355x_layer_info{};
    out->layer_id = layer;
    // out-degrees: everything from the histogram (the integer sum as int64, then one division: LINQ's Average)
    const int stride = layer == 0 ? g_stride0_ : g_strideU_;
    long long nodes = 0, out_sum = 0;
    int out_min = -1, out_max = 0;
    for (int c = 0; c < stride && c < kGraphInfoMaxStride; ++c) {
        if (!a.out_hist[c]) continue;
        nodes += a.out_hist[c];
        out_sum += (long long)c * a.out_hist[c];
        if (out_min < 0) out_min = c;
        out_max = c;
    }
    if (nodes > 0) {
        out->nodes_count = (int)nodes;
        out->max_out_edges = out_max; out->min_out_edges = out_min;
        out->avg_out_edges = (double)out_sum / (double)nodes;
        out->out_edges_median = hist_median(a.out_hist, stride, nodes);
    }
    if (nodes > 0 && with_in_edges) {
        out->max_in_edges = a.in_max; out->min_in_edges = 0x7fffffff - a.in_min_inv;
        out->avg_in_edges = (double)(long long)a.in_sum / (double)nodes;
        // the median: a histogram with max + 1 bins, exact whatever the maximum is
        const long long bins = (long long)a.in_max + 1;
        if (!gi_inhist_.grow((size_t)bins)) return false;
        HIP_OK(hipMemsetAsync(gi_inhist_, 0, sizeof(int) * (size_t)bins, st));
        hipLaunchKernelGGL(graph_indeg_hist_kernel, dim3(node_blocks), dim3(kGraphInfoBlock), 0, st, g, gi_indeg_.get(), gi_inhist_.get(), bins);
        HIP_OK(hipGetLastError());
        ++launches;
        std::vector<int> hist((size_t)bins);
        if (!exact_copy_out(hist.data(), gi_inhist_, sizeof(int) * (size_t)bins)) return false;
        long long seen = 0;
        for (int v : hist) seen += v;
        if (seen != nodes) { set_dev_error("graph_info: the in-degree histogram does not add up to the layer's nodes"); return false; }
        out->in_edges_median = hist_median(hist.data(), bins, nodes);
    }
    using Slot = slot::graph_info_counters;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::info_layers] += 1; ctr[Slot::entries] += a.entries; ctr[Slot::launches] += launches;
    return true;
}

bool Device::graph_components(int layer, const uint32_t *live_bits, long long nbits, int *out_count)
{
    if (!out_count) { set_dev_error("graph_components: null argument"); return false; }
    *out_count = 0;
    LayerView g;
    if (!graph_info_begin("graph_components", layer, live_bits, nbits, &g)) return false;
    hipStream_t st = S(stream_);
    GraphAcc *d_acc = reinterpret_cast<GraphAcc *>(gi_acc_.get());
    if (!gi_parent_.grow((size_t)g_n_, (size_t)std::max<long long>(g_n_, g_cap_n()))) return false;
    const unsigned edge_blocks = graph_info_blocks(g_n_ * (layer == 0 ? g_stride0_ : g_strideU_), num_cu_), node_blocks = graph_info_blocks(g_n_, num_cu_);
    hipLaunchKernelGGL(graph_uf_init_kernel, dim3(node_blocks), dim3(kGraphInfoBlock), 0, st, g, gi_parent_.get());
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(graph_edge_pass_kernel<true>, dim3(edge_blocks), dim3(kGraphInfoBlock), 0, st, g, gi_parent_.get(), d_acc);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(graph_uf_roots_kernel, dim3(node_blocks), dim3(kGraphInfoBlock), 0, st, g, gi_parent_.get(), d_acc);
    HIP_OK(hipGetLastError());
    const GraphAcc *h;
    if (!graph_info_fetch(&h)) return false;
    *out_count = (int)h->roots;
    using Slot = slot::graph_info_counters;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::component_layers] += 1; ctr[Slot::entries] += h->entries; ctr[Slot::launches] += 3;
    return true;
}

// The C ABI's layer test: a committed graph, and a layer of 0 .. its top level
bool Device::graph_info_layer(const char *who, int layer)
{
    if (!hg_ || g_n_ <= 0) { set_dev_error(std::string(who) + ": no graph committed"); return false; }
    if (layer < 0 || layer > hg_->top) {
        set_dev_error(std::string(who) + ": layer " + std::to_string(layer) + " outside 0 .. " + std::to_string(hg_->top) + " (the graph's top level)");
        return false;
    }
    return true;
}

// ---- reachability over out-edges on the mirror (device code in dk_graph_reach.h) ---------------------------
// The call's scratch, sized with the mirror's node capacity as gi_parent_ is: two hop arrays, two queues, the bitset, the ReachAcc.
bool Device::graph_reach_room()
{
    const size_t n = (size_t)g_n_, cap = (size_t)std::max<long long>(g_n_, g_cap_n());
    for (int i = 0; i < 2; ++i)
        if (!gr_hop_[i].grow(n, cap) || !gr_q_[i].grow(n, cap)) return false;
    return gr_bits_.grow((n + 31) / 32, (cap + 31) / 32) && gr_acc_.grow((sizeof(ReachAcc) + 7) / 8);
}

// One layer (g.layer) from `seeds` into gr_hop_[which]: init, a round per BFS level, pack.  After every round the host reads the two
// queue lengths (8 bytes) and stops at an empty frontier.  Every round but the first expands nodes that the round before reached for
// the first time, so there are at most `members` rounds: the loop is bounded by that number and fails beyond it.
bool Device::graph_reach_run(const LayerView &g, const ReachSeeds &seeds, int which, bool want_bits, uint64_t summary[4])
{
    hipStream_t st = S(stream_);
    ReachAcc *d_acc = reinterpret_cast<ReachAcc *>(gr_acc_.get());
    int *hop = gr_hop_[which].get();
    ReachAcc *h = static_cast<ReachAcc *>(pinned_stage(sizeof(ReachAcc)));
    if (!h) return false;
    const unsigned node_blocks = graph_info_blocks(g_n_, num_cu_);
    HIP_OK(hipMemsetAsync(d_acc, 0, sizeof(ReachAcc), st));
    hipLaunchKernelGGL(graph_reach_init_kernel, dim3(node_blocks), dim3(kGraphInfoBlock), 0, st, g, seeds, hop, gr_q_[0].get(), d_acc);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, d_acc, sizeof(ReachAcc), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const unsigned long long members = h->members, n_seeds = h->seeds;
    long long q_n = h->qn[0];
    if (members > (unsigned long long)g_n_ || n_seeds > members || q_n != (long long)n_seeds) { set_dev_error("graph_reach: the seed queue does not add up"); return false; }
    const int per = (g.layer == 0 ? g_stride0_ : g_strideU_) - 1;
    unsigned long long rounds = 0, queued = n_seeds;
    for (int src = 0; q_n > 0; src ^= 1) {
        if (rounds >= members) { set_dev_error("graph_reach: more rounds than the layer has members"); return false; }
        hipLaunchKernelGGL(graph_reach_expand_kernel, dim3(graph_info_blocks(q_n * per, num_cu_)), dim3(kGraphInfoBlock), 0, st, g, gr_q_[src].get(), (int)q_n,
                           gr_q_[src ^ 1].get(), hop, (int)rounds, src, d_acc);
        HIP_OK(hipGetLastError());
        ++rounds;
        HIP_OK(hipMemcpyAsync(h->qn, d_acc->qn, sizeof(h->qn), hipMemcpyDeviceToHost, st));
        HIP_OK(hipStreamSynchronize(st));
        q_n = h->qn[src ^ 1];
        if (q_n < 0 || queued + (unsigned long long)q_n > members) { set_dev_error("graph_reach: a frontier larger than the members left"); return false; }
        queued += (unsigned long long)q_n;
    }
    hipLaunchKernelGGL(graph_reach_pack_kernel, dim3(node_blocks), dim3(kGraphInfoBlock), 0, st, (long long)g_n_, hop, want_bits ? gr_bits_.get() : nullptr, d_acc);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, d_acc, sizeof(ReachAcc), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (h->reached != queued) { set_dev_error("graph_reach: the reached set is not what the rounds queued"); return false; }
    summary[0] = members; summary[1] = n_seeds; summary[2] = h->reached; summary[3] = (uint64_t)h->max_hop;
    using Slot = slot::graph_reach_counters;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::layers] += 1; ctr[Slot::rounds] += rounds; ctr[Slot::entries] += h->entries; ctr[Slot::launches] += rounds + 2;
    return true;
}

bool Device::graph_reach_copy_out(int which, uint32_t *out_reached_bits, int *out_hops)
{
    if (out_reached_bits && !exact_copy_out(out_reached_bits, gr_bits_.get(), 4 * (size_t)((g_n_ + 31) / 32))) return false;
    return !out_hops || exact_copy_out(out_hops, gr_hop_[which].get(), sizeof(int) * (size_t)g_n_);
}

bool Device::graph_reach_layer(int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits,
                               uint32_t *out_reached_bits, int *out_hops, uint64_t out_summary[4])
{
    if (!seed_bits || seed_nbits < 0 || !out_summary) { set_dev_error("graph_reach_layer: seed_bits and out_summary must not be NULL and seed_nbits must be >= 0"); return false; }
    LayerView g;
    if (!graph_info_begin("graph_reach_layer", layer, live_bits, nbits, &g) || !graph_reach_room()) return false;
    hipStream_t st = S(stream_);
    HIP_OK(hipStreamSynchronize(st)); // (the live set has left the pinned stage: the seeds take its place)
    const long long sb = std::min(seed_nbits, g_n_);
    const size_t words = (size_t)((sb + 31) / 32);
    void *hs = pinned_stage(std::max<size_t>(4 * words, sizeof(ReachAcc)));
    if (!hs || !gr_seed_.grow(std::max<size_t>(words, 1))) return false;
    memcpy(hs, seed_bits, 4 * words);
    if (words) HIP_OK(hipMemcpyAsync(gr_seed_, hs, 4 * words, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st)); // (... and graph_reach_run reads its figures through the same stage)
    const ReachSeeds seeds{kReachSeedBits, -1, gr_seed_.get(), sb, nullptr};
    return graph_reach_run(g, seeds, 0, out_reached_bits != nullptr, out_summary) && graph_reach_copy_out(0, out_reached_bits, out_hops);
}

int Device::graph_reach(int entry_point, int top, const uint32_t *live_bits, long long nbits, int min_layer, hnsw_mi355x_layer_reach *out_layers, int cap,
                        uint32_t *out_reached_bits, int *out_hops)
{
    if (top < 0 || min_layer < 0 || min_layer > top || cap < 0 || (cap > 0 && !out_layers)) {
        set_dev_error("graph_reach: min_layer " + std::to_string(min_layer) + " outside 0 .. " + std::to_string(top) + " (the entry point's top layer), or a bad argument");
        return -1;
    }
    LayerView g;
    if (!graph_info_begin("graph_reach", top, live_bits, nbits, &g) || !graph_reach_room()) return -1;
    if (hipStreamSynchronize(S(stream_)) != hipSuccess) { set_dev_error("graph_reach: hipStreamSynchronize failed"); return -1; }
    int which = 0;
    for (int layer = top; layer >= min_layer; --layer, which ^= 1) {
        g.layer = layer;
        // the top layer starts at the entry point (-1: an id that is nobody's); every other at what the layer above reached
        const bool in_range = entry_point >= 0 && (long long)entry_point < g_n_;
        const ReachSeeds seeds = layer == top ? ReachSeeds{kReachSeedId, in_range ? entry_point : -1, nullptr, 0, nullptr}
                                              : ReachSeeds{kReachSeedHops, -1, nullptr, 0, gr_hop_[which ^ 1].get()};
        uint64_t sum[4];
        if (!graph_reach_run(g, seeds, which, layer == min_layer && out_reached_bits, sum)) return -1;
        if (layer < cap) out_layers[layer] = hnsw_mi355x_layer_reach{layer, (int32_t)sum[0], (int32_t)sum[1], (int32_t)sum[2], (int32_t)sum[3]};
    }
    return graph_reach_copy_out(which ^ 1, out_reached_bits, out_hops) ? top + 1 : -1;
}

// The C ABI's `top`: the staged level of the entry point; of an entry point out of range (it reaches nothing) the graph's top level
bool Device::graph_reach_top(const char *who, int entry_point, int *top)
{
    if (!hg_ || g_n_ <= 0) { set_dev_error(std::string(who) + ": no graph committed"); return false; }
    *top = entry_point >= 0 && entry_point < hg_->n ? hg_->level[(size_t)entry_point] : hg_->top;
    return true;
}

// ---- one round of repair_reachability on the mirror (device code in dk_graph_repair.h) ---------------------------
// BFS (graph_reach_run into gr_hop_[which]); then, where it is asked for and members are left without a hop: U and the reached set
// as ascending id lists (collect -> offsets -> exact_compact_kernel: the order is the bitset's, nothing is sorted and nothing goes
// through the host), the rows of U as the scan's queries, the flat scan over the reached ids, and the proposal kernel.  What comes
// back is U, the candidates and the codes, in pinned memory of the call's own; the hop array stays on the device.
bool Device::graph_repair_round(int layer, const uint32_t *live_bits, long long nbits, int seed_mode, int entry_point, const uint32_t *seed_bits,
                                long long seed_nbits, int which, int cands, int max_edges, bool propose, GraphRepairRound *out)
{
    static_assert(kRepairSeedEntry == kReachSeedId && kRepairSeedBits == kReachSeedBits && kRepairSeedAbove == kReachSeedHops, "the seed modes of device_backend.h");
    const char *who = "graph_repair_round";
    if (!out || which < 0 || which > 1 || seed_mode < kReachSeedId || seed_mode > kReachSeedHops || (seed_mode == kReachSeedBits && (!seed_bits || seed_nbits < 0))) {
        set_dev_error(std::string(who) + ": bad argument");
        return false;
    }
    if (cands < 1 || cands > kRepairMaxCands) { set_dev_error(std::string(who) + ": cands = " + std::to_string(cands) + " is outside 1 .. " + std::to_string(kRepairMaxCands)); return false; }
    *out = GraphRepairRound{};
    LayerView g;
    if (!graph_info_begin(who, layer, live_bits, nbits, &g) || !graph_reach_room()) return false;
    const int list_cap = (layer == 0 ? g_stride0_ : g_strideU_) - 1;
    if (max_edges < 1 || max_edges > list_cap) {
        set_dev_error(std::string(who) + ": max_edges = " + std::to_string(max_edges) + " is outside 1 .. " + std::to_string(list_cap) + " (what a list of the mirror holds)");
        return false;
    }
    hipStream_t st = S(stream_);
    HIP_OK(hipStreamSynchronize(st)); // (the live set has left the pinned stage)
    ReachSeeds seeds{seed_mode, -1, nullptr, 0, nullptr};
    if (seed_mode == kReachSeedId) seeds.id = entry_point >= 0 && (long long)entry_point < g_n_ ? entry_point : -1;
    else if (seed_mode == kReachSeedHops) seeds.prev_hop = gr_hop_[which ^ 1].get();
    else {
        const long long sb = std::min(seed_nbits, g_n_);
        const size_t words = (size_t)((sb + 31) / 32);
        void *hs = pinned_stage(std::max<size_t>(4 * words, sizeof(ReachAcc)));
        if (!hs || !gr_seed_.grow(std::max<size_t>(words, 1))) return false;
        memcpy(hs, seed_bits, 4 * words);
        if (words) HIP_OK(hipMemcpyAsync(gr_seed_, hs, 4 * words, hipMemcpyHostToDevice, st));
        HIP_OK(hipStreamSynchronize(st));
        seeds.bits = gr_seed_.get(); seeds.nbits = sb;
    }
    if (!graph_reach_run(g, seeds, which, false, out->summary)) return false;
    const long long n_u = (long long)(out->summary[0] - out->summary[2]), reached = (long long)out->summary[2];
    out->n_u = (int)n_u;
    if (!propose || n_u <= 0) return true;
    if (g_n_ > n_rows_hw_) { set_dev_error(std::string(who) + ": the graph has nodes whose rows were never uploaded"); return false; }
    const size_t C = (size_t)cands, pairs = (size_t)n_u * C;
    if (!rp_host_.grow((size_t)n_u + 2 * pairs + 4)) return false;
    int *h_ids = rp_host_.get(), *h_cand = h_ids + n_u, *h_code = h_cand + pairs;
    out->ids = h_ids; out->cands = h_cand; out->codes = h_code;

    // U and the reached set, ascending
    const long long words = (g_n_ + 31) / 32;
    const int blocks = (int)((words + kExactCompactWords - 1) / kExactCompactWords);
    const size_t cap_n = (size_t)std::max<long long>(g_n_, g_cap_n()), cap_w = (cap_n + 31) / 32, cap_b = (cap_w + kExactCompactWords - 1) / kExactCompactWords;
    if (!rp_bits_.grow(2 * (size_t)words, 2 * cap_w) || !rp_bcnt_.grow(2 * (size_t)blocks, 2 * cap_b) || !rp_boff_.grow(2 * (size_t)blocks, 2 * cap_b) ||
        !rp_uids_.grow((size_t)n_u) || !x_ids_.grow((size_t)std::max<long long>(reached, 1)) || !rp_cand_.grow(2 * pairs) || !rp_meas_.grow(1)) return false;
    const unsigned node_blocks = graph_info_blocks(g_n_, num_cu_);
    const int *hop = gr_hop_[which].get();
    HIP_OK(hipMemsetAsync(rp_bcnt_, 0, sizeof(int) * 2 * (size_t)blocks, st));
    for (int sel = 0; sel < 2; ++sel) { // 0: U, 1: the reached set
        hipLaunchKernelGGL(graph_repair_collect_kernel, dim3(node_blocks), dim3(kRepairBlock), 0, st, (long long)g_n_, hop, sel == 0 ? 1 : 0, rp_bits_.get() + sel * words,
                           rp_bcnt_.get() + sel * blocks);
        HIP_OK(hipGetLastError());
        hipLaunchKernelGGL(graph_repair_offsets_kernel, dim3(1), dim3(64), 0, st, rp_bcnt_.get() + sel * blocks, blocks, rp_boff_.get() + sel * blocks);
        HIP_OK(hipGetLastError());
        if (sel == 0 || reached > 0)
            HIP_OK(exact_compact_launch(rp_bits_.get() + sel * words, words, rp_boff_.get() + sel * blocks, sel == 0 ? rp_uids_.get() : x_ids_.get(), st));
    }
    HIP_OK(hipMemcpyAsync(h_ids, rp_uids_, sizeof(int) * (size_t)n_u, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (reached <= 0) { // nobody to link to: every candidate is padding, nothing is proposed
        std::fill(h_cand, h_cand + 2 * pairs, -1);
        return true;
    }

    // the rows of U as the scan's query set: what set_queries makes of hnswdev_download_rows' rows, without the host
    if (!rp_q_.grow((size_t)n_u * pitch_) || (metric_ == M_COS && !rp_qsn_.grow((size_t)n_u)) || (metric_ == M_I8 && !q_stage_.grow((size_t)n_u * (size_t)dim_))) return false;
    if (!gather_launch(rp_uids_.get(), n_u, metric_ == M_I8 ? q_stage_.get() : rp_q_.get())) return false;
    if (metric_ == M_I8) {
        hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)((n_u + 3) / 4)), dim3(256), 0, st, q_stage_, dim_, (int)n_u, rp_q_, 0LL, pitch_);
        HIP_OK(hipGetLastError());
    }
    if (metric_ == M_COS) {
        hipLaunchKernelGGL(row_sqrtnorm_kernel, dim3((unsigned)((n_u * 8 + 255) / 256)), dim3(256), 0, st, rp_q_, pitch_, 0LL, (int)n_u, rp_qsn_);
        HIP_OK(hipGetLastError());
    }
    int *d_cand = rp_cand_.get(), *d_code = d_cand + pairs;
    if (!exact_knn_rounds(rp_q_, metric_ == M_COS ? rp_qsn_.get() : nullptr, (int)n_u, x_ids_, reached, cands, h_cand, nullptr, d_cand)) return false;

    // the proposals
    using Slot = slot::graph_repair_counters;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::rounds] += 1;
    RepairProposeArgs a;
    a.g = g; a.rows = d_rows_; a.row_sn = d_row_sn_; a.dim = pitch_; a.n_rows = n_rows_hw_; a.hop = hop; a.cand = d_cand; a.n_pairs = (long long)pairs;
    a.max_edges = max_edges; a.code = d_code; a.measured = rp_meas_;
    HIP_OK(hipMemsetAsync(rp_meas_, 0, sizeof(unsigned long long), st));
    hipError_t e = hipSuccess;
    with_metric(metric_, [&](auto mt) { e = graph_repair_propose_launch<mt>(a, graph_info_blocks((long long)pairs * 64, num_cu_), st); });
    HIP_OK(e);
    unsigned long long *h_meas = reinterpret_cast<unsigned long long *>(h_ids + (((size_t)n_u + 2 * pairs + 1) & ~(size_t)1));
    HIP_OK(hipMemcpyAsync(h_code, d_code, sizeof(int) * pairs, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(h_meas, rp_meas_, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    uint64_t real = 0;
    for (size_t i = 0; i < pairs; ++i) real += h_cand[i] >= 0;
    ctr[Slot::pairs] += real; ctr[Slot::distances] += *h_meas;
    return true;
}

bool Device::graph_repair_patch(const int *recs, int nrows, int row_stride)
{
    if (!patch_lists(recs, nrows, row_stride)) return false;
    counter_block(CounterBlock::graph_repair_counters)[slot::graph_repair_counters::lists_patched] += (uint64_t)std::max(nrows, 0);
    return true;
}

// hnswdev_graph_repair_propose: steps 1 - 3 of one round on the committed graph, which is read and not changed
int Device::graph_repair_propose(int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits, int cands, int max_edges,
                                 int *out_n, int *out_ids, int *out_cands, int *out_codes, int cap)
{
    if (!out_n || cap < 0 || (cap > 0 && (!out_ids || !out_cands || !out_codes))) { set_dev_error("graph_repair_propose: bad argument"); return -1; }
    GraphRepairRound r;
    if (!graph_repair_round(layer, live_bits, nbits, kReachSeedBits, -1, seed_bits, seed_nbits, 0, cands, max_edges, true, &r)) return -1;
    *out_n = r.n_u;
    const size_t n = (size_t)std::min(cap, r.n_u), C = (size_t)cands;
    if (n) {
        memcpy(out_ids, r.ids, sizeof(int) * n);
        memcpy(out_cands, r.cands, sizeof(int) * n * C);
        memcpy(out_codes, r.codes, sizeof(int) * n * C);
    }
    return 0;
}

// ---- query by stored id: rows back out, and stored rows as queries without crossing the host boundary --------
// n ids from the host to d_ids, enqueued: through the pinned stage (the caller synchronises before it uses the stage again), or in
// pieces as query sets go up.
bool Device::upload_ids(const int *ids, int n, DevBuf<int> &d_ids)
{
    const size_t bytes = 4u * (size_t)n;
    if (!d_ids.grow((size_t)n)) return false;
    if (bytes >= (4u << 20)) return staged_upload(reinterpret_cast<float *>(d_ids.get()), reinterpret_cast<const float *>(ids), bytes);
    void *hs = pinned_stage(bytes);
    if (!hs) return false;
    memcpy(hs, ids, bytes);
    HIP_OK(hipMemcpyAsync(d_ids, hs, bytes, hipMemcpyHostToDevice, S(stream_)));
    return true;
}

// gather_rows_kernel over n ids on the device: out[i] = the stored row d_ids[i] as dim_ floats, zeros for an id outside the uploaded rows
bool Device::gather_launch(const int *d_ids, long long n, float *out)
{
    const int kind = metric_ == M_I8 ? 2 : metric_f16(metric_) ? 1 : 0;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(graph_info_blocks(n * dim_, num_cu_)), dim3(kGatherBlock), 0, S(stream_), d_rows_.get(), row_pitch_, n_rows_hw_, kind, d_ids, n,
                       dim_, out);
    HIP_OK(hipGetLastError());
    return true;
}

bool Device::gather_rows(const int *ids, int n, float *out)
{
    if (n <= 0) return true;
    if (!ids || !out) { set_dev_error("gather_rows: null argument"); return false; }
    if (!bind() || !q_stage_.grow((size_t)n * (size_t)dim_) || !upload_ids(ids, n, x_self_) || !gather_launch(x_self_, n, q_stage_)) return false;
    HIP_OK(hipMemcpyAsync(out, q_stage_, (size_t)n * dim_ * sizeof(float), hipMemcpyDeviceToHost, S(stream_)));
    HIP_OK(hipStreamSynchronize(S(stream_)));
    counter_block(CounterBlock::by_id_info)[slot::by_id_info::rows_gathered] += (uint64_t)n;
    return true;
}

// The stored rows of ids[0, n) as a query set in d_q (pitch_ words a query; d_qsn: the cosine norms): the steps set_queries takes
// for rows that come from the host, on rows that are gathered on the device.  The ids stay in d_ids.  The stream is idle and the
// pinned stage free when this returns.
bool Device::gather_queries(const int *ids, int n, DevBuf<int> &d_ids, float *d_q, double *d_qsn)
{
    hipStream_t st = S(stream_);
    if (metric_ == M_I8 && !q_stage_.grow((size_t)n * (size_t)dim_)) return false;
    if (!upload_ids(ids, n, d_ids) || !gather_launch(d_ids, n, metric_ == M_I8 ? q_stage_.get() : d_q)) return false;
    if (metric_ == M_I8) {
        hipLaunchKernelGGL(quantize_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, q_stage_, dim_, n, d_q, 0LL, pitch_);
        HIP_OK(hipGetLastError());
    }
    if (metric_ == M_COS) {
        hipLaunchKernelGGL(row_sqrtnorm_kernel, dim3((unsigned)(((long long)n * 8 + 255) / 256)), dim3(256), 0, st, d_q, pitch_, 0LL, n, d_qsn);
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(st));
    counter_block(CounterBlock::by_id_info)[slot::by_id_info::rows_gathered] += (uint64_t)n;
    return true;
}

// The ids of a by-id call that are no uploaded row: "" when there is none, else the message that names the first.
static std::string by_id_rows_error(const char *who, const int *ids, int n, long long n_rows)
{
    for (int i = 0; i < n; ++i)
        if (ids[i] < 0 || ids[i] >= n_rows) return std::string(who) + ": ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) + " is no uploaded row";
    return std::string();
}

bool Device::set_queries_by_id(const int *ids, int nq)
{
    if (nq < 0 || (nq > 0 && !ids)) { set_dev_error("set_queries_by_id: bad argument"); return false; }
    if (tail_.n > 0) { set_dev_error("set_queries_by_id: a streamed query set is still being uploaded"); return false; }
    if (const std::string why = by_id_rows_error("set_queries_by_id", ids, nq, n_rows_hw_); !why.empty()) { set_dev_error(why); return false; }
    if (!bind() || !query_room(nq)) return false;
    n_queries_ = nq;
    q_by_id_ = false;
    if (nq == 0) return true;
    if (!gather_queries(ids, nq, s_self_, d_queries_, d_q_sn_)) { n_queries_ = 0; return false; }
    q_by_id_ = true;
    return true;
}

// KnnQuery by stored id (graph_search_self_kernel): search_filtered's launch with the ids set_queries_by_id left in s_self_ where
// the allow words were -- nothing goes up for the filter.
bool Device::search_self(int nq, int entry, int entry_layer, int k, int k_out, int *out_ids, float *out_d, int *out_flag, int search_layer)
{
    if (nq <= 0) return true;
    const PredicateCall c{"search_self", nq, entry, entry_layer, search_layer, k, k_out, out_ids, out_d, out_flag};
    const auto own_rules = [&] { return std::string(q_by_id_ ? "" : "search_self: the resident queries were not set by id (set_queries_by_id)"); };
    if (!predicate_call_ok(c, own_rules)) return false;
    const auto p = plan_predicate_search(c, [](auto m, auto h) { return &graph_search_self_kernel<m, h>; });
    if (!p.ok) return false;
    const auto upload = [](char *) { return true; };
    const auto every_query = [](long long, int nj) { return nj; };
    const auto filter = [&](long long off) { return std::make_tuple(static_cast<const int *>(s_self_.get()) + off); };
    if (!run_predicate_search(c, p, 0, upload, every_query, filter)) return false;
    using Slot = slot::by_id_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::calls] += 1;
    ctr[Slot::traversed] += (uint64_t)nq;
    ctr[Slot::handbacks] += count_search_overflows(c);
    return true;
}

bool Device::knn_search_by_id(const int *ids, int nq, int entry_point, int k_beam, int k_out, int *out_ids, float *out_d, int *out_flag, int layer)
{
    if (nq <= 0) return true;
    if (!ids || !out_ids || !out_d || !out_flag) { set_dev_error("knn_search_by_id: null argument"); return false; }
    int top;
    const bool args_ok = k_out >= 1 && k_beam >= k_out; // (false: "knn_search_by_id: bad argument", in abi_entry's place for it)
    if (!abi_begin("knn_search_by_id", nullptr, 0, entry_point, layer, &top, args_ok)) return false; // (no query goes up: the set is gathered below)
    if (const std::string why = by_id_rows_error("knn_search_by_id", ids, nq, std::min<long long>(n_rows_hw_, g_n_)); !why.empty()) { set_dev_error(why); return false; }
    return set_queries_by_id(ids, nq) && search_self(nq, entry_point, top, k_beam, k_out, out_ids, out_d, out_flag, layer);
}

// The flat scan by stored id: exact_knn with the queries gathered into the scan's own buffer and ExactTopKSelf as the sink.  The id
// list, the chunks, the rounds and the merge are exact_knn's.
bool Device::exact_knn_by_id(const int *ids, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d)
{
    if (nq <= 0) return true;
    if (!ids || !out_ids || !out_d || k < 1 || n_rows < 0 || (allow_bits && nbits < 0)) { set_dev_error("exact_knn_by_id: bad argument"); return false; }
    if (k > kExactMaxK) { set_dev_error("exact_knn_by_id: k = " + std::to_string(k) + " is above the limit of " + std::to_string(kExactMaxK)); return false; }
    if (const std::string why = by_id_rows_error("exact_knn_by_id", ids, nq, n_rows_hw_); !why.empty()) { set_dev_error(why); return false; }
    if (!allow_bits) nbits = 0;
    const long long n = std::min(n_rows, n_rows_hw_), n_allow = allow_bits ? std::min(nbits, n) : n;
    if (n_allow <= 0 || (allow_bits && !allows_any(allow_bits, nbits, n))) { // no candidate: padding, no launch
        pad_results(out_ids, out_d, (size_t)nq * (size_t)k);
        return true;
    }
    if (!bind()) return false;
    const size_t cap = (size_t)std::max(nq, 1024);
    if (!x_queries_.grow((size_t)nq * pitch_, cap * pitch_) || (metric_ == M_COS && !x_q_sn_.grow((size_t)nq, cap))) return false;
    const double *d_qsn = metric_ == M_COS ? x_q_sn_.get() : nullptr;
    if (!gather_queries(ids, nq, x_self_, x_queries_, x_q_sn_)) return false;
    long long m = 0;
    if (!exact_id_list(allow_bits, n_allow, &m)) return false;
    uint64_t skipped = 0; // the queries whose own id is a candidate: one pair each
    for (int i = 0; i < nq; ++i) {
        const long long id = ids[i];
        skipped += (uint64_t)(id < n_allow && (!allow_bits || ((allow_bits[id >> 5] >> (id & 31)) & 1u)));
    }
    if (!exact_knn_rounds(x_queries_, d_qsn, nq, allow_bits ? x_ids_.get() : nullptr, m, k, out_ids, out_d, nullptr, x_self_)) return false;
    using Slot = slot::by_id_info;
    uint64_t *ctr = counter_block(Slot::kBlock);
    ctr[Slot::calls] += 1;
    ctr[Slot::scanned] += (uint64_t)nq;
    ctr[Slot::self_skipped] += skipped;
    return true;
}

// ---- near-duplicates of stored rows ---------------------------------------------------------------------------------
// The range scan by stored id: exact_range's rounds (exact_range_rounds) with the queries gathered as exact_knn_by_id gathers them
// and ExactRangeSelf as the sink.
bool Device::exact_range_by_id(const int *ids, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_counts)
{
    return exact_range_call(nq, out_counts, [&]() -> bool {
        if (nq <= 0) return true;
        const char *who = "exact_range_by_id";
        if (!ids || !out_counts || n_rows < 0 || (allow_bits && nbits < 0)) { set_dev_error(std::string(who) + ": bad argument"); return false; }
        for (int i = 0; i < nq; ++i) out_counts[i] = 0;
        if (const std::string why = by_id_rows_error(who, ids, nq, n_rows_hw_); !why.empty()) { set_dev_error(why); return false; }
        if (!allow_bits) nbits = 0;
        const long long n = std::min(n_rows, n_rows_hw_), n_allow = allow_bits ? std::min(nbits, n) : n;
        if (n_allow <= 0 || (allow_bits && !allows_any(allow_bits, nbits, n))) return true; // no candidate: empty lists, no launch
        if (!bind()) return false;
        const size_t cap = (size_t)std::max(nq, 1024);
        if (!x_queries_.grow((size_t)nq * pitch_, cap * pitch_) || (metric_ == M_COS && !x_q_sn_.grow((size_t)nq, cap))) return false;
        if (!gather_queries(ids, nq, x_self_, x_queries_, x_q_sn_)) return false;
        ExactScanInput in;
        in.d_q = x_queries_; in.d_qsn = metric_ == M_COS ? x_q_sn_.get() : nullptr;
        if (!exact_id_list(allow_bits, n_allow, &in.m)) return false;
        in.ids = allow_bits ? x_ids_.get() : nullptr;
        uint64_t skipped = 0; // the queries whose own id is a candidate: one pair each
        for (int i = 0; i < nq; ++i) {
            const long long id = ids[i];
            skipped += (uint64_t)(id < n_allow && (!allow_bits || ((allow_bits[id >> 5] >> (id & 31)) & 1u)));
        }
        if (!exact_range_rounds(who, in, nq, range, x_self_, out_counts)) return false;
        using Slot = slot::by_id_info;
        uint64_t *ctr = counter_block(Slot::kBlock);
        ctr[Slot::calls] += 1;
        ctr[Slot::scanned] += (uint64_t)nq;
        ctr[Slot::self_skipped] += skipped;
        return true;
    });
}

// The duplicate groups: the members' list goes up once and is both the candidates and, a round of `exact_union_round` (65 536) at a
// time, the queries -- gathered as the by-id calls gather theirs.  Every round is one launch of the scan with ExactRangeUnion as
// its sink, counted and timed like any (exact_timed_scan: exact_evals are the pairs measured); then one kernel turns parent[] into
// labels.  The members are listed on the host -- the bitset is the host's -- so that the rounds' ids need no copy back.
constexpr long long kExactUnionChunk = 2048; // rows of a chunk of the groups' scan unless `exact_chunk` forces them

// A scan over the pairs a < b of the members (exact_range_groups, exact_range_density): who they are, and how the triangle is cut.
struct ExactTriangle {
    std::vector<int> members; // ascending
    long long n = 0, m = 0;   // the rows that exist below n_rows; the members
    long long round = 0;      // members that are the queries of one launch
    ExactPlan p;              // tile, piece, chunks; lds for a sink that keeps no list
};

// The members: the rows below min(n_rows, uploaded) that allow_bits allows.  No device work.
bool Device::exact_triangle_begin(const char *who, long long n_rows, const uint32_t *allow_bits, long long nbits, ExactTriangle *t)
{
    if (n_rows < 0 || (allow_bits && nbits < 0)) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    if (!allow_bits) nbits = 0;
    t->n = std::min(n_rows, n_rows_hw_);
    const long long n_allow = allow_bits ? std::min(nbits, t->n) : t->n;
    for (long long id = 0; id < n_allow; ++id)
        if (!allow_bits || ((allow_bits[id >> 5] >> (id & 31)) & 1u)) t->members.push_back((int)id);
    t->m = (long long)t->members.size();
    return true;
}

// Two members or more: the context bound, the round, the tile and the chunks, the query buffers, the members' ids in x_ids_ (enqueued:
// the caller synchronises behind its own initialisation, before the first scan uses the pinned stage again).
bool Device::exact_triangle_ready(const char *who, ExactTriangle *t)
{
    if (!bind()) return false;
    const long long m = t->m;
    const int forced_round = diag("exact_union_round", 0);
    t->round = std::min<long long>(m, forced_round > 0 ? forced_round : 65536);
    ExactPlan &p = t->p;
    p = exact_plan((int)t->round, m, 1, pitch_, num_cu_); // the tile as for lists of one key: these sinks keep none
    p.lds = exact_scan_lds(p.qtile, p.piece, pitch_, 0);
    if (p.lds > 64 * 1024) { set_dev_error(std::string(who) + ": tile exceeds the LDS budget"); return false; }
    if (diag("exact_chunk", 0) <= 0) {
        // The picker's chunks exist to fill the chip, and a round of many tiles fills it alone: it would leave ONE chunk, whose last id
        // is above every query's, so that no block could leave early and every pair were measured twice.  Here the chunks are what the
        // blocks below the diagonal are cut off by: about kExactUnionChunk rows each, so that what is measured twice is the
        // (tile, chunk) blocks on the diagonal alone.
        const long long chunks = std::max<long long>(1, std::min<long long>(m / kExactUnionChunk, kExactMaxChunks));
        p.chunk = ((m + chunks - 1) / chunks + kExactIterRows - 1) / kExactIterRows * kExactIterRows;
        p.n_chunks = (int)((m + p.chunk - 1) / p.chunk);
    }
    const size_t cap = (size_t)std::max<long long>(t->round, 1024);
    if (!x_queries_.grow((size_t)t->round * pitch_, cap * pitch_) || (metric_ == M_COS && !x_q_sn_.grow((size_t)t->round, cap))) return false;
    return upload_ids(t->members.data(), (int)m, x_ids_);
}

// One scan of the triangle: a round of members at a time are gathered as the queries (their ids in x_self_) and `launch` enqueues the
// scan with the caller's sink, counted and timed like any (exact_timed_scan).  *measured += the pairs the kernel counted.
template <class Launch>
bool Device::exact_triangle_scan(const ExactTriangle &t, Launch &&launch, unsigned long long *measured)
{
    hipStream_t st = S(stream_);
    const ExactPlan &p = t.p;
    for (long long off = 0; off < t.m; off += t.round) {
        const int nr = (int)std::min<long long>(t.round, t.m - off);
        if (!gather_queries(t.members.data() + off, nr, x_self_, x_queries_, x_q_sn_)) return false;
        unsigned long long *h_ev = static_cast<unsigned long long *>(pinned_stage(8));
        if (!h_ev) return false;
        ExactScanArgs a;
        if (!exact_scan_args(x_queries_, metric_ == M_COS ? x_q_sn_.get() : nullptr, 0, nr, p.qtile, p.piece, &a)) return false;
        a.ids = x_ids_; a.m = t.m; a.chunk = p.chunk; a.n_chunks = p.n_chunks;
        const unsigned tiles = (unsigned)((nr + p.qtile - 1) / p.qtile);
        const auto enqueue = [&]() -> bool {
            HIP_OK(launch(a, tiles, st));
            return true;
        };
        if (!exact_timed_scan(h_ev, enqueue, [] { return true; })) return false;
        *measured += *h_ev;
    }
    return true;
}

bool Device::exact_range_groups(long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, uint64_t *out_info)
{
    const char *who = "exact_range_groups";
    if (!out_info) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    ExactTriangle t;
    if (!exact_triangle_begin(who, n_rows, allow_bits, nbits, &t)) return false;
    for (int i = 0; i < 4; ++i) out_info[i] = 0;
    const long long n = t.n, m = t.m;
    const std::vector<int> &members = t.members;
    if (n > 0 && !out_labels) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    for (long long v = 0; v < n; ++v) out_labels[v] = -1;
    for (const int v : members) out_labels[v] = v; // (what fewer than two members leave; the device's labels replace it otherwise)
    out_info[0] = (unsigned long long)m;
    out_info[1] = (unsigned long long)m;
    if (m < 2) return true; // nothing to measure: no launch
    if (!exact_triangle_ready(who, &t)) return false;
    if (!x_uparent_.grow(2 * (size_t)n) || !x_upairs_.grow(1)) return false;
    hipStream_t st = S(stream_);
    HIP_OK(exact_union_init_launch(x_ids_, m, x_uparent_, n, st));
    HIP_OK(hipMemsetAsync(x_upairs_, 0, sizeof(unsigned long long), st));
    HIP_OK(hipStreamSynchronize(st)); // the pinned stage is used again by the rounds
    unsigned long long measured = 0;
    const auto launch = [&](const ExactScanArgs &a, unsigned tiles, hipStream_t s) {
        const ExactRangeUnion sink{range, x_uparent_, x_self_, x_upairs_}; // (x_self_ as the round's gather left it)
        hipError_t e = hipSuccess;
        with_metric(metric_, [&](auto mt) { e = exact_range_union_scan_launch<mt>(a, sink, tiles, t.p.lds, s); });
        return e;
    };
    if (!exact_triangle_scan(t, launch, &measured)) return false;
    int *d_labels = x_uparent_.get() + n;
    HIP_OK(exact_union_labels_launch(x_uparent_, n, d_labels, st));
    if (!exact_copy_out(out_labels, d_labels, 4 * (size_t)n)) return false;
    unsigned long long *h = static_cast<unsigned long long *>(pinned_stage(8));
    if (!h) return false;
    HIP_OK(hipMemcpyAsync(h, x_upairs_, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    unsigned long long groups = 0;
    for (const int v : members) groups += (unsigned long long)(out_labels[v] == v);
    out_info[1] = groups;
    out_info[2] = *h;
    out_info[3] = measured;
    return true;
}

// The density clusters: exact_range_groups' members, rounds, chunks and accounting, in two phases.  Phase A is one
// scan of the triangle with ExactRangeDensity: counts[] and the number of within pairs are complete behind it whatever the arena
// held.  The number comes to the host (8 bytes), which chooses phase B: density_pairs_kernel over the arena where every record
// fitted, a second scan with ExactRangeDensityJoin where not.  Then one kernel turns parents and attach keys into labels, and the
// host counts clusters, core, border and noise members from what it copied out, as exact_range_groups counts its groups.
constexpr long long kDensityPairCap = 1LL << 24; // records of the pair arena (256 MiB) unless `density_pair_cap` says otherwise
bool Device::exact_range_density(long long n_rows, float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels, int *out_counts,
                                 uint64_t *out_info)
{
    const char *who = "exact_range_density";
    if (!out_info) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    if (min_samples < 1) { set_dev_error(std::string(who) + ": min_samples = " + std::to_string(min_samples) + " is below 1"); return false; }
    ExactTriangle t;
    if (!exact_triangle_begin(who, n_rows, allow_bits, nbits, &t)) return false;
    for (int i = 0; i < 8; ++i) out_info[i] = 0;
    const long long n = t.n, m = t.m;
    const std::vector<int> &members = t.members;
    if (n > 0 && !out_counts) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    for (long long v = 0; v < n; ++v) out_counts[v] = -1;
    for (const int v : members) out_counts[v] = 0;
    if (out_labels) {
        for (long long v = 0; v < n; ++v) out_labels[v] = -1;
        if (min_samples == 1) for (const int v : members) out_labels[v] = v; // (what fewer than two members leave: a lone member is core when it alone is enough)
    }
    // clusters, core, border and noise members from the labels and counts as they stand on the host
    const auto count_kinds = [&]() {
        unsigned long long clusters = 0, core = 0, border = 0;
        for (const int v : members) {
            const bool is_core = (long long)out_counts[v] + 1 >= (long long)min_samples;
            core += (unsigned long long)is_core;
            clusters += (unsigned long long)(is_core && out_labels[v] == v);
            border += (unsigned long long)(!is_core && out_labels[v] >= 0);
        }
        out_info[1] = clusters; out_info[2] = core; out_info[3] = border; out_info[4] = (unsigned long long)m - core - border;
    };
    out_info[0] = (unsigned long long)m;
    if (m < 2) { // nothing to measure: no launch
        if (out_labels) count_kinds();
        return true;
    }
    if (!exact_triangle_ready(who, &t)) return false;
    hipStream_t st = S(stream_);
    const int forced_cap = diag("density_pair_cap", 0);
    // (no more records than there are pairs: a small member set does not allocate the whole arena)
    const unsigned long long all_pairs = (unsigned long long)m * (unsigned long long)(m - 1) / 2;
    const unsigned long long cap = !out_labels ? 0ull : forced_cap > 0 ? (unsigned long long)forced_cap : std::min<unsigned long long>(kDensityPairCap, all_pairs);
    if (!x_dcounts_.grow((size_t)n) || !x_upairs_.grow(1)) return false;
    if (out_labels && (!x_uparent_.grow(2 * (size_t)n) || !x_dattach_.grow((size_t)n) || !x_darena_.grow((size_t)cap))) return false;
    HIP_OK(density_init_launch(x_ids_, m, x_dcounts_, out_labels ? x_dattach_.get() : nullptr, n, x_upairs_, st));
    if (out_labels) HIP_OK(exact_union_init_launch(x_ids_, m, x_uparent_, n, st));
    HIP_OK(hipStreamSynchronize(st)); // the pinned stage is used again by the rounds
    const size_t lds_a = exact_density_lds(t.p.qtile, t.p.piece, pitch_);
    if (lds_a > 64 * 1024) { set_dev_error(std::string(who) + ": tile exceeds the LDS budget"); return false; }
    unsigned long long measured = 0, scans = 1;
    const auto phase_a = [&](const ExactScanArgs &a, unsigned tiles, hipStream_t s) {
        const ExactRangeDensity sink{range, x_self_, x_dcounts_, x_darena_, cap, x_upairs_}; // (x_self_ as the round's gather left it)
        hipError_t e = hipSuccess;
        with_metric(metric_, [&](auto mt) { e = exact_range_density_scan_launch<mt>(a, sink, tiles, lds_a, s); });
        return e;
    };
    if (!exact_triangle_scan(t, phase_a, &measured)) return false;
    unsigned long long *h = static_cast<unsigned long long *>(pinned_stage(8));
    if (!h) return false;
    HIP_OK(hipMemcpyAsync(h, x_upairs_, 8, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    const unsigned long long pairs_within = *h;
    if (!exact_copy_out(out_counts, x_dcounts_, 4 * (size_t)n)) return false;
    if (out_labels) {
        if (pairs_within <= cap) {
            HIP_OK(density_pairs_launch(x_darena_, pairs_within, x_dcounts_, min_samples, x_uparent_, x_dattach_, st));
        } else { // the arena dropped records: the triangle once more, joined straight from the distances
            const auto phase_b = [&](const ExactScanArgs &a, unsigned tiles, hipStream_t s) {
                const ExactRangeDensityJoin sink{range, x_self_, x_dcounts_, min_samples, x_uparent_, x_dattach_};
                hipError_t e = hipSuccess;
                with_metric(metric_, [&](auto mt) { e = exact_range_density_join_scan_launch<mt>(a, sink, tiles, t.p.lds, s); });
                return e;
            };
            if (!exact_triangle_scan(t, phase_b, &measured)) return false;
            scans = 2;
        }
        int *d_labels = x_uparent_.get() + n;
        HIP_OK(density_labels_launch(x_uparent_, x_dattach_, x_dcounts_, min_samples, n, d_labels, st));
        if (!exact_copy_out(out_labels, d_labels, 4 * (size_t)n)) return false;
        count_kinds();
    }
    out_info[5] = pairs_within;
    out_info[6] = measured;
    out_info[7] = scans;
    return true;
}

// ---- near-duplicates over the graph's edges -------------------------------------------------------------------------
// exact_range_groups' host loop around graph_edge_kernel: the members are listed on the host, go up once as ids (the union-find's
// roots) and once as a bitset (the kernel's member test), and a round of `edge_round` (65 536) of them at a time are the OWNERS --
// their rows gathered into the exact family's query buffer as the by-id calls gather theirs, their ids left in x_self_.  One launch
// per round.  The union sink ends as exact_range_groups does; the list sink copies a round's counts and segments back and
// appends the edges, which the kernel left in their final order, to ge_*.
bool Device::graph_edges_run(const char *who, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, uint64_t *out_info,
                             bool keep_list)
{
    if (n_rows < 0 || (allow_bits && nbits < 0)) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    if (!allow_bits) nbits = 0;
    const long long n = std::min(n_rows, n_rows_hw_), n_allow = allow_bits ? std::min(nbits, n) : n;
    if (n > 0 && !keep_list && !out_labels) { set_dev_error(std::string(who) + ": bad argument"); return false; }
    if (n > 0 && (g_n_ <= 0 || !g_adj0_)) { set_dev_error(std::string(who) + ": no graph committed"); return false; }
    const long long n_mem = std::min<long long>(n_allow, g_n_); // a member is a row, allowed, and a node of the graph
    std::vector<int> members;
    std::vector<unsigned> bits((size_t)((std::max<long long>(n_mem, 0) + 31) / 32), 0u);
    for (long long id = 0; id < n_mem; ++id)
        if (!allow_bits || ((allow_bits[id >> 5] >> (id & 31)) & 1u)) {
            members.push_back((int)id);
            bits[(size_t)(id >> 5)] |= 1u << (id & 31);
        }
    const long long m = (long long)members.size();
    if (!keep_list) {
        for (long long v = 0; v < n; ++v) out_labels[v] = -1;
        for (const int v : members) out_labels[v] = v; // (what fewer than two members leave; the device's labels replace it otherwise)
        out_info[0] = (unsigned long long)m;
        out_info[1] = (unsigned long long)m;
    }
    if (m < 2) return true; // no edge between two members: no launch
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    const int seg = std::max(g_stride0_ - 1, 1);  // the longest layer-0 list
    const int nbc = std::max((seg + 7) & ~7, 8);
    const size_t lds = search_lds_bytes(0, 0, pitch_, false, nbc);
    if (lds > 64 * 1024) { set_dev_error(std::string(who) + ": dimension exceeds the LDS budget"); return false; }
    const int forced_round = diag("edge_round", 0);
    const long long round = std::min<long long>(m, forced_round > 0 ? forced_round : 65536);
    const size_t cap = (size_t)std::max<long long>(round, 1024);
    if (!x_queries_.grow((size_t)round * pitch_, cap * pitch_) || (metric_ == M_COS && !x_q_sn_.grow((size_t)round, cap))) return false;
    if (!e_bits_.grow(bits.size()) || !e_ctr_.grow(3)) return false;
    if (keep_list ? !e_cnt_.grow((size_t)round) || !e_keys_.grow((size_t)round * (size_t)seg) : !x_uparent_.grow(2 * (size_t)n)) return false;
    HIP_OK(hipMemcpyAsync(e_bits_, bits.data(), 4 * bits.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemsetAsync(e_ctr_, 0, 3 * sizeof(unsigned long long), st));
    if (!keep_list) {
        if (!upload_ids(members.data(), (int)m, x_ids_)) return false;
        HIP_OK(exact_union_init_launch(x_ids_, m, x_uparent_, n, st));
    }
    HIP_OK(hipStreamSynchronize(st)); // (a pageable source; the pinned stage is used again by the rounds)
    const AllowSet member_set{e_bits_, n_mem};
    const double *d_qsn = metric_ == M_COS ? x_q_sn_.get() : nullptr;
    int *job_counter = reinterpret_cast<int *>(e_ctr_.get());
    unsigned long long launches = 0;
    std::vector<int> h_cnt;
    std::vector<unsigned long long> h_keys;
    for (long long off = 0; off < m; off += round) {
        const int nr = (int)std::min<long long>(round, m - off);
        if (!gather_queries(members.data() + off, nr, x_self_, x_queries_, x_q_sn_)) return false;
        HIP_OK(hipMemsetAsync(job_counter, 0, sizeof(int), st));
        const auto launch = [&](auto kernel, const auto &sink) -> bool {
            const int slots = std::min(max_slots(), resident_blocks(kernel, lds, num_cu_));
            if (slots < 1) { set_dev_error(std::string(who) + ": the edge kernel does not fit a compute unit"); return false; }
            hipLaunchKernelGGL(kernel, dim3(std::min(nr, slots)), dim3(64), lds, st, d_rows_, d_row_sn_, x_queries_.get(), d_qsn, pitch_, g_adj0_, g_stride0_,
                               x_self_.get(), member_set, range, sink, nbc, nr, job_counter);
            HIP_OK(hipGetLastError());
            return true;
        };
        bool ok = false;
        if (keep_list) {
            const EdgeList sink{e_keys_, e_cnt_, seg};
            with_metric(metric_, [&](auto mt) { ok = launch(&graph_edge_kernel<mt, EdgeList>, sink); });
        } else {
            const EdgeUnion sink{x_uparent_, e_ctr_.get() + 1};
            with_metric(metric_, [&](auto mt) { ok = launch(&graph_edge_kernel<mt, EdgeUnion>, sink); });
        }
        if (!ok) return false;
        launches += 1;
        if (!keep_list) continue;
        h_cnt.resize((size_t)nr);
        h_keys.resize((size_t)nr * (size_t)seg);
        if (!exact_copy_out(h_cnt.data(), e_cnt_, 4 * (size_t)nr) || !exact_copy_out(h_keys.data(), e_keys_, 8 * (size_t)nr * (size_t)seg)) return false;
        for (int j = 0; j < nr; ++j) {
            const int c = std::min(std::max(h_cnt[(size_t)j], 0), seg);
            for (int e = 0; e < c; ++e) {
                const unsigned long long key = h_keys[(size_t)j * (size_t)seg + (size_t)e];
                const uint32_t db = (uint32_t)(key >> 32);
                float d;
                memcpy(&d, &db, 4);
                ge_src_.push_back(members[(size_t)(off + j)]);
                ge_dst_.push_back((int)(uint32_t)key);
                ge_d_.push_back(d);
            }
        }
    }
    if (keep_list) {
        HIP_OK(hipStreamSynchronize(st));
        return true;
    }
    int *d_labels = x_uparent_.get() + n;
    HIP_OK(exact_union_labels_launch(x_uparent_, n, d_labels, st));
    if (!exact_copy_out(out_labels, d_labels, 4 * (size_t)n)) return false;
    unsigned long long *h = static_cast<unsigned long long *>(pinned_stage(16));
    if (!h) return false;
    HIP_OK(hipMemcpyAsync(h, e_ctr_.get() + 1, 16, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    unsigned long long groups = 0;
    for (const int v : members) groups += (unsigned long long)(out_labels[v] == v);
    out_info[1] = groups;
    out_info[2] = h[0];
    out_info[3] = h[1];
    out_info[4] = launches;
    return true;
}

bool Device::graph_edge_groups(long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, uint64_t *out_info)
{
    if (!out_info) { set_dev_error("graph_edge_groups: bad argument"); return false; }
    for (int i = 0; i < 5; ++i) out_info[i] = 0;
    return graph_edges_run("graph_edge_groups", n_rows, range, allow_bits, nbits, out_labels, out_info, false);
}

bool Device::graph_near_edges(long long n_rows, float range, const uint32_t *allow_bits, long long nbits, long long *out_count)
{
    ge_src_.clear();
    ge_dst_.clear();
    ge_d_.clear();
    if (out_count) *out_count = 0;
    if (!out_count) { set_dev_error("graph_near_edges: bad argument"); return false; }
    if (!graph_edges_run("graph_near_edges", n_rows, range, allow_bits, nbits, nullptr, nullptr, true)) {
        ge_src_.clear();
        ge_dst_.clear();
        ge_d_.clear();
        return false;
    }
    *out_count = (long long)ge_src_.size();
    return true;
}

bool Device::graph_near_edges_results(int *out_src, int *out_dst, float *out_d)
{
    if (ge_src_.empty()) return true;
    if (!out_src || !out_dst || !out_d) { set_dev_error("graph_near_edges_results: null argument"); return false; }
    memcpy(out_src, ge_src_.data(), 4 * ge_src_.size());
    memcpy(out_dst, ge_dst_.data(), 4 * ge_dst_.size());
    memcpy(out_d, ge_d_.data(), 4 * ge_d_.size());
    return true;
}

// ---- synchronous conveniences behind the C ABI ---------------------------------------
// Distance(int, TVector) for nq (query, candidate list) pairs.  Runs on the context's two step-
// buffer sets, ping-pong: while the GPU measures one set the host packs the next and unpacks the
// previous -- nothing is allocated per call once the sets exist.
bool Device::dist_query_batch(const float *queries, int nq, const int *offsets, const int *ids, float *out)
{
    if (nq <= 0) return true;
    if (!offsets || !out) { set_dev_error("dist_query_batch: null argument"); return false; }
    if (offsets[0] != 0) { set_dev_error("dist_query_batch: cand_offsets[0] must be 0"); return false; }
    for (int i = 0; i < nq; ++i)
        if (offsets[i + 1] < offsets[i]) { set_dev_error("dist_query_batch: cand_offsets must be non-decreasing"); return false; }
    const int total = offsets[nq];
    if (total > 0 && !ids) { set_dev_error("dist_query_batch: null cand_ids"); return false; }
    if (queries) { if (!set_queries(queries, nq)) return false; }
    else if (nq > n_queries_) { set_dev_error("dist_query_batch: queries == NULL needs a resident query set of at least nq rows (hnswdev_set_queries)"); return false; }
    const int stride = 64, NS = 8192;
    int *rec[2]; float *dist[2];
    StepBuffers **sets = abi_sb_ + 2; // private sets: a caller's hnswdev_step_buffers pointers stay valid
    for (int g = 0; g < 2; ++g)
        if (!step_buffers(2 + g, NS, stride, &rec[g], &dist[g], true)) return false;
    const int rec_stride = sets[0]->rec_stride;
    std::vector<std::pair<int, int>> where[2]; // (global offset, count) per slot of each set
    bool pend[2] = {false, false};
    auto collect = [&](int g) -> bool {
        if (!pend[g]) return true;
        pend[g] = false;
        if (!wait_step(sets[g])) return false;
        for (size_t sidx = 0; sidx < where[g].size(); ++sidx)
            memcpy(out + where[g][sidx].first, dist[g] + sidx * (size_t)stride, sizeof(float) * (size_t)where[g][sidx].second);
        return true;
    };
    int qi = 0, pos = 0, g = 0; // next (query, offset within its list) to schedule
    bool ok = true;
    while (ok && qi < nq) {
        ok = collect(g); // this set's previous step
        if (!ok) break;
        where[g].clear();
        uint64_t ev = 0;
        int used = 0;
        while (qi < nq && used < NS) {
            const int m = offsets[qi + 1] - offsets[qi] - pos;
            if (m <= 0) { ++qi; pos = 0; continue; }
            const int take = std::min(m, stride);
            const int at = offsets[qi] + pos;
            int *r = rec[g] + (size_t)used * rec_stride;
            r[0] = take;
            r[1] = qi;
            memcpy(r + 2, ids + at, sizeof(int) * (size_t)take);
            where[g].emplace_back(at, take);
            ev += (uint64_t)take;
            ++used;
            pos += take;
        }
        if (used == 0) break;
        ok = launch_step(sets[g], used, ev);
        pend[g] = ok;
        g ^= 1;
    }
    // drain in submission order; on failure still wait for what is in flight
    const bool a = collect(g), b = collect(g ^ 1);
    return ok && a && b;
}

bool Device::dist_pair_batch(const int *a, const int *b, int n, float *out)
{
    if (n <= 0) return true;
    if (!a || !b || !out) { set_dev_error("dist_pair_batch: null argument"); return false; }
    if (!bind()) return false;
    hipStream_t st = S(stream_);
    if (!d_guard_) { if (!d_guard_.grow(1)) return false; HIP_OK(hipMemsetAsync(d_guard_, 0, sizeof(int), st)); }
    if (!pair_dev_.grow(3 * (size_t)n)) return false; // [a | b | out], grown on demand, kept
    int *hs = static_cast<int *>(pinned_stage(sizeof(int) * (3 * (size_t)n + 1)));
    if (!hs) return false;
    memcpy(hs, a, sizeof(int) * (size_t)n);
    memcpy(hs + n, b, sizeof(int) * (size_t)n);
    int *da = pair_dev_, *db = pair_dev_ + n;
    float *dout = reinterpret_cast<float *>(pair_dev_.get() + 2 * (size_t)n);
    HIP_OK(hipMemcpyAsync(da, hs, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice, st));
    dim3 grid((unsigned)(((long long)n * 8 + 255) / 256)), block(256);
    with_metric(metric_, [&](auto m) {
        hipLaunchKernelGGL(pair_distance_kernel<m>, grid, block, 0, st, d_rows_, d_row_sn_, pitch_, da, db, dout, n, n_rows_hw_, d_guard_);
    });
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(hs + 2 * (size_t)n, dout, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hs + 3 * (size_t)n, d_guard_, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    memcpy(out, hs + 2 * (size_t)n, sizeof(float) * (size_t)n);
    stats_.launches++;
    stats_.evals += (uint64_t)n;
    if (hs[3 * (size_t)n] != 0) {
        HIP_OK(hipMemsetAsync(d_guard_, 0, sizeof(int), st));
        set_dev_error("dist_pair_batch: id outside uploaded rows (those distances are NaN)");
        return false;
    }
    return true;
}

// test hook (exported through the C ABI as hnswdev_test_sqrt_rn)
bool device_sqrt_rn(int device, const double *in, double *out, int n)
{
    HIP_OK(hipSetDevice(device));
    DevBuf<double> di, dout;
    if (!di.grow((size_t)n) || !dout.grow((size_t)n)) return false;
    HIP_OK(hipMemcpy(di, in, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sqrt_rn_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, di.get(), dout.get(), n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    return true;
}

} // namespace hnsw

// ------------------------------------------------------------------------------------
// C ABI (B): hnswdev_*
// ------------------------------------------------------------------------------------
using hnsw::Device;

extern "C" {

#define DEV_API __attribute__((visibility("default")))

DEV_API int hnswdev_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { hnsw::set_dev_error(std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); return -1; }
    return n;
}

DEV_API int hnswdev_create(int device, int dim, int metric, long long capacity, void **ctx)
{
    if (!ctx) { hnsw::set_dev_error("hnswdev_create: null ctx"); return -1; }
    *ctx = nullptr;
    Device *d = Device::create(device, dim, metric, capacity);
    if (!d) return -1;
    *ctx = d;
    return 0;
}
DEV_API int hnswdev_destroy(void *ctx)
{
    delete (Device *)ctx;
    return 0;
}
// every call on a context: serialised, and its errors are filed under that context
#define CTX_OR_FAIL()                                                     \
    Device *d = (Device *)ctx;                                            \
    if (!d) { hnsw::set_dev_error("null hnswdev context"); return -1; }   \
    std::lock_guard<std::mutex> ctx_lock_(d->mutex());                    \
    hnsw::ErrorScope ctx_scope_(d)

DEV_API int hnswdev_reserve(void *ctx, long long capacity) { CTX_OR_FAIL(); return d->reserve(capacity) ? 0 : -1; }
DEV_API int hnswdev_upload_rows(void *ctx, int first_id, int n, const float *rows) { CTX_OR_FAIL(); return d->upload_rows(first_id, n, rows) ? 0 : -1; }
DEV_API int hnswdev_download_rows(void *ctx, int first_id, int n, float *rows) { CTX_OR_FAIL(); return d->download_rows(first_id, n, rows) ? 0 : -1; }
DEV_API int hnswdev_dist_query_batch(void *ctx, const float *queries, int nq, const int *cand_offsets, const int *cand_ids, float *out)
{
    CTX_OR_FAIL();
    return d->dist_query_batch(queries, nq, cand_offsets, cand_ids, out) ? 0 : -1;
}
DEV_API int hnswdev_dist_pair_batch(void *ctx, const int *a_ids, const int *b_ids, int n, float *out)
{
    CTX_OR_FAIL();
    return d->dist_pair_batch(a_ids, b_ids, n, out) ? 0 : -1;
}
DEV_API int hnswdev_set_queries(void *ctx, const float *queries, int nq) { CTX_OR_FAIL(); return d->set_queries(queries, nq) ? 0 : -1; }
DEV_API int hnswdev_step_buffers(void *ctx, int set, int nslots, int stride, int **rec, float **dist) { CTX_OR_FAIL(); return d->step_buffers(set, nslots, stride, rec, dist) ? 0 : -1; }
DEV_API int hnswdev_step_submit(void *ctx, int set, int nslots_used) { CTX_OR_FAIL(); return d->step_submit(set, nslots_used) ? 0 : -1; }
DEV_API int hnswdev_step_wait(void *ctx, int set) { CTX_OR_FAIL(); return d->step_wait(set) ? 0 : -1; }
DEV_API int hnswdev_graph_begin(void *ctx, int n, int max_edges, const int *levels) { CTX_OR_FAIL(); return d->graph_begin(n, max_edges, levels) ? 0 : -1; }
DEV_API int hnswdev_graph_set_layer(void *ctx, int layer, const int *counts, const int *edges, int stride) { CTX_OR_FAIL(); return d->graph_set_layer(layer, counts, edges, stride) ? 0 : -1; }
DEV_API int hnswdev_graph_commit(void *ctx) { CTX_OR_FAIL(); return d->graph_commit() ? 0 : -1; }
DEV_API int hnswdev_knn_search(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int *out_ids, float *out_dists, int *out_flags)
{
    CTX_OR_FAIL();
    return d->knn_search(queries, nq, entry_point, k_beam, k_out, out_ids, out_dists, out_flags) ? 0 : -1;
}
DEV_API int hnswdev_knn_search_filtered(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, const uint32_t *allow_bits,
                                        long long nbits, int *out_ids, float *out_dists, int *out_flags)
{
    CTX_OR_FAIL();
    return d->knn_search_filtered(queries, nq, entry_point, k_beam, k_out, allow_bits, nbits, out_ids, out_dists, out_flags) ? 0 : -1;
}
DEV_API int hnswdev_knn_search_grouped(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int layer, const int *row_group,
                                       long long n_row_group, const int *query_group, int n_groups, int *out_ids, float *out_dists, int *out_flags)
{
    CTX_OR_FAIL();
    return d->knn_search_grouped(queries, nq, entry_point, k_beam, k_out, row_group, n_row_group, query_group, n_groups, out_ids, out_dists, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_knn_search_tagged(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int layer, const uint32_t *row_tags,
                                      long long n_row_tags, const uint32_t *query_tags, int match, int *out_ids, float *out_dists, int *out_flags)
{
    CTX_OR_FAIL();
    return d->knn_search_tagged(queries, nq, entry_point, k_beam, k_out, row_tags, n_row_tags, query_tags, match, out_ids, out_dists, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_exact_knn_tagged(void *ctx, const float *queries, int nq, long long n_rows, int k, const uint32_t *row_tags, long long n_row_tags,
                                     const uint32_t *query_tags, int match, int *out_ids, float *out_dists)
{
    CTX_OR_FAIL();
    return d->exact_knn_tagged(queries, nq, n_rows, k, row_tags, n_row_tags, query_tags, match, out_ids, out_dists) ? 0 : -1;
}
DEV_API int hnswdev_tag_list_ms(void *ctx, double *out_ms)
{
    CTX_OR_FAIL();
    if (!out_ms) return -1;
    *out_ms = d->tag_list_ms();
    return 0;
}
DEV_API int hnswdev_range_search(void *ctx, const float *queries, int nq, int entry_point, float range, int *out_counts, int *out_flags)
{
    CTX_OR_FAIL();
    return d->range_search(queries, nq, entry_point, range, out_counts, out_flags) ? 0 : -1;
}
DEV_API int hnswdev_range_search_filtered(void *ctx, const float *queries, int nq, int entry_point, float range, const uint32_t *allow_bits, long long nbits,
                                          int *out_counts, int *out_flags)
{
    CTX_OR_FAIL();
    if (!allow_bits || nbits < 0) { hnsw::set_dev_error("hnswdev_range_search_filtered: allow_bits must not be NULL and nbits must be >= 0"); return -1; }
    return d->range_search_filtered(queries, nq, entry_point, range, allow_bits, nbits, out_counts, out_flags) ? 0 : -1;
}
DEV_API int hnswdev_knn_search_at_layer(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int layer,
                                        const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists, int *out_flags)
{
    CTX_OR_FAIL();
    if (!allow_bits) return d->knn_search(queries, nq, entry_point, k_beam, k_out, out_ids, out_dists, out_flags, layer) ? 0 : -1;
    return d->knn_search_filtered(queries, nq, entry_point, k_beam, k_out, allow_bits, nbits, out_ids, out_dists, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_range_search_at_layer(void *ctx, const float *queries, int nq, int entry_point, float range, int layer, const uint32_t *allow_bits,
                                          long long nbits, int *out_counts, int *out_flags)
{
    CTX_OR_FAIL();
    if (allow_bits && nbits < 0) { hnsw::set_dev_error("hnswdev_range_search_at_layer: nbits must be >= 0"); return -1; }
    return d->range_search_filtered(queries, nq, entry_point, range, allow_bits, allow_bits ? nbits : 0, out_counts, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_range_search_grouped(void *ctx, const float *queries, int nq, int entry_point, float range, int layer, const int *row_group,
                                         long long n_row_group, const int *query_group, int n_groups, int *out_counts, int *out_flags)
{
    CTX_OR_FAIL();
    return d->range_search_grouped(queries, nq, entry_point, range, row_group, n_row_group, query_group, n_groups, out_counts, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_range_search_tagged(void *ctx, const float *queries, int nq, int entry_point, float range, int layer, const uint32_t *row_tags,
                                        long long n_row_tags, const uint32_t *query_tags, int match, int *out_counts, int *out_flags)
{
    CTX_OR_FAIL();
    return d->range_search_tagged(queries, nq, entry_point, range, row_tags, n_row_tags, query_tags, match, out_counts, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_multilayer_search(void *ctx, const float *queries, int nq, int entry_point, int k, int max_layer, int min_layer, int layers_cap,
                                      int *out_ids, float *out_dists, int *out_flags)
{
    CTX_OR_FAIL();
    return d->multilayer_search_abi(queries, nq, entry_point, k, max_layer, min_layer, layers_cap, out_ids, out_dists, out_flags);
}
DEV_API int hnswdev_exact_knn(void *ctx, const float *queries, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids,
                              float *out_dists)
{
    CTX_OR_FAIL();
    return d->exact_knn(queries, nq, n_rows, k, allow_bits, nbits, out_ids, out_dists) ? 0 : -1;
}
// query by stored id
DEV_API int hnswdev_gather_rows(void *ctx, const int *ids, int n, float *out)
{
    CTX_OR_FAIL();
    return d->gather_rows(ids, n, out) ? 0 : -1;
}
DEV_API int hnswdev_knn_search_by_id(void *ctx, const int *ids, int nq, int entry_point, int k_beam, int k_out, int layer, int *out_ids, float *out_dists,
                                     int *out_flags)
{
    CTX_OR_FAIL();
    return d->knn_search_by_id(ids, nq, entry_point, k_beam, k_out, out_ids, out_dists, out_flags, layer) ? 0 : -1;
}
DEV_API int hnswdev_exact_knn_by_id(void *ctx, const int *ids, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids,
                                    float *out_dists)
{
    CTX_OR_FAIL();
    return d->exact_knn_by_id(ids, nq, n_rows, k, allow_bits, nbits, out_ids, out_dists) ? 0 : -1;
}
DEV_API int hnswdev_exact_range(void *ctx, const float *queries, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits,
                                int *out_counts)
{
    CTX_OR_FAIL();
    return d->exact_range(queries, nq, n_rows, range, allow_bits, nbits, out_counts) ? 0 : -1;
}
DEV_API int hnswdev_exact_range_results(void *ctx, int *out_ids, float *out_dists) { CTX_OR_FAIL(); return d->exact_range_results(out_ids, out_dists) ? 0 : -1; }
DEV_API int hnswdev_exact_range_by_id(void *ctx, const int *ids, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits,
                                      int *out_counts)
{
    CTX_OR_FAIL();
    return d->exact_range_by_id(ids, nq, n_rows, range, allow_bits, nbits, out_counts) ? 0 : -1;
}
DEV_API int hnswdev_exact_range_groups(void *ctx, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels,
                                       uint64_t *out_info)
{
    CTX_OR_FAIL();
    return d->exact_range_groups(n_rows, range, allow_bits, nbits, out_labels, out_info) ? 0 : -1;
}
DEV_API int hnswdev_exact_range_density(void *ctx, long long n_rows, float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels,
                                        int *out_counts, uint64_t *out_info)
{
    CTX_OR_FAIL();
    return d->exact_range_density(n_rows, range, min_samples, allow_bits, nbits, out_labels, out_counts, out_info) ? 0 : -1;
}
DEV_API int hnswdev_graph_edge_groups(void *ctx, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels,
                                      uint64_t *out_info)
{
    CTX_OR_FAIL();
    return d->graph_edge_groups(n_rows, range, allow_bits, nbits, out_labels, out_info) ? 0 : -1;
}
DEV_API int hnswdev_graph_near_edges(void *ctx, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, long long *out_count)
{
    CTX_OR_FAIL();
    return d->graph_near_edges(n_rows, range, allow_bits, nbits, out_count) ? 0 : -1;
}
DEV_API int hnswdev_graph_near_edges_results(void *ctx, int *out_src, int *out_dst, float *out_dists, long long cap)
{
    CTX_OR_FAIL();
    if (cap < (long long)d->graph_near_edges_total()) {
        hnsw::set_dev_error("graph_near_edges_results: cap = " + std::to_string(cap) + " is below the " + std::to_string(d->graph_near_edges_total()) + " edges kept");
        return -1;
    }
    return d->graph_near_edges_results(out_src, out_dst, out_dists) ? 0 : -1;
}
DEV_API int hnswdev_exact_knn_grouped(void *ctx, const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group,
                                      const int *query_group, int n_groups, int *out_ids, float *out_dists)
{
    CTX_OR_FAIL();
    return d->exact_knn_grouped(queries, nq, n_rows, k, row_group, n_row_group, query_group, n_groups, out_ids, out_dists) ? 0 : -1;
}
DEV_API int hnswdev_exact_knn_collapsed(void *ctx, const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group,
                                        int per_group, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists)
{
    CTX_OR_FAIL();
    return d->exact_knn_collapsed(queries, nq, n_rows, k, row_group, n_row_group, per_group, allow_bits, nbits, out_ids, out_dists) ? 0 : -1;
}
DEV_API int hnswdev_exact_range_grouped(void *ctx, const float *queries, int nq, long long n_rows, float range, const int *row_group, long long n_row_group,
                                        const int *query_group, int n_groups, int *out_counts)
{
    CTX_OR_FAIL();
    return d->exact_range_grouped(queries, nq, n_rows, range, row_group, n_row_group, query_group, n_groups, out_counts) ? 0 : -1;
}
DEV_API int hnswdev_exact_range_tagged(void *ctx, const float *queries, int nq, long long n_rows, float range, const uint32_t *row_tags, long long n_row_tags,
                                       const uint32_t *query_tags, int match, int *out_counts)
{
    CTX_OR_FAIL();
    return d->exact_range_tagged(queries, nq, n_rows, range, row_tags, n_row_tags, query_tags, match, out_counts) ? 0 : -1;
}
DEV_API int hnswdev_exact_grouped_list_ms(void *ctx, double *out_ms)
{
    CTX_OR_FAIL();
    if (!out_ms) return -1;
    *out_ms = d->exact_grouped_list_ms();
    return 0;
}
DEV_API int hnswdev_graph_info(void *ctx, int layer, const uint32_t *live_bits, long long nbits, int with_in_edges, hnsw_mi355x_layer_info *out)
{
    CTX_OR_FAIL();
    return d->graph_info_layer("hnswdev_graph_info", layer) && d->graph_info(layer, live_bits, nbits, with_in_edges != 0, out) ? 0 : -1;
}
DEV_API int hnswdev_graph_components(void *ctx, int layer, const uint32_t *live_bits, long long nbits, int *out_count)
{
    CTX_OR_FAIL();
    return d->graph_info_layer("hnswdev_graph_components", layer) && d->graph_components(layer, live_bits, nbits, out_count) ? 0 : -1;
}
DEV_API int hnswdev_graph_reach_layer(void *ctx, int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits,
                                     uint32_t *out_reached_bits, int *out_hops, uint64_t out_summary[4])
{
    CTX_OR_FAIL();
    return d->graph_info_layer("hnswdev_graph_reach_layer", layer) &&
                   d->graph_reach_layer(layer, live_bits, nbits, seed_bits, seed_nbits, out_reached_bits, out_hops, out_summary) ? 0 : -1;
}
DEV_API int hnswdev_graph_reach(void *ctx, int entry_point, const uint32_t *live_bits, long long nbits, int min_layer, hnsw_mi355x_layer_reach *out_layers,
                               int cap, uint32_t *out_reached_bits, int *out_hops)
{
    CTX_OR_FAIL();
    int top;
    if (!d->graph_reach_top("hnswdev_graph_reach", entry_point, &top)) return -1;
    return d->graph_reach(entry_point, top, live_bits, nbits, min_layer, out_layers, cap, out_reached_bits, out_hops);
}
DEV_API int hnswdev_graph_repair_propose(void *ctx, int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits, int cands,
                                         int max_edges, int *out_n, int *out_ids, int *out_cands, int *out_codes, int cap)
{
    CTX_OR_FAIL();
    if (!d->graph_info_layer("hnswdev_graph_repair_propose", layer)) return -1;
    return d->graph_repair_propose(layer, live_bits, nbits, seed_bits, seed_nbits, cands, max_edges, out_n, out_ids, out_cands, out_codes, cap);
}
DEV_API int hnswdev_range_results(void *ctx, int *out_ids, float *out_dists) { CTX_OR_FAIL(); return d->range_results(out_ids, out_dists) ? 0 : -1; }
DEV_API int hnswdev_sync(void *ctx) { CTX_OR_FAIL(); return d->sync() ? 0 : -1; }
DEV_API int hnswdev_set_profiling(void *ctx, int enabled) { CTX_OR_FAIL(); d->set_profiling(enabled != 0); return 0; }
DEV_API int hnswdev_get_stats(void *ctx, hnswdev_stats *out)
{
    CTX_OR_FAIL();
    if (!out) return -1;
    d->get_stats(out);
    return 0;
}
DEV_API int hnswdev_reset_stats(void *ctx) { CTX_OR_FAIL(); d->reset_stats(); return 0; }
// The getters of the counter blocks, hnswdev_<block>(ctx, out[slots]), one per row of counter_blocks.h
#define HNSW_COUNTER_GETTER(NAME, SCOPE, ...)                   \
    DEV_API int hnswdev_##NAME(void *ctx, uint64_t *out)        \
    {                                                           \
        CTX_OR_FAIL();                                          \
        if (!out) return -1;                                    \
        d->counters(hnsw::CounterBlock::NAME, out);             \
        return 0;                                               \
    }
HNSW_FOR_EACH_COUNTER_BLOCK(HNSW_COUNTER_GETTER)
#undef HNSW_COUNTER_GETTER
static int copy_error(const std::string &s, char *buf, int buf_len)
{
    if (buf && buf_len > 0) {
        int w = std::min<int>((int)s.size(), buf_len - 1);
        memcpy(buf, s.data(), (size_t)w);
        buf[w] = 0;
    }
    return (int)s.size();
}
DEV_API int hnswdev_last_error(char *buf, int buf_len) { return copy_error(hnsw::get_dev_error(), buf, buf_len); }
DEV_API int hnswdev_ctx_last_error(void *ctx, char *buf, int buf_len)
{
    Device *d = (Device *)ctx;
    if (!d) return copy_error("null hnswdev context", buf, buf_len);
    return copy_error(d->error(), buf, buf_len);
}
// test hook: correctly rounded device double sqrt (cosine epilogue), checked against the host's
DEV_API int hnswdev_test_sqrt_rn(int device, const double *in, double *out, int n)
{
    return hnsw::device_sqrt_rn(device, in, out, n) ? 0 : -1;
}

} // extern "C"
