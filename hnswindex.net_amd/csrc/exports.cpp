// exports.cpp -- C ABI (A): the reference's 16 `hnsw_*` exports
// (/root/reference/bindings/HNSWIndex.Native/HNSWIndexExports.cs:27-273), same names,
// signatures, return codes and padding, over the MI355X-backed HnswIndex.
#include <algorithm>
#include <thread>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/hnsw_mi355x.h"
#include "hnsw_index.h"
#include "diag.h"
#include "range_replay.h"
#include "snapshot_io.h"

using hnsw::HnswIndex;
using hnsw::Params;

namespace {
// Exports.cs:11-12,16: process-global last error and pending parameters (unsynchronised in
// the reference; a mutex here costs nothing and changes no observable behaviour).
std::mutex g_mu;
std::string g_last_error;
Params g_pending;

void set_error(const std::string &s)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_last_error = s;
}
} // namespace

#define API extern "C" __attribute__((visibility("default")))
// exclusive use of one handle (HnswIndex::mutex; hnsw_knn_query calls share it, see hnsw_index.h)
#define LOCK_INDEX(h) std::unique_lock<std::shared_mutex> index_lock_(static_cast<HnswIndex *>(h)->mutex())

API int hnsw_get_last_error_utf8(void *buf, int buf_len) // :27-39
{
    std::lock_guard<std::mutex> lk(g_mu);
    const int need = (int)g_last_error.size();
    if (buf_len > 0 && buf != nullptr) {
        int to_write = std::max(0, buf_len - 1);
        int written = std::min(need, to_write);
        std::memcpy(buf, g_last_error.data(), (size_t)written);
        static_cast<char *>(buf)[written] = 0;
    }
    return need;
}

static int parse_metric(const char *distance_metric) // :47-60
{
    return distance_metric ? hnsw::metric_by_name(distance_metric) : -1; // the names: device_backend.h, HNSW_FOR_EACH_METRIC
}

API void *hnsw_create(const char *distance_metric) // :41-65
{
    const int metric = parse_metric(distance_metric);
    if (metric < 0) {
        set_error(std::string("System.ArgumentException: Unsupported distance metric: ") + (distance_metric ? distance_metric : "(null)"));
        return nullptr;
    }
    Params p;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        p = g_pending;
    }
    std::string err;
    HnswIndex *ix = HnswIndex::create(metric, p, err);
    if (!ix) { set_error(err); return nullptr; }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_pending = Params(); // :61 reset parameters for next instance
    }
    return ix;
}

API void hnsw_free(void *handle) // :67-73
{
    if (!handle) return;
    delete static_cast<HnswIndex *>(handle);
}

API int hnsw_add(void *handle, const float *vectors, int count, int dim, int *out_ids) // :75-100
{
    if (!handle) return 0;
    if (!vectors || count <= 0 || dim <= 0) return 0;
    LOCK_INDEX(handle);
    std::string err;
    int n = static_cast<HnswIndex *>(handle)->add(vectors, count, dim, out_ids, err);
    if (n < 0) { set_error(err); return -1; }
    return n;
}

API int hnsw_remove(void *handle, const int *ids, int count) // :102-117
{
    if (!handle) return 0;
    if (!ids || count <= 0) return 0;
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->remove(ids, count, err) < 0) { set_error(err); return -1; }
    return 0;
}

API int hnsw_knn_query(void *handle, const float *vectors, int count, int dim, int k, int *out_ids, float *out_dists) // :119-149
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || dim <= 0) { set_error("System.ArgumentNullException: hnsw_knn_query"); return -1; }
    std::string err;
    HnswIndex *ix = static_cast<HnswIndex *>(handle);
    {   // same-type calls overlap (README.md:64-65): shared lock, a query lane per call
        std::shared_lock<std::shared_mutex> rd(ix->mutex());
        int rc = 0;
        if (ix->knn_query_concurrent(vectors, count, dim, k, out_ids, out_dists, rc, err)) {
            if (rc < 0) { set_error(err); return -1; }
            return 0;
        }
    }
    LOCK_INDEX(handle);
    int rc = ix->knn_query(vectors, count, dim, k, out_ids, out_dists, err);
    if (rc < 0) { set_error(err); return -1; }
    return 0;
}

// hnsw_knn_query with an allow-set (BatchKnnQuery(queries, k, filterFnc), HNSWIndex.cs:129-137): filtered calls take the handle
// exclusively (no query lane)
API int hnsw_mi355x_knn_query_filtered(void *handle, const float *vectors, int count, int dim, int k, const uint32_t *allow_bits, long long nbits,
                                       int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_knn_query_filtered"); return -1; }
    if (!allow_bits || nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_knn_query_filtered: allow_bits must not be NULL and nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->knn_query_general(vectors, count, dim, k, 0, allow_bits, nbits, out_ids, out_dists, err) < 0) { set_error(err); return -1; }
    return 0;
}

// Exact k nearest neighbours: the flat scan over the live ids an allow-set allows.  Exclusive, like the filtered call.
API int hnsw_mi355x_exact_knn_query(void *handle, const float *vectors, int count, int dim, int k, const uint32_t *allow_bits, long long nbits,
                                    int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_knn_query"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_exact_knn_query: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->exact_knn_query(vectors, count, dim, k, allow_bits, nbits, out_ids, out_dists, err) < 0) { set_error(err); return -1; }
    return 0;
}

// ---- query by stored id.  Exclusive, like the filtered calls: they make the stored rows the resident queries or
// use the scan's buffers.  An id that is not live: -1 and a message that names it.
// HNSWIndex.Items() for a list of ids: the stored rows as floats, ids in any order, repeats allowed.
API int hnsw_mi355x_get_vectors(void *handle, const int *ids, int n, float *out)
{
    if (!handle) return 0;
    if (n <= 0) return 0;
    if (!ids || !out) { set_error("System.ArgumentNullException: hnsw_mi355x_get_vectors"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->get_vectors(ids, n, out, err) < 0) { set_error(err); return -1; }
    return 0;
}
// KnnQuery on `layer` for the stored rows of ids, each answered from every id but its own: one gather and one traversal on the device.
API int hnsw_mi355x_knn_query_by_id(void *handle, const int *ids, int count, int k, int layer, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!ids || !out_ids || !out_dists) { set_error("System.ArgumentNullException: hnsw_mi355x_knn_query_by_id"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->knn_query_by_id(ids, count, k, layer, out_ids, out_dists, err) < 0) { set_error(err); return -1; }
    return 0;
}
// The flat scan for the stored rows of ids: the candidates are allow_bits (NULL: every live id) minus the query's own id.
API int hnsw_mi355x_exact_knn_query_by_id(void *handle, const int *ids, int count, int k, const uint32_t *allow_bits, long long nbits, int *out_ids,
                                          float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!ids || !out_ids || !out_dists) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_knn_query_by_id"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_exact_knn_query_by_id: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->exact_knn_query_by_id(ids, count, k, allow_bits, nbits, out_ids, out_dists, err) < 0) { set_error(err); return -1; }
    return 0;
}

// Exact k nearest neighbours with a candidate group per query: one scan for every group.  Exclusive, like the call above.
API int hnsw_mi355x_exact_knn_query_grouped(void *handle, const float *vectors, int count, int dim, int k, const int *row_group, long long n_row_group,
                                            const int *query_group, int n_groups, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !query_group || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_knn_query_grouped"); return -1; }
    if (!row_group || n_row_group < 0) {
        set_error("System.ArgumentException: hnsw_mi355x_exact_knn_query_grouped: row_group must not be NULL and n_row_group must be >= 0");
        return -1;
    }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->exact_knn_query_grouped(vectors, count, dim, k, row_group, n_row_group, query_group, n_groups, out_ids, out_dists, err) < 0) {
        set_error(err);
        return -1;
    }
    return 0;
}

// Exact k nearest neighbours with at most per_group results per label.  Exclusive, like the calls above.
API int hnsw_mi355x_exact_knn_query_collapsed(void *handle, const float *vectors, int count, int dim, int k, const int *row_group, long long n_row_group,
                                              int per_group, const uint32_t *allow_words, long long nbits, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_knn_query_collapsed"); return -1; }
    if (allow_words && nbits < 0) { set_error("System.ArgumentOutOfRangeException: hnsw_mi355x_exact_knn_query_collapsed: nbits < 0"); return -1; }
    if (!row_group || n_row_group < 0) {
        set_error("System.ArgumentException: hnsw_mi355x_exact_knn_query_collapsed: row_group must not be NULL and n_row_group must be >= 0");
        return -1;
    }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->exact_knn_query_collapsed(vectors, count, dim, k, row_group, n_row_group, per_group, allow_words, nbits, out_ids, out_dists, err) < 0) {
        set_error(err);
        return -1;
    }
    return 0;
}

// KnnQuery with at most per_group results per label: the traversal at k = beam, collapsed to k.
API int hnsw_mi355x_knn_query_collapsed(void *handle, const float *vectors, int count, int dim, int k, int beam, const int *row_group, long long n_row_group,
                                        int per_group, int layer, const uint32_t *allow_words, long long nbits, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_knn_query_collapsed"); return -1; }
    if (allow_words && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_knn_query_collapsed: nbits must be >= 0"); return -1; }
    if (!row_group || n_row_group < 0) {
        set_error("System.ArgumentException: hnsw_mi355x_knn_query_collapsed: row_group must not be NULL and n_row_group must be >= 0");
        return -1;
    }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->knn_query_collapsed(vectors, count, dim, k, beam, row_group, n_row_group, per_group, layer, allow_words, nbits, out_ids, out_dists, err) < 0) {
        set_error(err); // (hnsw_index.cpp names the exception per case: a device failure is no argument error)
        return -1;
    }
    return 0;
}

// The tagged calls: a tag word per id, a mask per query, `match` 0 any / 1 all.  The arguments both check here.
static bool tagged_args(const char *who, bool pointers_ok, const uint32_t *row_tags, long long n_row_tags, int match)
{
    if (!pointers_ok) { set_error(std::string("System.ArgumentNullException: ") + who); return false; }
    if (!row_tags || n_row_tags < 0) { set_error(std::string("System.ArgumentException: ") + who + ": row_tags must not be NULL and n_row_tags must be >= 0"); return false; }
    if (match != 0 && match != 1) { set_error(std::string("System.ArgumentOutOfRangeException: ") + who + ": match = " + std::to_string(match) + " is neither 0 (any) nor 1 (all)"); return false; }
    return true;
}
// The flat scan with a tag mask per query: every distinct mask a candidate list, built on the device.
API int hnsw_mi355x_exact_knn_query_tagged(void *handle, const float *vectors, int count, int dim, int k, const uint32_t *row_tags, long long n_row_tags,
                                           const uint32_t *query_tags, int match, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    const bool ok = vectors && out_ids && out_dists && query_tags && dim > 0;
    if (!tagged_args("hnsw_mi355x_exact_knn_query_tagged", ok, row_tags, n_row_tags, match)) return -1;
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->exact_knn_query_tagged(vectors, count, dim, k, row_tags, n_row_tags, query_tags, match, out_ids, out_dists, err) < 0) {
        set_error(err);
        return -1;
    }
    return 0;
}
// KnnQuery with a tag mask per query: one device traversal for every mask.  Exclusive, like the filtered call.
API int hnsw_mi355x_knn_query_tagged(void *handle, const float *vectors, int count, int dim, int k, int layer, const uint32_t *row_tags, long long n_row_tags,
                                     const uint32_t *query_tags, int match, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    const bool ok = vectors && out_ids && out_dists && query_tags && dim > 0;
    if (!tagged_args("hnsw_mi355x_knn_query_tagged", ok, row_tags, n_row_tags, match)) return -1;
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->knn_query_tagged(vectors, count, dim, k, layer, row_tags, n_row_tags, query_tags, match, out_ids, out_dists, err) < 0) {
        set_error(err);
        return -1;
    }
    return 0;
}

// KnnQuery with a group filter per query: one device traversal for every group.  Exclusive, like the filtered call.
API int hnsw_mi355x_knn_query_grouped(void *handle, const float *vectors, int count, int dim, int k, int layer, const int *row_group, long long n_row_group,
                                      const int *query_group, int n_groups, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !query_group || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_knn_query_grouped"); return -1; }
    if (!row_group || n_row_group < 0) {
        set_error("System.ArgumentException: hnsw_mi355x_knn_query_grouped: row_group must not be NULL and n_row_group must be >= 0");
        return -1;
    }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->knn_query_grouped(vectors, count, dim, k, layer, row_group, n_row_group, query_group, n_groups, out_ids, out_dists, err) < 0) {
        set_error(err);
        return -1;
    }
    return 0;
}

API void hnsw_free_results(void **ids_array, void **dists_array, int count);

// hnsw_range_query and its filtered, grouped and tagged siblings: `name` for the errors, allow (none: no filter), or grp: a group per
// query, or tags: a tag mask per query
struct RangeGroupArgs { const int *row_group; long long n_row_group; const int *query_group; int n_groups; };
struct RangeTagArgs { const uint32_t *row_tags; long long n_row_tags; const uint32_t *query_tags; int match; };
static int range_query_export(void *handle, const float *vectors, int count, int dim, float range, hnsw::AllowBits allow, void **out_ids,
                              void **out_dists, int *counts, const char *name, int layer = 0, const RangeGroupArgs *grp = nullptr,
                              const RangeTagArgs *tags = nullptr)
{
    if (!vectors || !out_ids || !out_dists || !counts || dim <= 0) { set_error(std::string("System.ArgumentNullException: ") + name); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    std::string err;
    std::vector<std::vector<hnsw::NodeDist>> res;
    {
        LOCK_INDEX(handle);
        HnswIndex *ix = static_cast<HnswIndex *>(handle);
        const int rc = tags ? ix->range_query_tagged(vectors, count, dim, range, layer, tags->row_tags, tags->n_row_tags, tags->query_tags, tags->match, res, err)
                     : grp ? ix->range_query_grouped(vectors, count, dim, range, layer, grp->row_group, grp->n_row_group, grp->query_group, grp->n_groups, res, err)
                           : ix->range_query(vectors, count, dim, range, res, err, allow, layer);
        if (rc < 0) { set_error(err); return -1; }
    }
    const bool trace = hnsw::diag("trace", 0) != 0;
    const auto t_out0 = std::chrono::steady_clock::now();
    struct OutTimer { bool on; std::chrono::steady_clock::time_point t0; int count; const char *name; ~OutTimer() { if (on) fprintf(stderr, "[hnsw trace] %s: handing out %d per-query arrays %.4fs\n", name, count, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); } } out_timer{trace, t_out0, count, name};
    // callee-allocated per-query arrays (Marshal.AllocHGlobal :172-173), freed by hnsw_free_results: a call of thousands of queries hands out
    // millions of results, so the copies are spread over host threads (malloc is thread-safe; a failed allocation fails the call as before)
    std::atomic<int> next{0};
    std::atomic<bool> oom{false};
    auto work = [&]() {
        for (int i0; (i0 = next.fetch_add(256, std::memory_order_relaxed)) < count;)
            for (int i = i0, e = std::min(count, i0 + 256); i < e; ++i) {
                const int n = (int)res[(size_t)i].size();
                if (n > 0) {
                    int *ids = static_cast<int *>(std::malloc(sizeof(int) * (size_t)n));
                    float *ds = static_cast<float *>(std::malloc(sizeof(float) * (size_t)n));
                    if (!ids || !ds) { std::free(ids); std::free(ds); oom.store(true); continue; }
                    for (int j = 0; j < n; ++j) { ids[j] = res[(size_t)i][(size_t)j].id; ds[j] = res[(size_t)i][(size_t)j].dist; }
                    out_ids[i] = ids;
                    out_dists[i] = ds;
                    counts[i] = n;
                }
            }
    };
    {
        const int nth = count >= 2048 ? (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 8u) : 1;
        std::vector<std::thread> pool;
        for (int t = 1; t < nth; ++t) pool.emplace_back(work);
        work();
        for (std::thread &t : pool) t.join();
    }
    if (oom.load()) {
        hnsw_free_results(out_ids, out_dists, count);
        for (int j = 0; j < count; ++j) counts[j] = 0;
        set_error(std::string("System.OutOfMemoryException: ") + name);
        return -1;
    }
    return 0;
}

API int hnsw_range_query(void *handle, const float *vectors, int count, int dim, float range, void **out_ids, void **out_dists, int *counts) // :151-197
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    return range_query_export(handle, vectors, count, dim, range, hnsw::AllowBits{}, out_ids, out_dists, counts, "hnsw_range_query");
}

// hnsw_range_query with an allow-set (BatchRangeQuery(queries, range, filterFnc), HNSWIndex.cs:158-168): the bitset as for
// hnsw_mi355x_knn_query_filtered.  Where the reference pops an empty heap (range < 0) the call returns -1 with
// every array NULL and every count 0, as the reference export's catch block leaves them (:187-196).
API int hnsw_mi355x_range_query_filtered(void *handle, const float *vectors, int count, int dim, float range, const uint32_t *allow_bits,
                                         long long nbits, void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!allow_bits || nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_range_query_filtered: allow_bits must not be NULL and nbits must be >= 0"); return -1; }
    return range_query_export(handle, vectors, count, dim, range, hnsw::AllowBits{allow_bits, nbits}, out_ids, out_dists, counts,
                              "hnsw_mi355x_range_query_filtered");
}

// hnsw_mi355x_range_query_at_layer with a group filter per query: query i's list is what that call returns for it
// with the ids j < n_row_group, row_group[j] == query_group[i] as the allow-set, the order among equal distances and the empty-heap
// failure (-1, every array NULL, every count 0) included.  hnsw_mi355x_knn_query_grouped's group arguments.
API int hnsw_mi355x_range_query_grouped(void *handle, const float *vectors, int count, int dim, float range, int layer, const int *row_group,
                                        long long n_row_group, const int *query_group, int n_groups, void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !counts || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_range_query_grouped"); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    if (!query_group) { set_error("System.ArgumentNullException: hnsw_mi355x_range_query_grouped: query_group"); return -1; }
    if (!row_group || n_row_group < 0) {
        set_error("System.ArgumentException: hnsw_mi355x_range_query_grouped: row_group must not be NULL and n_row_group must be >= 0");
        return -1;
    }
    const RangeGroupArgs grp{row_group, n_row_group, query_group, n_groups};
    return range_query_export(handle, vectors, count, dim, range, hnsw::AllowBits{}, out_ids, out_dists, counts, "hnsw_mi355x_range_query_grouped", layer, &grp);
}

// hnsw_mi355x_range_query_at_layer with a tag mask per query: query i's list is what that call returns for it with
// the ids j < n_row_tags whose word row_tags[j] matches query_tags[i] under `match` as the allow-set, the order among equal
// distances and the empty-heap failure (-1, every array NULL, every count 0) included.  hnsw_mi355x_knn_query_tagged's tag arguments.
API int hnsw_mi355x_range_query_tagged(void *handle, const float *vectors, int count, int dim, float range, int layer, const uint32_t *row_tags,
                                       long long n_row_tags, const uint32_t *query_tags, int match, void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !counts || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_range_query_tagged"); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    if (!query_tags) { set_error("System.ArgumentNullException: hnsw_mi355x_range_query_tagged: query_tags"); return -1; }
    if (!tagged_args("hnsw_mi355x_range_query_tagged", true, row_tags, n_row_tags, match)) return -1;
    const RangeTagArgs tags{row_tags, n_row_tags, query_tags, match};
    return range_query_export(handle, vectors, count, dim, range, hnsw::AllowBits{}, out_ids, out_dists, counts, "hnsw_mi355x_range_query_tagged", layer, nullptr, &tags);
}

// The lists of a flat range scan, concatenated in query order in ids / ds, handed out as hnsw_range_query hands its lists out: a
// malloc'ed pair per query with results.  Out of memory: everything released, every count 0, -1.
static int exact_range_hand_out(const char *name, int count, int *counts, const std::vector<int> &ids, const std::vector<float> &ds, void **out_ids, void **out_dists)
{
    size_t at = 0;
    for (int i = 0; i < count; ++i) {
        const size_t n = (size_t)counts[i];
        if (n == 0) continue;
        int *pi = static_cast<int *>(std::malloc(sizeof(int) * n));
        float *pd = static_cast<float *>(std::malloc(sizeof(float) * n));
        if (!pi || !pd) {
            std::free(pi); std::free(pd);
            hnsw_free_results(out_ids, out_dists, count);
            for (int j = 0; j < count; ++j) counts[j] = 0;
            set_error(std::string("System.OutOfMemoryException: ") + name);
            return -1;
        }
        std::memcpy(pi, ids.data() + at, sizeof(int) * n);
        std::memcpy(pd, ds.data() + at, sizeof(float) * n);
        out_ids[i] = pi;
        out_dists[i] = pd;
        at += n;
    }
    return 0;
}

// Every live, allowed id within `range` per query, ascending by (distance, id): the flat scan with the range sink.
// hnsw_range_query's allocation contract (hnsw_free_results); exclusive, like the other scan.
API int hnsw_mi355x_exact_range_query(void *handle, const float *vectors, int count, int dim, float range, const uint32_t *allow_bits, long long nbits,
                                      void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !counts || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_range_query"); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_exact_range_query: nbits must be >= 0"); return -1; }
    std::string err;
    std::vector<int> ids;
    std::vector<float> ds;
    {
        LOCK_INDEX(handle);
        if (static_cast<HnswIndex *>(handle)->exact_range_query(vectors, count, dim, range, allow_bits, nbits, counts, ids, ds, err) < 0) {
            for (int i = 0; i < count; ++i) counts[i] = 0;
            set_error(err);
            return -1;
        }
    }
    return exact_range_hand_out("hnsw_mi355x_exact_range_query", count, counts, ids, ds, out_ids, out_dists);
}

// hnsw_mi355x_exact_range_query for the stored rows of ids: that call's lists and allocation contract; the
// candidates are allow_bits (NULL: every live id) minus the query's own id.  Exclusive, like the other by-id calls.
API int hnsw_mi355x_exact_range_query_by_id(void *handle, const int *ids, int count, float range, const uint32_t *allow_bits, long long nbits, void **out_ids,
                                            void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!ids || !out_ids || !out_dists || !counts) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_range_query_by_id"); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_exact_range_query_by_id: nbits must be >= 0"); return -1; }
    std::string err;
    std::vector<int> found;
    std::vector<float> ds;
    {
        LOCK_INDEX(handle);
        if (static_cast<HnswIndex *>(handle)->exact_range_query_by_id(ids, count, range, allow_bits, nbits, counts, found, ds, err) < 0) {
            for (int i = 0; i < count; ++i) counts[i] = 0;
            set_error(err);
            return -1;
        }
    }
    return exact_range_hand_out("hnsw_mi355x_exact_range_query_by_id", count, counts, found, ds, out_ids, out_dists);
}

// The single-linkage groups of the live, allowed ids within `range` of each other: one scan whose sink is a
// union-find on the device.  Exclusive: it uses the scan's buffers.
API int hnsw_mi355x_duplicate_groups(void *handle, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, long long cap, uint64_t *out_info)
{
    if (out_info) for (int i = 0; i < 4; ++i) out_info[i] = 0;
    if (!handle) return 0;
    if (!out_info) { set_error("System.ArgumentNullException: hnsw_mi355x_duplicate_groups: out_info"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_duplicate_groups: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->duplicate_groups(range, allow_bits, nbits, out_labels, cap, out_info, err) < 0) { set_error(err); return -1; }
    return 0;
}

// DBSCAN over the live, allowed ids: hnsw_mi355x_duplicate_groups' members and pair rule; clusters grow through core
// members only, the others are border or noise, and out_counts is every member's number of neighbours.  out_labels == NULL: the
// counts alone.  Exclusive: it uses the scan's buffers.
API int hnsw_mi355x_density_clusters(void *handle, float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels, int *out_counts,
                                     long long cap, uint64_t *out_info)
{
    if (out_info) for (int i = 0; i < 8; ++i) out_info[i] = 0;
    if (!handle) return 0;
    if (!out_info) { set_error("System.ArgumentNullException: hnsw_mi355x_density_clusters: out_info"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_density_clusters: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->density_clusters(range, min_samples, allow_bits, nbits, out_labels, out_counts, cap, out_info, err) < 0) {
        set_error(err);
        return -1;
    }
    return 0;
}

// Near-duplicates over the graph's edges: hnsw_mi355x_duplicate_groups' members and label convention, joined along
// the layer-0 edges within `range`; and those edges themselves, counted and kept by the first call and fetched by the second, as
// hnswdev_exact_range / hnswdev_exact_range_results do it.  Exclusive: they use the scan's query buffer and bring the mirror up to date.
API int hnsw_mi355x_graph_duplicate_groups(void *handle, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, long long cap,
                                           uint64_t *out_info)
{
    if (out_info) for (int i = 0; i < 5; ++i) out_info[i] = 0;
    if (!handle) return 0;
    if (!out_info) { set_error("System.ArgumentNullException: hnsw_mi355x_graph_duplicate_groups: out_info"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_graph_duplicate_groups: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->graph_duplicate_groups(range, allow_bits, nbits, out_labels, cap, out_info, err) < 0) { set_error(err); return -1; }
    return 0;
}

API int hnsw_mi355x_near_edges(void *handle, float range, const uint32_t *allow_bits, long long nbits, long long *out_count)
{
    if (out_count) *out_count = 0;
    if (!handle) return 0;
    if (!out_count) { set_error("System.ArgumentNullException: hnsw_mi355x_near_edges: out_count"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_near_edges: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->near_edges(range, allow_bits, nbits, out_count, err) < 0) { set_error(err); return -1; }
    return 0;
}

API int hnsw_mi355x_near_edges_results(void *handle, int *out_src, int *out_dst, float *out_dists, long long cap)
{
    if (!handle) return 0;
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->near_edges_results(out_src, out_dst, out_dists, cap, err) < 0) { set_error(err); return -1; }
    return 0;
}

// hnsw_mi355x_exact_range_query with a candidate group per query: that call's lists and allocation contract,
// hnsw_mi355x_exact_knn_query_grouped's group arguments.
API int hnsw_mi355x_exact_range_query_grouped(void *handle, const float *vectors, int count, int dim, float range, const int *row_group, long long n_row_group,
                                              const int *query_group, int n_groups, void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !counts || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_range_query_grouped"); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    if (!query_group) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_range_query_grouped: query_group"); return -1; }
    if (!row_group || n_row_group < 0) {
        set_error("System.ArgumentException: hnsw_mi355x_exact_range_query_grouped: row_group must not be NULL and n_row_group must be >= 0");
        return -1;
    }
    std::string err;
    std::vector<int> ids;
    std::vector<float> ds;
    {
        LOCK_INDEX(handle);
        if (static_cast<HnswIndex *>(handle)->exact_range_query_grouped(vectors, count, dim, range, row_group, n_row_group, query_group, n_groups, counts, ids, ds, err) < 0) {
            for (int i = 0; i < count; ++i) counts[i] = 0;
            set_error(err);
            return -1;
        }
    }
    return exact_range_hand_out("hnsw_mi355x_exact_range_query_grouped", count, counts, ids, ds, out_ids, out_dists);
}

// hnsw_mi355x_exact_range_query with a tag mask per query: that call's lists and allocation contract,
// hnsw_mi355x_exact_knn_query_tagged's tag arguments.
API int hnsw_mi355x_exact_range_query_tagged(void *handle, const float *vectors, int count, int dim, float range, const uint32_t *row_tags, long long n_row_tags,
                                             const uint32_t *query_tags, int match, void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (!vectors || !out_ids || !out_dists || !counts || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_range_query_tagged"); return -1; }
    for (int i = 0; i < count; ++i) { out_ids[i] = nullptr; out_dists[i] = nullptr; counts[i] = 0; }
    if (!query_tags) { set_error("System.ArgumentNullException: hnsw_mi355x_exact_range_query_tagged: query_tags"); return -1; }
    if (!tagged_args("hnsw_mi355x_exact_range_query_tagged", true, row_tags, n_row_tags, match)) return -1;
    std::string err;
    std::vector<int> ids;
    std::vector<float> ds;
    {
        LOCK_INDEX(handle);
        if (static_cast<HnswIndex *>(handle)->exact_range_query_tagged(vectors, count, dim, range, row_tags, n_row_tags, query_tags, match, counts, ids, ds, err) < 0) {
            for (int i = 0; i < count; ++i) counts[i] = 0;
            set_error(err);
            return -1;
        }
    }
    return exact_range_hand_out("hnsw_mi355x_exact_range_query_tagged", count, counts, ids, ds, out_ids, out_dists);
}

// KnnQuery / RangeQuery with the reference's `layer` argument (BatchKnnQuery / BatchRangeQuery(queries, ., filterFnc, layer),
// HNSWIndex.cs:107-168); allow_bits == NULL: no filter.  Layer 0 goes through the code of the calls without a layer.
API int hnsw_mi355x_knn_query_at_layer(void *handle, const float *vectors, int count, int dim, int k, int layer, const uint32_t *allow_bits,
                                       long long nbits, int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (layer == 0 && !allow_bits) return hnsw_knn_query(handle, vectors, count, dim, k, out_ids, out_dists);
    if (!vectors || !out_ids || !out_dists || dim <= 0) { set_error("System.ArgumentNullException: hnsw_mi355x_knn_query_at_layer"); return -1; }
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_knn_query_at_layer: nbits must be >= 0"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    if (static_cast<HnswIndex *>(handle)->knn_query_general(vectors, count, dim, k, layer, allow_bits, nbits, out_ids, out_dists, err) < 0) {
        set_error("System.IndexOutOfRangeException: hnsw_mi355x_knn_query_at_layer: " + err);
        return -1;
    }
    return 0;
}

API int hnsw_mi355x_range_query_at_layer(void *handle, const float *vectors, int count, int dim, float range, int layer, const uint32_t *allow_bits,
                                         long long nbits, void **out_ids, void **out_dists, int *counts)
{
    if (!handle) return 0;
    if (count <= 0) return 0;
    if (allow_bits && nbits < 0) { set_error("System.ArgumentException: hnsw_mi355x_range_query_at_layer: nbits must be >= 0"); return -1; }
    return range_query_export(handle, vectors, count, dim, range, allow_bits ? hnsw::AllowBits{allow_bits, nbits} : hnsw::AllowBits{}, out_ids, out_dists,
                              counts, "hnsw_mi355x_range_query_at_layer", layer);
}

// MultiLayerKnnQuery (HNSWIndex.cs:173-187) for a batch of independent queries: the number of layer slots, or -1
API int hnsw_mi355x_multilayer_knn_query(void *handle, const float *vectors, int count, int dim, int k, int max_layer, int min_layer, int layers_cap,
                                         int *out_ids, float *out_dists)
{
    if (!handle) return 0;
    if (count > 0 && k > 1 && (!vectors || !out_ids || !out_dists || dim <= 0)) { set_error("System.ArgumentNullException: hnsw_mi355x_multilayer_knn_query"); return -1; }
    LOCK_INDEX(handle);
    std::string err;
    const int n = static_cast<HnswIndex *>(handle)->multilayer_knn_query(vectors, count, dim, k, max_layer, min_layer, layers_cap, out_ids, out_dists, err);
    if (n < 0) { set_error("System.ArgumentOutOfRangeException: hnsw_mi355x_multilayer_knn_query: " + err); return -1; }
    return n;
}

API void hnsw_free_results(void **ids_array, void **dists_array, int count) // :199-217
{
    if (!ids_array && !dists_array) return;
    for (int i = 0; i < count; ++i) {
        if (ids_array && ids_array[i]) { std::free(ids_array[i]); ids_array[i] = nullptr; }
        if (dists_array && dists_array[i]) { std::free(dists_array[i]); dists_array[i] = nullptr; }
    }
}

#define SETTER(name, field, type)                      \
    API int name(type v)                               \
    {                                                  \
        std::lock_guard<std::mutex> lk(g_mu);          \
        g_pending.field = v;                           \
        return 0;                                      \
    }
SETTER(hnsw_set_collection_size, collection_size, int)             // :219
SETTER(hnsw_set_max_edges, max_edges, int)                         // :226
SETTER(hnsw_set_max_candidates, max_candidates, int)               // :233
SETTER(hnsw_set_remove_max_candidates, remove_max_candidates, int) // :240
SETTER(hnsw_set_random_seed, random_seed, int)                     // :254
SETTER(hnsw_set_min_nn, min_nn, int)                               // :261
SETTER(hnsw_set_allow_removals, allow_removals, bool)              // :268
SETTER(hnsw_mi355x_set_device, device, int)
SETTER(hnsw_mi355x_set_insert_batch, insert_batch, int)
SETTER(hnsw_mi355x_set_remove_batch, remove_batch, int)
SETTER(hnsw_mi355x_set_search_slots, search_slots, int)
SETTER(hnsw_mi355x_set_host_threads, host_threads, int)
SETTER(hnsw_mi355x_set_device_traversal, device_traversal, int)
SETTER(hnsw_mi355x_set_devices, devices, int)

// The knobs as one versioned struct (include/hnsw_mi355x.h): the documented way to configure the backend.
API int hnsw_mi355x_default_options(hnsw_mi355x_options *out)
{
    if (!out) return -1;
    const Params d;
    *out = hnsw_mi355x_options{(uint32_t)sizeof(hnsw_mi355x_options), 0, 1, d.insert_batch, d.remove_batch, d.host_threads, d.search_slots, d.device_traversal, nullptr};
    return 0;
}
API int hnsw_mi355x_set_options(const hnsw_mi355x_options *opt)
{
    if (!opt || opt->struct_size < 8 || opt->struct_size > 4096) { set_error("hnsw_mi355x_set_options: struct_size not set"); return -1; }
    hnsw_mi355x_options o;
    (void)hnsw_mi355x_default_options(&o);
    std::memcpy(&o, opt, std::min<size_t>(opt->struct_size, sizeof o)); // an older caller's shorter struct: the rest keeps the defaults
    if (o.insert_batch == -1 || o.remove_batch < 1 || o.devices < 0 || o.devices > 64 || o.device < -1 || o.host_threads < 0 || o.search_slots < 0) {
        set_error("hnsw_mi355x_set_options: value out of range");
        return -1;
    }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_pending.device = o.device; g_pending.devices = o.devices; g_pending.insert_batch = o.insert_batch; g_pending.remove_batch = o.remove_batch;
        g_pending.host_threads = o.host_threads; if (o.search_slots > 0) g_pending.search_slots = o.search_slots; g_pending.device_traversal = o.device_traversal;
    }
    if (opt->struct_size >= offsetof(hnsw_mi355x_options, diagnostics) + sizeof(const char *)) hnsw::set_diag_string(o.diagnostics);
    return 0;
}

API int hnsw_set_distribution_rate(float dist_rate) // :247 -- crosses the ABI as float, widened to double
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_pending.distribution_rate = (double)dist_rate;
    return 0;
}

// ---- introspection / counters ----
// Which sources this binary was compiled from: sha256 over csrc/* and include/* (build.py: source_id()), also findable
// in the file itself behind the tag.  __graft_entry__.build() rebuilds when it differs from the tree's, and the test
// tier asserts that the library that got loaded is the tree's.
#ifndef HNSW_MI355X_BUILD_ID_STR
#define HNSW_MI355X_BUILD_ID_STR "unidentified"
#endif
extern "C" __attribute__((visibility("default"), used)) const char hnsw_mi355x_build_id_tag[] = "HNSW_MI355X_BUILD_ID=" HNSW_MI355X_BUILD_ID_STR;
API const char *hnsw_mi355x_build_id(void) { return hnsw_mi355x_build_id_tag + sizeof("HNSW_MI355X_BUILD_ID=") - 1; }

API int hnsw_mi355x_count(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->count();
}
// measurement aid: queries resident in HBM across calls (bench.py's timed region)
API int hnsw_mi355x_set_queries(void *h, const float *queries, int count, int dim)
{
    if (!h || !queries || count <= 0 || dim <= 0) return -1;
    LOCK_INDEX(h);
    std::string err;
    if (static_cast<HnswIndex *>(h)->set_resident_queries(queries, count, dim, err) < 0) { set_error(err); return -1; }
    return 0;
}
API int hnsw_mi355x_resident_count(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->resident_count();
}
API int hnsw_mi355x_knn_query_resident(void *h, int k, int *out_ids, float *out_dists)
{
    if (!h || !out_ids || !out_dists) return -1;
    LOCK_INDEX(h);
    std::string err;
    if (static_cast<HnswIndex *>(h)->knn_query_resident(k, out_ids, out_dists, err) < 0) { set_error(err); return -1; }
    return 0;
}
API int hnsw_mi355x_index_set_insert_batch(void *h, int max_batch)
{
    if (!h || max_batch == -1) { set_error("insert batch must be >= 1, 0 (the host's hardware threads), or -W with W >= 2"); return -1; }
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->set_insert_batch(max_batch);
    return 0;
}
API int hnsw_mi355x_host_parallelism(void) { return HnswIndex::host_parallelism(); }
API int hnsw_mi355x_index_insert_batch(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->insert_batch_cap();
}
API int hnsw_mi355x_exact_window_stats(void *h, uint64_t out[4])
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->exact_window_stats(out);
    return 0;
}
API int hnsw_mi355x_row_prefilter_stats(void *h, uint64_t out[4])
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->row_prefilter_stats(out);
    return 0;
}
API int hnsw_mi355x_row_prefilter_form_stats(void *h, uint64_t out[2])
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->row_prefilter_form_stats(out);
    return 0;
}
API int hnsw_mi355x_row_prefilter_peek(void *h, int first_id, int count, uint64_t out[2], float *rows)
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    std::string err;
    if (!static_cast<HnswIndex *>(h)->row_prefilter_peek(first_id, count, out, rows, err)) { set_error(err); return -1; }
    return 0;
}
// The 8-bit shadow's own counters and read-back.  Argument errors: -1 with a message.
API int hnsw_mi355x_row_prefilter8_stats(void *h, uint64_t out[6])
{
    if (!h || !out) { set_error("System.ArgumentNullException: hnsw_mi355x_row_prefilter8_stats"); return -1; }
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->row_prefilter8_stats(out);
    return 0;
}
API int hnsw_mi355x_row_prefilter8_peek(void *h, int first_id, int count, uint64_t out[4], uint8_t *codes)
{
    if (!h || !out || (count > 0 && !codes)) { set_error("System.ArgumentNullException: hnsw_mi355x_row_prefilter8_peek"); return -1; }
    LOCK_INDEX(h);
    std::string err;
    if (!static_cast<HnswIndex *>(h)->row_prefilter8_peek(first_id, count, out, codes, err)) { set_error(err); return -1; }
    return 0;
}
// HNSWIndex.GetInfo() / GetConnectedComponentCounts() (HNSWIndex.cs:192-205) from the graph mirror on the device:
// top + 1, with min(cap, top + 1) entries written.  Exclusive: Add edits the mirror.
API int hnsw_mi355x_get_info(void *h, hnsw_mi355x_layer_info *out, int cap)
{
    if (!h) return 0;
    if (cap < 0 || (cap > 0 && !out)) { set_error("System.ArgumentNullException: hnsw_mi355x_get_info"); return -1; }
    std::string err;
    LOCK_INDEX(h);
    const int n = static_cast<HnswIndex *>(h)->get_info(out, cap, err);
    if (n < 0) set_error(err);
    return n;
}
API int hnsw_mi355x_connected_component_counts(void *h, int *out, int cap)
{
    if (!h) return 0;
    if (cap < 0 || (cap > 0 && !out)) { set_error("System.ArgumentNullException: hnsw_mi355x_connected_component_counts"); return -1; }
    std::string err;
    LOCK_INDEX(h);
    const int n = static_cast<HnswIndex *>(h)->connected_component_counts(out, cap, err);
    if (n < 0) set_error(err);
    return n;
}
// Reachability from the entry point over out-edges on the graph mirror.  Exclusive, as hnsw_mi355x_get_info.
API int hnsw_mi355x_reachability(void *h, hnsw_mi355x_layer_reach *out, int cap)
{
    if (!h) return 0;
    if (cap < 0 || (cap > 0 && !out)) { set_error("System.ArgumentNullException: hnsw_mi355x_reachability"); return -1; }
    std::string err;
    LOCK_INDEX(h);
    const int n = static_cast<HnswIndex *>(h)->reachability(out, cap, err);
    if (n < 0) set_error(err);
    return n;
}
API int hnsw_mi355x_unreachable_ids(void *h, int layer, int *out, int cap)
{
    if (!h) return 0;
    if (cap < 0 || (cap > 0 && !out)) { set_error("System.ArgumentNullException: hnsw_mi355x_unreachable_ids"); return -1; }
    std::string err;
    std::vector<int> ids;
    LOCK_INDEX(h);
    if (static_cast<HnswIndex *>(h)->unreachable_ids(layer, ids, err) < 0) { set_error(err); return -1; }
    std::copy(ids.begin(), ids.begin() + std::min<size_t>(ids.size(), (size_t)cap), out);
    return (int)ids.size();
}
API int hnsw_mi355x_hop_counts(void *h, int layer, int *out, int cap)
{
    if (!h) return 0;
    if (cap < 0 || (cap > 0 && !out)) { set_error("System.ArgumentNullException: hnsw_mi355x_hop_counts"); return -1; }
    std::string err;
    LOCK_INDEX(h);
    const int n = static_cast<HnswIndex *>(h)->hop_counts(layer, out, cap, err);
    if (n < 0) set_error(err);
    return n;
}
// repair_reachability.  Exclusive, as hnsw_mi355x_remove: it edits lists.
API int hnsw_mi355x_repair_reachability(void *h, int cands, int max_rounds, hnsw_mi355x_layer_repair *out, int cap)
{
    if (!h) return 0;
    if (cap < 0 || (cap > 0 && !out)) { set_error("System.ArgumentNullException: hnsw_mi355x_repair_reachability"); return -1; }
    if (cands < 1 || cands > 64 || max_rounds < 1 || max_rounds > 64) {
        set_error("System.ArgumentOutOfRangeException: hnsw_mi355x_repair_reachability: cands = " + std::to_string(cands) + " and max_rounds = " +
                  std::to_string(max_rounds) + " must both be in 1 .. 64");
        return -1;
    }
    std::string err;
    LOCK_INDEX(h);
    const int n = static_cast<HnswIndex *>(h)->repair_reachability(cands, max_rounds, out, cap, err);
    if (n < 0) set_error(err);
    return n;
}
API int hnsw_mi355x_dim(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->dim();
}
API int hnsw_mi355x_length(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->graph().length;
}
API int hnsw_mi355x_active_ids(void *h, int *out, int cap)
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    const hnsw::Graph &g = static_cast<HnswIndex *>(h)->graph();
    int n = std::min(g.count, cap);
    std::memcpy(out, g.dense.data(), sizeof(int) * (size_t)n);
    return g.count;
}
API int hnsw_mi355x_entry_point(void *h)
{
    if (!h) return -1;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->graph().entry;
}
API int hnsw_mi355x_node_max_layer(void *h, int id)
{
    if (!h) return -1;
    LOCK_INDEX(h);
    const hnsw::Graph &g = static_cast<HnswIndex *>(h)->graph();
    return (id < 0 || id >= g.length) ? -1 : g.level[(size_t)id];
}
API int hnsw_mi355x_get_out_edges(void *h, int id, int layer, int *out, int cap)
{
    if (!h) return -1;
    LOCK_INDEX(h);
    const hnsw::Graph &g = static_cast<HnswIndex *>(h)->graph();
    if (id < 0 || id >= g.length || layer < 0 || layer > g.level[(size_t)id]) return -1;
    const int *l = g.list(id, layer);
    int n = std::min(l[0], cap);
    if (out && n > 0) std::memcpy(out, l + 1, sizeof(int) * (size_t)n);
    return l[0];
}
API int hnsw_mi355x_export_levels(void *h, int *out, int cap)
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    const hnsw::Graph &g = static_cast<HnswIndex *>(h)->graph();
    int n = std::min(g.length, cap);
    std::memcpy(out, g.level.data(), sizeof(int) * (size_t)n);
    return g.length;
}
// counts[id] = out-degree of (id, layer) or -1 if the node has no such layer;
// edges[id*stride ...] = its ids (stride >= max degree + 1).
API int hnsw_mi355x_export_edges(void *h, int layer, int *counts, int *edges, int stride, int cap)
{
    if (!h || !counts || !edges || layer < 0) return -1;
    LOCK_INDEX(h);
    const hnsw::Graph &g = static_cast<HnswIndex *>(h)->graph();
    int n = std::min(g.length, cap);
    for (int i = 0; i < n; ++i) {
        if (g.level[(size_t)i] < layer) { counts[i] = -1; continue; }
        const int *l = g.list(i, layer);
        if (l[0] > stride) return -1;
        counts[i] = l[0];
        std::memcpy(edges + (size_t)i * stride, l + 1, sizeof(int) * (size_t)l[0]);
    }
    return g.length;
}
// HNSWIndex.Serialize / Deserialize (src/HNSWIndex/HNSWIndex.cs:210-229); the reference's C ABI
// does not export them, its C# API does.
API int hnsw_mi355x_serialize(void *h, const char *path_utf8)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    std::string err;
    if (static_cast<HnswIndex *>(h)->serialize(path_utf8, err) < 0) { set_error(err); return -1; }
    return 0;
}
API void *hnsw_mi355x_deserialize(const char *distance_metric, const char *path_utf8)
{
    const int metric = parse_metric(distance_metric);
    if (metric < 0) {
        set_error(std::string("System.ArgumentException: Unsupported distance metric: ") + (distance_metric ? distance_metric : "(null)"));
        return nullptr;
    }
    Params p;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        p = g_pending; // backend knobs only; the HNSW parameters come from the snapshot
    }
    std::string err;
    HnswIndex *ix = HnswIndex::deserialize(metric, p, path_utf8, err);
    if (!ix) { set_error(err); return nullptr; }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        g_pending = Params();
    }
    return ix;
}
API int hnsw_mi355x_import_nodes(void *h, const float *rows, int n, int dim, const int *levels, int entry_point)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    std::string err;
    if (static_cast<HnswIndex *>(h)->import_nodes(rows, n, dim, levels, entry_point, err) < 0) { set_error(err); return -1; }
    return 0;
}
API int hnsw_mi355x_import_edges(void *h, int layer, const int *counts, const int *edges, int stride)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    std::string err;
    if (static_cast<HnswIndex *>(h)->import_edges(layer, counts, edges, stride, err) < 0) { set_error(err); return -1; }
    return 0;
}
API uint64_t hnsw_mi355x_graph_hash(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->graph_hash();
}
API int hnsw_mi355x_get_stats(void *h, hnswdev_stats *out)
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->collect_stats(out); // the primary context plus the query lanes
    return 0;
}
API int hnsw_mi355x_device_count(void *h)
{
    if (!h) return 0;
    LOCK_INDEX(h);
    return static_cast<HnswIndex *>(h)->device_count();
}
API int hnsw_mi355x_get_stats_at(void *h, int context, hnswdev_stats *out)
{
    if (!h || !out) return -1;
    LOCK_INDEX(h);
    hnsw::Device *d = static_cast<HnswIndex *>(h)->device_at(context);
    if (!d) { std::memset(out, 0, sizeof(*out)); return context >= 0 && context < static_cast<HnswIndex *>(h)->device_count() ? 0 : -1; }
    d->get_stats(out);
    return 0;
}
// The getters of the counter blocks, hnsw_mi355x_<block>(handle, out[slots]), one per row of counter_blocks.h
#define HNSW_COUNTER_GETTER(NAME, SCOPE, ...)                                       \
    API int hnsw_mi355x_##NAME(void *h, uint64_t *out)                              \
    {                                                                               \
        if (!h || !out) return -1;                                                  \
        LOCK_INDEX(h);                                                              \
        static_cast<HnswIndex *>(h)->counters(hnsw::CounterBlock::NAME, out);       \
        return 0;                                                                   \
    }
HNSW_FOR_EACH_COUNTER_BLOCK(HNSW_COUNTER_GETTER)
#undef HNSW_COUNTER_GETTER
API int hnsw_mi355x_reset_stats(void *h)
{
    if (!h) return -1;
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->reset_all_stats();
    return 0;
}
API int hnsw_mi355x_set_profiling(void *h, int enabled)
{
    if (!h) return -1;
    LOCK_INDEX(h);
    static_cast<HnswIndex *>(h)->set_profiling(enabled != 0);
    return 0;
}

// ---- host-logic test hooks (no device involved): the restated BCL pieces, so that the CPU
// test tier can compare them with the oracle's independent restatement ----
// Snapshot codec without a device: decode `in_path`, re-encode to `out_path`.
// info = {length, dim, count, entry, capacity, max_edges, allow_removals, random_seed}
API int hnswhost_test_snapshot_transcode(const char *in_path, const char *out_path, int *info, uint64_t *graph_hash)
{
    std::string err;
    FILE *f = std::fopen(in_path, "rb");
    if (!f) { set_error("cannot open input"); return -1; }
    std::vector<uint8_t> buf;
    std::fseek(f, 0, SEEK_END);
    long sz = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    buf.resize((size_t)std::max(0L, sz));
    if (sz > 0 && std::fread(buf.data(), 1, (size_t)sz, f) != (size_t)sz) { std::fclose(f); set_error("short read"); return -1; }
    std::fclose(f);
    hnsw::SnapshotParams sp;
    hnsw::Graph g;
    std::vector<float> rows;
    int dim = 0;
    long long cap = 0;
    if (!hnsw::read_snapshot(buf.data(), buf.size(), sp, g, rows, dim, cap, err)) { set_error(err); return -1; }
    if (info) {
        info[0] = g.length; info[1] = dim; info[2] = g.count; info[3] = g.entry; info[4] = (int)cap;
        info[5] = sp.max_edges; info[6] = sp.allow_removals ? 1 : 0; info[7] = sp.random_seed;
    }
    if (graph_hash) *graph_hash = hnsw::graph_hash_of(g);
    if (out_path && !hnsw::write_snapshot(out_path, sp, g, rows.data(), dim, cap, err)) { set_error(err); return -1; }
    return 0;
}

API int hnswhost_test_diag(const char *name, int dflt) { return name ? hnsw::diag(name, dflt) : dflt; } // what csrc/diag.h answers right now
API void hnswhost_test_random_next(int seed, int n, int *out)
{
    hnsw::DotnetRandom r(seed);
    for (int i = 0; i < n; ++i) out[i] = r.internal_sample();
}
// NextSingle's redraw rule on an injected stream of InternalSample() values
API float hnswhost_test_next_single_from_samples(const int *samples, int n, int *used)
{
    for (int i = 0; i < n; ++i) {
        const float f = hnsw::DotnetRandom::single_of_sample(samples[i]);
        if (f < 1.0f) { *used = i + 1; return f; }
    }
    *used = n;
    return -1.0f;
}
API void hnswhost_test_random_levels(int seed, double rate, int n, int *out)
{
    hnsw::DotnetRandom r(seed);
    for (int i = 0; i < n; ++i) out[i] = hnsw::level_from_uniform(r.next_single(), rate);
}
API void hnswhost_test_sort(int *ids, float *dists, int n)
{
    std::vector<hnsw::NodeDist> k((size_t)n);
    for (int i = 0; i < n; ++i) k[(size_t)i] = hnsw::NodeDist{ids[i], dists[i]};
    hnsw::dotnet_sort(k.data(), n);
    for (int i = 0; i < n; ++i) { ids[i] = k[(size_t)i].id; dists[i] = k[(size_t)i].dist; }
}
// RangeQuery's order among equal distances (range_replay.h) on a graph handed in as layer-0 lists [count, ids...]
// of `stride` ints per node: `found` = the query's result set in ANY order; out_ids = the reference's order.
API int hnswhost_test_range_replay(const int *adj0, int stride, int max_edges0, int entry, float range, const int *found_ids, const float *found_d,
                                   int m, int *out_ids, float *out_d)
{
    struct Hit { int id; float dist; };
    std::vector<Hit> found((size_t)m);
    for (int i = 0; i < m; ++i) found[(size_t)i] = Hit{found_ids[i], found_d[i]};
    std::vector<hnsw::NodeDist> out;
    hnsw::replay_range_heaps([&](int id) { return adj0 + (size_t)id * (size_t)stride; }, max_edges0, entry, range, found.data(), m, out);
    for (size_t i = 0; i < out.size(); ++i) { out_ids[i] = out[i].id; out_d[i] = out[i].dist; }
    return (int)out.size();
}
// ... with an allow-set (ids >= nbits not allowed): found = the query's whole closure.  Returns the result count, or -2 where the
// reference pops an empty heap (range_replay.h).
API int hnswhost_test_range_replay_filtered(const int *adj0, int stride, int max_edges0, int entry, float range, const int *found_ids, const float *found_d,
                                            int m, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d)
{
    struct Hit { int id; float dist; };
    std::vector<Hit> found((size_t)m);
    for (int i = 0; i < m; ++i) found[(size_t)i] = Hit{found_ids[i], found_d[i]};
    std::vector<hnsw::NodeDist> out;
    if (hnsw::replay_range_heaps([&](int id) { return adj0 + (size_t)id * (size_t)stride; }, max_edges0, entry, range, found.data(), m, out,
                                 hnsw::AllowBits{allow_bits, nbits}) == hnsw::kRangeHeapEmpty)
        return -2;
    for (size_t i = 0; i < out.size(); ++i) { out_ids[i] = out[i].id; out_d[i] = out[i].dist; }
    return (int)out.size();
}
API int hnswhost_test_heap_script(int closer_first, const int *ops, const float *d, int n, int *out_ids, float *out_d, int *popped_ids, int *n_popped)
{
    hnsw::BinaryHeap<hnsw::FartherFirst> hf;
    hnsw::BinaryHeap<hnsw::CloserFirst> hc;
    hf.reset(4); hc.reset(4);
    int np = 0;
    for (int i = 0; i < n; ++i) {
        if (ops[i] >= 0) { hnsw::NodeDist v{ops[i], d[i]}; if (closer_first) hc.push(v); else hf.push(v); }
        else if ((closer_first ? hc.count : hf.count) > 0) {
            hnsw::NodeDist v = closer_first ? hc.pop() : hf.pop();
            if (popped_ids) popped_ids[np] = v.id;
            ++np;
        }
    }
    int c = closer_first ? hc.count : hf.count;
    for (int i = 0; i < c; ++i) {
        const hnsw::NodeDist &v = closer_first ? hc.buf[(size_t)i] : hf.buf[(size_t)i];
        out_ids[i] = v.id; out_d[i] = v.dist;
    }
    if (n_popped) *n_popped = np;
    return c;
}
