// device_backend.h -- internal C++ face of the gfx950 distance backend.
// The C ABI (include/hnsw_mi355x.h, hnswdev_*) and the host driver (search_engine.cpp,
// hnsw_index.cpp) both sit on this class.  Nothing here computes a distance on the CPU.
#pragma once
#include <cstddef>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>
#include <thread>

#include "../../include/hnsw_mi355x.h"
#include "counter_blocks.h"
#include "dev_buf.h"

namespace hnsw {

// The metrics, one row each: X(id, unit tag, ABI name).  The id is the ABI's HNSWDEV_* value; the tag names the metric's kernel
// units (build.py METRICS; a unit is compiled with -DHNSW_UNIT_METRIC=<tag>); the name is what hnsw_create() takes.  Whatever
// walks the metrics is written from this list: with_metric and Device::create's range check (device_backend.hip), the metrics x
// kinds grids of the traversal kernels (device_kernels.h), parse_metric (exports.cpp).  The last three are not in the
// reference: int8 records (BASELINE config 5) and rows stored as binary16.  This header rather than dk_base.h,
// where the ids are used, because exports.cpp is a host-only unit.
#define HNSW_FOR_EACH_METRIC(X)      \
    X(M_SQ, sq, "sq_euclid")         \
    X(M_COS, cos, "cosine")          \
    X(M_UCOS, ucos, "ucosine")       \
    X(M_I8, i8, "sq_euclid_i8")      \
    X(M_SQH, sqh, "sq_euclid_f16")   \
    X(M_UCOSH, ucosh, "ucosine_f16")
enum { M_SQ = HNSWDEV_SQ_EUCLID, M_COS = HNSWDEV_COSINE, M_UCOS = HNSWDEV_UCOSINE, M_I8 = HNSWDEV_SQ_EUCLID_I8,
       M_SQH = HNSWDEV_SQ_EUCLID_F16, M_UCOSH = HNSWDEV_UCOSINE_F16 };
#define HNSW_METRIC_ID(ID, TAG, NAME) ID,
constexpr int kMetricIds[] = {HNSW_FOR_EACH_METRIC(HNSW_METRIC_ID)};
#undef HNSW_METRIC_ID
constexpr int kMetricCount = (int)(sizeof(kMetricIds) / sizeof(kMetricIds[0]));
constexpr bool metric_ids_in_order()
{
    for (int i = 0; i < kMetricCount; ++i)
        if (kMetricIds[i] != i) return false;
    return true;
}
static_assert(metric_ids_in_order(), "HNSW_FOR_EACH_METRIC lists the ids 0 .. kMetricCount - 1 in order");
constexpr bool metric_str_eq(const char *a, const char *b)
{
    for (; *a && *a == *b; ++a, ++b) {}
    return *a == *b;
}
// the id of a unit tag / of an ABI name, -1 when the list has none such
constexpr int metric_by_tag(const char *tag)
{
#define HNSW_METRIC_TAG(ID, TAG, NAME) if (metric_str_eq(tag, #TAG)) return ID;
    HNSW_FOR_EACH_METRIC(HNSW_METRIC_TAG)
#undef HNSW_METRIC_TAG
    return -1;
}
constexpr int metric_by_name(const char *name)
{
#define HNSW_METRIC_NAME(ID, TAG, NAME) if (metric_str_eq(name, NAME)) return ID;
    HNSW_FOR_EACH_METRIC(HNSW_METRIC_NAME)
#undef HNSW_METRIC_NAME
    return -1;
}
// A kernel unit's metric: the id of the tag it was compiled with (kernel_unit.hip, exact_unit.hip)
#define HNSW_STR_(X) #X
#define HNSW_STR(X) HNSW_STR_(X)
#define HNSW_UNIT_METRIC_ID ::hnsw::metric_by_tag(HNSW_STR(HNSW_UNIT_METRIC))

// Last error: one process-wide string (hnswdev_last_error: creation failures have no context yet)
// and one per context (hnswdev_ctx_last_error).  set_dev_error() files the message under the context
// the calling thread is currently inside (ErrorScope), if any.
void set_dev_error(const std::string &msg);
std::string get_dev_error();

// Limits of the flat scan (dk_exact.h) that the host checks as well: here, because hnsw_index.cpp is a host-only unit.
constexpr int kExactMaxK = 1024;
constexpr int kExactMaxGroups = 65536;   // groups of a grouped call: exact_group_offsets_kernel is one block that walks the counts
// The argument rules every grouped call shares -- n_groups in 1 .. kExactMaxGroups, every query_group value inside 0 .. n_groups - 1 --
// and the one wording of a breach: "" when the arguments are good, else "<who>: ..." (the index adds its exception prefix in front).
inline std::string group_args_error(const char *who, const int *query_group, int nq, int n_groups)
{
    if (n_groups < 1 || n_groups > kExactMaxGroups)
        return std::string(who) + ": n_groups = " + std::to_string(n_groups) + " is outside 1 .. " + std::to_string(kExactMaxGroups);
    for (int i = 0; i < nq; ++i)
        if (query_group[i] < 0 || query_group[i] >= n_groups)
            return std::string(who) + ": query_group[" + std::to_string(i) + "] = " + std::to_string(query_group[i]) + " is outside 0 .. n_groups - 1 = " + std::to_string(n_groups - 1);
    return std::string();
}
// The tagged calls: a uint32 of tag bits per id, a uint32 mask per query, one mode for the call -- 0 "any": an id
// is a candidate when it shares a tag with the mask, 1 "all": when it carries every tag of a mask that is not 0.  The word 0
// matches no mask and the mask 0 no word, in either mode.
constexpr long long kTagListEntries = 1LL << 28; // ids in the candidate lists of one batch of masks of exact_knn_tagged: 1 GiB (`tag_list_cap` lowers it)
// (the rule itself on the host: tag_match_host, host_structs.h)
// The distinct masks of a call in the order they first appear, and each query's place among them.
struct TagCall {
    std::vector<uint32_t> masks; // at most kExactMaxGroups
    std::vector<int> of;         // [nq] query i's mask is masks[of[i]]
};
// The argument rules every tagged call shares -- match 0 or 1, at most kExactMaxGroups distinct masks -- and the one wording of a
// breach: "" when the arguments are good (tc filled), else "<who>: ...".
inline std::string tag_args_error(const char *who, const uint32_t *query_tags, int nq, int match, TagCall *tc)
{
    if (match != 0 && match != 1) return std::string(who) + ": match = " + std::to_string(match) + " is neither 0 (any) nor 1 (all)";
    std::unordered_map<uint32_t, int> seen;
    tc->masks.clear();
    tc->of.assign((size_t)std::max(nq, 0), 0);
    for (int i = 0; i < nq; ++i) {
        const auto it = seen.emplace(query_tags[i], (int)tc->masks.size());
        if (it.second) {
            if ((int)tc->masks.size() == kExactMaxGroups)
                return std::string(who) + ": more than " + std::to_string(kExactMaxGroups) + " distinct masks in query_tags (the " + std::to_string(kExactMaxGroups + 1) + "th at index " + std::to_string(i) + ")";
            tc->masks.push_back(query_tags[i]);
        }
        tc->of[(size_t)i] = it.first->second;
    }
    return std::string();
}
class Device;
struct VisitedScratch;   // device_backend.hip: the visited-set memory of a traversal launch
struct TraversalLaunch;  // ... which traversal kernel form a launch runs, on how many waves, with which flags
struct LaunchFamily;     // ... the hnswdev_stats counters of one kernel family
struct AllowPred;        // host_structs.h: an allow-set or a group label over ids
struct RangeFilter;      // ... the filter of one range call: its kind, per-id array and per-query keys
struct PredicateCall;    // device_backend.hip: the arguments every KnnQuery with a predicate over ids has
template <class K> struct PredicatePlan; // ... and what its launches need, K the kernel's type
struct ExactScanArgs;    // dk_exact.h: what one launch of the flat scan reads
struct ExactDensityPair; // ... a within pair of the density clusters: 16 bytes of the pair arena
struct ExactTriangle;    // device_backend.hip: the members and the plan of a scan over the pairs a < b of an id list
enum class ExactStart;   // device_backend.hip: how a flat-scan call begins -- failed, nothing to measure, ready
struct ExactScanInput;   // ... the queries and the id list of an ungrouped flat scan
struct ExactCollapseArgs; // ... the labels on the device, the cap and the device counters of a collapsed one
struct ExactGroupedCall; // ... the group lists and the tile of a grouped one
struct ExactRangeWork;   // ... the knobs and the scratch of the range calls
struct ReachSeeds;       // dk_graph_reach.h: the seed set of one layer's reachability pass
// What one round of repair_reachability brings back (Device::graph_repair_round).  The three arrays are pinned memory of the
// context, valid until its next round; they are nullptr where no proposal ran (propose == false, or nothing is unreached).
constexpr int kRepairSeedEntry = 0, kRepairSeedBits = 1, kRepairSeedAbove = 2; // graph_repair_round's seed_mode (dk_graph_reach.h's kReachSeed*)
struct GraphRepairRound {
    uint64_t summary[4] = {0, 0, 0, 0}; // the BFS's: members, member seeds, reached, largest hop
    int n_u = 0;                        // members without a hop: members - reached
    const int *ids = nullptr;           // [n_u] U, ascending
    const int *cands = nullptr;         // [n_u][cands] the nearest reached members by (distance, id), padded with -1
    const int *codes = nullptr;         // [n_u][cands] where in the candidate's list u could go, -1: nowhere
};
struct LayerView;        // dk_graph_info.h: the mirror as the graph-info kernels see one layer of it
struct GraphAcc;         // ... what those kernels add up
struct ErrorScope { // RAII: the calling thread is inside a call on `d`
    explicit ErrorScope(Device *d);
    ~ErrorScope();
    Device *prev;
};

// One lock-step "step" worth of work for up to nslots concurrent searches.
// The host driver fills one packed record per slot in pinned host memory,
//     rec[s*rec_stride + 0]      = cnt   : number of candidate ids this step
//     rec[s*rec_stride + 1]      = qidx  : >= 0 resident query index; < 0: ~row id (id<->id)
//     rec[s*rec_stride + 2 ...]  = ids   : candidate row ids (capacity = stride)
// launch_step() moves the used prefix to HBM with ONE async H2D copy, runs the kernel on
// device-resident inputs, and brings the distances back with ONE async D2H copy -- all on
// the context's stream.  (Letting the kernel read pinned host memory directly was measured
// 2-3x slower: tools/kbench.hip, DESIGN.md "Step buffers".)
//   slot s evaluates metric(row[ids[c]], Q(s)) for c < cnt
struct StepBuffers {
    enum { kHeader = 16 }; // floats in front of the distances; word 0 = the kernel's guard flag, so one D2H copy brings both
    int nslots = 0, stride = 0, rec_stride = 0;
    int *rec = nullptr;     // pinned host, nslots * rec_stride
    float *dist = nullptr;  // pinned host, nslots * stride (dist - kHeader is the allocation)
    int *d_rec = nullptr;   // HBM mirrors
    float *d_dist = nullptr; // kHeader + nslots * stride
    void *done = nullptr;      // hipEvent_t recorded after the D2H copy
    void *t0 = nullptr, *t1 = nullptr; // hipEvent_t pair around the kernel when profiling
    bool timed = false, in_flight = false;
    uint64_t evals = 0;
};

// One traversal for the graph-resident search kernel: greedy descent from `entry` at
// `entry_layer` down to (exclusive) `search_layer`, then the beam search at `search_layer`.
struct SearchJob {
    int qref;         // >= 0 resident query index; < 0: ~row id
    int entry;        // entry node id
    int entry_layer;  // layer the descent starts at (== search_layer: no descent)
    int search_layer; // layer of the beam search
    int aux;          // insert search: index of the item's first upper-layer output slot (-1: none)
    int stop_layer;   // insert search: the last layer this job searches (0 = all the way down; the exact-window Add
                      // runs the upper layers of a multi-layer item ahead of time, and its layer 0 as a job of its own)
};
// RangeQuery: state of a job's result list after the finishing kernels (dk_range_finish.h).  The list in the arena is ...
constexpr int kRangeFinal = 0;    // ... in the reference's order
constexpr int kRangeTied = 2;     // ... ascending, with equal distances in it: to be replayed (range_replay_kernel did not: the host does)
constexpr int kRangeHostSort = 5; // ... as found: too long for the device ranking, or a -0 distance (host: sort, replay if tied)

struct SearchHit {
    int id;
    float dist;
};

class Device {
public:
    static Device *create(int device, int dim, int metric, long long capacity);
    // A second context on the same GPU that BORROWS the primary's stored rows and graph mirror and owns everything
    // a query needs besides (stream, resident query set, per-wave scratch, staging): two hnsw_knn_query calls on one
    // index then run side by side, the head of one launch filling the tail of the other.  rebind() refreshes the
    // borrowed pointers (the primary may have grown); the caller guarantees the primary is not being written.
    static Device *create_view(Device *primary);
    void rebind(const Device *primary);
    ~Device();

    int dim() const { return dim_; }
    int metric() const { return metric_; }
    long long capacity() const { return capacity_; }

    bool reserve(long long capacity);
    bool upload_rows(int first_id, int n, const float *rows);
    bool download_rows(int first_id, int n, float *rows);
    // The same upload in the background: a helper thread stages the rows through its own pinned buffers
    // and stream while the caller already works on the rows that have landed.  begin() returns at once;
    // wait(upto) blocks until every row with id < upto is resident (upto < 0: all of them, and the
    // helper has finished).  `rows` stays borrowed until wait(-1) returned.  Float metrics only.
    bool upload_rows_begin(int first_id, int n, const float *rows);
    bool upload_rows_wait(long long upto);
    // Replaces the resident query set (nq x dim); norms for cosine computed on device.
    bool set_queries(const float *queries, int nq);
    // The same, with only the first `head` rows uploaded now: the rest follows behind the traversal launch of the next
    // search_batch (which must come next), the kernel waiting for rows that have not landed yet.  Falls back to
    // set_queries where that does not apply (cosine / int8 rows, head >= nq).
    bool set_queries_streamed(const float *queries, int nq, int head);
    // Forgets a tail that no launch picked up (an error between the two calls): the resident set is then empty.
    void cancel_streamed() { if (tail_.n > 0) { tail_.n = 0; n_queries_ = 0; } }
    // ---- replicas (query sharding over the GPUs of one node, one context per GPU in one process) ----
    // Makes this context a replica of `src`: stored rows (only those it does not hold yet when `rows_from` >= 0 says
    // where they start to differ), per-row norms and the whole graph mirror, copied device to device
    // (hipMemcpyPeerAsync: over xGMI between two GPUs).  pool_len: used ints of src's upper-layer pool.
    bool clone_from(Device *src, long long pool_len);
    // Rows [first, first + n) of src's resident query set land at [at, at + n) of this context's (which is grown to
    // `total` rows and then counts `total` queries): the lock-step fallback gathers every shard on the primary.
    bool adopt_queries(Device *src, long long first, long long n, long long at, long long total);
    int ordinal() const { return device_; }

    StepBuffers *alloc_step(int nslots, int stride);
    void free_step(StepBuffers *sb);
    // Asynchronous: one kernel over slots [0, nslots_used).  `evals` = sum of cnt (for stats).
    bool launch_step(StepBuffers *sb, int nslots_used, uint64_t evals);
    bool wait_step(StepBuffers *sb);
    bool sync();
    // Makes this context's HIP device current on the calling thread.
    bool bind_thread() { return bind(); }

    // --- graph-resident traversal (DESIGN.md "Graph-resident search") ---
    // Mirrors the host adjacency in HBM (layer 0: n x stride0 ints [count, e...]; upper layers:
    // per-node offset into a pool of strideU-int blocks).  Full replace.
    long long graph_nodes() const { return g_n_; }
    // capacity of the kernels' id / distance scratch: the longest adjacency list, rounded up to 8
    int nbcap() const { int m = (g_stride0_ > g_strideU_ ? g_stride0_ : g_strideU_) - 1; m = (m + 7) & ~7; return m < 8 ? 8 : m; }
    // Can the graph-resident kernels run this shape?  (LDS budget for beam width k at this dim;
    // MaxEdges <= 63.)  When not, callers use the host lock-step traversal instead.
    bool traversal_fits(int k, bool with_heuristic, int max_edges) const;
    bool set_graph(const int *adj0, long long n, int stride0, const int *level, const int64_t *upper, const int *pool,
                   long long pool_len, int strideU);
    // Runs njobs KnnQuery traversals with beam width k and returns the first k_out results of
    // the stable distance order (padded with -1 / NaN); out_flag: 1 where the candidate heap
    // outgrew LDS + spill capacity (caller re-runs that job on the lock-step path).  Synchronous.
    // two_heap: the exact two-heap traversal for every job (jobs with aux == -2: the entry point is filtered out of the
    // results and the output is the result heap's ARRAY, the removal search's return value)
    bool search_batch(const SearchJob *jobs, int njobs, int k, int k_out, int *out_ids, float *out_d, int *out_flag, bool keep_repeat_flag = false,
                      bool two_heap = false);
    // search_batch for KnnQuery's own jobs -- resident query i from the entry point, i = 0 .. nq-1: the job array is written
    // on this side and stays on the device while entry point and top layer do not change (a call then uploads no jobs)
    bool search_queries(int nq, int entry, int entry_layer, int k, int k_out, int *out_ids, float *out_d, int *out_flag);
    // search_queries with an allow-set (KnnQuery's filterFnc at layer 0, graph_search_filtered_kernel): a bitset of nbits bits over
    // ids, bit i = bit i & 31 of word i >> 5, ids >= nbits not allowed.  The descent is not filtered; a disallowed node is a
    // candidate but never a result.  The bitset is uploaded to this context for the call.  out_flag as search_batch (1: handed back).
    // search_layer: KnnQuery's `layer` (the descent stops above it, the search reads that layer's lists).
    bool search_filtered(int nq, int entry, int entry_layer, int k, int k_out, const uint32_t *allow_bits, long long nbits, int *out_ids,
                         float *out_d, int *out_flag, int search_layer = 0);
    // search_filtered with a group filter per query (graph_search_grouped_kernel): resident query i is answered from
    // the graph ids j < n_row_group with row_group[j] == query_group[i] -- byte for byte what search_filtered returns for it with
    // that group's ids as the allow-set.  row_group values outside 0 .. n_groups - 1 are in no group; query_group values must lie
    // inside (checked, with n_groups in 1 .. 65536, before anything runs).  The labels and the queries' groups are uploaded to this
    // context for the call, as int32, to a buffer of their own.  A query whose group holds no graph id is padded and never launched
    // (out_flag 0); the others are launched longest traversal first (ascending by their group's id count).  out_flag as search_filtered.
    bool search_grouped(int nq, int entry, int entry_layer, int k, int k_out, const int *row_group, long long n_row_group, const int *query_group,
                        int n_groups, int *out_ids, float *out_d, int *out_flag, int search_layer = 0);
    // search_grouped with a tag mask per query (graph_search_tagged_kernel): resident query i is answered from the
    // graph ids j < n_row_tags whose word row_tags[j] matches query_tags[i] under `match` (0 any, 1 all) -- byte for byte what
    // search_filtered returns for it with those ids as the allow-set.  The words, the masks and the order table are uploaded to this
    // context for the call, to buffers of their own; the candidates of every distinct mask are counted on the device
    // (dk_tag_lists.h).  A query whose mask has no candidate is padded and never launched (out_flag 0); the others are launched
    // ascending by their mask's count.  match outside 0 / 1 and more than 65 536 distinct masks are errors, checked before
    // anything runs.  out_flag as search_filtered.
    bool search_tagged(int nq, int entry, int entry_layer, int k, int k_out, const uint32_t *row_tags, long long n_row_tags, const uint32_t *query_tags,
                       int match, int *out_ids, float *out_d, int *out_flag, int search_layer = 0);
    // MultiLayerKnnQuery's chains (graph_multilayer_kernel): resident query i searched with beam k (>= 2) on every layer from
    // first_layer (<= entry_layer) down to min_layer, each step entering at the nearest result of the one before.
    // out_ids / out_d: [nq][first_layer + 1][k - 1], padded; out_flag[i] = 1: handed back whole.
    bool multilayer_search(int nq, int entry, int entry_layer, int first_layer, int min_layer, int k, int *out_ids, float *out_d, int *out_flag);
    // Remove, second half, for the `n` affected nodes of one (removed node, layer) step (graph_relink_kernel): per node
    // the new neighbour selection out_sel[i * sel_stride ..][0 .. out_cnt[i]); out_flag[i] = 1: this node's answer
    // depends on the heap-array order of the candidates (the caller repeats the step on the lock-step path).
    // Reads the HBM graph mirror; writes nothing to it.  Synchronous.
    // heap_order: `cands` are in the reference's heap-array order (search_batch with two_heap): nothing is flagged.
    // Jobs i < n: affected[i] at layer[i], un-linking removed[i], with the search candidates of step[i]:
    // cands[cand_off[s] ..][0 .. cand_cnt[s]) for the nsteps (removed node, layer) steps.  max_edges0 = MaxEdges(0).
    bool relink_batch(const int *affected, const int *layer, const int *removed, const int *step, int n, const int *cands, const int *cand_off,
                      const int *cand_cnt, int nsteps, int max_edges0, int *out_sel, int *out_cnt, int *out_flag, int sel_stride,
                      bool heap_order = false);
    // Overwrites adjacency lists of the mirror: records [node, layer, count, ids...] of `row_stride` ints; the lists are
    // marked as NOT being a heuristic's ordered output (the link kernel's tested-prefix shortcut starts from 0).
    bool patch_lists(const int *recs, int nrows, int row_stride);
    // Insert, search half, fused on the device: for every job (new item) the descent from
    // (entry, entry_layer) to search_layer = the item's first layer, then on every layer from there
    // down to 0 the traversal with beam k (= MaxCandidates) + RelativeNeighborPruning, the next
    // layer entering at selected[0].  jobs[].qref must be ~item_id; jobs[].aux = the item's first
    // upper-layer output slot (layer L >= 1 goes to slot aux + L - 1), n_upper = slots in total.
    // Results stay in pinned host buffers owned by the context (valid until the next call):
    //   sel0 [njobs x sel_stride] / cnt0 [njobs]: layer 0;  selU [n_upper x sel_stride] / cntU;
    //   flag [njobs]: 1 = handed back.  sel_stride = max_edges0 = MaxEdges(0) = 2M.
    struct InsertResults {
        const int *sel0, *cnt0, *selU, *cntU, *flag;
        int sel_stride;
    };
    // read_log_cap > 0 (the reference-exact windowed Add): every job also records which adjacency lists its searches
    // read -- *read_log = njobs records of read_log_cap ints [n, entries...], a marker -(layer + 1) in front of each
    // layer's node ids, n > read_log_cap - 1 on overflow -- and the selected ids come back with the flags (one wait).
    // The dry run of every selected entry's back-edge append (graph_link_dry_sel_kernel) follows in the same stream:
    // dry0 / dryU, shaped like sel0 / selU, 0 = the append would leave that neighbour's list reading as it does.
    struct WindowExtras {
        int read_log_cap;       // in
        const int *upper_owner; // in: job index per upper-layer output slot (n_upper)
        const int *read_log, *dry0, *dryU; // out: pinned, valid until the next call
        const int *drop0;    // out: per layer-0 selection entry, up to three ids the neighbour's list would lose (dry0's code says how many)
        const int *repeated; // out: per job, 1 = a layer was answered by the exact two-heap traversal (equal distances)
    };
    bool insert_search_batch(const SearchJob *jobs, int njobs, int k, int max_edges0, int n_upper, InsertResults *res, WindowExtras *win = nullptr);
    // insert_search_batch brings back the flags only; this fetches the selected ids into the arrays `res`
    // names (the device-side link half never needs them on the host).
    bool fetch_insert_selections(const InsertResults *res);
    // Keeps the HBM graph mirror in step with nodes appended on the host since the last call:
    // levels / upper offsets of nodes [first, first+n) and the pool tail [pool_from, pool_len).
    // Returns false (with no error set) when capacity is exceeded: caller falls back to set_graph.
    bool graph_append_nodes(long long first, long long n, const int *level, const int64_t *upper, const int *pool,
                            long long pool_from, long long pool_len, bool *need_full_sync);
    // Insert, link half, on the HBM graph mirror (one launch):
    //  rows:   nrows records [node, layer, cnt, ids...] (row_stride ints): OutEdges[layer] = selected
    //  groups: for group g, node g_node[g] / layer g_layer[g] receives the back-edge appends
    //          g_items[g_off[g] .. g_off[g+1]) in order, pruning on overflow (PruneOverflow).
    //  out_lists: ngroups x list_stride ints [cnt, ids...]: the final adjacency list of every group.
    bool link_batch(const int *rows, int nrows, int row_stride, const int *g_node, const int *g_layer, const int *g_off,
                    const int *g_items, int ngroups, int max_edges0, int *out_lists, int list_stride);
    // The same in two halves, so that the host can prepare the next sub-batch while this one runs:
    // begin copies the inputs to one of two pinned staging sets and enqueues copy-in, kernels and
    // copy-out on the stream; finish waits for that set and returns its lists (valid until the set
    // is used again).  Sub-batches are applied in the order they were begun.
    bool link_batch_begin(int set, const int *rows, int nrows, int row_stride, const int *g_node, const int *g_layer, const int *g_off,
                          const int *g_items, int ngroups, int max_edges0, int list_stride, bool want_lists = true);
    bool link_batch_finish(int set, const int **out_lists);
    // Dry run of n single appends [node, layer, item] on the mirror as it stands (graph_link_dry_kernel): changed[i] = 1
    // when list (node, layer) would hold another sequence of ids afterwards.  Nothing is written.  Synchronous.
    bool link_dry_run(const int *jobs3, int n, int max_edges0, int *changed);
    // Link half of the batch whose insert_search_batch just ran (its jobs and selections are still on
    // the device): own lists, grouping of the back-edge appends and the appends / prunes, all on the
    // device, nothing copied back.  Requires that no job of that batch was handed back.
    bool link_batch_planned(int njobs, int n_upper, int max_edges0);
    // The adjacency mirror back to the host (adj0: n x stride0 ints, pool: pool_len ints).
    bool download_graph(int *adj0, long long n, int *pool, long long pool_len);

    // ---- the inner boundary as a foreign host drives it (hnswdev_step_* / hnswdev_dist_*) ----
    // Two step-buffer sets owned by the context (pinned host + HBM mirror), (re)allocated only when
    // they grow: the host fills set A's records while the GPU works on set B.  The lock-step engine
    // of this library is a client of exactly these calls.
    bool step_buffers(int set, int nslots, int stride, int **rec, float **dist, bool internal = false);
    bool step_submit(int set, int nslots_used); // async: H2D, kernel, D2H on the context's stream
    bool step_wait(int set);                    // distances of that set are in its pinned array
    long long resident_queries() const { return n_queries_; }
    // Synchronous conveniences on the same buffers (ids are guarded on the device).  queries ==
    // nullptr: the resident set (hnswdev_set_queries) is used, otherwise it is replaced first.
    bool dist_query_batch(const float *queries, int nq, const int *offsets, const int *ids, float *out);
    bool dist_pair_batch(const int *a, const int *b, int n, float *out);

    // C-ABI staging of a host graph given layer by layer (hnswdev_graph_*)
    bool graph_begin(int n, int max_edges, const int *levels);
    bool graph_set_layer(int layer, const int *counts, const int *edges, int stride);
    bool graph_commit();
    bool knn_search(const float *queries, int nq, int entry_point, int k_beam, int k_out, int *out_ids, float *out_d, int *out_flag, int layer = 0);
    bool knn_search_filtered(const float *queries, int nq, int entry_point, int k_beam, int k_out, const uint32_t *allow_bits, long long nbits,
                             int *out_ids, float *out_d, int *out_flag, int layer = 0);
    bool knn_search_grouped(const float *queries, int nq, int entry_point, int k_beam, int k_out, const int *row_group, long long n_row_group,
                            const int *query_group, int n_groups, int *out_ids, float *out_d, int *out_flag, int layer = 0);
    bool knn_search_tagged(const float *queries, int nq, int entry_point, int k_beam, int k_out, const uint32_t *row_tags, long long n_row_tags,
                           const uint32_t *query_tags, int match, int *out_ids, float *out_d, int *out_flag, int layer = 0);
    // hnswdev_multilayer_search: the slot count, or -1
    int multilayer_search_abi(const float *queries, int nq, int entry_point, int k, int max_layer, int min_layer, int layers_cap, int *out_ids,
                              float *out_d, int *out_flag);
    // RangeQuery on the device (graph_range_kernel): per job the results within `range`, UNSORTED, at
    // found[off[i] .. off[i] + cnt[i]); flag[i] = 1: handed back (cnt 0).  jobs[].qref must name a resident query; the jobs of
    // a call share one search_layer (RangeQuery's `layer`).
    struct RangeResults {
        std::vector<unsigned long long> off;
        std::vector<int> cnt, flag, entry; // entry[i]: the layer-0 entry node FindEntryPointQuery reached
        std::vector<int> state;            // kRangeFinal: found[] holds the reference's order; kRangeTied: ascending, equal distances to replay; kRangeHostSort: as found
        SearchHit *found = nullptr;        // the lists, in pinned memory the context owns: valid until its next range_batch
        size_t found_n = 0;
    };
    // f (host_structs.h): the call's filter.  kBits (a filtered RangeQuery): the traversal is the unfiltered one, and
    // what crosses back is packed -- a kRangeFinal job's cnt[i] entries are its RESULTS in the reference's order, any other job's are
    // its whole CLOSURE (every node within range the traversal reached, allowed or not; kRangeTied: its allowed entries first,
    // ascending), for the host to partition, sort and replay.  range < 0 leaves every closure to the host (the empty-heap rule).
    // kLabels (range_query_grouped): "label[id] == keys[job's query]", ranked by range_sort_grouped_kernel.  kTags
    // (range_query_tagged): "words[id] matches keys[job's query] under `match`" (tag_match_host's rule), ranked by
    // range_sort_tagged_kernel, which also finishes a closure beyond kRangeSortMax entries when its allowed entries fit the table and
    // hold no equal keys (diag range_sort_long=0: handed to the host as the other two sorts do).  What crosses back for those two is
    // the filtered call's.  The per-id array goes to s_allow_ / s_glabel_ / s_ttags_ -- the part that covers graph ids -- unless
    // f.resident says s_ttags_ holds it already.
    bool range_batch(const SearchJob *jobs, int njobs, float range, RangeResults *res, const RangeFilter &f);
    // The candidates of every distinct mask among ids [0, n) of row_tags, counted on the device (tag_count_kernel): cnt[d] for
    // masks[d].  The words stay in s_ttags_ for a range_batch that follows (RangeFilter::resident).  n <= 0: every count 0, no launch.
    bool tag_candidates(const uint32_t *row_tags, long long n, const std::vector<uint32_t> &masks, int match, std::vector<int> &cnt);
    // the C ABI's form: sorted per query, equal distances handed back; results kept until the next call
    bool range_search(const float *queries, int nq, int entry_point, float range, int *out_counts, int *out_flags);
    // ... with an allow-set (ids >= nbits not allowed); false with "System.InvalidOperationException: Heap is empty" where the
    // reference throws (range_replay.h)
    bool range_search_filtered(const float *queries, int nq, int entry_point, float range, const uint32_t *allow_bits, long long nbits,
                               int *out_counts, int *out_flags, int layer = 0);
    // ... with a group filter per query (hnswdev_range_search_grouped): query i as with the allow-set
    // { id : row_group[id] == query_group[i] }; the group arguments and their errors are knn_search_grouped's
    bool range_search_grouped(const float *queries, int nq, int entry_point, float range, const int *row_group, long long n_row_group,
                              const int *query_group, int n_groups, int *out_counts, int *out_flags, int layer = 0);
    // ... with a tag mask per query (hnswdev_range_search_tagged): query i as with the allow-set
    // { id : row_tags[id] matches query_tags[i] under `match` }; the tag arguments and their errors are knn_search_tagged's.  A query
    // whose mask has no candidate among the graph's ids (counted on the device) gets an empty list without a job when range >= 0.
    bool range_search_tagged(const float *queries, int nq, int entry_point, float range, const uint32_t *row_tags, long long n_row_tags,
                             const uint32_t *query_tags, int match, int *out_counts, int *out_flags, int layer = 0);
    bool range_results(int *out_ids, float *out_d);
    // hnswdev_exact_knn (dk_exact.h): for each query the k uploaded rows of smallest (distance, id) among ids
    // [0, min(n_rows, uploaded)) that allow_bits allows (nullptr: all of them; else nbits bits as for search_filtered), ascending,
    // padded with -1 / NaN (nbits is ignored without a bitset).  A flat scan: no graph is read.  queries == nullptr: the resident
    // set (nq of its rows); otherwise the queries are staged by set_queries' code into a buffer of the scan's own and the
    // resident set stays what it was.  1 <= k <= 1024.  Synchronous.
    bool exact_knn(const float *queries, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d);
    // hnswdev_exact_knn_collapsed: exact_knn whose result is shaped, not its candidates -- walk exact_knn's
    // candidates in ascending (distance, id) order, keep an id while fewer than per_group kept ids have its label row_group[id], stop
    // at k; padding as exact_knn.  Labels are compared for equality only.  row_group must cover every candidate id: n_row_group >=
    // min(n_rows, uploaded), checked before anything is launched; 1 <= per_group <= k <= 1024.  With per_group == k the rows are
    // exact_knn's, byte for byte.  The labels go up once per call; queries == nullptr and the resident set as exact_knn.  Synchronous.
    bool exact_knn_collapsed(const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group, int per_group,
                             const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d);
    // knn_query_collapsed on one context: search_filtered (allow_bits != nullptr) or search_batch's traversal of
    // resident queries 0 .. nq - 1 with a result of `beam` entries per query, which stays on the device: collapse_rows_kernel
    // walks every row there -- an entry is kept while fewer than per_group kept entries have its label row_group[id] -- and only
    // the first k columns are copied out.  out_ids / out_d: nq x k.  row_group must cover the graph's ids (n_row_group >=
    // graph_nodes()); 1 <= per_group <= k <= beam.  out_flag as search_filtered: a flagged row holds nothing.
    bool search_collapsed(int nq, int entry, int entry_layer, int ef, int beam, int k, const int *row_group, long long n_row_group, int per_group,
                          const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d, int *out_flag, int search_layer = 0);
    // ---- query by stored id --------------------------------------------------------------------------------
    // hnswdev_gather_rows: out[i] = the stored row ids[i] as dim floats -- hnswdev_download_rows' values for the row kind (f32: a
    // copy; f16: the rounded row widened; int8: q * scale), gathered on the device in one launch (gather_rows_kernel) and copied back
    // in one copy.  ids may repeat, in any order; an id outside the uploaded rows gives a row of zeros.  n <= 0: nothing is written.
    bool gather_rows(const int *ids, int n, float *out);
    // The resident query set made of stored rows: resident query i is what set_queries makes of gather_rows' row ids[i] (int8:
    // quantised again by quantize_rows_kernel; cosine: norms by row_sqrtnorm_kernel), built on the device.  The ids stay on the
    // device beside the set, for search_self, until the resident set is replaced.
    bool set_queries_by_id(const int *ids, int nq);
    // KnnQuery for the resident queries set_queries_by_id left (graph_search_self_kernel): query i is answered from every graph id
    // but ids[i] -- byte for byte what search_filtered returns for it with that allow-set.  out_flag as search_filtered.
    bool search_self(int nq, int entry, int entry_layer, int k, int k_out, int *out_ids, float *out_d, int *out_flag, int search_layer = 0);
    // hnswdev_knn_search_by_id: set_queries_by_id + search_self on the committed graph
    bool knn_search_by_id(const int *ids, int nq, int entry_point, int k_beam, int k_out, int *out_ids, float *out_d, int *out_flag, int layer = 0);
    // hnswdev_exact_knn_by_id: exact_knn whose query i is the stored row ids[i] (gathered into the scan's own query buffer: the
    // resident set stays what it was) and whose candidates are exact_knn's minus ids[i] -- the scan's sink drops the pair
    // (exact_scan_kernel<M, ExactTopKSelf>), which is not counted in exact_evals.  An id outside the uploaded rows is an error.
    bool exact_knn_by_id(const int *ids, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_d);
    // hnswdev_exact_range: exact_knn's candidates, queries and distances; per query EVERY candidate with
    // distance <= range (the float compare), ascending by (distance, id), of any number.  out_counts[i]: query i's; the lists stay
    // in the context, concatenated in query order, until the next exact_range and are copied out by exact_range_results (the
    // traversal's range_results has buffers of its own).  false: no results are kept and every count is 0.  Synchronous.
    bool exact_range(const float *queries, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_counts);
    bool exact_range_results(int *out_ids, float *out_d);
    size_t exact_range_total() const { return xr_ids_.size(); }
    // hnswdev_exact_range_by_id: exact_range whose query i is the stored row ids[i] -- gathered into the scan's own
    // query buffer as exact_knn_by_id gathers it, the resident set untouched -- and whose candidates are exact_range's minus ids[i]
    // (exact_scan_kernel<M, ExactRangeSelf>: the pair is not counted in exact_evals).  Rounds, capacities, the repeated pass, the sort
    // limit and exact_range_results are exact_range's.  An id outside the uploaded rows is an error, in front of any launch.
    bool exact_range_by_id(const int *ids, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_counts);
    // hnswdev_exact_range_groups: the single-linkage groups of the MEMBERS -- exact_range's candidates, ascending.
    // a < b are joined when the distance with the stored row of a as the query (handled as exact_range_by_id handles it) and row b as
    // the candidate is <= range; out_labels[v] for v in [0, min(n_rows, uploaded)): the smallest member of v's group, -1 where v is
    // no member.  out_info: [members, groups, pairs a < b within the range, pairs measured = m (m - 1) / 2].  One scan with a
    // union-find as its sink (exact_scan_kernel<M, ExactRangeUnion>): no list is kept or copied.  Fewer than two members: no launch.
    // Neither the resident set nor exact_range's pending results are touched.
    bool exact_range_groups(long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, uint64_t *out_info);
    // hnswdev_exact_range_density: DBSCAN over exact_range_groups' members and within pairs.  out_counts[v]: the
    // within pairs that hold v, -1 where v is no member.  v is core when out_counts[v] + 1 >= min_samples (min_samples < 1: an error);
    // the clusters are the components of the core members under the within pairs between two of them, labelled with their smallest
    // core id; a member that is not core takes the label of its core within-neighbour of smallest (distance, id), -1 without one.
    // out_info: [members, clusters, core, border, noise, pairs within, pairs measured, scans].  out_labels == nullptr: the counts
    // alone -- one scan, no arena, no union-find, the slots that need labels 0.  Otherwise one scan (ExactRangeDensity) and the pairs
    // kept in an arena, or two scans where the arena could not hold them (ExactRangeDensityJoin).  Fewer than two members: no launch.
    // Neither the resident set nor exact_range's pending results are touched.
    bool exact_range_density(long long n_rows, float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels, int *out_counts,
                             uint64_t *out_info);
    // hnswdev_graph_edge_groups / hnswdev_graph_near_edges: near-duplicates over the EDGES of layer 0 of the
    // committed graph.  The MEMBERS are exact_range_groups' -- the uploaded rows of [0, n_rows) that allow_bits allows -- that are
    // nodes of the graph.  An edge (i, j): i a member, j in i's layer-0 list, j a member (directed); it is within the range when the
    // distance with the stored row of i as the query (gathered as the by-id calls gather it) and row j as the candidate is
    // <= range.  graph_edge_kernel<M, Sink> measures every edge once, in rounds of at most 65 536 owners (`edge_round`).
    // graph_edge_groups (sink EdgeUnion): out_labels[v], v in [0, min(n_rows, uploaded)), the smallest member of v's component under
    // the within-edges read both ways, -1 where v is no member; out_info: [members, groups, edges within, edges measured, launches
    // of the edge kernel].  graph_near_edges (sink EdgeList): keeps the within-edges, ascending by owner and inside one owner by
    // (distance, id), for graph_near_edges_results; *out_count is their number.  Fewer than two members: no launch.  No graph
    // committed (and n_rows > 0): an error.  Neither the resident set nor exact_range's pending results are touched.
    bool graph_edge_groups(long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, uint64_t *out_info);
    bool graph_near_edges(long long n_rows, float range, const uint32_t *allow_bits, long long nbits, long long *out_count);
    bool graph_near_edges_results(int *out_src, int *out_dst, float *out_d);
    size_t graph_near_edges_total() const { return ge_src_.size(); }
    // hnswdev_exact_knn_grouped: exact_knn with a candidate set per query.  Query i's candidates are the uploaded
    // ids j < min(n_rows, uploaded, n_row_group) with row_group[j] == query_group[i]; a row_group value outside [0, n_groups) puts
    // the id in no group, a query_group value outside it is an error (nothing is written).  The groups' id lists are built on the
    // device from row_group (one upload, one copy back of the n_groups counts) and every group is scanned in the same launch.
    // Everything else -- distances, order, padding, k, queries == nullptr, the untouched resident set -- is exact_knn's.  Synchronous.
    bool exact_knn_grouped(const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group, const int *query_group,
                           int n_groups, int *out_ids, float *out_d);
    // hnswdev_exact_knn_tagged: exact_knn_grouped where query i's candidates are the uploaded ids
    // j < min(n_rows, uploaded, n_row_tags) whose word row_tags[j] matches query_tags[i] under `match` (0 any, 1 all).  Every
    // distinct mask is a list; the lists overlap, and are built on the device (dk_tag_lists.h) in batches of masks whose counts sum
    // to at most kTagListEntries (`tag_list_cap`); a mask with more is a batch alone.  Each batch is one grouped scan -- rounds,
    // work items, scan and merge kernels are exact_knn_grouped's -- over the queries of its masks.  Distances, order, padding, k,
    // queries == nullptr and the untouched resident set as exact_knn.  Synchronous.
    bool exact_knn_tagged(const float *queries, int nq, long long n_rows, int k, const uint32_t *row_tags, long long n_row_tags, const uint32_t *query_tags,
                          int match, int *out_ids, float *out_d);
    // HIP-event time of the tagged calls' list-building kernels (count, offsets, fill) made while profiling was on
    double tag_list_ms() const { return xt_list_ms_; }
    // hnswdev_exact_range_grouped: exact_range with exact_knn_grouped's candidate set per query -- the group
    // arguments, their errors and the group lists are that call's; radius, order, counts, capacities and the results kept for
    // exact_range_results are exact_range's.  A query whose group has no member gets an empty list without being scanned.
    // false: no results are kept and every count is 0.  Synchronous.
    bool exact_range_grouped(const float *queries, int nq, long long n_rows, float range, const int *row_group, long long n_row_group,
                             const int *query_group, int n_groups, int *out_counts);
    // hnswdev_exact_range_tagged: exact_range with exact_knn_tagged's candidate set per query -- the tag arguments,
    // their errors, the lists and the batches of masks are that call's; each batch is one grouped range scan (exact_range_grouped's
    // rounds, capacities, pass B and sort limit) over the queries of its masks.  The lists are kept for exact_range_results
    // concatenated in the CALLER's query order, however many batches ran.  A query whose mask has no candidate gets an empty list
    // without a scan.  false: no results are kept and every count is 0.  Synchronous.
    bool exact_range_tagged(const float *queries, int nq, long long n_rows, float range, const uint32_t *row_tags, long long n_row_tags,
                            const uint32_t *query_tags, int match, int *out_counts);
    // HIP-event time of the list-building kernels (count, offsets, place) of the grouped calls made while profiling was on
    double exact_grouped_list_ms() const { return xg_list_ms_; }
    // hnswdev_graph_info / hnswdev_graph_components (dk_graph_info.h): HNSWInfo.LayerInfo (HNSWInfo.cs:18-43) and the
    // number of weakly connected components (GraphNavigator.cs:350-419) of one layer of the mirror, computed on the device from the
    // mirror as it stands; nothing of it is copied back.  The layer's members: ids < graph_nodes() that are live -- live_bits ==
    // nullptr: all of them; else nbits bits as for search_filtered, ids >= nbits not live -- with level >= layer.  A list entry that
    // names no member counts in its owner's out-degree and nowhere else.  with_in_edges == false (AllowRemovals off): the in-edge
    // fields are 0 and no in-degree pass runs.  No member: nodes_count 0, every statistic 0, 0 components.  Any layer >= 0 may be
    // asked for (graph_info_layer is the C ABI's range test).  Synchronous.
    bool graph_info(int layer, const uint32_t *live_bits, long long nbits, bool with_in_edges, hnsw_mi355x_layer_info *out);
    bool graph_components(int layer, const uint32_t *live_bits, long long nbits, int *out_count);
    bool graph_info_layer(const char *who, int layer);
    // hnswdev_graph_reach_layer / hnswdev_graph_reach (dk_graph_reach.h): what can be reached over OUT-edges.  Members
    // and the live set are graph_info's; an entry u -> v counts only between two members.  graph_reach_layer: one layer, the seeds a
    // bitset (seed_nbits bits, ids beyond it and ids that are no members are no seeds; an empty set reaches nothing and launches no
    // expansion).  out_reached_bits: ceil(graph_nodes() / 32) words or nullptr; out_hops: graph_nodes() ints or nullptr (>= 0: the BFS
    // distance from the seeds, -1: a member not reached, -2: no member); out_summary: members, member seeds, reached, largest hop.
    // graph_reach: the chain F_top = reach_top({entry_point}), F_L = reach_L(F_{L + 1}) down to min_layer, `top` the level the caller
    // knows the entry point to have (graph_reach_top is the C ABI's); the seeds of a layer are the hop array of the layer above,
    // on the device.  out_layers[L] is filled for min_layer <= L < min(cap, top + 1), the two arrays describe min_layer.  An entry
    // point that is out of range or no member of layer `top` reaches nothing.  top + 1, or -1.  Synchronous; the rounds of a layer
    // are bounded by its member count (every round reaches a new node), beyond that the call fails.
    bool graph_reach_layer(int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits,
                           uint32_t *out_reached_bits, int *out_hops, uint64_t out_summary[4]);
    int graph_reach(int entry_point, int top, const uint32_t *live_bits, long long nbits, int min_layer, hnsw_mi355x_layer_reach *out_layers, int cap,
                    uint32_t *out_reached_bits, int *out_hops);
    bool graph_reach_top(const char *who, int entry_point, int *top);

    // One round of repair_reachability (dk_graph_repair.h), steps 1 - 3, on one layer of the mirror; the mirror is read,
    // never written.  Members and the live set are graph_info's.  The seeds: seed_mode kRepairSeedEntry: the one id entry_point,
    // kRepairSeedBits: seed_bits / seed_nbits as graph_reach_layer's, kRepairSeedAbove: the nodes that the round last run into
    // slot which ^ 1 reached (the layer above).  The BFS writes slot `which` of the two hop arrays, which stay on the device.  With
    // `propose` and members left unreached: for each of them, ascending, the `cands` nearest reached members -- the ids exact_knn
    // returns for its stored row as the query, k = cands, the reached set as allow-set -- and for each such candidate v the slot of
    // v's list that the proposal rule names (max_edges: MaxEdges(layer)).  1 <= cands <= 64.  Synchronous.
    bool graph_repair_round(int layer, const uint32_t *live_bits, long long nbits, int seed_mode, int entry_point, const uint32_t *seed_bits, long long seed_nbits,
                            int which, int cands, int max_edges, bool propose, GraphRepairRound *out);
    // patch_lists for the lists a round's apply step changed, counted
    bool graph_repair_patch(const int *recs, int nrows, int row_stride);
    // hnswdev_graph_repair_propose: a round with seed_bits on slot 0, copied out: *out_n = |U|, min(cap, |U|) rows written.  0 or -1.
    int graph_repair_propose(int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits, int cands, int max_edges,
                             int *out_n, int *out_ids, int *out_cands, int *out_codes, int cap);

    void set_profiling(bool on) { profiling_ = on; }

    // search launches of a call that shares the chip with another call (query lanes) keep no idle waves behind as shadows

    void set_shadows_allowed(bool on) { shadows_allowed_ = on; }
    void get_stats(hnswdev_stats *out);
    void reset_stats();
    // The counter blocks of counter_blocks.h: a block's kCounterSlots values since reset_stats, copied to out[]
    void counters(CounterBlock b, uint64_t *out) const { std::copy_n(counters_[(int)b], kCounterSlots[(int)b], out); }
    // The row prefilter's counters (a view adds to its primary's): launches that ran with it, rows measured on the shadow, rows
    // measured again from f32, shadow rows packed.  All zero on a context that has none (every metric but sq_euclid, diag row_prefilter=0).
    void row_prefilter_stats(uint64_t out[4]);
    // Which kernel form those launches took: out[0] the run-time-length form (kFormLeanPF), out[1] the fixed-length one (kFormLeanPFFixed).
    void row_prefilter_form_stats(uint64_t out[2]);
    // The shadow as it stands, read only (nothing is packed or allocated): out[0] the watermark (shadow rows [0, out[0]) are current),
    // out[1] the 32 bits of E; rows: the shadow rows [first_id, first_id + count) widened to f32, `count` x dim floats (count 0: none).
    // false for a range that is not below the watermark.  A context without a shadow has watermark 0.
    bool row_prefilter_peek(long long first_id, int count, uint64_t out[2], float *rows);
    // The 8-bit shadow's own counters: launches, rows packed, rows measured on it, rows re-read, full packs (a fresh grid), switches to f16.
    void row_prefilter8_stats(uint64_t out[6]);
    // ... and the shadow as it stands, read only: out[0] the watermark, out[1] lo's bits, out[2] step's bits, out[3] E8's bits; codes: the
    // code bytes of rows [first_id, first_id + count), kPfFixedDim each (count 0: none).  false for a range not below the watermark.
    bool row_prefilter8_peek(long long first_id, int count, uint64_t out[4], unsigned char *codes);

    // C-ABI callers: one call at a time per context (hnswdev_* exports hold this), and the
    // context's own last-error string.
    std::mutex &mutex() { return mu_; }
    void set_error(const std::string &msg) { std::lock_guard<std::mutex> lk(err_mu_); err_ = msg; }
    std::string error() { std::lock_guard<std::mutex> lk(err_mu_); return err_; }

private:
    Device() = default;
    std::mutex mu_, err_mu_;
    std::string err_;
    bool bind();
    bool abi_entry(const char *who, int entry_point, int *top, bool args_ok = true);
    bool abi_begin(const char *who, const float *queries, int nq, int entry_point, int layer, int *top, bool args_ok = true);
    int device_ = 0, dim_ = 0, metric_ = 0;
    int pitch_ = 0; // 32-bit words per resident query, and what the kernels get as `dim` (== dim_ for the float metrics, f16 rows included; the int8 record otherwise)
    int row_pitch_ = 0; // 32-bit words per STORED row: pitch_, but the half-precision record (8 * ceil(dim / 16)) for the _f16 metrics, whose queries stay f32
    // Every buffer, event and stream below is a holder (dev_buf.h): it frees itself, and its cap() is the only record of its size.
    DevBuf<float> q_stage_; // int8 and f16 rows: float staging area on the device (quantise / round on upload, dequantise / widen on download)
    long long capacity_ = 0;
    long long n_rows_hw_ = 0; // high-water mark of uploaded rows (id validation)
    DevBuf<float> d_rows_;    // (a view borrows the rows, their norms and the graph mirror: rebind)
    DevBuf<double> d_row_sn_; // cosine: sqrt((double)|row|^2_f32)
    // The half-precision SHADOW of the stored rows (sq_euclid contexts; dk_sorted_top.h "row prefilter"): shared by a
    // primary and its views, allocated by the first launch that takes the lean search form.  Rows [0, packed) are current; every
    // writer of stored rows goes through rows_written(), which lowers `packed`, and a launch packs [packed, n) before it reads.
    struct RowPrefilter {
        std::mutex mu;
        DevBuf<float> rows;                // f16_row_words(dim) words per row, `row_cap` rows
        DevBuf<unsigned long long> words;  // [bits of E, rows measured on the shadow, rows re-read] (device-side, cumulative)
        long long row_cap = 0, packed = 0;
        bool lost = false;                 // a launch re-read more than half of its rows: the lean form until the next repack
        bool no_memory = false;            // the shadow could not be allocated: the lean form, no error
        uint64_t launches = 0, on_shadow = 0, reread = 0, rows_packed = 0;
        uint64_t form_launches[2] = {0, 0}; // of `launches`: in the run-time-length form, in the fixed-length form (kFormLeanPFFixed)
        // The 8-bit shadow (kFormLeanPF8Fixed; rows of kPfFixedDim words): a watermark, a fallback and counters of its own beside the
        // f16 ones, allocated by the first launch that takes it.  The counters above stay the f16 forms'; the ABI reports the totals.
        struct Codes {
            DevBuf<unsigned char> bytes;        // kPfFixedDim code bytes per row, `row_cap` rows
            DevBuf<unsigned long long> words;   // [bits of E8, rows on the shadow, rows re-read, smallest | largest element key, .., word kPf8GridWord: lo | step << 32] (device-side)
            long long row_cap = 0, packed = 0;
            bool lost = false;                  // a launch re-read more than a quarter of its rows: the f16 prefilter until rows are written again
            bool no_memory = false;
            uint64_t launches = 0, on_shadow = 0, reread = 0, rows_packed = 0, full_packs = 0, fallbacks = 0;
        } c8;
    };
    std::shared_ptr<RowPrefilter> pf_;
    void rows_written(long long first_id); // stored rows [first_id, ...) have changed, or the row matrix has moved
    int row_prefilter_ready();             // 0: none; 1: the f16 shadow, 2: the 8-bit shadow is allocated and current for rows [0, n_rows_hw_) (packs what is missing)
    bool row_prefilter8_ready();           // ... the 8-bit one (pf_->mu held)
    DevBuf<float> d_queries_;
    DevBuf<double> d_q_sn_;
    long long q_capacity() const { return (long long)(d_queries_.cap() / (size_t)pitch_); }
    long long n_queries_ = 0;
    // graph mirror; the node arrays are replaced together and g_tested0_, allocated last, stands for their capacity in nodes,
    // as g_testedU_ does for the pool pair's
    DevBuf<int> g_adj0_, g_level_, g_pool_;
    DevBuf<int64_t> g_upper_;
    long long g_n_ = 0;
    long long g_cap_n() const { return (long long)g_tested0_.cap(); }
    long long g_pool_cap() const { return (long long)g_testedU_.cap(); }
    bool graph_room(long long n, long long node_cap, int stride0, long long pool_len);
    // per adjacency list: how many leading entries are the ordered, mutually tested output of a
    // RelativeNeighborPruning run (graph_link_kernel's shortcut); 0 = unknown
    DevBuf<int> g_tested0_, g_testedU_;
    int g_stride0_ = 0, g_strideU_ = 0;
    // search scratch
    DevBuf<unsigned> s_visited_;
    DevBuf<int> s_jobctr_; // persistent launches: next job
    DevBuf<int> lp_slot_[3]; // device-side link grouping: per list slot count / fill / offset
    DevBuf<int> lp_grp_[6];  // per group node / layer / start / count; items as filed; items in batch order
    DevBuf<int> lp_counters_;
    int last_insert_jobs_ = 0, last_insert_upper_ = 0, last_insert_stride_ = 0; // what insert_search_batch left on the device
    int fetch_njobs_ = 0, fetch_nupper_ = 0;                                    // ... and what fetch_insert_selections would copy
    DevBuf<int> s_vistab_; // per-wave visited-id hash tables
    int s_vistab_each_ = 0;
    DevBuf<int> s_fvistab_; // ... and those of the filtered search launches
    int s_fvistab_each_ = 0;
    bool visited_scratch(int k, int min_cap, bool allow_hash, VisitedScratch *out, bool filtered = false);
    bool plan_traversal(bool insert, int k, bool two_heap, size_t lds, TraversalLaunch *out, bool filtered = false);
    template <class Upload, class Launch> // the one launcher of the resident-query kernels (search_filtered, multilayer_search)
    bool run_resident(size_t row, long long chunk, size_t extra, bool hashed, int nq, int *out_ids, float *out_d, int *out_flag, Upload &&upload,
                      Launch &&launch);
    // what search_filtered / search_grouped / search_tagged share: the entry checks, the planning step, the launches, the overflow count
    template <class OwnRules> bool predicate_call_ok(const PredicateCall &c, OwnRules &&own_rules);
    template <class Of> auto plan_predicate_search(const PredicateCall &c, Of of);
    template <class K, class Upload, class JobsOf, class Predicate>
    bool run_predicate_search(const PredicateCall &c, const PredicatePlan<K> &p, size_t extra, Upload &&upload, JobsOf &&jobs_of, Predicate &&predicate);
    uint64_t count_search_overflows(const PredicateCall &c);
    bool count_launch(const LaunchFamily *family, unsigned long long evals, bool hashed, bool timed, void *t0, void *t1);
    int num_cu_ = 256;
    // Persistent launches never use more than 16 one-wave blocks per CU (the traversal kernels need
    // >= 128 VGPRs): the per-wave scratch (visited bitsets, spill areas, logs) is sized for that.
    int max_slots() const { return num_cu_ * max_waves_per_cu(); }
    static int max_waves_per_cu(); // persistent waves per CU the per-wave scratch is sized for
    DevBuf<SearchJob> s_jobs_; // s_jobs_, s_cnt_ and s_flag_ are replaced together: s_flag_, allocated last, stands for the job capacity
    DevBuf<SearchHit> s_hits_;
    DevBuf<int> s_cnt_, s_flag_;
    DevBuf<unsigned long long> s_evals_;
    DevBuf<int> s_sel_, s_lcnt_, s_selU_, s_cntU_, s_iflag_;
    PinBuf<char> h_res_; // pinned: results of insert_search_batch
    DevBuf<int> s_rl_; // relink / patch staging on the device
    DevBuf<int> s_order_; // insert search: processing order of a batch's jobs
    DevBuf<int> s_rlog_; // insert search: per-job read logs (exact-window Add)
    struct QueryTail { const float *src = nullptr; long long first = 0, n = 0; } tail_; // set_queries_streamed: rows still on the host
    PinBuf<int> h_ready_; // rows of the query set that have landed (host memory, read by the kernel ...
    int *d_ready_ = nullptr; // ... through this device address of it)
    DevStream copy_stream_;
    bool upload_tail();
    DevBuf<int> s_dry_;  // link_dry_run: [jobs | flags]
    DevBuf<int> s_wdry_; // windowed insert search: upper_owner
    DevBuf<int> s_win_;  // windowed insert search: every output of the launch, laid out like the pinned result block
    DevBuf<SearchHit> s_spill_;
    DevBuf<SearchHit> s_fspill_; // filtered searches: their own, larger spill areas (allocated by the first such call)
    DevBuf<unsigned> s_allow_;   // filtered searches: the call's allow-set
    DevBuf<int> s_glabel_;       // grouped searches: the call's row_group
    DevBuf<int> s_gquery_;       // ... [query_group of the call | order tables of its launches]
    DevBuf<unsigned> s_ttags_;   // tagged calls: the call's row_tags
    DevBuf<unsigned> s_tmask_;   // ... its distinct masks
    DevBuf<int> s_tcnt_;         // ... per distinct mask: [candidates | offset of its segment in x_ids_ | the filling kernel's cursor]
    DevBuf<int> s_tquery_;       // tagged searches: [query_tags of the call | order tables of its launches]
    double xt_list_ms_ = 0.0;
    bool tag_counts(const unsigned *row_tags, long long n, const std::vector<uint32_t> &masks, int match, std::vector<int> &cnt);
    DevBuf<int> s_self_;         // by-id calls: the ids whose rows are the resident queries (valid while q_by_id_)
    DevBuf<int> x_self_;         // ... the ids of exact_knn_by_id's queries, and gather_rows' ids
    bool q_by_id_ = false;       // the resident set was made by set_queries_by_id and s_self_ holds its n_queries_ ids
    bool query_room(int nq);
    bool upload_ids(const int *ids, int n, DevBuf<int> &d_ids);
    bool gather_launch(const int *d_ids, long long n, float *out);
    bool gather_queries(const int *ids, int n, DevBuf<int> &d_ids, float *d_q, double *d_qsn);
    DevBuf<int> x_ids_;                 // exact_knn: the call's ascending id list (exact_compact_kernel)
    DevBuf<long long> x_boff_;          // ... set bits in front of each block of bitset words
    DevBuf<unsigned long long> x_lists_; // ... the per-(query, chunk) lists of a round: at most 1 GiB, allocated by the first call and kept
    DevBuf<int> x_out_;                 // ... a round's [ids | distances]
    DevBuf<unsigned long long> x_evals_; // ... (query, row) pairs the scan kernel measured, counted on the device
    DevBuf<float> x_queries_;           // ... its own query set (set_queries writes it while it stands in for d_queries_)
    DevBuf<double> x_q_sn_;
    bool exact_queries(const char *who, const float *queries, int nq, const float **d_q, const double **d_qsn);
    bool exact_id_list(const uint32_t *allow_bits, long long n_allow, long long *m);
    bool exact_knn_rounds(const float *d_q, const double *d_qsn, int nq, const int *d_idlist, long long m, int k, int *out_ids, float *out_d, int *d_keep_ids,
                          const int *d_self = nullptr, const ExactCollapseArgs *collapse = nullptr);
    // the two calls over the graph's edges: out_labels / out_info, or -- keep_list -- the edges into ge_*
    bool graph_edges_run(const char *who, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, uint64_t *out_info,
                         bool keep_list);
    DevBuf<unsigned> e_bits_;             // graph_edges_run: the members as a bitset
    DevBuf<unsigned long long> e_ctr_;    // ... [next job (an int) | edges within | edges measured]
    DevBuf<int> e_cnt_;                   // ... EdgeList: within-edges per owner of a round
    DevBuf<unsigned long long> e_keys_;   // ... EdgeList: a round's segments of stride0 - 1 keys
    std::vector<int> ge_src_, ge_dst_;    // graph_near_edges' result, until the next graph_near_edges
    std::vector<float> ge_d_;
    DevBuf<int> x_clabels_;               // exact_knn_collapsed: row_group as uploaded
    DevBuf<unsigned long long> x_cinfo_;  // ... [keys dropped by the cap | entries evicted], counted on the device
    // search_collapsed: while set, run_resident and search_batch_impl collapse a launch's rows on the device (width -> k columns)
    // before the copy-out and write rows of k entries to the caller's arrays
    struct RowCollapse { const int *d_labels; long long n_labels; int per_group, k; };
    const RowCollapse *row_collapse_ = nullptr;
    bool collapse_and_fetch(int *d_ids, float *d_d, int nj, size_t width, int *h_ids, float *h_d);
    bool exact_copy_out(void *dst, const void *src, size_t bytes);
    ExactStart exact_scan_begin(const char *who, const float *queries, int nq, long long n_rows, const uint32_t *allow_bits, long long nbits, ExactScanInput *in);
    bool exact_scan_args(const float *d_q, const double *d_qsn, long long off, int nr, int qt, int piece, ExactScanArgs *a);
    template <class Enqueue, class Fetch> // the one timed, counted launch of the flat scan: every exact_* statistic is written there
    bool exact_timed_scan(unsigned long long *h_ev, Enqueue &&enqueue, Fetch &&fetch);
    bool exact_range_call(int nq, int *out_counts, const std::function<bool()> &body);
    // the rounds of exact_range and exact_range_by_id: d_self nullptr, or the nq ids on the device whose rows the queries are
    bool exact_range_rounds(const char *who, const ExactScanInput &in, int nq, float range, const int *d_self, int *out_counts);
    DevBuf<int> x_uparent_;               // exact_range_groups: the union-find's parent[], then the labels behind it
    DevBuf<unsigned long long> x_upairs_; // ... pairs within the range, counted on the device
    // what exact_range_groups and exact_range_density share (device_backend.hip): the members listed, the plan of the triangle's
    // scans and their buffers; then one scan of the triangle, a timed launch per round of members
    bool exact_triangle_begin(const char *who, long long n_rows, const uint32_t *allow_bits, long long nbits, ExactTriangle *t);
    bool exact_triangle_ready(const char *who, ExactTriangle *t);
    template <class Launch> // launch(args, tiles, stream) -> hipError_t: the scan with the call's sink, its queries' ids in x_self_
    bool exact_triangle_scan(const ExactTriangle &t, Launch &&launch, unsigned long long *measured);
    DevBuf<int> x_dcounts_;               // exact_range_density: within pairs per id, -1 off the members
    DevBuf<unsigned long long> x_dattach_; // ... per id: the smallest (distance, core id) key offered to a member that is not core
    DevBuf<ExactDensityPair> x_darena_;   // ... phase A's within pairs: 2^24 records (256 MiB) unless `density_pair_cap` says otherwise
    bool exact_range_finish(ExactRangeWork &w, int ns, const unsigned *c, const long long *seg, const int *sq, const long long *obase, size_t base,
                            bool counts_on_device, uint64_t *by_device, uint64_t *by_host);
    DevBuf<unsigned long long> x_rarena_; // exact_range: the round's keys, a segment per query: at most 1 GiB, grown on demand and kept
    DevBuf<long long> x_rseg_, x_rooff_;  // ... per query of a round: where its segment starts (one more: the end), where its ordered list goes
    DevBuf<unsigned> x_rcnt_;             // ... keys within the range
    DevBuf<int> x_rout_;                  // ... the lists ordered on the device: [ids | distances]
    std::vector<int> xr_ids_;             // ... the call's results until the next call (exact_range_results)
    std::vector<float> xr_d_;
    DevBuf<int> x_grow_;                  // exact_knn_grouped: row_group as uploaded
    DevBuf<int> x_gcnt_;                  // ... per group: [members | offset of its segment in x_ids_ | the placing kernel's cursor]
    DevBuf<int> x_gperm_;                 // ... queries == NULL: where each query of the sorted order is in the resident set
    DevBuf<unsigned char> x_gwork_;       // ... a round's tables: [ExactMergeItem per query | ExactWorkItem per scan block]
    bool exact_group_lists(const char *who, const int *row_group, long long n, int n_groups, std::vector<int> &cnt, std::vector<int> &goff, uint64_t *listed);
    bool exact_sorted_queries(const char *who, const float *queries, int nq, const std::vector<int> &order, const float **d_q, const double **d_qsn,
                              const int *resident = nullptr);
    bool exact_grouped_plan(const char *who, int k, ExactGroupedCall *gc);
    template <class OnBatch> // the batches of masks of exact_knn_tagged / exact_range_tagged, each handed to on_batch (device_backend.hip)
    bool exact_tag_batches(const char *who, const float *queries, int nq, long long n, int k, const uint32_t *row_tags, const TagCall &tc, int match,
                           std::vector<int> &cnt, uint64_t *info, OnBatch &&on_batch);
    bool exact_knn_grouped_scan(const char *who, const float *queries, const int *resident, int nq, int k, const int *query_group, int n_groups,
                                const ExactGroupedCall &gc, int *out_ids, float *out_d, uint64_t *blocks);
    bool exact_range_grouped_scan(const char *who, const float *queries, const int *resident, int nq, float range, const int *query_group, int n_groups,
                                  const ExactGroupedCall &gc, int *out_counts, uint64_t *info);
    ExactStart exact_grouped_begin(const char *who, bool args_ok, const float *queries, int nq, long long n_rows, int k, const int *row_group,
                                   long long n_row_group, const int *query_group, int n_groups, ExactGroupedCall *gc);
    double xg_list_ms_ = 0.0;
    bool graph_info_begin(const char *who, int layer, const uint32_t *live_bits, long long nbits, LayerView *g);
    bool graph_info_fetch(const GraphAcc **acc);
    DevBuf<unsigned long long> gi_acc_; // graph_info / graph_components: the call's GraphAcc
    DevBuf<unsigned> gi_live_;          // ... its live set
    DevBuf<int> gi_indeg_, gi_parent_;  // ... per node: in-degree on the layer; parent in the union-find's forest
    DevBuf<int> gi_inhist_;             // ... nodes per in-degree, max in-degree + 1 bins
    bool graph_reach_room();
    bool graph_reach_run(const LayerView &g, const ReachSeeds &seeds, int which, bool want_bits, uint64_t summary[4]);
    bool graph_reach_copy_out(int which, uint32_t *out_reached_bits, int *out_hops);
    DevBuf<int> gr_hop_[2], gr_q_[2];   // graph_reach: per node the hop (two arrays: a layer's is the seed set of the layer below); the two frontier queues
    DevBuf<unsigned> gr_bits_, gr_seed_; // ... the reached set as a bitset; graph_reach_layer's seed set
    DevBuf<unsigned long long> gr_acc_; // ... the layer's ReachAcc
    DevBuf<unsigned> rp_bits_;          // graph_repair_round: [the unreached members | the reached set] as bitsets
    DevBuf<int> rp_bcnt_;               // ... their set bits per block of kExactCompactWords words
    DevBuf<long long> rp_boff_;         // ... and the exclusive prefix of those (exact_compact_kernel's block offsets)
    DevBuf<int> rp_uids_, rp_cand_;     // ... U ascending; [candidates | codes]
    DevBuf<float> rp_q_;                // ... the rows of U as the scan's queries
    DevBuf<double> rp_qsn_;
    DevBuf<unsigned long long> rp_meas_; // ... distances the proposal kernel measured
    PinBuf<int> rp_host_;               // ... [U | candidates | codes | measured] on the host
    DevBuf<SearchHit> s_arena_; // range search: the launch's results, packed
    DevBuf<unsigned long long> s_roff_, s_arena_used_; // s_roff_ stands for the capacity of range_batch's per-job arrays
    DevBuf<int> s_rentry_;
    PinBuf<SearchHit> h_range_;     // RangeQuery results on the host (pinned, grown on demand, filled by ONE device-to-host copy per launch)
    bool range_host_room(size_t entries, size_t keep);
    DevBuf<int> s_rstate_, s_rtied_, s_rfin_ctr_; // RangeQuery's finishing kernels: per-job state, the tied jobs, two job counters
    DevBuf<int> s_rres_;                  // filtered RangeQuery: allowed entries per job (range_sort_kernel<true>)
    DevBuf<unsigned long long> s_rdst_;   // ... where each job's list lands in the packed copy-back (range_pack_kernel)
    DevBuf<SearchHit> s_rpack_;           // ... the packed copy-back
    DevBuf<SearchHit> s_rlists_; // range search: long per-wave result lists for the few jobs that outgrow s_spill_'s
    double range_hint_ = 48.0;      // results per query of the last range search (sizes the next arena)
    std::vector<SearchHit> abi_range_; // hnswdev_range_search's results until hnswdev_range_results
    auto host_list_of(int layer) const;  // what the range_search_* forms share: the host graph's lists of a layer ...
    bool finish_closure(int layer, int entry, float range, SearchHit *b, int m, const AllowPred &allow, int nq, int *out_counts, int *count); // ... and "finish a closure or fail the whole call"
    template <class HasCandidate> // ... and their body: the jobs, the launch, the lists collected in query order (device_backend.hip)
    bool range_search_run(int nq, int entry_point, int top, float range, RangeFilter f, HasCandidate &&has_candidate, int *out_counts, int *out_flags, int layer);
    DevBuf<int> s_lk_[5];
    bool ensure_search_scratch(long long chunk, long long slots, int k, size_t vis_bytes_per_job);
    void *pinned_stage(size_t bytes);
    bool staged_upload(float *dst, const float *src, size_t bytes);
    PinBuf<char> up_pin_[8]; // staged_upload: two pinned chunks per helper thread
    DevEvent up_ev_[8];
    bool up_busy_[8] = {false, false, false, false, false, false, false, false};
    struct HostGraphStage;
    HostGraphStage *hg_ = nullptr;
    PinBuf<char> h_stage_;
    DevEvent ev0_, ev1_, ev2_;
    struct LinkSet { // pinned staging of one in-flight link sub-batch
        PinBuf<int> h_in, h_out;
        PinBuf<unsigned long long> h_ev;
        DevEvent ev_start, ev_stop, ev_done;
        bool busy = false, timed = false;
        int ngroups = 0;
    } lset_[2];
    struct BgUpload {
        std::thread th;
        std::atomic<long long> resident{0}; // rows with id < resident have landed
        std::atomic<bool> failed{false}, active{false};
        std::string err;
        DevStream stream;
        PinBuf<char> pin[2];
        DevEvent ev[2];
    } bg_;
    StepBuffers *abi_sb_[4] = {nullptr, nullptr, nullptr, nullptr}; // context-owned step-buffer sets: 0/1 handed out by hnswdev_step_buffers, 2/3 private to dist_query_batch (so it never moves buffers a caller holds)
    DevBuf<int> d_guard_;                         // guard flag of pair_distance_kernel
    DevBuf<int> pair_dev_;                        // dist_pair_batch: [a | b | out] on the device
    DevStream stream_; // (destroyed by ~Device itself, before any holder lets go of its memory)
    bool profiling_ = false;
    hnswdev_stats stats_{};
    uint64_t counters_[kCounterBlocks][kMaxCounterSlots] = {}; // the blocks of counter_blocks.h, a row each
    uint64_t *counter_block(CounterBlock b) { return counters_[(int)b]; } // a block to count in, subscripted by its slot:: names
    bool shadows_allowed_ = true;
    int uj_len_ = 0, uj_entry_ = -1, uj_layer_ = -1; // s_jobs_ holds search_queries' jobs 0 .. uj_len_-1 for that entry point
    bool search_batch_impl(const SearchJob *jobs, int njobs, int k, int k_out, int *out_ids, float *out_d, int *out_flag, bool keep_repeat_flag,
                           bool two_heap, int u_entry, int u_layer);
};

} // namespace hnsw
