// hnsw_index.h -- host-side mirror of HNSWIndex<float[],float> for the Add / KnnQuery path
// (src/HNSWIndex/HNSWIndex.cs:20-29,55-78,107-137), with every distance evaluated by the
// gfx950 backend through the lock-step engine.
#pragma once
#include <memory>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "device_backend.h"
#include "host_structs.h"
#include "search_engine.h"

namespace hnsw {

// src/HNSWIndex/HNSWParameters.cs:13-55 plus the backend knobs.
struct Params {
    int max_edges = 16;
    double distribution_rate = 0.36067376022224085; // 1 / Math.Log(16)
    int min_nn = 5;
    int max_candidates = 100;
    int remove_max_candidates = 100;
    int collection_size = 65536;
    int random_seed = 31337;
    bool allow_removals = true;
    // backend
    int device = -1;         // -1: what hnsw_mi355x_set_device chose, or 0
    int insert_batch = 0;     // cap of a snapshot batch (which is also <= linked/16).  0 (default) = the host's hardware threads:
                              // B items searching one snapshot and linking in id order is an interleaving the reference's
                              // Parallel.For (HNSWIndex.cs:70-78) can produce iff B <= its threads, so the default stays inside
                              // the reference's outcome set on this host; larger caps (the 65 536-item snapshots of rounds 1-4)
                              // are opt-in.  1 = strictly sequential inserts; -W = the sequential graph through speculative
                              // windows of W items (insert_exact_window)
    int remove_batch = 1;     // > 1: hnsw_remove takes removals with disjoint neighbourhoods together (snapshot batches of up to this many)
    int search_slots = 16384;
    int host_threads = 0;    // 0: min(hardware threads, 16)
    int device_traversal = 1; // 1: graph-resident search kernel; 0: host lock-step traversal
    int devices = 0;          // 0: what hnsw_mi355x_set_devices chose, or 1; > 1: KnnQuery shards its queries over this many device contexts (replicas of rows + graph)
};

class HnswIndex {
public:
    static HnswIndex *create(int metric, const Params &p, std::string &err);
    ~HnswIndex();

    // hnsw_add: returns number of ids written or -1.
    int add(const float *vectors, int count, int dim, int *out_ids, std::string &err);
    // hnsw_knn_query: 0 or -1.
    int knn_query(const float *queries, int count, int dim, int k, int *out_ids, float *out_dists, std::string &err);

    // hnsw_mi355x_knn_query_at_layer, hnsw_mi355x_knn_query_filtered (layer 0): KnnQuery(query, k, filterFnc, layer) -- allow_bits ==
    // nullptr: no filter; else a bitset of nbits bits over ids, ids >= nbits not allowed.  layer outside 0 .. the entry point's top
    // layer on a non-empty index: -1.  The caller holds the index lock EXCLUSIVELY (these calls take no query lane).  0 or -1.
    // hnsw_mi355x_exact_knn_query: the flat scan (Device::exact_knn) over the live ids that allow_bits allows (nullptr: no filter).
    // Reads no graph; runs on the primary context, on the device whatever device_traversal says.
    int exact_knn_query(const float *queries, int count, int dim, int k, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists,
                        std::string &err);
    // hnsw_mi355x_exact_range_query: the same scan and candidates; per query every candidate within `range` (Device::exact_range),
    // counts[count] and the lists concatenated in query order.  -1: counts are 0 and the lists empty.
    int exact_range_query(const float *queries, int count, int dim, float range, const uint32_t *allow_bits, long long nbits, int *counts,
                          std::vector<int> &ids, std::vector<float> &dists, std::string &err);
    // hnsw_mi355x_exact_knn_query_grouped: exact_knn_query with a candidate group per query (Device::exact_knn_grouped):
    // query i's candidates are the live ids j < n_row_group with row_group[j] == query_group[i].
    int exact_knn_query_grouped(const float *queries, int count, int dim, int k, const int *row_group, long long n_row_group, const int *query_group,
                                int n_groups, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_exact_knn_query_collapsed: exact_knn_query's candidates, at most per_group results per label
    // row_group[id] (Device::exact_knn_collapsed).  row_group must cover the index's length.
    int exact_knn_query_collapsed(const float *queries, int count, int dim, int k, const int *row_group, long long n_row_group, int per_group,
                                  const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_knn_query_collapsed: per query the first k survivors of the collapse walk over the row that
    // knn_query_general(queries, beam, layer, allow) returns -- the same traversal, through answer_resident; on the device the rows are
    // collapsed before the copy-out (Device::search_collapsed), a host answer is walked by collapse_host_row.
    int knn_query_collapsed(const float *queries, int count, int dim, int k, int beam, const int *row_group, long long n_row_group, int per_group, int layer,
                            const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_exact_knn_query_tagged: exact_knn_query with a tag mask per query (Device::exact_knn_tagged): query i's
    // candidates are the live ids j < n_row_tags whose word row_tags[j] matches query_tags[i] under `match` (0 any, 1 all).  0 or -1.
    int exact_knn_query_tagged(const float *queries, int count, int dim, int k, const uint32_t *row_tags, long long n_row_tags, const uint32_t *query_tags,
                               int match, int *out_ids, float *out_dists, std::string &err);
    // ---- query by stored id.  Every id must be live: otherwise -1 with a message that names the first that is not,
    // before anything is launched.
    // hnsw_mi355x_get_vectors: out[i] = the stored row ids[i] as dim floats (Device::gather_rows: hnswdev_download_rows' values).
    int get_vectors(const int *ids, int n, float *out, std::string &err);
    // hnsw_mi355x_knn_query_by_id: row i is byte for byte what knn_query_general returns for the vector get_vectors gives for ids[i]
    // with every id but ids[i] as the allow-set.  The queries are gathered on the device (Device::set_queries_by_id, every context
    // its shard) and traversed by graph_search_self_kernel; hand-backs, and the whole call when the traversal does not run on the
    // device, go the lock-step way with the id as the job's `exclude`.  Exclusive lock.  0 or -1.
    int knn_query_by_id(const int *ids, int count, int k, int layer, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_exact_knn_query_by_id: row i is exact_knn_query's for that vector with allow_bits (nullptr: every live id) minus
    // ids[i] as the candidates (Device::exact_knn_by_id).  Runs on the primary context; the resident set stays what it was.
    int exact_knn_query_by_id(const int *ids, int count, int k, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_exact_range_query_by_id: list i is exact_range_query's for the stored row of ids[i] with allow_bits
    // (nullptr: every live id) minus ids[i] (Device::exact_range_by_id); counts / ids / dists as exact_range_query fills them.
    int exact_range_query_by_id(const int *ids, int count, float range, const uint32_t *allow_bits, long long nbits, int *counts, std::vector<int> &out_ids,
                                std::vector<float> &out_dists, std::string &err);
    // hnsw_mi355x_duplicate_groups: the single-linkage groups of the live, allowed ids (Device::exact_range_groups);
    // out_labels[0, length), cap >= length.
    int duplicate_groups(float range, const uint32_t *allow_bits, long long nbits, int *out_labels, long long cap, uint64_t *out_info, std::string &err);
    // hnsw_mi355x_density_clusters: DBSCAN over duplicate_groups' members and within pairs (Device::exact_range_density);
    // out_counts[0, length) and, where given, out_labels[0, length), cap >= length; out_labels == nullptr: the neighbour counts alone.
    int density_clusters(float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels, int *out_counts, long long cap,
                         uint64_t *out_info, std::string &err);
    // hnsw_mi355x_graph_duplicate_groups / hnsw_mi355x_near_edges: duplicate_groups' members, joined along the
    // within-edges of layer 0 of the graph mirror (Device::graph_edge_groups / graph_near_edges), which is brought up to date first
    // (sync_graph) as for get_info.  On the primary context; liveness and allow_bits go down as one bitset.  out_labels[0, length),
    // cap >= length; out_info has five entries.  near_edges keeps the edges in the context (*out_count of them) until
    // near_edges_results copies them out (cap >= that count) or the next near_edges replaces them.
    int graph_duplicate_groups(float range, const uint32_t *allow_bits, long long nbits, int *out_labels, long long cap, uint64_t *out_info, std::string &err);
    int near_edges(float range, const uint32_t *allow_bits, long long nbits, long long *out_count, std::string &err);
    int near_edges_results(int *out_src, int *out_dst, float *out_dists, long long cap, std::string &err);
    // hnsw_mi355x_exact_range_query_grouped: exact_range_query with exact_knn_query_grouped's group per query
    // (Device::exact_range_grouped); the labels of vacant slots are taken out as for that call
    int exact_range_query_grouped(const float *queries, int count, int dim, float range, const int *row_group, long long n_row_group, const int *query_group,
                                  int n_groups, int *counts, std::vector<int> &ids, std::vector<float> &dists, std::string &err);
    // hnsw_mi355x_exact_range_query_tagged: exact_range_query with exact_knn_query_tagged's tag mask per query
    // (Device::exact_range_tagged); the words of vacant slots are taken out as for that call
    int exact_range_query_tagged(const float *queries, int count, int dim, float range, const uint32_t *row_tags, long long n_row_tags,
                                 const uint32_t *query_tags, int match, int *counts, std::vector<int> &ids, std::vector<float> &dists, std::string &err);
    // hnsw_mi355x_get_info / hnsw_mi355x_connected_component_counts: HNSWIndex.GetInfo() / GetConnectedComponentCounts() for the
    // layers 0 .. top, computed by the primary context from the graph mirror (Device::graph_info / graph_components)
    // whatever device_traversal says.  The mirror is brought up to date first (sync_graph); when it is current the adjacency lists
    // are neither uploaded nor fetched, and host_lists_stale_ stays what it was.  Both return top + 1 and write min(cap, top + 1)
    // entries, or -1; an index with no live item: get_info -1 (the reference's IndexOutOfRangeException), the counts 0.
    int get_info(hnsw_mi355x_layer_info *out, int cap, std::string &err);
    int connected_component_counts(int *out, int cap, std::string &err);
    // hnsw_mi355x_reachability / _unreachable_ids / _hop_counts: the chain of out-edge reachability from the entry
    // point (Device::graph_reach) down to layer 0, or down to `layer`.  Locking, sync_graph, the live set and "always on the device,
    // on the primary context" are connected_component_counts'.  reachability: top + 1 with min(cap, top + 1) entries written.
    // unreachable_ids: the live members of `layer` outside F_layer, ascending, in `ids` (only the reached bitset crosses back; the
    // member test is the host's).  hop_counts: length, with min(cap, length) entries written.  An empty index: 0.  -1 on error.
    int reachability(hnsw_mi355x_layer_reach *out, int cap, std::string &err);
    int unreachable_ids(int layer, std::vector<int> &ids, std::string &err);
    int hop_counts(int layer, int *out, int cap, std::string &err);
    // hnsw_mi355x_repair_reachability: links the members that reachability() reports as lost into the lists of their
    // nearest reached members, layer by layer from the top, at most max_rounds rounds per layer.  Locking, sync_graph, the live set
    // and "always on the device, on the primary context" are reachability's; the host lists are fetched first where the mirror is
    // ahead of them.  The only call besides Add and Remove that edits lists: graph_ and the mirror are changed together, replicas
    // clone again, the in-edge sets are rebuilt by the next Remove.  top + 1 with min(cap, top + 1) entries written; an empty index: 0;
    // -1 on error, and once a list has been patched a device failure fails the index as a failed Remove does.
    int repair_reachability(int cands, int max_rounds, hnsw_mi355x_layer_repair *out, int cap, std::string &err);
    int knn_query_general(const float *queries, int count, int dim, int k, int layer, const uint32_t *allow_bits, long long nbits, int *out_ids,
                          float *out_dists, std::string &err);
    // hnsw_mi355x_knn_query_grouped: KnnQuery on `layer` with a group filter per query -- query i is answered from the
    // ids j < n_row_group with row_group[j] == query_group[i], byte for byte what knn_query_general returns for it with that group's
    // ids as the allow-set.  One device traversal for every group (Device::search_grouped); jobs handed back, and the whole call when
    // the traversal does not run on the device, go the lock-step way once per group.  Exclusive lock.  0 or -1.
    int knn_query_grouped(const float *queries, int count, int dim, int k, int layer, const int *row_group, long long n_row_group, const int *query_group,
                          int n_groups, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_knn_query_tagged: KnnQuery on `layer` with a tag mask per query -- query i is answered from the ids
    // j < n_row_tags whose word row_tags[j] matches query_tags[i] under `match` (0 any, 1 all), byte for byte what knn_query_general
    // returns for it with those ids as the allow-set.  One device traversal for every mask (Device::search_tagged); jobs handed back,
    // and the whole call when the traversal does not run on the device, go the lock-step way once per distinct mask.  Exclusive
    // lock.  0 or -1.
    int knn_query_tagged(const float *queries, int count, int dim, int k, int layer, const uint32_t *row_tags, long long n_row_tags, const uint32_t *query_tags,
                         int match, int *out_ids, float *out_dists, std::string &err);
    // hnsw_mi355x_multilayer_knn_query: the number of layer slots (min(top, max_layer) + 1; 0 for an empty index, k < 1 or
    // max_layer == -1), or -1.  out_*: [count][layers_cap][k - 1].  Exclusive lock.
    int multilayer_knn_query(const float *queries, int count, int dim, int k, int max_layer, int min_layer, int layers_cap, int *out_ids,
                             float *out_dists, std::string &err);
    int top_layer() const { return graph_.entry < 0 ? -1 : graph_.top_layer(); }

    // Measurement aid: upload a query set once (resident in HBM), then run KnnQuery on it any
    // number of times without host->device traffic for the inputs.
    int set_resident_queries(const float *queries, int count, int dim, std::string &err, bool streamed = false);
    int knn_query_resident(int k, int *out_ids, float *out_dists, std::string &err);

    // hnsw_range_query (HNSWIndex.RangeQuery, src/HNSWIndex/HNSWIndex.cs:144-168): per query the
    // in-range results ordered by distance.  Host lock-step traversal.
    // allow: RangeQuery(query, range, filterFnc) as a bitset over ids (none: no filter).  Where the reference pops an empty
    // top heap (range < 0, range_replay.h) the call fails with kHeapEmptyError.
    // layer: RangeQuery's `layer` (outside 0 .. the entry point's top layer on a non-empty index: -1).
    int range_query(const float *queries, int count, int dim, float range, std::vector<std::vector<NodeDist>> &out, std::string &err,
                    AllowBits allow = AllowBits{}, int layer = 0);

    // hnsw_mi355x_range_query_grouped: RangeQuery on `layer` with a group filter per query -- query i's list is byte
    // for byte what range_query returns for it with the ids j < n_row_group, row_group[j] == query_group[i] as the allow-set; the
    // empty-heap rule fails the whole call as there.  One device traversal for every group (Device::range_batch with a RangeFilter of labels);
    // hand-backs, and the whole call when the traversal does not run on the device, go the lock-step way with the label predicate.
    // A query whose group holds no graph id is answered with an empty list without a traversal when range >= 0.  Exclusive lock.
    int range_query_grouped(const float *queries, int count, int dim, float range, int layer, const int *row_group, long long n_row_group,
                            const int *query_group, int n_groups, std::vector<std::vector<NodeDist>> &out, std::string &err);
    // hnsw_mi355x_range_query_tagged: RangeQuery on `layer` with a tag mask per query -- query i's list is byte for
    // byte what range_query returns for it with the ids j < n_row_tags whose word row_tags[j] matches query_tags[i] under `match`
    // (0 any, 1 all) as the allow-set; the empty-heap rule fails the whole call as there.  One device traversal for every mask
    // (Device::range_batch with a RangeFilter of tags); hand-backs, and the whole call when the traversal does not run on the device, go the
    // lock-step way with the tag predicate.  A query whose mask matches no graph id (counted on the device) is answered with an
    // empty list without a traversal when range >= 0.  Primary context only.  Exclusive lock.
    int range_query_tagged(const float *queries, int count, int dim, float range, int layer, const uint32_t *row_tags, long long n_row_tags,
                           const uint32_t *query_tags, int match, std::vector<std::vector<NodeDist>> &out, std::string &err);

    // hnsw_remove (HNSWIndex.Remove, src/HNSWIndex/HNSWIndex.cs:83-102), ids in order.
    int remove(const int *ids, int count, std::string &err);

    // HNSWIndex.Serialize / Deserialize (src/HNSWIndex/HNSWIndex.cs:210-229): the reference's
    // protobuf-net snapshot (csrc/snapshot_io.h).  `backend` supplies the device knobs only;
    // the HNSW parameters come from the file.
    int serialize(const char *path, std::string &err);
    static HnswIndex *deserialize(int metric, const Params &backend, const char *path, std::string &err);

    // hnsw_mi355x_import_nodes / _edges: a graph built elsewhere into an empty index (see include/hnsw_mi355x.h)
    int import_nodes(const float *rows, int n, int dim, const int *levels, int entry_point, std::string &err);
    int import_edges(int layer, const int *counts, const int *edges, int stride, std::string &err);

    int count() const { return graph_.count; }
    int resident_count() const { return resident_queries_; }
    int device_count() const { return p_.devices; }
    Device *device_at(int g) { return g == 0 ? dev_.get() : (g - 1 < (int)replicas_.size() ? replicas_[(size_t)g - 1].get() : nullptr); }
    int dim() const { return dim_; }
    // The host copy of the graph.  After a device-linked Add the neighbour lists live in the HBM
    // mirror only and are fetched back here on demand.
    const Graph &graph() { std::string e; (void)refresh_host_lists(e); return graph_; }
    Device *device() { return dev_.get(); }
    uint64_t graph_hash();
    void set_insert_batch(int v) { p_.insert_batch = v; }
    // Threads this process may run on (std::thread::hardware_concurrency(): the affinity mask on Linux) = what bounds the items a
    // Parallel.For on this host holds in flight.  (.NET also clamps Environment.ProcessorCount to a cgroup CPU quota; a
    // container host that wants that bound passes it to hnsw_mi355x_set_insert_batch itself.)
    static int host_parallelism();
    int insert_batch_cap() const { return p_.insert_batch == 0 ? host_parallelism() : p_.insert_batch; }
    // hnsw_mi355x_<block>: a counter block of counter_blocks.h, out[kCounterSlots of it] -- the primary context's values, plus every
    // replica's where the table says `summed`; all zero before a context exists
    void counters(CounterBlock b, uint64_t *out) const;
    void exact_window_stats(uint64_t out[4]) const { out[0] = xw_rounds_; out[1] = xw_searches_; out[2] = xw_alone_; out[3] = xw_linked_; }
    void row_prefilter_stats(uint64_t out[4]); // the primary context's (its views add to it) plus every replica's
    void row_prefilter_form_stats(uint64_t out[2]); // summed the same way
    bool row_prefilter_peek(long long first_id, int count, uint64_t out[2], float *rows, std::string &err); // the primary context's shadow, read only
    void row_prefilter8_stats(uint64_t out[6]); // the 8-bit shadow's counters, summed the same way
    bool row_prefilter8_peek(long long first_id, int count, uint64_t out[4], unsigned char *codes, std::string &err); // the primary context's 8-bit shadow, read only
    void set_profiling(bool on)
    {
        profiling_ = on;
        if (dev_) dev_->set_profiling(on);
        for (auto &r : replicas_) r->set_profiling(on);
        for (auto &l : lanes_) if (l) l->set_profiling(on);
    }

    // Calls on one handle.  The reference promises that operations of one type may overlap on an index
    // (/root/reference/README.md:64-65; BatchKnnQuery / Add(List) are Parallel.For, HNSWIndex.cs:70-78,129-137).  Here:
    //   * hnsw_knn_query calls DO overlap: each takes the index lock shared and a query lane of its own -- a Device view
    //     (stream, resident query set, per-wave scratch) that borrows the rows and the graph mirror -- so two host
    //     threads' launches run side by side on the GPU, the head of one filling the tail of the other
    //     (knn_query_concurrent; whatever it cannot serve -- sharded indices, host traversal, a graph mirror that is
    //     not current, hand-backs -- goes through the exclusive path);
    //   * everything else (Add, Remove, RangeQuery, ...) takes the lock exclusively: those calls already fan out over
    //     the whole GPU and own the index's staging buffers.
    // Calls on different handles run concurrently.
    std::shared_mutex &mutex() { return mu_; }
    // 1: answered (rc = the call's return value); 0: not eligible, take the exclusive path.  Call with the lock held SHARED.
    int knn_query_concurrent(const float *queries, int count, int dim, int k, int *out_ids, float *out_dists, int &rc, std::string &err);
    void collect_stats(hnswdev_stats *out);
    void reset_all_stats();

private:
    std::shared_mutex mu_;
    static constexpr int kLanes = 2;
    std::unique_ptr<Device> lanes_[kLanes];
    bool lane_busy_[kLanes] = {false, false};
    std::mutex lane_mu_;
    std::condition_variable lane_cv_;
    HnswIndex() = default;
    // A device failure in the middle of an Add leaves appended nodes without rows / links: the
    // index then refuses every further call with the original message.
    std::string failed_msg_;
    bool failed(std::string &err) const { if (failed_msg_.empty()) return false; err = failed_msg_; return true; }
    int fail(const std::string &why, std::string &err)
    {
        failed_msg_ = "HNSWIndex MI355X backend: the index is unusable after a failed Add / Remove (" + why + ")";
        err = failed_msg_;
        return -1;
    }
    bool ensure_dim(int dim, std::string &err);
    bool ensure_capacity(long long need, std::string &err);
    bool insert_batch(const std::vector<int> &bid, std::string &err);
    long long exact_candidates(const uint32_t *&allow_bits, long long &nbits, std::vector<uint32_t> &live) const;
    bool live_labels(const int *&row_group, long long &n_row_group, std::vector<int> &live) const;
    bool ids_live(const char *who, const int *ids, int n, std::string &err) const;
    bool live_tags(const uint32_t *&row_tags, long long &n_row_tags, std::vector<uint32_t> &live) const;
    int reach_chain(const char *who, int min_layer, hnsw_mi355x_layer_reach *out, int cap, uint32_t *bits, int *hops, std::string &err);
    bool insert_exact_window(const std::vector<int> &fresh, int &p, int W, bool background, std::string &err);
    // Selected neighbour ids per (batch item, layer).  Device results are read in place from the
    // context's pinned buffers (layer 0: slot = item; layer L >= 1: slot upper_base[item] + L - 1);
    // items processed on the host (lock-step mode, hand-backs) carry their own lists.
    struct Selection {
        int n = 0, n_upper = 0;
        Device::InsertResults dev{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
        std::vector<int> upper_base;
        std::vector<char> has_own;
        std::vector<std::vector<std::vector<int>>> own;
        inline void get(int i, int layer, const int *&ids, int &cnt) const
        {
            if (has_own[(size_t)i]) { const std::vector<int> &v = own[(size_t)i][(size_t)layer]; ids = v.data(); cnt = (int)v.size(); return; }
            if (layer == 0) { ids = dev.sel0 + (size_t)i * dev.sel_stride; cnt = dev.cnt0[i]; }
            else { const size_t s = (size_t)(upper_base[(size_t)i] + layer - 1); ids = dev.selU + s * dev.sel_stride; cnt = dev.cntU[s]; }
        }
    };
    bool search_half_lockstep(const std::vector<int> &bid, const std::vector<int> &items, Selection &sel, std::string &err);
    bool search_half_device(const std::vector<int> &bid, Selection &sel, std::string &err);
    bool link_half_lockstep(const std::vector<int> &bid, const Selection &sel, std::string &err);
    bool link_half_device(const std::vector<int> &bid, const Selection &sel, std::string &err);
    bool link_prefix_begin(const std::vector<int> &bid, const Selection &sel, int set, std::string &err);
    bool sync_graph(std::string &err);
    // ---- query sharding over several devices inside one process (hnsw_mi355x_set_devices) ----
    // BatchKnnQuery is a Parallel.For over independent read-only searches (HNSWIndex.cs:129-137): with n contexts,
    // context g answers queries [g nq / n, (g + 1) nq / n) on its own replica of the rows and the graph mirror and
    // writes its slice of the caller's arrays.  The primary (dev_) builds; replicas are brought up to date device to
    // device (Device::clone_from) when the graph has changed since they were last used.
    std::vector<std::unique_ptr<Device>> replicas_; // contexts 1 .. devices - 1
    std::vector<uint64_t> replica_epoch_;
    uint64_t graph_epoch_ = 1;                       // bumped by everything that changes rows or lists
    std::vector<long long> shard_lo_;                // resident query set: shard bounds (devices + 1 entries)
    bool sharded_resident_ = false;
    Device *context(int g) { return g == 0 ? dev_.get() : replicas_[(size_t)g - 1].get(); }
    bool ensure_replicas(bool clone, std::string &err);
    bool gather_queries_to_primary(int count, std::string &err);
    bool refresh_host_lists(std::string &err);
    // every KnnQuery form over the resident set: on the device, one launch per context, or on the host, hand-backs included (hnsw_index.cpp)
    template <class OnDevice, class OnHost>
    int answer_resident(int count, int ef, OnDevice on_device, OnHost on_host, const char *fallback, std::string &err);
    // what knn_query_grouped / knn_query_tagged share: the prologue, the lock-step way class by class, the answer_resident call
    template <class ArgsOk>
    int predicate_query_begin(const char *who, int count, int k, int layer, int *out_ids, float *out_dists, std::string &err, ArgsOk args_ok);
    template <class ClassOf, class Matches>
    int lockstep_by_class(const int *which, int n, int k, int layer, long long n_lab, size_t n_classes, ClassOf class_of, Matches matches, int *out_ids,
                          float *out_dists, std::string &err);
    template <class Search, class ClassOf, class Matches>
    int answer_by_class(int count, int k, int layer, long long n_lab, size_t n_classes, ClassOf class_of, Matches matches, Search search, const char *fallback,
                        int *out_ids, float *out_dists, std::string &err);
    // exclude: nullptr, or per resident query the id that is no result of it (knn_query_by_id: the query's own)
    int knn_query_lockstep(const int *which, int count, int k, int *out_ids, float *out_dists, std::string &err, AllowBits allow = AllowBits{},
                           int layer = 0, const int *exclude = nullptr);
    // RangeQuery for the resident queries listed in `which` (nullptr: all `count` of them) under the call's filter f (host_structs.h),
    // the lock-step way and on the device; and what range_query_grouped / range_query_tagged share (hnsw_index.cpp)
    int range_query_lockstep(const int *which, int count, float range, std::vector<std::vector<NodeDist>> &out, std::string &err, const RangeFilter &f, int layer);
    int range_query_device(const int *which, int count, float range, std::vector<std::vector<NodeDist>> &out, std::string &err, const RangeFilter &f, int layer);
    template <class ClassOf, class ClassesWithId>
    int range_by_class(const char *who, const float *queries, int count, int dim, float range, int layer, RangeFilter f, ClassOf class_of,
                       ClassesWithId classes_with_id, std::vector<std::vector<NodeDist>> &out, std::string &err);
    int multilayer_lockstep(const int *which, int count, int k, int first, int min_layer, int *out_ids, float *out_dists, std::string &err);
    bool layer_ok(int layer, std::string &err) const;
    int remove_batched(const int *ids, int count, std::string &err);

    int metric_ = 0;
    int dim_ = 0; // fixed by the first add (the reference takes it from the arrays)
    Params p_;
    Graph graph_;
    DotnetRandom rng_;
    std::unique_ptr<Device> dev_;
    std::unique_ptr<LockStepEngine> engine_;
    LockStepEngine *engine();
    int engine_stride_ = 0;
    long long capacity_ = 0; // GraphData.Capacity (doubling, GraphData.cs:98-111)
    int skipped_ = 0;
    int device_ordinal_ = 0;
    int threads_ = 1;
    bool profiling_ = false;
    int resident_queries_ = 0;
    bool graph_dirty_ = true;       // HBM mirror needs a full re-upload
    // in-edge sets for Remove (content only, see remove()): built by transposing the out-lists on the first removal
    // after anything else changed the graph, kept current by the removals themselves
    std::vector<std::vector<int>> in0_;
    std::unordered_map<uint64_t, std::vector<int>> inU_;
    bool in_valid_ = false;
    // exact-window Add: per adjacency list the sequence number of the last insert that wrote it (0 = never);
    // seq_ = inserts linked so far.  Only compared within one Add call; monotone across calls.
    std::vector<uint32_t> mod0_;
    std::unordered_map<uint64_t, uint32_t> modU_;
    uint32_t seq_ = 0;
    uint64_t xw_rounds_ = 0, xw_searches_ = 0, xw_alone_ = 0, xw_linked_ = 0, xw_pairs_ = 0;
    double xw_prefix_ema_ = 16.0;                          // items linked per round, recent average (sizes the next window)
    struct XwChange { int t, e; bool known; };             // first change of a layer-0 list in the current round: window item, selection entry
    std::unordered_map<int, XwChange> xw_first_;
    std::unordered_map<int, int> xw_second_;               // ... and the item that touches it next
    std::vector<int> pa_, pb_;                             // id<->id distances asked for (reader row, gained / lost row)
    std::vector<uint32_t> pfar_;
    std::vector<std::pair<int, int>> powner_;              // (reader item, writer item)
    std::vector<float> pd_; // exact-window statistics (hnsw_mi355x_exact_window_stats)
    bool host_lists_stale_ = false; // the HBM mirror holds newer neighbour lists than graph_ (device-linked Add)
    long long dev_pool_len_ = 0;    // pool ints already mirrored
    std::vector<int> grp_of_node0_; // link half: group index per layer-0 neighbour (-1 = none)
    std::vector<int> lk_rows_, lk_node_, lk_layer_, lk_cnt_, lk_off_, lk_items_, lk_fill_, lk_out_; // link half: per-batch work arrays
    std::vector<std::pair<int, int>> lk_seq_;
};

} // namespace hnsw
