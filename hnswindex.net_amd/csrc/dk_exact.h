// dk_exact.h -- the flat scan behind hnswdev_exact_knn: every (query, row) pair of an id list measured with the
// metric's own arithmetic (dk_metric.h: eight lane partials in element order, the collapse tree, the scalar tail, the epilogue --
// bit for bit group_metric's value) and the k smallest (distance, id) kept per query.  No graph is read.
//   exact_compact_kernel   bitset (allow AND live, masked on the host) -> ascending id list
//   exact_scan_kernel<M>   a tile of queries x a chunk of the id list per block; per (query, chunk) a sorted list of k keys in LDS
//   exact_merge_kernel     one wave per query: the chunks' lists -> the final k, ids and distances in the output layout
// and, behind the same measured pairs, hnswdev_exact_range: every key within a radius, of any number.  The scan
// kernel takes its sink as a type -- ExactTopK, the lists above, or ExactRange:
//   exact_scan_kernel<M, ExactRange>  keys with d <= range go from the pending lists to the query's segment of an arena; the count per query is exact
//   exact_range_sort_kernel           one block per query: a segment of up to kExactRangeSortMax keys ordered in LDS -> ids and distances
// and hnswdev_exact_knn_grouped: a candidate group per query.  row_group[id] names the group of an id; the groups' id
// lists are built on the device as one CSR and the scan's blocks take their (queries, list segment) from a table of work items:
//   exact_group_kernel<false> / exact_group_offsets_kernel / exact_group_kernel<true>   row_group -> counts, offsets, the members of each group in its segment (unordered)
//   exact_gather_queries_kernel                 the resident queries in the call's sorted order (queries == NULL)
//   exact_scan_kernel<M, ExactTopKGrouped>      a block = one work item: a tile of one group's queries x a chunk of that group's list
//   exact_merge_grouped_kernel                  one wave per query: its chunks' lists -> the final k at the query's original row
// and hnswdev_exact_range_grouped: the range sink behind the same work items.
//   exact_scan_kernel<M, ExactRangeGrouped>     a block = one work item; the keys within the range go to the segment that a table names for the
//                                               query -- its place in the caller's order -- so exact_range_sort_kernel runs as it is
// and hnswdev_exact_knn_by_id: the queries are stored rows, and a query's own row is no candidate.
//   exact_scan_kernel<M, ExactTopKSelf>         ExactTopK, but the pair (query q, row id self[q]) produces no key and is not counted
// and hnswdev_exact_knn_collapsed: at most per_group results per label row_group[id] -- the result is shaped, not the candidates.
//   exact_scan_kernel<M, ExactTopKCollapse>     ExactTopK's lists with a label beside every key; exact_list_insert_collapsed drops, evicts or inserts
//   exact_merge_collapsed_kernel                one wave per query: the chunks' collapsed lists -> the collapsed final k
// and hnswdev_exact_range_by_id / hnswdev_exact_range_groups: near-duplicates of stored rows.
//   exact_scan_kernel<M, ExactRangeSelf>        ExactRange, with ExactTopKSelf's rule: the query's own row offers no key and is not counted
//   exact_scan_kernel<M, ExactRangeUnion>       no keys at all: a pair (a < b) within the range joins a and b in a union-find (dk_union_find.h)
//   exact_union_init_kernel / exact_union_labels_kernel   every id its own root before the scans; labels = roots = smallest ids after them
// and hnswdev_exact_range_density: DBSCAN over ExactRangeUnion's triangle, in two phases.
//   exact_scan_kernel<M, ExactRangeDensity>      a pair within the range adds 1 to the counts of both ids and goes to a pair arena as a record
//   density_pairs_kernel                         per record: both ends core -> uf_union; one end core -> a 64-bit min on the other's attach key
//   exact_scan_kernel<M, ExactRangeDensityJoin>  the same per pair from a second scan, where the arena did not hold every record
//   density_init_kernel / density_labels_kernel  counts 0 for the members before the scans; core: its root, border: its core's root, else -1
// The kernels are compiled in the exact_<metric> units (exact_unit.hip, HNSW_EXACT_UNIT) and reached through the launchers declared here, so
// that device_backend.hip holds none of their code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_backend.h" // kExactMaxK, kExactMaxGroups: the limits the host checks as well

namespace hnsw {

constexpr int kExactThreads = 256;   // 4 waves = 32 groups of 8 lanes
constexpr int kExactRQ = 4;          // queries of a group's register tile (= waves of a block: wave w merges query w of the tile)
constexpr int kExactRR = 4;          // rows of a group's register tile
constexpr int kExactIterRows = (kExactThreads / 8) * kExactRR; // rows a block measures per step: 128
constexpr int kExactMaxQTile = 32;
constexpr int kExactCompactWords = 256; // bitset words per block of exact_compact_kernel (one per thread)
constexpr int kExactRangeSortMax = 4096; // keys exact_range_sort_kernel orders in LDS (32 KB); longer lists are ordered on the host
constexpr int kExactMaxChunks = 4096;    // chunks per query (the merge walks them)

struct ExactScanArgs {
    const float *rows;      // stored rows (f32 rows, int8 records, f16 records)
    const double *row_sn;   // cosine: sqrt((double)|row|^2)
    const float *queries;   // this round's resident queries (f32 in element order; int8: records)
    const double *q_sn;     // cosine, this round's
    int dim;                // what the kernels get as `dim`: elements, or the int8 record's words
    const int *ids;         // the ascending id list, nullptr: the identity (row i is id i)
    long long m;            // entries of the list
    long long chunk;        // entries per chunk (blockIdx.y)
    int nq;                 // queries of this round
    int qtile;              // queries per block (blockIdx.x)
    int piece;              // query words staged in LDS at a time: dim, or a multiple of 16 below it
    int k;
    unsigned long long *lists; // out: [nq][n_chunks][k] keys, ascending, ~0 where a list has no more
    int n_chunks;
    unsigned long long *evals; // out: (query, row) pairs measured, added up over the blocks
};

// The sinks of exact_scan_kernel.  ExactTopK: the k smallest keys per (query, chunk), in ExactScanArgs::lists.  ExactRange: every
// key whose distance is <= range (the IEEE compare: a NaN distance or a NaN range admits nothing).  Query q of the round owns
// arena[seg_off[q], seg_off[q + 1]); counts[q] (zeroed before the launch) ends as the number of keys within range, whether they
// fitted the segment or not -- keys past the segment's end are dropped, in no particular order.  (ExactScanArgs::k is 0 and lists
// unused for this sink.)
struct ExactTopK {
    static constexpr bool kRange = false;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = false;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
};
// ExactTopKSelf: ExactTopK where query q of the round is the stored row of id self[q] and that id is no candidate of it: the pair
// produces no key and is not counted in ExactScanArgs::evals.  A duplicate of the row under another id is a candidate like any.
struct ExactTopKSelf {
    static constexpr bool kRange = false;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = true;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
    const int *self;               // [nq of the round]
};
// ExactTopKCollapse: the lists hold the COLLAPSED k smallest keys -- the first k keys of the ascending order that
// have fewer than per_group keys of their own label row_group[id] in front of them.  A list of labels stands beside every list of
// keys in LDS (4 more bytes per entry: exact_scan_lds' entry_bytes is 12).  Labels are compared for equality, nothing else.
// info[0]: keys below their list's k-th that the cap dropped; info[1]: entries a key of their label evicted -- added up over
// the scan's and the merge's waves (what they are depends on the order the keys arrive in; the lists do not).
struct ExactTopKCollapse {
    static constexpr bool kRange = false;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = false;
    static constexpr bool kCollapse = true;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
    const int *row_group;          // [every id of the list]
    int per_group;                 // 1 <= per_group <= k
    unsigned long long *info;      // [2]
};
struct ExactRange {
    static constexpr bool kRange = true;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = false;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
    float range;
    unsigned *counts;              // [nq]
    const long long *seg_off;      // [nq + 1]
    unsigned long long *arena;
};
// ExactRangeSelf: ExactRange where query q of the round is the stored row of id self[q] and that id is no candidate
// of it -- ExactTopKSelf's rule in the range branch: the pair offers no key and is not counted in ExactScanArgs::evals.  A repeated
// pass over a piece of a round brings the piece's own self: self[0] belongs to the first query the launch scans.
struct ExactRangeSelf {
    static constexpr bool kRange = true;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = true;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
    float range;
    unsigned *counts;              // [nq]
    const long long *seg_off;      // [nq + 1]
    unsigned long long *arena;
    const int *self;               // [nq of the launch]
};
// ExactRangeUnion: no key is kept.  The queries of a launch are a contiguous, ascending piece of the id list itself
// -- query q is the stored row of id self[q] -- and a pair (self, rid) is measured where rid > self: counted in ExactScanArgs::evals,
// and where its distance is <= range counted in *pairs and joined in parent[] (uf_union, from the lane that holds the distance).
// A pair with rid <= self is skipped without being counted.  No pending list, no arena: the sink touches nothing of LDS behind the
// staged queries.  A block whose chunk ends at or below its tile's first query id has nothing to measure and leaves before its first
// barrier (the test is the same for the whole block).  parent[v] == v for every id of the list before the first launch
// (exact_union_init_launch); labels[v] = uf_find(parent, v) after the last (exact_union_labels_launch).
struct ExactRangeUnion {
    static constexpr bool kRange = true;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = true;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = true;
    static constexpr bool kDensity = false;
    float range;
    int *parent;                   // [every id of the list]
    const int *self;               // [nq of the launch]: ascending
    unsigned long long *pairs;     // out: measured pairs within the range, added up over the blocks
};
// ExactRangeDensity, phase A of the density clusters: ExactRangeUnion's triangle -- the same queries, the same
// rid > self rule, the same early leave, the same count in ExactScanArgs::evals -- but a pair within the range joins nothing yet.
// Whether it joins depends on whether its two ends are CORE, and that is a matter of counts[] that are complete only when the whole
// scan is: one pass cannot do it.  So a within pair (a = self, b = rid, distance d)
//   * adds 1 to counts[a] and to counts[b] (0 for every id of the list before the first launch: density_init_launch).  The self side
//     is added up in LDS over the block (an int per query of the tile behind the layout of exact_scan_lds: exact_density_lds) and
//     leaves with one global atomic per query and block; the row side is added up in registers over all the tile's queries and
//     leaves with one global atomic per row and step of kExactIterRows rows;
//   * is appended to arena[] as the record {a, b, bits of d, 0}.  A wave takes the places of all its within pairs of a step with ONE
//     atomic on *n_pairs: a ballot says whether the wave has any, the popcounts of the eight group leaders' pair masks are read
//     lane by lane into the wave's total and into every leader's offset; a record whose place is at or past arena_cap is dropped
//     while the counter goes on counting -- *n_pairs ends as the number of within pairs whatever the capacity, and the counts are
//     complete either way.  arena_cap == 0: counts only.
struct alignas(16) ExactDensityPair { int a, b; unsigned d_bits, zero; }; // 16 bytes: one vector store
struct ExactRangeDensity {
    static constexpr bool kRange = true;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = true;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = true;
    static constexpr bool kJoin = false;
    float range;
    const int *self;               // [nq of the launch]: ascending
    int *counts;                   // [every id of the list]
    ExactDensityPair *arena;       // [arena_cap]
    unsigned long long arena_cap;
    unsigned long long *n_pairs;   // out: within pairs, kept or dropped
};
// ExactRangeDensityJoin, phase B where the arena did not hold every record: the triangle once more, counts[] now
// complete and read-only, every within pair handed to density_join straight from its distance (the bits are phase A's: the same
// kernel body measures).  No LDS behind the staged queries, no arena.
struct ExactRangeDensityJoin {
    static constexpr bool kRange = true;
    static constexpr bool kGrouped = false;
    static constexpr bool kSelf = true;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = true;
    static constexpr bool kJoin = true;
    float range;
    const int *self;               // [nq of the launch]: ascending
    const int *counts;             // [every id of the list]: phase A's, complete
    int min_samples;               // v is core when counts[v] + 1 >= min_samples
    int *parent;                   // [every id of the list]: exact_union_init_launch
    unsigned long long *attach;    // [every id of the list]: kExactEmpty before phase B
};
struct ExactRangeSortArgs {
    const unsigned long long *arena;
    const long long *seg_off;      // [nq + 1]: as the scan's
    const unsigned *counts;        // [nq]
    const long long *out_off;      // [nq]: where query q's list goes in out_ids / out_d; only read for the lists this kernel orders
    int *out_ids;
    float *out_d;
    int sort_max;                  // lists longer than this (<= kExactRangeSortMax) are left to the host
};

// ExactTopKGrouped: ExactTopK's lists, but block b of a 1-D grid takes its queries and its rows from items[b] instead of from
// blockIdx and ExactScanArgs::m / chunk / nq / n_chunks (not read for this sink).  ExactScanArgs::ids is the groups' CSR, queries
// the round's queries sorted by group, qtile the LDS layout's tile (an item has at most that many queries).
struct ExactWorkItem {
    int q0, nq;          // the tile: queries [q0, q0 + nq) of the round, one group's, 1 <= nq <= qtile
    int off, len;        // the chunk: entries [off, off + len) of ids, len >= 1
    long long list0;     // the first list of query q0: query q0 + i, chunk slot c writes list list0 + i * n_chunks + c
    int n_chunks, slot;  // chunks of this group's list, and which of them this is
};
struct ExactTopKGrouped {
    static constexpr bool kRange = false;
    static constexpr bool kGrouped = true;
    static constexpr bool kSelf = false;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
    const ExactWorkItem *items;
};
// ExactRangeGrouped: ExactRange's segments behind ExactTopKGrouped's work items (list0, n_chunks and slot of an item are not read).
// Query q of the round's sorted order owns segment dest[q]: counts[dest[q]] and arena[seg_off[dest[q]], seg_off[dest[q] + 1]).  In a
// first pass dest[q] is the query's place in the caller's order, so counts, segments and the ordered lists are in that order and
// nothing is permuted afterwards; in a repeated pass it numbers the queries that are scanned again and is -1 for the others of a
// tile, whose keys are dropped.
struct ExactRangeGrouped {
    static constexpr bool kRange = true;
    static constexpr bool kGrouped = true;
    static constexpr bool kSelf = false;
    static constexpr bool kCollapse = false;
    static constexpr bool kUnion = false;
    static constexpr bool kDensity = false;
    float range;
    unsigned *counts;              // [segments]
    const long long *seg_off;      // [segments + 1]
    unsigned long long *arena;
    const ExactWorkItem *items;
    const int *dest;               // [nq of the round, sorted order]: the query's segment, or -1
};
// what exact_merge_grouped_kernel reads per query of the round (in sorted order)
struct ExactMergeItem {
    long long list0;     // its first list
    int n_chunks;        // 0: its group has no member, the row is padding
    int out_row;         // its row of the round's output: the query's original place in the round
};

// LDS of one scan block.  entry_bytes: what a list entry takes -- 8, the key; 12 with ExactTopKCollapse's label (the labels of all
// lists, and then those of the pending keys, stand behind everything else, so the rest of the layout is the same for every sink).
constexpr int kExactKeyBytes = 8, kExactCollapseEntryBytes = 12;
inline size_t exact_scan_lds(int qtile, int piece, int dim, int k, int entry_bytes = kExactKeyBytes)
{
    const size_t qtr = (size_t)((qtile + kExactRQ - 1) / kExactRQ * kExactRQ), qw = (size_t)(piece < dim ? piece : dim);
    const size_t pending = (size_t)kExactRQ * kExactIterRows * (entry_bytes > kExactKeyBytes ? 12 : 8); // (a pending key's label travels with it)
    return ((qtr * qw * 4 + 15) & ~(size_t)15) + qtr * (size_t)k * (size_t)entry_bytes + qtr * 8 + pending + 16;
}

// ... of ExactRangeDensity: the layout above without lists (k = 0) and, where ExactTopKCollapse's labels would begin, an int per
// query slot of the tile: the within pairs of the block that hold that query
inline size_t exact_density_lds(int qtile, int piece, int dim)
{
    return exact_scan_lds(qtile, piece, dim, 0) + (size_t)((qtile + kExactRQ - 1) / kExactRQ * kExactRQ) * 4;
}

template <int METRIC>
hipError_t exact_scan_launch(const ExactScanArgs &a, unsigned n_qtiles, size_t lds, hipStream_t st);
template <int METRIC> // lds: exact_density_lds
hipError_t exact_range_density_scan_launch(const ExactScanArgs &a, const ExactRangeDensity &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
template <int METRIC> // lds: exact_scan_lds with k = 0, as ExactRangeUnion's
hipError_t exact_range_density_join_scan_launch(const ExactScanArgs &a, const ExactRangeDensityJoin &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
// counts[0, n) = -1, then counts[id] = 0 for the m ids of the list; attach (nullptr: counts only) [0, n) = kExactEmpty; *n_pairs = 0
hipError_t density_init_launch(const int *ids, long long m, int *counts, unsigned long long *attach, long long n, unsigned long long *n_pairs, hipStream_t st);
// phase B over the arena's n_pairs records (all of them were kept): what ExactRangeDensityJoin does per within pair
hipError_t density_pairs_launch(const ExactDensityPair *arena, unsigned long long n_pairs, const int *counts, int min_samples, int *parent,
                                unsigned long long *attach, hipStream_t st);
// labels[v], v in [0, n): a core member its root; a member that is not core its attach key's id's root, -1 without a key; -1 where counts[v] < 0
hipError_t density_labels_launch(int *parent, const unsigned long long *attach, const int *counts, int min_samples, long long n, int *labels, hipStream_t st);
template <int METRIC>
hipError_t exact_range_scan_launch(const ExactScanArgs &a, const ExactRange &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
template <int METRIC>
hipError_t exact_self_scan_launch(const ExactScanArgs &a, const ExactTopKSelf &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
template <int METRIC>
hipError_t exact_range_self_scan_launch(const ExactScanArgs &a, const ExactRangeSelf &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
template <int METRIC>
hipError_t exact_range_union_scan_launch(const ExactScanArgs &a, const ExactRangeUnion &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
// parent[0, n) = -1, then parent[id] = id for the m ids of the list (enqueued in this order)
hipError_t exact_union_init_launch(const int *ids, long long m, int *parent, long long n, hipStream_t st);
// labels[v] = the root of v's tree -- the smallest id of its group -- for v in [0, n); -1 where parent[v] is -1
hipError_t exact_union_labels_launch(int *parent, long long n, int *labels, hipStream_t st);
template <int METRIC> // lds: exact_scan_lds with kExactCollapseEntryBytes
hipError_t exact_collapsed_scan_launch(const ExactScanArgs &a, const ExactTopKCollapse &sink, unsigned n_qtiles, size_t lds, hipStream_t st);
// exact_merge_launch for the collapsed lists: the labels are looked up in row_group, info as ExactTopKCollapse::info
hipError_t exact_merge_collapsed_launch(const unsigned long long *lists, int n_chunks, int k, int nq, const int *row_group, int per_group,
                                        unsigned long long *info, int *out_ids, float *out_d, hipStream_t st);
// words: the masked bitset; block_off[b]: set bits in front of word b * kExactCompactWords
hipError_t exact_compact_launch(const unsigned *words, long long n_words, const long long *block_off, int *out_ids, hipStream_t st);
hipError_t exact_merge_launch(const unsigned long long *lists, int n_chunks, int k, int nq, int *out_ids, float *out_d, hipStream_t st);
hipError_t exact_range_sort_launch(const ExactRangeSortArgs &a, int nq, hipStream_t st);
template <int METRIC>
hipError_t exact_grouped_scan_launch(const ExactScanArgs &a, const ExactTopKGrouped &sink, unsigned n_items, size_t lds, hipStream_t st);
template <int METRIC>
hipError_t exact_range_grouped_scan_launch(const ExactScanArgs &a, const ExactRangeGrouped &sink, unsigned n_items, size_t lds, hipStream_t st);
// row_group[0, n) -> counts[g] (zeroed here), offsets[g] (exclusive prefix), ids: group g's members in [offsets[g], offsets[g] + counts[g]),
// in no particular order; values outside [0, n_groups) are in no group.  cursors: n_groups ints of scratch.
hipError_t exact_group_lists_launch(const int *row_group, long long n, int n_groups, int *counts, int *offsets, int *cursors, int *ids, hipStream_t st);
// dst row i = src row perm[i] (words 4-byte words each), dst_sn[i] = src_sn[perm[i]] where src_sn is not nullptr
hipError_t exact_gather_queries_launch(const float *src, const double *src_sn, const int *perm, int nq, int words, float *dst, double *dst_sn, hipStream_t st);
hipError_t exact_merge_grouped_launch(const unsigned long long *lists, const ExactMergeItem *items, int k, int nq, int *out_ids, float *out_d, hipStream_t st);

} // namespace hnsw

#ifdef HNSW_EXACT_UNIT
#include "dk_base.h"
#include "dk_metric.h"
#include "dk_heaps.h"
#include "dk_union_find.h"

namespace hnsw {

constexpr unsigned long long kExactEmpty = ~0ull;

// (distance, id) as one integer with np.lexsort((ids, dist))'s order: the distance key above the id.  dk_heaps.h's f2key orders
// every number; -0 is made +0 first (they are equal: the lower id goes first) and every NaN becomes the one key above +inf's
// (NaNs order among themselves by id).  No real entry equals kExactEmpty: ids are below 2^31.
__device__ __forceinline__ unsigned long long exact_key(float d, int id)
{
    unsigned dk;
    if (d != d) dk = 0xffffffffu;
    else dk = f2key(__float_as_uint(d) == 0x80000000u ? 0.0f : d);
    return ((unsigned long long)dk << 32) | (unsigned)id;
}
__device__ __forceinline__ float exact_key_dist(unsigned long long key)
{
    const unsigned dk = (unsigned)(key >> 32);
    return dk == 0xffffffffu ? __uint_as_float(0x7fc00000u) : key2f(dk);
}

// One within pair (a < b, distance d with a's row as the query) of the density clusters, once counts[] is complete:
// both ends core -- the pair is an edge of a cluster: uf_union; exactly one end core -- the other end is a border candidate and keeps
// the smallest (distance, core id) it is offered, a relaxed agent-scope 64-bit min on attach[border] (kExactEmpty before the first);
// neither core: nothing.  The minimum does not depend on the order the pairs arrive in, and neither do the roots.
__device__ __forceinline__ void density_join(const int *counts, int min_samples, int *parent, unsigned long long *attach, int a, int b, float d)
{
    const bool ca = counts[a] + 1 >= min_samples, cb = counts[b] + 1 >= min_samples;
    if (ca && cb) uf_union(parent, a, b);
    else if (ca != cb) (void)__hip_atomic_fetch_min(attach + (ca ? b : a), exact_key(d, ca ? a : b), GI_RELAXED);
}

// x into the ascending list L[0, k) of one wave (x < L[k - 1]: the last entry drops out).  From the top down, 64 entries at a time:
// every entry above x moves up one place, x lands below the lowest of them.  One wave: its LDS operations execute in order.
__device__ __forceinline__ void exact_list_insert(unsigned long long *L, int k, unsigned long long x, int lane)
{
    for (int base = (k - 1) & ~63; base >= 0; base -= 64) {
        const int i = base + lane;
        const bool in = i < k;
        const unsigned long long v = in ? L[i] : 0ull, pv = (in && i > 0) ? L[i - 1] : 0ull;
        wave_lds_sync();
        if (in && v > x) L[i] = pv > x ? pv : x;
        wave_lds_sync();
        if (L[base] <= x) break; // x (or something below it) is this piece's first entry: nothing further down moves
    }
}

// x, whose label is g, into the COLLAPSED ascending list L[0, k) of one wave, G[0, k) the labels of its entries and m the cap per
// label (ExactTopKCollapse).  The list stays what the walk over everything offered so far keeps: ascending keys, at
// most m of a label.  First the wave counts, 64 entries at a time from the bottom up to the first empty slot (an empty slot is
// key == kExactEmpty; its label is never read): `ins`, the entries below x -- x's place; `below` / `total`, the entries of label g
// below x / at all; `last`, the place of the largest entry of label g.  Then
//   below >= m                 x is dropped: m of its label go before it
//   total >= m                 the largest entry of label g leaves (it is above x): entries [ins, last) move up one, x goes in at ins
//   otherwise, x < L[k - 1]    the ordinary insert: entries [ins, end) move up one, end the first empty slot, or k - 1 whose entry drops out
// x may be any key: the check against the k-th is this function's (a key that is not below the k-th can never enter: in a full list every
// entry of its label is then below it, so below == total, and either that is >= m or the ordinary insert has no place for it).  The
// callers skip such keys before the call only to save the counting pass.
// Every count comes from a ballot and every bound of both loops is the same in all lanes: no lane leaves a loop on its own.
// One wave: its LDS operations execute in order.
__device__ __forceinline__ void exact_list_insert_collapsed(unsigned long long *L, int *G, int k, int m, unsigned long long x, int g, int lane,
                                                            unsigned &dropped, unsigned &evicted)
{
    int ins = 0, below = 0, total = 0, last = -1, filled = 0;
    for (int base = 0; base < k; base += 64) {
        const int i = base + lane;
        const unsigned long long v = i < k ? L[i] : kExactEmpty;
        const bool same = v != kExactEmpty && G[i] == g; // (v is a real key: i < k)
        const unsigned long long b_same = __ballot(same);
        ins += __popcll(__ballot(v < x));
        below += __popcll(__ballot(same && v < x));
        total += __popcll(b_same);
        filled += __popcll(__ballot(v != kExactEmpty));
        if (b_same) last = base + 63 - __clzll((long long)b_same);
        if (__ballot(v == kExactEmpty)) break; // the list ends in this piece
    }
    int end = -1; // the place that is vacated, -1: x does not enter
    if (below >= m) ++dropped;
    else if (total >= m) { ++evicted; end = last; }
    else if (x < L[k - 1]) end = filled < k ? filled : k - 1; // a list that is not full gives up its first empty slot: nothing above it moves
    if (end >= 0) {
        for (int base = end & ~63; base >= (ins & ~63); base -= 64) { // from the top down: a piece reads the one below it before that is written
            const int i = base + lane;
            const bool in = i >= ins && i <= end, moved = in && i > ins;
            const unsigned long long nk = moved ? L[i - 1] : x;
            const int ng = moved ? G[i - 1] : g;
            wave_lds_sync();
            if (in) { L[i] = nk; G[i] = ng; }
            wave_lds_sync();
        }
    }
}

template <int METRIC, class SINK>
__global__ void __launch_bounds__(kExactThreads) exact_scan_kernel(const ExactScanArgs a, const SINK sink)
{
    static_assert(kExactRQ == kExactThreads / 64, "wave w merges query w of a register tile");
    constexpr int RQ = kExactRQ, RR = kExactRR;
    extern __shared__ __align__(16) unsigned char exact_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 3, j = tid & 7;
    const int dim = a.dim, k = a.k, QT = a.qtile, QTR = (QT + RQ - 1) / RQ * RQ;
    const int P = a.piece, qw = P < dim ? P : dim, npieces = (dim + P - 1) / P;
    float *qs = reinterpret_cast<float *>(exact_lds);
    unsigned long long *lists = reinterpret_cast<unsigned long long *>(exact_lds + (((size_t)QTR * qw * 4 + 15) & ~(size_t)15));
    unsigned long long *thr = lists + (size_t)QTR * k;
    unsigned long long *pend = thr + QTR;
    int *pend_cnt = reinterpret_cast<int *>(pend + RQ * kExactIterRows);
    [[maybe_unused]] int *labels = pend_cnt + 4; // ExactTopKCollapse: [QTR][k], the label of every list entry (exact_scan_lds: behind the rest)
    [[maybe_unused]] int *pend_lab = labels + (size_t)QTR * k; // ... [RQ][kExactIterRows], the label of every pending key
    [[maybe_unused]] unsigned dropped = 0, evicted = 0; // ... what this wave's inserts dropped and evicted (the same in all its lanes)
    [[maybe_unused]] int *dens_cnt = pend_cnt + 4; // ExactRangeDensity: [QTR], the block's within pairs per query slot (exact_density_lds: in the labels' place)
    // the block's queries [q0, q0 + its number) of the round and entries [lo, hi) of the id list: a work item's, or worked out from
    // blockIdx.  q_in: a query of the round that this block answers; q_clamp: past the last of them a slot shadows it.
    long long q0, lo, hi;
    [[maybe_unused]] int item_qend = 0;
    if constexpr (SINK::kGrouped) { // (the item is the same for the whole block: its fields are kept in scalar registers)
        const ExactWorkItem &it = sink.items[blockIdx.x];
        const int iq0 = __builtin_amdgcn_readfirstlane(it.q0), ioff = __builtin_amdgcn_readfirstlane(it.off);
        item_qend = iq0 + __builtin_amdgcn_readfirstlane(it.nq);
        q0 = iq0;
        lo = ioff; hi = ioff + __builtin_amdgcn_readfirstlane(it.len);
    } else {
        q0 = (long long)blockIdx.x * QT;
        lo = (long long)blockIdx.y * a.chunk; hi = lo + a.chunk < a.m ? lo + a.chunk : a.m;
    }
    const auto q_in = [&](long long q) {
        if constexpr (SINK::kGrouped) return q < item_qend;
        else return q < a.nq;
    };
    const auto q_clamp = [&](long long q) {
        if constexpr (SINK::kGrouped) return q >= item_qend ? item_qend - 1 : q;
        else { if (q >= a.nq) q = a.nq - 1; return q; }
    };
    if constexpr (SINK::kUnion || SINK::kDensity) {
        // nothing to measure where the chunk's last id is not above the tile's first query id (both lists ascend): the whole block
        // leaves, in front of its first barrier
        const int last = a.ids ? a.ids[hi - 1] : (int)(hi - 1);
        if (__builtin_amdgcn_readfirstlane(last) <= __builtin_amdgcn_readfirstlane(sink.self[q0])) return;
    }
    const int rw = row_words<METRIC>(dim);
    const int nblk = dim >> 3;
    [[maybe_unused]] unsigned joined = 0; // ExactRangeUnion: pairs within the range that this lane met

    for (int i = tid; i < QTR * k; i += kExactThreads) lists[i] = kExactEmpty;
    if (tid < QTR) thr[tid] = kExactEmpty;
    if (tid < RQ) pend_cnt[tid] = 0;
    if constexpr (SINK::kDensity) {
        if constexpr (!SINK::kJoin) { if (tid < QTR) dens_cnt[tid] = 0; }
    }
    // (the first staging's barriers order these writes before their first readers)

    unsigned measured = 0; // pairs this lane turned into keys (lane 0 of a group: shadows of rows and queries excluded)
    bool staged = false;
    for (long long base = lo; base < hi; base += kExactIterRows) {
        // this group's rows; past the chunk's end a group shadows the chunk's last row and discards (all eight lanes of every
        // group stay live for the collapses)
        int rid[RR];
        bool rvalid[RR];
        const float *rp[RR];
        [[maybe_unused]] int rlab[RR]; // ExactTopKCollapse: the rows' labels, asked for here so that they arrive behind the measuring
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            long long idx = base + grp * RR + r;
            rvalid[r] = idx < hi;
            if (!rvalid[r]) idx = hi - 1;
            rid[r] = a.ids ? a.ids[idx] : (int)idx;
            rp[r] = a.rows + (size_t)rid[r] * (size_t)rw;
            if constexpr (SINK::kCollapse) rlab[r] = sink.row_group[rid[r]];
        }
        [[maybe_unused]] int rc[RR] = {}; // ExactRangeDensity: within pairs of this step that hold row r, over all the tile's queries
        for (int qsub = 0; qsub < QT && q_in(q0 + qsub); qsub += RQ) {
            float acc[RQ][RR];
            int iacc[RQ][RR], ta[RR], tb[RQ];
            float dist[RQ][RR];
#pragma unroll
            for (int q = 0; q < RQ; ++q) {
                tb[q] = 0;
#pragma unroll
                for (int r = 0; r < RR; ++r) { acc[q][r] = 0.0f; iacc[q][r] = 0; ta[r] = 0; }
            }
            for (int p = 0; p < npieces; ++p) {
                const int w0 = p * P, w1 = w0 + P < dim ? w0 + P : dim, len = w1 - w0;
                if (npieces > 1 || !staged) { // the queries of the tile, words [w0, w1); past the last query a slot shadows it
                    __syncthreads();
                    for (int qi = wave; qi < QTR; qi += kExactThreads / 64) {
                        const long long src = q_clamp(q0 + qi);
                        const float *s = a.queries + (size_t)src * dim + w0;
                        for (int o = lane; o < len; o += 64) qs[(size_t)qi * qw + o] = s[o];
                    }
                    __syncthreads();
                    staged = true;
                }
                const int s0 = w0 >> 3, s1 = w1 >> 3; // the 8-element steps of this piece (P is a multiple of 16)
                const float *qb = qs + (size_t)qsub * qw + j;
                if constexpr (METRIC == M_I8) {
                    const int *qi8 = reinterpret_cast<const int *>(qb);
#pragma unroll 2
                    for (int s = s0; s < s1; ++s) {
                        int wa[RR], wb[RQ];
#pragma unroll
                        for (int r = 0; r < RR; ++r) wa[r] = reinterpret_cast<const int *>(rp[r])[8 * s + j];
#pragma unroll
                        for (int q = 0; q < RQ; ++q) wb[q] = qi8[q * qw + 8 * (s - s0)];
                        if (s == nblk - 1 && j >= 6) { // the record's scale / sumsq words
#pragma unroll
                            for (int r = 0; r < RR; ++r) ta[r] = wa[r];
#pragma unroll
                            for (int q = 0; q < RQ; ++q) tb[q] = wb[q];
                        } else {
#pragma unroll
                            for (int q = 0; q < RQ; ++q)
#pragma unroll
                                for (int r = 0; r < RR; ++r) iacc[q][r] = dot4_i8(wa[r], wb[q], iacc[q][r]);
                        }
                    }
                } else if constexpr (metric_f16(METRIC)) {
                    for (int s = s0; s < s1; s += 2) { // one record word holds this lane's element of two consecutive steps
                        unsigned w[RR];
#pragma unroll
                        for (int r = 0; r < RR; ++r) w[r] = reinterpret_cast<const unsigned *>(rp[r])[8 * (s >> 1) + j];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            if (s + h < s1) {
                                float y[RQ];
#pragma unroll
                                for (int q = 0; q < RQ; ++q) y[q] = qb[q * qw + 8 * (s + h - s0)];
#pragma unroll
                                for (int r = 0; r < RR; ++r) {
                                    const float x = h ? half_hi(w[r]) : half_lo(w[r]);
#pragma unroll
                                    for (int q = 0; q < RQ; ++q) {
                                        if (metric_is_sq(METRIC)) { const float d = x - y[q]; acc[q][r] = __builtin_fmaf(d, d, acc[q][r]); }
                                        else { const float m = x * y[q]; acc[q][r] = acc[q][r] + m; }
                                    }
                                }
                            }
                        }
                    }
                } else {
#pragma unroll 2
                    for (int s = s0; s < s1; ++s) {
                        float x[RR], y[RQ];
#pragma unroll
                        for (int r = 0; r < RR; ++r) x[r] = rp[r][8 * s + j];
#pragma unroll
                        for (int q = 0; q < RQ; ++q) y[q] = qb[q * qw + 8 * (s - s0)];
#pragma unroll
                        for (int q = 0; q < RQ; ++q)
#pragma unroll
                            for (int r = 0; r < RR; ++r) {
                                if (metric_is_sq(METRIC)) { const float d = x[r] - y[q]; acc[q][r] = __builtin_fmaf(d, d, acc[q][r]); } // EuclideanMetric.cs:30
                                else { const float m = x[r] * y[q]; acc[q][r] = acc[q][r] + m; }                                       // CosineMetric.cs:114-115
                            }
                    }
                }
                if (p != npieces - 1) continue;
                // the last piece holds the tail elements: collapse, scalar tail, epilogue (group_metric's, pair by pair)
                if constexpr (METRIC == M_I8) {
                    const int g6 = (lane & ~7) | 6, g7 = (lane & ~7) | 7;
                    float sb[RQ];
                    int nb[RQ];
#pragma unroll
                    for (int q = 0; q < RQ; ++q) { sb[q] = __int_as_float(__shfl(tb[q], g6, 64)); nb[q] = __shfl(tb[q], g7, 64); }
#pragma unroll
                    for (int r = 0; r < RR; ++r) {
                        const float sa = __int_as_float(__shfl(ta[r], g6, 64));
                        const int na = __shfl(ta[r], g7, 64);
#pragma unroll
                        for (int q = 0; q < RQ; ++q) dist[q][r] = i8_epilogue(sa, na, sb[q], nb[q], group_sum_i32(iacc[q][r]));
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < RQ; ++q) {
                        double sqn = 0.0;
                        if constexpr (METRIC == M_COS) {
                            sqn = a.q_sn[q_clamp(q0 + qsub + q)];
                        }
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            float s = metric_is_sq(METRIC) ? collapse_l2(acc[q][r]) : collapse_cos(acc[q][r]);
                            for (int i = dim & ~7; i < dim; ++i) { // every lane redundantly; mul then add, no fma
                                const float x = row_elem<METRIC>(rp[r], i), y = qs[(size_t)(qsub + q) * qw + (i - w0)];
                                if (metric_is_sq(METRIC)) { const float d = x - y; const float m = d * d; s = s + m; }
                                else { const float m = x * y; s = s + m; }
                            }
                            if (metric_is_sq(METRIC)) dist[q][r] = s;
                            else if (metric_is_ucos(METRIC)) dist[q][r] = 1.0f - s;
                            else {
                                const float denom = (float)(a.row_sn[rid[r]] * sqn); // CosineMetric.cs:88
                                dist[q][r] = denom < 1e-30f ? 1.0f : 1.0f - s / denom; // :89-91
                            }
                        }
                    }
                }
            }
            if constexpr (SINK::kDensity) {
                // no offers: a pair above the diagonal is counted; within the range it is joined at once (the second scan) or leaves a
                // bit in wmask -- bit q * RR + r -- for the counting and the arena, which the whole wave does together below
                unsigned wmask = 0;
                int selfq[RQ] = {};
                if (j == 0) {
#pragma unroll
                    for (int q = 0; q < RQ; ++q) {
                        if (qsub + q >= QT || !q_in(q0 + qsub + q)) continue;
                        selfq[q] = sink.self[q0 + qsub + q];
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            if (!rvalid[r] || rid[r] <= selfq[q]) continue; // the pair's other half, or the query's own row: not counted
                            ++measured;
                            if (dist[q][r] <= sink.range) {
                                if constexpr (SINK::kJoin) density_join(sink.counts, sink.min_samples, sink.parent, sink.attach, selfq[q], rid[r], dist[q][r]);
                                else wmask |= 1u << (q * RR + r);
                            }
                        }
                    }
                }
                if constexpr (!SINK::kJoin) {
                    if (__ballot(wmask != 0)) { // (all 64 lanes are here, and the test is the same in all of them)
#pragma unroll
                        for (int q = 0; q < RQ; ++q) {
                            const int qc = __popc((wmask >> (q * RR)) & ((1u << RR) - 1u));
                            if (qc) atomicAdd(&dens_cnt[qsub + q], qc); // LDS: flushed once per query at the block's end
                        }
                        unsigned total = 0;
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            unsigned col = 0;
#pragma unroll
                            for (int q = 0; q < RQ; ++q) col += (wmask >> (q * RR + r)) & 1u;
                            rc[r] += (int)col; // the row side: added up over the tile's queries, flushed behind their loop
                        }
                        // the places: the wave's within pairs of this step are those of its eight group leaders (lanes 0, 8, .. 56), so
                        // the wave's total and the pairs in front of a leader's own are sums of eight lane reads -- nothing per pair
                        const int mine = __popc(wmask);
                        unsigned before = 0;
#pragma unroll
                        for (int g = 0; g < 8; ++g) {
                            const unsigned cg = (unsigned)__builtin_amdgcn_readlane(mine, 8 * g);
                            before += (lane >> 3) > g ? cg : 0u;
                            total += cg;
                        }
                        unsigned long long first = 0;
                        if (lane == 0) first = atomicAdd(sink.n_pairs, (unsigned long long)total); // one global atomic per (wave, step)
                        first = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(first >> 32)) << 32) | __builtin_amdgcn_readfirstlane((unsigned)first);
#pragma unroll
                        for (int q = 0; q < RQ; ++q)
#pragma unroll
                            for (int r = 0; r < RR; ++r) {
                                if (!((wmask >> (q * RR + r)) & 1u)) continue;
                                const unsigned long long place = first + before + (unsigned)__popc(wmask & ((1u << (q * RR + r)) - 1u));
                                if (place < sink.arena_cap) sink.arena[place] = ExactDensityPair{selfq[q], rid[r], __float_as_uint(dist[q][r]), 0u};
                            }
                    }
                }
            } else if constexpr (SINK::kUnion) {
                // no offers: a pair above the diagonal is counted and, within the range, joined from the lane that holds its distance.
                // uf_union waits for no other lane, and the lanes meet again behind this branch, in front of the next step's barriers.
                if (j == 0) {
#pragma unroll
                    for (int q = 0; q < RQ; ++q) {
                        if (qsub + q >= QT || !q_in(q0 + qsub + q)) continue;
                        const int self = sink.self[q0 + qsub + q];
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            if (!rvalid[r] || rid[r] <= self) continue; // the pair's other half, or the query's own row: not counted
                            ++measured;
                            if (dist[q][r] <= sink.range) {
                                ++joined;
                                uf_union(sink.parent, self, rid[r]);
                            }
                        }
                    }
                }
            } else if constexpr (SINK::kRange) {
                // offers: every key within the range goes to its query's pending list (kExactIterRows entries per query of the
                // register tile: what one step can produce)
                int offered = 0;
                if (j == 0) {
#pragma unroll
                    for (int q = 0; q < RQ; ++q) {
                        if (qsub + q >= QT || !q_in(q0 + qsub + q)) continue;
                        [[maybe_unused]] int self = -1;
                        if constexpr (SINK::kSelf) self = sink.self[q0 + qsub + q]; // (a query of the round: q_in above)
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            if (!rvalid[r]) continue;
                            if constexpr (SINK::kSelf) { if (rid[r] == self) continue; } // the query's own row: no key, not counted
                            ++measured;
                            if (dist[q][r] <= sink.range) {
                                const int slot = atomicAdd(&pend_cnt[q], 1);
                                pend[q * kExactIterRows + slot] = exact_key(dist[q][r], rid[r]);
                                offered = 1;
                            }
                        }
                    }
                }
                if (__syncthreads_or(offered)) {
                    if constexpr (SINK::kGrouped) {
                        // wave w: query qsub + w of the item.  Everything but the lane's place is the same for the whole wave and is
                        // kept in scalar registers.  seg: the query's segment; -1: its keys are not wanted.  (A second copy of the
                        // flush below, to be kept in step with it: addressing the segment through the branch-free form of both costs
                        // 129 VGPRs against 127 here, 3 waves per SIMD against 4 -- DESIGN.md 3.23.)
                        const int wv = __builtin_amdgcn_readfirstlane(wave);
                        const int cnt = __builtin_amdgcn_readfirstlane(pend_cnt[wv]);
                        if (cnt > 0) {
                            const int seg = __builtin_amdgcn_readfirstlane(sink.dest[q0 + qsub + wv]);
                            if (seg >= 0) {
                                unsigned first = 0;
                                if (lane == 0) first = atomicAdd(&sink.counts[seg], (unsigned)cnt); // one global atomic per (query, step)
                                first = __builtin_amdgcn_readfirstlane(first); // (all 64 lanes are here: the first is lane 0)
                                const long long off = sink.seg_off[seg], room = sink.seg_off[seg + 1] - off - (long long)first;
                                for (int i = lane; i < cnt; i += 64)
                                    if (i < room) sink.arena[off + first + i] = pend[wv * kExactIterRows + i];
                            }
                            wave_lds_sync();
                            if (lane == 0) pend_cnt[wv] = 0;
                        }
                    } else {
                        const int cnt = pend_cnt[wave]; // wave w: query qsub + w, a real query when anything was offered to it
                        if (cnt > 0) {
                            const long long qg = q0 + qsub + wave;
                            unsigned first = 0;
                            if (lane == 0) first = atomicAdd(&sink.counts[qg], (unsigned)cnt); // one global atomic per (query, step)
                            first = __shfl(first, 0, 64);
                            const long long off = sink.seg_off[qg], cap = sink.seg_off[qg + 1] - off;
                            for (int i = lane; i < cnt; i += 64) {
                                const long long slot = (long long)first + i;
                                if (slot < cap) sink.arena[off + slot] = pend[wave * kExactIterRows + i];
                            }
                            wave_lds_sync();
                            if (lane == 0) pend_cnt[wave] = 0;
                        }
                    }
                    __syncthreads();
                }
            } else {
                // offers: a key goes to its query's pending list only when it is below that query's current k-th
                int offered = 0;
                if (j == 0) {
#pragma unroll
                    for (int q = 0; q < RQ; ++q) {
                        if (qsub + q >= QT || !q_in(q0 + qsub + q)) continue;
                        const unsigned long long t = thr[qsub + q];
                        [[maybe_unused]] int self = -1;
                        if constexpr (SINK::kSelf) self = sink.self[q0 + qsub + q]; // (a query of the round: q_in above)
#pragma unroll
                        for (int r = 0; r < RR; ++r) {
                            if (!rvalid[r]) continue;
                            if constexpr (SINK::kSelf) { if (rid[r] == self) continue; } // the query's own row: no key, not counted
                            ++measured;
                            const unsigned long long key = exact_key(dist[q][r], rid[r]);
                            if (key < t) {
                                const int slot = atomicAdd(&pend_cnt[q], 1);
                                pend[q * kExactIterRows + slot] = key;
                                if constexpr (SINK::kCollapse) pend_lab[q * kExactIterRows + slot] = rlab[r];
                                offered = 1;
                            }
                        }
                    }
                }
                if (__syncthreads_or(offered)) {
                    const int cnt = pend_cnt[wave]; // wave w: query qsub + w (the set that results does not depend on the order of the offers)
                    if (cnt > 0) {
                        unsigned long long *L = lists + (size_t)(qsub + wave) * k;
                        for (int i = 0; i < cnt; ++i) {
                            const unsigned long long x = pend[wave * kExactIterRows + i];
                            if constexpr (SINK::kCollapse) { // (the label travelled with the key: no flush waits for memory)
                                const int g = pend_lab[wave * kExactIterRows + i];
                                if (x < L[k - 1]) exact_list_insert_collapsed(L, labels + (size_t)(qsub + wave) * k, k, sink.per_group, x, g, lane, dropped, evicted);
                            } else {
                                if (x < L[k - 1]) exact_list_insert(L, k, x, lane);
                            }
                        }
                        wave_lds_sync();
                        if (lane == 0) { thr[qsub + wave] = L[k - 1]; pend_cnt[wave] = 0; }
                    }
                    __syncthreads();
                }
            }
        }
        if constexpr (SINK::kDensity) {
            if constexpr (!SINK::kJoin) { // the row side of the step's within pairs: one global atomic per row that has any
#pragma unroll
                for (int r = 0; r < RR; ++r)
                    if (rc[r]) atomicAdd(&sink.counts[rid[r]], rc[r]);
            }
        }
    }
    __syncthreads();
    if (measured) atomicAdd(a.evals, (unsigned long long)measured); // one atomic per group that measured anything
    if constexpr (SINK::kDensity) {
        if constexpr (!SINK::kJoin) { // the self side: one global atomic per query of the tile that has any (the barrier above orders the LDS adds)
            if (tid < QT && q_in(q0 + tid)) {
                const int c = dens_cnt[tid];
                if (c) atomicAdd(&sink.counts[sink.self[q0 + tid]], c);
            }
        }
    }
    if constexpr (SINK::kUnion) {
        if (joined) atomicAdd(sink.pairs, (unsigned long long)joined);
    }
    if constexpr (SINK::kCollapse) {
        if (lane == 0 && dropped) atomicAdd(&sink.info[0], (unsigned long long)dropped);
        if (lane == 0 && evicted) atomicAdd(&sink.info[1], (unsigned long long)evicted);
    }
    if constexpr (!SINK::kRange) {
        for (int qi = 0; qi < QT && q_in(q0 + qi); ++qi) {
            unsigned long long *dst;
            if constexpr (SINK::kGrouped) { // (the item is read again here rather than kept in registers through the scan)
                const ExactWorkItem &it = sink.items[blockIdx.x];
                dst = a.lists + (size_t)(it.list0 + (long long)qi * it.n_chunks + it.slot) * (size_t)k;
            } else dst = a.lists + ((size_t)(q0 + qi) * a.n_chunks + blockIdx.y) * (size_t)k;
            for (int i = tid; i < k; i += kExactThreads) dst[i] = lists[(size_t)qi * k + i];
        }
    }
}

template <int METRIC>
hipError_t exact_scan_launch(const ExactScanArgs &a, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactTopK>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, ExactTopK{});
    return hipGetLastError();
}
template <int METRIC>
hipError_t exact_range_scan_launch(const ExactScanArgs &a, const ExactRange &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactRange>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}

template <int METRIC>
hipError_t exact_range_self_scan_launch(const ExactScanArgs &a, const ExactRangeSelf &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactRangeSelf>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}
template <int METRIC>
hipError_t exact_range_union_scan_launch(const ExactScanArgs &a, const ExactRangeUnion &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactRangeUnion>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}

template <int METRIC>
hipError_t exact_range_density_scan_launch(const ExactScanArgs &a, const ExactRangeDensity &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactRangeDensity>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}
template <int METRIC>
hipError_t exact_range_density_join_scan_launch(const ExactScanArgs &a, const ExactRangeDensityJoin &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactRangeDensityJoin>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}

template <int METRIC>
hipError_t exact_self_scan_launch(const ExactScanArgs &a, const ExactTopKSelf &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactTopKSelf>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}

template <int METRIC>
hipError_t exact_collapsed_scan_launch(const ExactScanArgs &a, const ExactTopKCollapse &sink, unsigned n_qtiles, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactTopKCollapse>), dim3(n_qtiles, (unsigned)a.n_chunks), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}

template <int METRIC>
hipError_t exact_grouped_scan_launch(const ExactScanArgs &a, const ExactTopKGrouped &sink, unsigned n_items, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactTopKGrouped>), dim3(n_items), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}
template <int METRIC>
hipError_t exact_range_grouped_scan_launch(const ExactScanArgs &a, const ExactRangeGrouped &sink, unsigned n_items, size_t lds, hipStream_t st)
{
    hipLaunchKernelGGL((exact_scan_kernel<METRIC, ExactRangeGrouped>), dim3(n_items), dim3(kExactThreads), lds, st, a, sink);
    return hipGetLastError();
}

#ifdef HNSW_EXACT_COMMON
// The bitset as an ascending id list: one word per thread, its place = the block's offset (counted on the host while the words
// were staged) + the prefix of the bit counts inside the block (wave prefix by shuffles rather than ballots: a lane holds a word, not a bit; wave totals through LDS).
__global__ void __launch_bounds__(kExactCompactWords) exact_compact_kernel(const unsigned *__restrict__ words, long long n_words,
                                                                           const long long *__restrict__ block_off, int *__restrict__ out_ids)
{
    __shared__ int wave_total[kExactCompactWords / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long w = (long long)blockIdx.x * kExactCompactWords + tid;
    unsigned v = w < n_words ? words[w] : 0u;
    const int c = __popc(v);
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    long long pos = block_off[blockIdx.x] + (incl - c);
    for (int i = 0; i < wave; ++i) pos += wave_total[i];
    const long long id0 = w << 5;
    while (v) {
        const int b = __ffs((int)v) - 1;
        out_ids[pos++] = (int)(id0 + b);
        v &= v - 1;
    }
}

// One wave per query: the chunks' ascending lists into the final k.  A list is left at its first entry that is not below the
// current k-th (the rest of it is larger still; ~0 marks a list's end).
__global__ void __launch_bounds__(64) exact_merge_kernel(const unsigned long long *__restrict__ lists, int n_chunks, int k, int *__restrict__ out_ids,
                                                         float *__restrict__ out_d)
{
    __shared__ unsigned long long L[kExactMaxK];
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    for (int i = lane; i < k; i += 64) L[i] = kExactEmpty;
    wave_lds_sync();
    for (int c = 0; c < n_chunks; ++c) {
        const unsigned long long *src = lists + (q * n_chunks + c) * (size_t)k;
        bool more = true;
        for (int i0 = 0; i0 < k && more; i0 += 64) {
            const unsigned long long mine = i0 + lane < k ? src[i0 + lane] : kExactEmpty;
            const int n = k - i0 < 64 ? k - i0 : 64;
            for (int t = 0; t < n; ++t) {
                const unsigned lo32 = __shfl((unsigned)mine, t, 64), hi32 = __shfl((unsigned)(mine >> 32), t, 64);
                const unsigned long long x = ((unsigned long long)hi32 << 32) | lo32;
                if (x >= L[k - 1]) { more = false; break; }
                exact_list_insert(L, k, x, lane);
            }
        }
    }
    wave_lds_sync();
    for (int i = lane; i < k; i += 64) {
        const unsigned long long key = L[i];
        out_ids[q * k + i] = key == kExactEmpty ? -1 : (int)(unsigned)key;
        out_d[q * k + i] = key == kExactEmpty ? __uint_as_float(0x7fc00000u) : exact_key_dist(key);
    }
}

// exact_merge_kernel over collapsed lists (ExactTopKCollapse): the chunks' lists hold keys only, so the label of an incoming key is
// looked up in row_group, and the insert is the collapsed one.  A list is still left at its first entry that is not below the
// current k-th: such a key cannot enter (in a full list every entry of its label is then below it), and the rest of its list is
// larger still.  (A copy of the merge's loop, as exact_merge_grouped_kernel's is and for its reason; a change goes into all three.)
__global__ void __launch_bounds__(64) exact_merge_collapsed_kernel(const unsigned long long *__restrict__ lists, int n_chunks, int k, const int *__restrict__ row_group,
                                                                   int per_group, unsigned long long *__restrict__ info, int *__restrict__ out_ids,
                                                                   float *__restrict__ out_d)
{
    __shared__ unsigned long long L[kExactMaxK];
    __shared__ int G[kExactMaxK];
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    unsigned dropped = 0, evicted = 0;
    for (int i = lane; i < k; i += 64) L[i] = kExactEmpty;
    wave_lds_sync();
    for (int c = 0; c < n_chunks; ++c) {
        const unsigned long long *src = lists + (q * n_chunks + c) * (size_t)k;
        bool more = true;
        for (int i0 = 0; i0 < k && more; i0 += 64) {
            const unsigned long long mine = i0 + lane < k ? src[i0 + lane] : kExactEmpty;
            const int mine_g = mine != kExactEmpty ? row_group[(unsigned)mine] : 0; // the labels of the piece's keys, looked up at once
            const int n = k - i0 < 64 ? k - i0 : 64;
            for (int t = 0; t < n; ++t) { // (x, and with it the break, is the same in all lanes)
                const unsigned lo32 = __shfl((unsigned)mine, t, 64), hi32 = __shfl((unsigned)(mine >> 32), t, 64);
                const unsigned long long x = ((unsigned long long)hi32 << 32) | lo32;
                if (x >= L[k - 1]) { more = false; break; } // (a list's end, ~0, leaves here)
                exact_list_insert_collapsed(L, G, k, per_group, x, __builtin_amdgcn_readfirstlane(__shfl(mine_g, t, 64)), lane, dropped, evicted);
            }
        }
    }
    wave_lds_sync();
    if (lane == 0 && dropped) atomicAdd(&info[0], (unsigned long long)dropped);
    if (lane == 0 && evicted) atomicAdd(&info[1], (unsigned long long)evicted);
    for (int i = lane; i < k; i += 64) {
        const unsigned long long key = L[i];
        out_ids[q * k + i] = key == kExactEmpty ? -1 : (int)(unsigned)key;
        out_d[q * k + i] = key == kExactEmpty ? __uint_as_float(0x7fc00000u) : exact_key_dist(key);
    }
}

// One block per query: its segment's keys (counts[q] <= sort_max of them; longer and empty lists are not touched) into LDS, padded
// with ~0 to a power of two, a bitonic network over them, ids and distances out.  n, and so every loop bound and barrier, is the
// same for all threads of the block.
__global__ void __launch_bounds__(256) exact_range_sort_kernel(const ExactRangeSortArgs a)
{
    __shared__ unsigned long long K[kExactRangeSortMax];
    const int tid = threadIdx.x;
    const size_t q = blockIdx.x;
    const unsigned cnt = a.counts[q];
    if (cnt == 0 || cnt > (unsigned)a.sort_max || cnt > (unsigned)kExactRangeSortMax) return;
    const int n = (int)cnt;
    int P = 1;
    while (P < n) P <<= 1;
    const unsigned long long *src = a.arena + a.seg_off[q];
    for (int i = tid; i < P; i += 256) K[i] = i < n ? src[i] : kExactEmpty;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const unsigned long long x = K[i], y = K[l];
                if ((x > y) == ((i & k) == 0)) { K[i] = y; K[l] = x; }
            }
            __syncthreads();
        }
    const long long o = a.out_off[q];
    for (int i = tid; i < n; i += 256) {
        const unsigned long long key = K[i];
        a.out_ids[o + i] = (int)(unsigned)key;
        a.out_d[o + i] = exact_key_dist(key);
    }
}

// ---- the union-find around ExactRangeUnion's launches: grid-stride, no kernel waits for another wave ----
// Every id of the list is the root of its own tree.  (parent[] was filled with -1 in front of this launch: an id outside the list
// stays -1 and is never dereferenced, because the scan's candidates are the list's ids and nothing else.)
__global__ void __launch_bounds__(256) exact_union_init_kernel(const int *__restrict__ ids, long long m, int *__restrict__ parent)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) {
        const int v = ids[i];
        parent[v] = v;
    }
}
// The label of every id: the root of its tree, which is the smallest id of its group (uf_union hooks the larger root under the
// smaller); -1 for an id outside the list.  The finds of other threads halve paths meanwhile: parents only ever decrease towards the
// same root, so the root found does not depend on them.
__global__ void __launch_bounds__(256) exact_union_labels_kernel(int *parent, long long n, int *__restrict__ labels)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n; v += step)
        labels[v] = __hip_atomic_load(parent + v, GI_RELAXED) < 0 ? -1 : uf_find(parent, (int)v);
}
static inline unsigned exact_union_blocks(long long n) { return (unsigned)((n + 255) / 256 < (1LL << 16) ? (n + 255) / 256 : (1LL << 16)); }
hipError_t exact_union_init_launch(const int *ids, long long m, int *parent, long long n, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(parent, 0xff, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(exact_union_init_kernel, dim3(exact_union_blocks(m)), dim3(256), 0, st, ids, m, parent);
    return hipGetLastError();
}
hipError_t exact_union_labels_launch(int *parent, long long n, int *labels, hipStream_t st)
{
    hipLaunchKernelGGL(exact_union_labels_kernel, dim3(exact_union_blocks(n)), dim3(256), 0, st, parent, n, labels);
    return hipGetLastError();
}

// ---- the density clusters around ExactRangeDensity's launches: grid-stride, no kernel waits for another wave ----
// Every id of the list has no neighbour yet.  (counts[] was filled with -1 in front of this launch: an id outside the list stays -1.)
__global__ void __launch_bounds__(256) density_init_kernel(const int *__restrict__ ids, long long m, int *__restrict__ counts)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < m; i += step) counts[ids[i]] = 0;
}
// Phase B from the arena: one thread per record.  A record is one 16-byte load.
__global__ void __launch_bounds__(256) density_pairs_kernel(const ExactDensityPair *__restrict__ arena, unsigned long long n_pairs, const int *__restrict__ counts,
                                                            int min_samples, int *parent, unsigned long long *attach)
{
    const unsigned long long step = (unsigned long long)gridDim.x * 256;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += step) {
        const ExactDensityPair p = arena[i];
        density_join(counts, min_samples, parent, attach, p.a, p.b, __uint_as_float(p.d_bits));
    }
}
// The label of every id.  A core member: the root of its tree, the smallest core id of its cluster (only cores were joined, and
// uf_union hooks the larger root under the smaller).  Any other member: the root of the core its attach key names -- the core
// neighbour with the smallest (distance, id) -- or -1 where no core offered itself.  No member: -1.
__global__ void __launch_bounds__(256) density_labels_kernel(int *parent, const unsigned long long *__restrict__ attach, const int *__restrict__ counts,
                                                             int min_samples, long long n, int *__restrict__ labels)
{
    const long long step = (long long)gridDim.x * 256;
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n; v += step) {
        const int c = counts[v];
        int label = -1;
        if (c >= 0 && c + 1 >= min_samples) label = uf_find(parent, (int)v);
        else if (c >= 0 && attach[v] != kExactEmpty) label = uf_find(parent, (int)(unsigned)attach[v]);
        labels[v] = label;
    }
}
hipError_t density_init_launch(const int *ids, long long m, int *counts, unsigned long long *attach, long long n, unsigned long long *n_pairs, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(counts, 0xff, sizeof(int) * (size_t)n, st);
    if (e == hipSuccess && attach) e = hipMemsetAsync(attach, 0xff, sizeof(unsigned long long) * (size_t)n, st); // kExactEmpty
    if (e == hipSuccess) e = hipMemsetAsync(n_pairs, 0, sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(density_init_kernel, dim3(exact_union_blocks(m)), dim3(256), 0, st, ids, m, counts);
    return hipGetLastError();
}
hipError_t density_pairs_launch(const ExactDensityPair *arena, unsigned long long n_pairs, const int *counts, int min_samples, int *parent,
                                unsigned long long *attach, hipStream_t st)
{
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(density_pairs_kernel, dim3(exact_union_blocks((long long)n_pairs)), dim3(256), 0, st, arena, n_pairs, counts, min_samples, parent, attach);
    return hipGetLastError();
}
hipError_t density_labels_launch(int *parent, const unsigned long long *attach, const int *counts, int min_samples, long long n, int *labels, hipStream_t st)
{
    hipLaunchKernelGGL(density_labels_kernel, dim3(exact_union_blocks(n)), dim3(256), 0, st, parent, attach, counts, min_samples, n, labels);
    return hipGetLastError();
}

// ---- the group lists of exact_knn_grouped: a CSR over the groups, built from row_group in three launches ----
// One thread per id.  The lanes of a wave that hold the same group are served by one atomic: the wave takes the group of its first
// unserved lane, ballots the lanes that share it, and that lane adds their number (with thousands of ids per group a wave would
// otherwise send 64 atomics to a handful of addresses).  PLACE: the add returns the first free place of the group's segment and
// lane r of the sharing lanes writes its id r places further -- the order inside a segment is that of the atomics: unordered.
template <bool PLACE>
__global__ void __launch_bounds__(256) exact_group_kernel(const int *__restrict__ row_group, long long n, int n_groups, int *__restrict__ counters,
                                                          int *__restrict__ ids)
{
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int g = id < n ? row_group[id] : -1;
    if (g < 0 || g >= n_groups) g = -1;
    unsigned long long todo = __ballot(g >= 0);
    while (todo) { // wave-uniform: every lane sees the same mask
        const int lead = __ffsll((long long)todo) - 1;
        const int gl = __shfl(g, lead, 64);
        const unsigned long long same = __ballot(g == gl) & todo; // (lanes with g == -1 never match: gl >= 0)
        int first = 0;
        if (lane == lead) first = atomicAdd(&counters[gl], __popcll(same));
        if constexpr (PLACE) {
            first = __shfl(first, lead, 64);
            if (g == gl) ids[first + __popcll(same & ((1ull << lane) - 1ull))] = (int)id;
        }
        todo &= ~same;
    }
}

// offsets[g] = cursors[g] = the counts in front of group g.  One block walks the counts 256 at a time (at most kExactMaxGroups of
// them): a wave prefix by shuffles, the wave totals through LDS, the running total carried by every thread.
__global__ void __launch_bounds__(256) exact_group_offsets_kernel(const int *__restrict__ counts, int n_groups, int *__restrict__ offsets,
                                                                  int *__restrict__ cursors)
{
    __shared__ int wave_total[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < n_groups; base += 256) { // (n_groups is the same for all threads: so is every barrier)
        const int g = base + tid;
        const int c = g < n_groups ? counts[g] : 0;
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        int pos = carry + incl - c, total = 0;
        for (int i = 0; i < 4; ++i) {
            if (i < wave) pos += wave_total[i];
            total += wave_total[i];
        }
        if (g < n_groups) { offsets[g] = pos; cursors[g] = pos; }
        carry += total;
        __syncthreads(); // wave_total is written again in the next step
    }
}

// The resident queries in the call's order: one wave per query, `words` 4-byte words each (the int8 record's words included).
__global__ void __launch_bounds__(256) exact_gather_queries_kernel(const float *__restrict__ src, const double *__restrict__ src_sn, const int *__restrict__ perm,
                                                                   int nq, int words, float *__restrict__ dst, double *__restrict__ dst_sn)
{
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= nq) return;
    const int from = perm[q];
    const float *s = src + (size_t)from * words;
    float *d = dst + (size_t)q * words;
    for (int o = lane; o < words; o += 64) d[o] = s[o];
    if (src_sn && lane == 0) dst_sn[q] = src_sn[from];
}

// exact_merge_kernel with the query's lists and its output row read from a table: block q is query q of the round in sorted order,
// and its result goes to the row the query has in the caller's order.  (A copy, not a shared body: with the loop in a function of
// its own exact_merge_kernel compiles to other code -- 55 SGPRs for 57 -- and that kernel is to stay as it was.  A change to the
// merge goes into both.)
__global__ void __launch_bounds__(64) exact_merge_grouped_kernel(const unsigned long long *__restrict__ lists, const ExactMergeItem *__restrict__ items, int k,
                                                                 int *__restrict__ out_ids, float *__restrict__ out_d)
{
    __shared__ unsigned long long L[kExactMaxK];
    const int lane = threadIdx.x;
    const ExactMergeItem it = items[blockIdx.x];
    for (int i = lane; i < k; i += 64) L[i] = kExactEmpty;
    wave_lds_sync();
    for (int c = 0; c < it.n_chunks; ++c) {
        const unsigned long long *src = lists + (size_t)(it.list0 + c) * (size_t)k;
        bool more = true;
        for (int i0 = 0; i0 < k && more; i0 += 64) {
            const unsigned long long mine = i0 + lane < k ? src[i0 + lane] : kExactEmpty;
            const int n = k - i0 < 64 ? k - i0 : 64;
            for (int t = 0; t < n; ++t) {
                const unsigned lo32 = __shfl((unsigned)mine, t, 64), hi32 = __shfl((unsigned)(mine >> 32), t, 64);
                const unsigned long long x = ((unsigned long long)hi32 << 32) | lo32;
                if (x >= L[k - 1]) { more = false; break; }
                exact_list_insert(L, k, x, lane);
            }
        }
    }
    wave_lds_sync();
    const size_t row = (size_t)it.out_row * (size_t)k;
    for (int i = lane; i < k; i += 64) {
        const unsigned long long key = L[i];
        out_ids[row + i] = key == kExactEmpty ? -1 : (int)(unsigned)key;
        out_d[row + i] = key == kExactEmpty ? __uint_as_float(0x7fc00000u) : exact_key_dist(key);
    }
}

hipError_t exact_group_lists_launch(const int *row_group, long long n, int n_groups, int *counts, int *offsets, int *cursors, int *ids, hipStream_t st)
{
    const unsigned blocks = (unsigned)((n + 255) / 256);
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)n_groups, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(exact_group_kernel<false>, dim3(blocks), dim3(256), 0, st, row_group, n, n_groups, counts, (int *)nullptr);
    hipLaunchKernelGGL(exact_group_offsets_kernel, dim3(1), dim3(256), 0, st, counts, n_groups, offsets, cursors);
    hipLaunchKernelGGL((exact_group_kernel<true>), dim3(blocks), dim3(256), 0, st, row_group, n, n_groups, cursors, ids);
    return hipGetLastError();
}
hipError_t exact_gather_queries_launch(const float *src, const double *src_sn, const int *perm, int nq, int words, float *dst, double *dst_sn, hipStream_t st)
{
    hipLaunchKernelGGL(exact_gather_queries_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, src, src_sn, perm, nq, words, dst, dst_sn);
    return hipGetLastError();
}
hipError_t exact_merge_grouped_launch(const unsigned long long *lists, const ExactMergeItem *items, int k, int nq, int *out_ids, float *out_d, hipStream_t st)
{
    hipLaunchKernelGGL(exact_merge_grouped_kernel, dim3((unsigned)nq), dim3(64), 0, st, lists, items, k, out_ids, out_d);
    return hipGetLastError();
}
hipError_t exact_range_sort_launch(const ExactRangeSortArgs &a, int nq, hipStream_t st)
{
    hipLaunchKernelGGL(exact_range_sort_kernel, dim3((unsigned)nq), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t exact_compact_launch(const unsigned *words, long long n_words, const long long *block_off, int *out_ids, hipStream_t st)
{
    const unsigned blocks = (unsigned)((n_words + kExactCompactWords - 1) / kExactCompactWords);
    hipLaunchKernelGGL(exact_compact_kernel, dim3(blocks), dim3(kExactCompactWords), 0, st, words, n_words, block_off, out_ids);
    return hipGetLastError();
}
hipError_t exact_merge_launch(const unsigned long long *lists, int n_chunks, int k, int nq, int *out_ids, float *out_d, hipStream_t st)
{
    hipLaunchKernelGGL(exact_merge_kernel, dim3((unsigned)nq), dim3(64), 0, st, lists, n_chunks, k, out_ids, out_d);
    return hipGetLastError();
}
hipError_t exact_merge_collapsed_launch(const unsigned long long *lists, int n_chunks, int k, int nq, const int *row_group, int per_group,
                                        unsigned long long *info, int *out_ids, float *out_d, hipStream_t st)
{
    hipLaunchKernelGGL(exact_merge_collapsed_kernel, dim3((unsigned)nq), dim3(64), 0, st, lists, n_chunks, k, row_group, per_group, info, out_ids, out_d);
    return hipGetLastError();
}
#endif // HNSW_EXACT_COMMON

} // namespace hnsw
#endif // HNSW_EXACT_UNIT
