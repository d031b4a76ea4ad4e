/*
 * hnsw_mi355x.h -- C ABI of the MI355X-native distance backend for HNSWIndex.Net's
 * Add / KnnQuery hot path.
 *
 * Two boundaries, one shared library (artifacts/native/linux-x64/HNSWIndex.Native.so):
 *
 *  (A) OUTER boundary -- the reference's own 16 cdecl exports, same names, argument order,
 *      C types, return codes and padding, so the reference's ctypes wrapper
 *      (bindings/bindings.py:45-119) and any C host bind unchanged.  Each prototype cites
 *      the [UnmanagedCallersOnly] export it replaces in
 *      /root/reference/bindings/HNSWIndex.Native/HNSWIndexExports.cs.
 *
 *  (B) INNER boundary -- the batched candidate-distance backend a C# (or any) host
 *      P/Invokes in place of the scalar-pair delegate
 *      `Func<float[],float[],float> distFnc` (src/HNSWIndex/HNSWIndex.cs:20) that
 *      GraphData.Distance invokes one pair at a time (src/HNSWIndex/GraphData.cs:255-277).
 *      The reference has no batched hook; this is the hook.  INTEGRATION.md shows the
 *      C# binding.
 *
 * Conventions: plain pointers and sizes only; inputs are borrowed for the duration of the
 * call; outputs are caller-allocated unless stated; no exception crosses the boundary.
 * Every distance is computed by hand-written HIP kernels on gfx950; there is no CPU
 * fallback -- with no HIP device the calls fail and say so.
 */
#ifndef HNSW_MI355X_H
#define HNSW_MI355X_H

#include <stdbool.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* =====================================================================================
 * (A) Outer boundary: the reference's 16 exports
 * ===================================================================================== */

/* HNSWIndexExports.cs:27-39  GetLastErrorUtf8.  Copies at most buf_len-1 bytes of the last
 * error (UTF-8) and NUL-terminates; returns the byte count needed (without the NUL). */
int hnsw_get_last_error_utf8(void *buf, int buf_len);

/* :41-65  Create.  metric: "sq_euclid" | "cosine" | "ucosine".  Consumes and resets the
 * process-global pending parameters set by hnsw_set_* (:16, :61).  Returns 0 on error. */
void *hnsw_create(const char *distance_metric);

/* :67-73  Free. handle == 0 is ignored. */
void hnsw_free(void *handle);

/* :75-100  Add.  vectors: count x dim row-major float32.  Writes the assigned ids to
 * out_ids[count]; returns the number written, 0 for a null handle / null vectors /
 * count <= 0 / dim <= 0, -1 on error.  The reference inserts with Parallel.For
 * (src/HNSWIndex/HNSWIndex.cs:70-78): a scheduler-dependent interleaving.  Here the batch
 * is inserted in id order with snapshot-batched searches (DESIGN.md "Add"); a call with
 * count == 1 -- the reference's own recipe for deterministic builds,
 * bindings/__tests__/parameters_test.py:65-68 -- is exactly the sequential
 * HNSWIndex.Add(item) (HNSWIndex.cs:55-65). */
int hnsw_add(void *handle, const float *vectors, int count, int dim, int *out_ids);

/* :102-117  Remove -> HNSWIndex.Remove(List<int>) (HNSWIndex.cs:83-102); the ids are removed in
 * the order given (the reference uses Parallel.For).  Returns 0; 0 for a null handle / null ids /
 * count <= 0; -1 on error (removals disabled: InvalidOperationException; unknown id). */
int hnsw_remove(void *handle, const int *ids, int count);

/* :119-149  KnnQuery -> BatchKnnQuery (HNSWIndex.cs:129-137).  out_ids / out_dists are
 * count x k row-major; rows with fewer than k results are padded with id -1, dist NaN
 * (:144).  Returns 0 on success (and for a null handle), -1 on error.
 * Threads (the reference: operations of one type may overlap on an index, README.md:64-65): calls on one handle
 * from several host threads run side by side on the GPU, each on a query lane of its own; a call of 32 768
 * queries or more has the handle to itself and uploads all but its first rows behind its launch; every other
 * export takes the handle exclusively.  Any mix of calls from any number of threads is safe. */
int hnsw_knn_query(void *handle, const float *vectors, int count, int dim, int k, int *out_ids, float *out_dists);

/* :151-197  RangeQuery -> BatchRangeQuery (HNSWIndex.cs:144-168).  For query i, out_ids[i] /
 * out_dists[i] receive callee-allocated arrays of counts[i] results ordered by distance (null when
 * counts[i] == 0); release them with hnsw_free_results.  Returns 0, or -1 on error. */
int hnsw_range_query(void *handle, const float *vectors, int count, int dim, float range, void **out_ids,
                     void **out_dists, int *counts);

/* :199-217  FreeRangeResults.  Frees (with free()) whatever hnsw_range_query allocated. */
void hnsw_free_results(void **ids_array, void **dists_array, int count);

/* :219-273  pending-parameter setters (defaults: src/HNSWIndex/HNSWParameters.cs:13-55).
 * They mutate a process-global parameter block that the NEXT hnsw_create consumes. */
int hnsw_set_collection_size(int collection_size);       /* :219 */
int hnsw_set_max_edges(int max_edges);                   /* :226 */
int hnsw_set_max_candidates(int max_candidates);         /* :233 */
int hnsw_set_remove_max_candidates(int max_candidates);  /* :240 */
int hnsw_set_distribution_rate(float dist_rate);         /* :247 */
int hnsw_set_random_seed(int seed);                      /* :254 */
int hnsw_set_min_nn(int min_nn);                         /* :261 */
int hnsw_set_allow_removals(bool allow_removals);        /* :268 */

/* ---- additions next to the reference's surface (not in the reference) ---------------- */

/* THE BACKEND'S KNOBS, all of them (version 1 = this layout; struct_size = sizeof(hnsw_mi355x_options) names the version, a
 * library that knows a longer struct fills the rest with defaults).  Pending like hnsw_set_*: consumed by the next hnsw_create /
 * hnsw_mi355x_deserialize and reset to the defaults afterwards.  The hnsw_mi355x_set_<knob>() functions below set one field each.
 * Nothing else configures the product: the HNSW_MI355X_* environment switches of rounds 1-4 are gone. */
typedef struct hnsw_mi355x_options {
    uint32_t struct_size;      /* sizeof(hnsw_mi355x_options) */
    int32_t device;            /* first HIP device ordinal (default 0) */
    int32_t devices;           /* device contexts hnsw_knn_query shards its queries over (default 1; see hnsw_mi355x_set_devices) */
    int32_t insert_batch;      /* hnsw_add's schedule: 0 = snapshot batches of at most the host's hardware threads (default: inside the
                                * reference's Parallel.For outcome set), 1 = one item after the other, B > 1 = that cap, -W = the sequential
                                * graph through exact windows (see hnsw_mi355x_set_insert_batch) */
    int32_t remove_batch;      /* hnsw_remove's schedule: 1 = sequential (default), B > 1 = disjoint neighbourhoods together */
    int32_t host_threads;      /* host worker threads, 0 = min(hardware threads, 16) */
    int32_t search_slots;      /* concurrent searches of the host lock-step driver (default 16384) */
    int32_t device_traversal;  /* 1 = graph traversal on the device (default), 0 = on the host, distances batched to the device */
    const char *diagnostics;   /* NULL (default), or test hooks "name=value,..." (csrc/diag.h; process-wide, replaces the environment
                                * variable HNSW_MI355X_DIAG while set): forces code paths for the test tiers, never needed by a caller */
} hnsw_mi355x_options;
/* Fills *out with the defaults (struct_size set).  0 / -1. */
int hnsw_mi355x_default_options(hnsw_mi355x_options *out);
/* Sets every pending knob from *opt (opt->struct_size must be set; fields beyond it keep their defaults).  0 / -1 on a bad value. */
int hnsw_mi355x_set_options(const hnsw_mi355x_options *opt);

/* Pending, like hnsw_set_*: HIP device ordinal for the next hnsw_create (default 0). */
int hnsw_mi355x_set_device(int device);
/* Pending: cap B on the snapshot batch of hnsw_add: B consecutive items search the graph as it stands, then link in id
 * order (a batch also never exceeds 1/16 of the linked graph -- 1/4 of it during the first min(65 536, final count / 16)
 * inserts).  That is an interleaving the reference's HNSWIndex.Add(List) -- a Parallel.For over the items,
 * src/HNSWIndex/HNSWIndex.cs:70-78 -- can produce iff B <= the threads it runs on, so:
 *   0 (default)  B = hnsw_mi355x_host_parallelism(), the hardware threads of this host: the graph stays inside the
 *                reference's outcome set on this machine;
 *   1            strictly sequential inserts, HNSWIndex.Add(item) per item (HNSWIndex.cs:55-65);
 *   B > 1        that cap, legal for a Parallel.For host with >= B threads; caps far beyond any host (the 65 536 of rounds
 *                1-4, ~10x the build rate) are this build's own schedule -- opt-in, checked only against its CPU restatement;
 *   -W (W >= 2)  the graph of strictly sequential inserts built through speculative windows: W consecutive items search
 *                one snapshot and record the adjacency lists they read; in item order, an item whose lists nobody has
 *                written since is linked, the first one that is not ends the round and searches again.  Same graph as
 *                max_batch = 1, bit for bit (DESIGN.md "exact window").
 * See DESIGN.md "Add". */
int hnsw_mi355x_set_insert_batch(int max_batch);
/* The same knob on an existing index (takes effect with the next hnsw_add): lets one index be continued under
 * another schedule, as bench.py's add_modes do. */
int hnsw_mi355x_index_set_insert_batch(void *handle, int max_batch);
/* The threads this process may run on (affinity mask) -- the default cap above -- and the cap an index is using. */
int hnsw_mi355x_host_parallelism(void);
int hnsw_mi355x_index_insert_batch(void *handle);
/* Counters of the exact-window schedule since the index was created: out[0] rounds (dependent search launches),
 * out[1] insert searches run (>= items: the re-searched ones count again), out[2] items inserted alone (entry-point
 * moves, hand-backs), out[3] items linked through windows. */
int hnsw_mi355x_exact_window_stats(void *handle, uint64_t out[4]);
/* Counters of the row prefilter of KnnQuery (sq_euclid indices) since the index was created, totals over both
 * shadow widths (half precision and 8-bit): out[0] search launches that ran with it, out[1] rows measured on a shadow, out[2] rows
 * measured again from their f32 row (the others were turned away on the shadow value), out[3] shadow rows packed.  All zero where
 * it does not run. */
int hnsw_mi355x_row_prefilter_stats(void *handle, uint64_t out[4]);
/* Which kernel form those launches took: out[0] launches in the form that reads the row length at run time, out[1] launches in the
 * form with the row length compiled in (dim 128; four waves per SIMD).  Both are half-precision forms: a launch on the
 * 8-bit shadow is neither (hnsw_mi355x_row_prefilter8_stats). */
int hnsw_mi355x_row_prefilter_form_stats(void *handle, uint64_t out[2]);
/* Diagnostic, read only: the half-precision shadow of the row prefilter as it stands (it packs nothing and allocates nothing).
 * out[0] the packed watermark (shadow rows [0, out[0]) are current), out[1] the 32 bits of E, the index-wide bound on
 * ||x - h(x)||_2 (a float; 0x7f800000 = +inf: nothing is turned away).  rows (may be NULL when count is 0): count x dim floats, the
 * shadow rows [first_id, first_id + count) widened to f32.  An index without a shadow (no lean launch yet, another metric, diag
 * row_prefilter=0) has watermark 0.  -1 for a NULL handle or out, or a range that does not lie below the watermark. */
int hnsw_mi355x_row_prefilter_peek(void *handle, int first_id, int count, uint64_t out[2], float *rows);
/* The 8-bit shadow's own counters (dim 128; one 128-byte line per row): out[0] launches on it, out[1] rows packed into
 * it, out[2] rows measured on it, out[3] rows measured again from f32, out[4] full packs (each derives a fresh grid), out[5] launches
 * that re-read more than a quarter of their rows and switched the index to the half-precision prefilter.  -1 (with a message) for a
 * NULL handle or out. */
int hnsw_mi355x_row_prefilter8_stats(void *handle, uint64_t out[6]);
/* Diagnostic, read only: the 8-bit shadow as it stands.  out[0] the packed watermark, out[1] the bits of lo, out[2] the bits of step
 * (floats: the shadow value of code c is fmaf(step, (float)c, lo)), out[3] the bits of E8, the index-wide bound on ||x - h8(x)||_2.
 * codes (may be NULL when count is 0): count x 128 code bytes, rows [first_id, first_id + count), element i at byte i.  An index
 * without an 8-bit shadow has watermark 0.  -1 (with a message) for a NULL handle or out, a NULL codes with count > 0, or a range that
 * does not lie below the watermark. */
int hnsw_mi355x_row_prefilter8_peek(void *handle, int first_id, int count, uint64_t out[4], uint8_t *codes);
/* Pending: hnsw_remove's schedule.  1 (default): the ids one after the other, exactly HNSWIndex.Remove(int) per id.
 * B > 1: the deterministic counterpart of Remove(List<int>) = Parallel.For under region locks (HNSWIndex.cs:95-101,
 * GraphLocker.cs:28-72): removals whose neighbourhoods (the node, its out- and in-neighbours on every layer) are
 * disjoint are taken together, up to B per batch out of the first 8 B remaining ids, all searching the graph as it
 * stands before the batch; the others wait, in order; the entry point is always removed alone.  With
 * hnsw_mi355x_set_device_traversal(0) removals stay sequential whatever B says -- and so they do wherever Remove leaves the
 * device: rows of more than 2048 elements, or too long for the traversal's LDS.  See DESIGN.md 9. */
int hnsw_mi355x_set_remove_batch(int max_batch);
/* Pending: number of concurrent search slots of the lock-step driver (default 16384) and
 * host worker threads (default: min(hardware threads, 16)). */
int hnsw_mi355x_set_search_slots(int slots);
int hnsw_mi355x_set_host_threads(int threads);
/* Pending: 1 (default) = KnnQuery traverses on the device (graph mirrored in HBM, heaps in LDS);
 * 0 = traversal on the host, distances batched to the device step by step.  Same results. */
int hnsw_mi355x_set_device_traversal(int enabled);

/* Pending: number of device contexts of the next index (default 1).  With n > 1,
 * hnsw_knn_query -- BatchKnnQuery, a Parallel.For over independent searches, src/HNSWIndex/HNSWIndex.cs:129-137 via
 * bindings/HNSWIndex.Native/HNSWIndexExports.cs:119-149 -- shards its queries over n GPUs of the node inside this
 * one process: context g (device ordinal hnsw_mi355x_set_device + g, modulo the devices present) holds a replica of
 * the rows and of the graph mirror, copied device to device (hipMemcpyPeerAsync over xGMI) whenever the graph has
 * changed, answers queries [g nq / n, (g + 1) nq / n) and writes that slice of the caller's out arrays.  Same ids and
 * distance bits as one device.  Add / Remove / RangeQuery run on the first context. */
int hnsw_mi355x_set_devices(int n);
/* The sha256 (hex) of the sources this binary was compiled from -- csrc and include, by name and content, plus the compiler
 * flags -- or that string with "+variant" for a diagnostic build.  hnswindex.net_amd/build.py: source_id(). */
const char *hnsw_mi355x_build_id(void);
int hnsw_mi355x_device_count(void *handle);
/* hnswdev_stats of context `context` (0 = the primary). */
struct hnswdev_stats;
int hnsw_mi355x_get_stats_at(void *handle, int context, struct hnswdev_stats *out);

/* KnnQuery / BatchKnnQuery with a filter (HNSWIndex.KnnQuery(query, k, filterFnc), src/HNSWIndex/HNSWIndex.cs:107-137, layer 0):
 * hnsw_knn_query restricted to an ALLOW-SET over ids -- a little-endian bitset allow_bits of nbits bits, bit i = bit (i & 31) of
 * word (i >> 5); ids >= nbits are not allowed.  The reference's filterFnc(Items[id]) is a pure predicate of the item, so
 * bits[id] = filterFnc(Items[id]) over the live ids computes the same results: the descent to layer 0 is not filtered, a
 * disallowed node is still a candidate of the layer-0 search but never a result, and the output is the stable OrderBy(Dist).Take(k)
 * of the allowed results found -- same ids, distance bits, order and -1 / NaN padding as the reference.  A selective filter makes a
 * query explore about k / selectivity nodes (all of layer 0 that it reaches when fewer than max(MinNN, k) ids are allowed): that
 * is the reference's cost.  A set that allows no id of the index returns padding at once.  Return codes, the null-handle rule
 * (0) and padding are those of hnsw_knn_query; a NULL allow_bits or nbits < 0 is an error (-1, message in
 * hnsw_get_last_error_utf8).  Filtered calls take the handle exclusively (they do not overlap with other calls on it).
 * Traversal on the device (graph_search_filtered_kernel) with hand-backs to the host path; with hnsw_mi355x_set_devices(n) every
 * context gets the bitset and answers its shard. */
int hnsw_mi355x_knn_query_filtered(void *handle, const float *vectors, int count, int dim, int k, const uint32_t *allow_bits,
                                   long long nbits, int *out_ids, float *out_dists);

/* RangeQuery / BatchRangeQuery with a filter (HNSWIndex.RangeQuery(query, range, filterFnc), src/HNSWIndex/HNSWIndex.cs:144-168,
 * layer 0): hnsw_range_query restricted to an allow-set, the bitset of hnsw_mi355x_knn_query_filtered (ids >= nbits not allowed).
 * The descent and the layer-0 traversal are those of the unfiltered call -- a disallowed node within range is still a candidate
 * and is expanded -- and only allowed nodes enter the result heap; each list is the stable OrderBy(Dist) of that heap's array:
 * same ids, distance bits and order as the reference, including the order among equal distances.  Allocation, freeing
 * (hnsw_free_results), the null-handle rule (0) and the exclusive lock are those of hnsw_range_query; a NULL allow_bits or
 * nbits < 0 is an error (-1).  With range < 0 (cosine / ucosine distances can be negative) the reference can pop its empty result
 * heap and throw: when the entry point is not both allowed and within range, its distance is not +inf, and the first id of its
 * layer-0 list within range is disallowed.  Then the whole call returns -1 with every out_ids / out_dists entry NULL and every
 * count 0, and hnsw_get_last_error_utf8 names System.InvalidOperationException: Heap is empty. */
int hnsw_mi355x_range_query_filtered(void *handle, const float *vectors, int count, int dim, float range, const uint32_t *allow_bits,
                                     long long nbits, void **out_ids, void **out_dists, int *counts);

/* KnnQuery / RangeQuery on an upper layer (the `layer` argument of HNSWIndex.KnnQuery / RangeQuery, src/HNSWIndex/HNSWIndex.cs:107-168):
 * FindEntryPointQuery descends, unfiltered, from the entry point's top layer down to but not including `layer`, and the search
 * runs on `layer`'s lists (MaxEdges ids per list above layer 0), so every result is a node of that layer -- about n / M^layer
 * of the data.  Everything else is hnsw_knn_query / hnsw_range_query: beam max(MinNN, k), stable OrderBy(Dist), -1 / NaN padding,
 * the allocation contract of hnsw_range_query (hnsw_free_results), the null-handle rule (0).  allow_bits == NULL: no filter;
 * otherwise the allow-set of hnsw_mi355x_knn_query_filtered / hnsw_mi355x_range_query_filtered with their rules (nbits < 0: -1; the
 * empty-heap failure of a filtered range < 0).  layer < 0 or layer > the entry point's top layer (hnsw_mi355x_max_layer of
 * hnsw_mi355x_entry_point) on a non-empty index is -1 with a message, where the reference indexes OutEdges out of range and throws;
 * an empty index (and k < 1) returns padding / empty lists and success whatever `layer` is.  layer == 0 takes the paths of the
 * calls without a layer.  Calls with layer > 0 or a filter take the handle exclusively. */
int hnsw_mi355x_knn_query_at_layer(void *handle, const float *vectors, int count, int dim, int k, int layer, const uint32_t *allow_bits,
                                   long long nbits, int *out_ids, float *out_dists);
int hnsw_mi355x_range_query_at_layer(void *handle, const float *vectors, int count, int dim, float range, int layer, const uint32_t *allow_bits,
                                     long long nbits, void **out_ids, void **out_dists, int *counts);

/* MultiLayerKnnQuery (src/HNSWIndex/HNSWIndex.cs:173-187) for a batch of independent queries: each query's neighbours on every
 * layer from min(top, max_layer) down to min_layer, top = the entry point's top layer.  The first search enters where
 * FindEntryPointQuery(min(top, max_layer)) arrives; every later one enters at the NEAREST result of the layer above.  Each layer's
 * search has beam k (not max(MinNN, k)), no filter, and yields the stable OrderBy(Dist) of its result heap WITHOUT its first entry
 * (that entry is the next layer's entry point): at most k - 1 results per layer.
 * Returns the number of layer slots, min(top, max_layer) + 1, or -1.  out_ids / out_dists: [count][layers_cap][k - 1]; slot L of
 * a query holds layer L's results, -1 / NaN where a layer has fewer; slots below min_layer are -1 / NaN (the reference leaves
 * them null), slots at or above the returned count are not written.  layers_cap below the returned count is an error whose message
 * names the count needed.  k == 1 writes nothing and returns the count; an empty index, k < 1 or max_layer == -1 returns 0;
 * max_layer < -1 or min_layer < 0 is -1 (the reference throws); max_layer above top means top; min_layer above the last slot:
 * nothing is searched, every slot padded.  A null handle returns 0.  Takes the handle exclusively.  The chain of a query runs
 * as one job of graph_multilayer_kernel; a job it hands back is redone on the host path. */
int hnsw_mi355x_multilayer_knn_query(void *handle, const float *vectors, int count, int dim, int k, int max_layer, int min_layer,
                                     int layers_cap, int *out_ids, float *out_dists);

/* Exact k nearest neighbours by a flat scan on the device (no reference counterpart): for each query the k
 * CANDIDATES of smallest distance, where a candidate is a live id (hnsw_mi355x_active_ids) that the allow-set allows -- the bitset
 * of hnsw_mi355x_knn_query_filtered with its rules (ids >= nbits not allowed); allow_bits == NULL: no filter.  No graph is read, so
 * the answer does not depend on how the index was filled.  Distances are the index metric's values, bit for bit those of
 * hnswdev_dist_query_batch (a NaN distance is returned as the quiet NaN 0x7fc00000, a -0 distance as +0).  Order: ascending by
 * (distance, id) -- distances as IEEE numbers, NaN after +inf, equal distances (and NaNs) by id: the result is unique.
 * out_ids / out_dists: [count][k] row-major, a row that runs out of candidates padded with -1 / NaN.  1 <= k <= 1024; k > 1024 is
 * -1 with a message; k < 1, count <= 0 and a NULL handle behave as in hnsw_mi355x_knn_query_filtered (0, nothing or padding
 * written); nbits < 0 with a bitset is -1.  A set that allows no live id is answered with padding and no launch.  Always runs on
 * the device, whatever hnsw_set_device_traversal says, and on the primary context alone under hnsw_mi355x_set_devices(n).  Takes
 * the handle exclusively.  The resident query set (hnsw_mi355x_set_queries, or what hnsw_knn_query left) is not touched: the scan
 * stages its queries in a buffer of its own.  nbits is ignored when allow_bits is NULL. */
int hnsw_mi355x_exact_knn_query(void *handle, const float *vectors, int count, int dim, int k, const uint32_t *allow_bits, long long nbits,
                                int *out_ids, float *out_dists);

/* Every candidate within a radius, by the same flat scan (no reference counterpart): for each query ALL candidates
 * of hnsw_mi355x_exact_knn_query -- the live ids the allow-set allows, allow_bits == NULL: no filter, nbits then ignored -- whose
 * distance d satisfies the float compare d <= range (the reference's neighborDistance <= range).  Distances are those of
 * hnsw_mi355x_exact_knn_query, with its two representation rules (-0 is returned as +0; a NaN distance is never a result).
 * range = NaN: empty lists; range = +inf: every candidate whose distance is a number, +inf included; range = -0.0 admits distance 0;
 * a negative range is an ordinary one (there is no empty-heap failure here).  Order: ascending by (distance, id); keys are unique,
 * so the result is.  The length of a list is limited by memory alone -- 2^27 results per query (1 GiB of keys on the device); a
 * longer list is -1 with a message naming the limit.
 * Allocation is hnsw_range_query's: out_ids[i] / out_dists[i] are malloc'ed arrays of counts[i] entries, NULL where counts[i] is 0,
 * released with hnsw_free_results.  A NULL handle and count <= 0 behave as in hnsw_mi355x_range_query_filtered (0, nothing
 * written); nbits < 0 with a bitset is -1.  An empty index, or a set that allows no live id, gives counts of 0 and no launch.  On
 * any error every out pointer is NULL and every count 0.  Always runs on the device, on the primary context alone under
 * hnsw_mi355x_set_devices(n); takes the handle exclusively; the resident query set is not touched. */
int hnsw_mi355x_exact_range_query(void *handle, const float *vectors, int count, int dim, float range, const uint32_t *allow_bits,
                                  long long nbits, void **out_ids, void **out_dists, int *counts);
/* Counters of hnsw_mi355x_exact_range_query on the primary context since hnsw_mi355x_reset_stats: out[0] lists of two or more entries
 * ordered on the device, out[1] lists ordered on the host, out[2] rounds repeated with exact capacities, out[3] results returned.
 * (Its launches and measured pairs count in hnswdev_stats.exact_*: both calls are the flat scan.)  0, or -1 for a NULL argument. */
int hnsw_mi355x_exact_range_info(void *handle, uint64_t out[4]);

/* hnsw_mi355x_exact_knn_query with a candidate group per query (no reference counterpart): rows partitioned by
 * tenant, category or language, every query answered from its own part, all parts in one scan.  row_group is int32[n_row_group],
 * indexed by id; query_group is int32[count].  The candidates of query i are the live ids j < n_row_group with
 * row_group[j] == query_group[i].  A row_group value outside [0, n_groups) puts the id in no group, and so do ids >= n_row_group;
 * n_row_group beyond the index's length is clamped (a row that does not exist is never dereferenced).  1 <= n_groups <= 65 536.
 * Everything else is hnsw_mi355x_exact_knn_query's contract: distances, -0 / NaN representation, order by (distance, id), padding
 * with -1 / NaN (a query whose group has no live member gets a row of padding; when that holds for every query nothing is
 * scanned), 1 <= k <= 1024, no graph read, always on the device and on the primary context alone, the handle taken exclusively,
 * the resident query set untouched.  For every group g the rows of the result at query_group == g are byte for byte what
 * hnsw_mi355x_exact_knn_query returns for those queries with the allow-set {j : row_group[j] == g}.
 * -1 with a message, nothing written: row_group NULL or n_row_group < 0; n_groups outside 1 .. 65 536; a query_group value outside
 * [0, n_groups) (the message names the first such index); k > 1024.  NULL handle, count <= 0 and k < 1 behave as in
 * hnsw_mi355x_exact_knn_query. */
int hnsw_mi355x_exact_knn_query_grouped(void *handle, const float *vectors, int count, int dim, int k, const int *row_group,
                                        long long n_row_group, const int *query_group, int n_groups, int *out_ids, float *out_dists);
/* Counters of hnsw_mi355x_exact_knn_query_grouped on the primary context since hnsw_mi355x_reset_stats: out[0] grouped calls that
 * launched a scan, out[1] groups scanned (groups with a query and a candidate, summed over those calls), out[2] scan blocks
 * launched, out[3] ids placed in group lists -- all four of the calls that launched a scan only.  (Launches -- one per round -- and measured pairs count in hnswdev_stats.exact_*.)
 * 0, or -1 for a NULL argument. */
int hnsw_mi355x_exact_grouped_info(void *handle, uint64_t out[4]);

/* hnsw_mi355x_exact_knn_query with a collapsed result (no reference counterpart): at most per_group results per
 * label.  row_group is int32[n_row_group], indexed by id: the label of a row -- the document a chunk belongs to.  Per query, the
 * live (and, with allow_words, allowed) ids are taken in hnsw_mi355x_exact_knn_query's order, ascending (distance, id); an id is
 * kept while fewer than per_group kept ids have its label; the row of the result is the first k kept ids and their distances,
 * padded with -1 / NaN when they run out.  Labels are compared for equality: no value is special, negative values are labels like
 * any.  The filter restricts the candidates and the labels shape the result: removed and disallowed ids never count towards a
 * label's cap.  With per_group == k the rows are hnsw_mi355x_exact_knn_query's, byte for byte.  Exact: one scan, no retry, whatever
 * the labels' sizes.  Everything else is hnsw_mi355x_exact_knn_query's contract: distances, -0 / NaN representation, 1 <= k <= 1024,
 * no graph read, always on the device and on the primary context alone, the handle taken exclusively, the resident query set
 * untouched.  -1 with a message, nothing written: row_group NULL; n_row_group below the index's length (the message says both
 * numbers); per_group < 1 or per_group > k; k > 1024.  NULL handle, count <= 0 and k < 1 behave as in hnsw_mi355x_exact_knn_query. */
int hnsw_mi355x_exact_knn_query_collapsed(void *handle, const float *vectors, int count, int dim, int k, const int *row_group,
                                          long long n_row_group, int per_group, const uint32_t *allow_words, long long nbits, int *out_ids,
                                          float *out_dists);
/* The traversal form of the collapse: per query the first k survivors of the same walk over the row that
 * hnsw_mi355x_knn_query_at_layer(vectors, k = beam, layer, allow_words) returns, byte for byte, in that row's own order (the
 * reference's order among equal distances included); padding is skipped and the result padded with -1 / NaN.  beam >= k, any value
 * the plain call accepts as k.  It is approximate exactly as far as the plain call at that beam is: an id the traversal does not
 * reach at width beam is not in the result, and a label with more than per_group near rows uses up beam entries.  Where the
 * traversal runs on the device its rows are collapsed there and k columns come back.  row_group, n_row_group (at least the index's
 * length), per_group (1 .. k) and allow_words as hnsw_mi355x_exact_knn_query_collapsed; layer as hnsw_mi355x_knn_query_at_layer.
 * -1 with a message and nothing written for a breach of these; NULL handle, count <= 0 and k < 1 as hnsw_knn_query. */
int hnsw_mi355x_knn_query_collapsed(void *handle, const float *vectors, int count, int dim, int k, int beam, const int *row_group,
                                    long long n_row_group, int per_group, int layer, const uint32_t *allow_words, long long nbits, int *out_ids,
                                    float *out_dists);
/* Counters of hnsw_mi355x_exact_knn_query_collapsed on the primary context since hnsw_mi355x_reset_stats: out[0] collapsed calls that
 * scanned, out[1] queries they scanned, out[2] keys that reached a list and were dropped because per_group nearer keys of their label
 * stood in it, out[3] list entries that a nearer key of their label evicted.  out[2] and out[3] are counted by the scan's and the
 * merge's waves and depend on the order in which keys arrive; the results do not.  (Launches and measured pairs count in
 * hnswdev_stats.exact_*.)  0, or -1 for a NULL argument. */
int hnsw_mi355x_exact_collapsed_info(void *handle, uint64_t out[4]);

/* hnsw_mi355x_exact_range_query with a candidate group per query (no reference counterpart): the group arguments of
 * hnsw_mi355x_exact_knn_query_grouped -- row_group int32[n_row_group] indexed by id, query_group int32[count], the candidates of
 * query i the live ids j < n_row_group with row_group[j] == query_group[i], a value outside [0, n_groups) or an id past the
 * array's end in no group, 1 <= n_groups <= 65 536 -- and everything else hnsw_mi355x_exact_range_query's contract: the compare
 * d <= range on the distance itself, NaN never a result, the radii NaN / +inf / -0.0 / negative, order by (distance, id), 2^27
 * results per query, malloc'ed lists released with hnsw_free_results, NULL where counts[i] is 0.  All groups are scanned in one
 * launch per round; a query whose group has no live member gets an empty list without being scanned.  For every group g the lists
 * of the queries with query_group == g are byte for byte what hnsw_mi355x_exact_range_query returns for those queries with the
 * allow-set {j : row_group[j] == g}, and they come back in the caller's query order.
 * -1 with a message, every out pointer NULL and every count 0: row_group NULL or n_row_group < 0; n_groups outside 1 .. 65 536; a
 * query_group value outside [0, n_groups) (the message names the first such index); a list above the limit.  NULL handle and
 * count <= 0: 0, nothing written.  Always on the device and on the primary context alone; takes the handle exclusively; the
 * resident query set and the pending results of a range traversal are not touched. */
int hnsw_mi355x_exact_range_query_grouped(void *handle, const float *vectors, int count, int dim, float range, const int *row_group,
                                          long long n_row_group, const int *query_group, int n_groups, void **out_ids, void **out_dists,
                                          int *counts);
/* Counters of hnsw_mi355x_exact_range_query_grouped on the primary context since hnsw_mi355x_reset_stats: out[0] grouped range
 * calls that launched a scan, out[1] lists of two or more entries ordered on the device, out[2] lists ordered on the host, out[3]
 * pieces of a round scanned again with exact capacities.  (Launches and measured pairs count in hnswdev_stats.exact_*.)  0, or -1
 * for a NULL argument. */
int hnsw_mi355x_exact_range_grouped_info(void *handle, uint64_t out[4]);

/* hnsw_mi355x_knn_query_at_layer with a group filter per query (no reference counterpart): rows partitioned by
 * tenant, category or language, every query answered from its own part by the GRAPH traversal, all parts in one launch.
 * row_group is int32[n_row_group], indexed by id; query_group is int32[count].  Query i's filter is
 * "j < n_row_group && row_group[j] == query_group[i]": a row_group value outside [0, n_groups) puts the id in no group, and so do
 * ids >= n_row_group and vacant slots (removed ids); n_row_group beyond the index's length is clamped.  1 <= n_groups <= 65 536.
 * For every group g the rows of the result at query_group == g are byte for byte -- ids and distance bits -- what
 * hnsw_mi355x_knn_query_at_layer returns for those queries with the allow-set {j : row_group[j] == g} and the same layer, and so
 * carry its rules: the descent is not filtered, the beam is max(MinNN, k), the stable OrderBy(Dist).Take(k), -1 / NaN padding, the
 * layer rule (layer outside 0 .. the entry point's top layer on a non-empty index: -1), padding for an empty index or k < 1.  A
 * query whose group holds no id of the graph gets a row of padding and costs no traversal.  The labels are uploaded with every call
 * (nothing is cached between calls); hnsw_mi355x_set_devices(n): every context answers its shard of the queries with the labels
 * uploaded to it.  A job the device hands back, and the whole call when the traversal does not run on the device
 * (hnsw_mi355x_set_device_traversal(0), shapes the kernels do not fit), is answered by the host traversal, one filtered pass per
 * group concerned, with the same results.  Takes the handle exclusively.
 * -1 with a message, nothing written: row_group NULL or n_row_group < 0; n_groups outside 1 .. 65 536; a query_group value outside
 * [0, n_groups) (the message names the first such index).  NULL handle and count <= 0: 0, nothing written.
 * When groups are small the flat scan (hnsw_mi355x_exact_knn_query_grouped) is the faster tool: see DESIGN.md 3.20. */
int hnsw_mi355x_knn_query_grouped(void *handle, const float *vectors, int count, int dim, int k, int layer, const int *row_group,
                                  long long n_row_group, const int *query_group, int n_groups, int *out_ids, float *out_dists);
/* Counters of hnsw_mi355x_knn_query_grouped's device launches, summed over the contexts, since hnsw_mi355x_reset_stats: out[0]
 * calls that reached a context (one per context and call), out[1] queries launched, out[2] queries padded without a job because
 * their group holds no graph id, out[3] queries the device handed back to the host traversal.  (The launches, evaluations and
 * hand-backs also count in hnswdev_stats.search_launches / search_evals / search_overflows, as a filtered call's do; a call
 * answered by the host traversal alone counts nowhere here.)  0, or -1 for a NULL argument. */
int hnsw_mi355x_knn_grouped_info(void *handle, uint64_t out[4]);

/* The tagged calls (no reference counterpart): metadata that is not a partition -- a document with several labels,
 * a user who may read several tenants' rows, a product in several categories.  row_tags is uint32[n_row_tags], indexed by id, one
 * bit per tag (32 tags); query_tags is uint32[count], a mask per query; match is the mode of the whole call:
 *   0 "any": id j is a candidate of query i iff (row_tags[j] & query_tags[i]) != 0;
 *   1 "all": iff query_tags[i] != 0 and (row_tags[j] & query_tags[i]) == query_tags[i].
 * An id past the end of row_tags, a vacant slot (a removed id) and a row whose word is 0 carry no tag and are candidates of no
 * query; a query whose mask is 0 has no candidate; n_row_tags beyond the index's length is clamped.  The words are unsigned: bit 31
 * is a tag like the others.  A call may hold at most 65 536 distinct masks.
 * hnsw_mi355x_knn_query_tagged: for every distinct mask m the rows of the result at query_tags == m are byte for byte -- ids and
 * distance bits -- what hnsw_mi355x_knn_query_at_layer returns for those queries with the allow-set {j : j matches m} and the same
 * layer, and so carry its rules: the descent is not filtered, the beam is max(MinNN, k), the stable OrderBy(Dist).Take(k), -1 / NaN
 * padding, the layer rule (layer outside 0 .. the entry point's top layer on a non-empty index: -1), padding for an empty index or
 * k < 1.  All masks are answered by one device traversal (graph_search_tagged_kernel); a query whose mask has no candidate among
 * the graph's ids gets a row of padding and costs no traversal.  The words and masks are uploaded with every call (nothing is
 * cached between calls); hnsw_mi355x_set_devices(n): every context answers its shard of the queries with the words uploaded to it.
 * A job the device hands back, and the whole call when the traversal does not run on the device, is answered by the host
 * traversal, one filtered pass per distinct mask concerned, with the same results.  Takes the handle exclusively.
 * hnsw_mi355x_exact_knn_query_tagged: the same candidates answered by the flat scan -- per distinct mask the rows of
 * hnsw_mi355x_exact_knn_query with that allow-set, 1 <= k <= 1024 (above: -1), padding behind a mask's last candidate.  Every
 * distinct mask is a candidate list built on the device; lists overlap, so the masks are scanned in batches whose lists hold at
 * most 2^28 ids together (a longer list is a batch alone).  Always on the primary context.
 * -1 with a message, nothing written: row_tags NULL or n_row_tags < 0; match other than 0 and 1; more than 65 536 distinct masks
 * (the message names the index of the first mask beyond).  NULL handle and count <= 0: 0, nothing written. */
int hnsw_mi355x_knn_query_tagged(void *handle, const float *vectors, int count, int dim, int k, int layer, const uint32_t *row_tags,
                                 long long n_row_tags, const uint32_t *query_tags, int match, int *out_ids, float *out_dists);
int hnsw_mi355x_exact_knn_query_tagged(void *handle, const float *vectors, int count, int dim, int k, const uint32_t *row_tags,
                                       long long n_row_tags, const uint32_t *query_tags, int match, int *out_ids, float *out_dists);
/* Counters of hnsw_mi355x_knn_query_tagged's device launches, summed over the contexts, since hnsw_mi355x_reset_stats: out[0] calls
 * that reached a context (one per context and call), out[1] distinct masks of those calls, out[2] queries launched, out[3] queries
 * padded without a job because their mask has no candidate, out[4] queries the device handed back to the host traversal.
 * (Launches, evaluations and hand-backs also count in hnswdev_stats.search_*, as a filtered call's do; a call answered by the host
 * traversal alone counts nowhere here.)  0, or -1 for a NULL argument. */
int hnsw_mi355x_knn_tagged_info(void *handle, uint64_t out[5]);
/* Counters of hnsw_mi355x_exact_knn_query_tagged since hnsw_mi355x_reset_stats: out[0] calls that counted candidates on the device,
 * out[1] distinct masks of those calls, out[2] queries scanned, out[3] queries padded because their mask has no candidate, out[4]
 * ids written into candidate lists, out[5] batches of masks scanned.  (Scan launches and pairs count in hnswdev_stats.exact_*.)
 * 0, or -1 for a NULL argument. */
int hnsw_mi355x_exact_tagged_info(void *handle, uint64_t out[6]);
/* QUERY BY STORED ID.  The rows of an index live in device memory; these calls read them back and use them as
 * queries without a copy on the host.  Every id must be live: one that is not (negative, beyond the ids handed out, or removed)
 * makes the call return -1 before anything is launched, with a message that names it.  ids may repeat and come in any order.
 * The calls take the handle exclusively, like the filtered calls.
 *
 * hnsw_mi355x_get_vectors: out[i * dim .. ) = the stored row of ids[i] as floats -- HNSWIndex.Items() for a list of ids.  The
 * values are what the index measures distances on, exactly hnswdev_download_rows' for the row kind: float32 rows are a copy,
 * half-precision rows the rounded row widened, int8 rows q * scale.  The rows are gathered on the device in one launch and
 * n * dim floats come back in one copy.  n <= 0: 0, nothing is written.  NULL ids or out with n > 0: -1. */
int hnsw_mi355x_get_vectors(void *handle, const int *ids, int n, float *out);
/* KnnQuery on `layer` for the stored rows of ids, each answered from every id but its own.  Row i of out_ids / out_dists
 * ([count][k], padded with -1 / NaN) is byte for byte -- ids, distance bits, the order among equal distances, the padding -- what
 * hnsw_mi355x_knn_query_at_layer with an allow-set of every id except ids[i] returns for the vector hnsw_mi355x_get_vectors
 * gives for ids[i].  A duplicate of the row under another id is an ordinary candidate (and ties at distance 0).  The queries are
 * gathered from the stored rows on the device (int8 rows are quantised again as any query is, cosine norms computed there) and
 * traversed in one launch per device context with the filter "id != ids[i]"; the descent is not filtered, the entry point is a
 * candidate even when it is ids[i], the beam is max(MinNN, k), and a job that meets NaN, -0 or a full heap is answered on the
 * host with the same exclusion.  hnsw_mi355x_set_device_traversal(0) answers everything that way, with the same bytes.
 * count <= 0: 0.  k < 1: 0, nothing is written.  NULL ids / out_ids / out_dists: -1.  layer outside 0 .. the entry point's top
 * layer: -1.  An index of one item answers with padding. */
int hnsw_mi355x_knn_query_by_id(void *handle, const int *ids, int count, int k, int layer, int *out_ids, float *out_dists);
/* The flat scan (hnsw_mi355x_exact_knn_query) for the stored rows of ids.  Row i is what hnsw_mi355x_exact_knn_query returns for
 * the vector hnsw_mi355x_get_vectors gives for ids[i] with the candidates "allow_bits (NULL: every live id) minus ids[i]":
 * ascending by (distance, id), unique, padded where the candidates run out -- an index of n live items gives at most n - 1
 * results.  The exclusion happens where the scan turns a pair into a key: the pair (query i, row ids[i]) produces none and is not
 * counted in hnswdev_stats.exact_evals; nothing is asked for k + 1 and dropped.  allow_bits / nbits as for
 * hnsw_mi355x_exact_knn_query; a set that holds only ids[i] gives padding, one that does not hold ids[i] changes nothing for
 * query i.  1 <= k <= 1024 (k < 1: 0, nothing written; k > 1024: -1).  The resident query set stays what it was. */
int hnsw_mi355x_exact_knn_query_by_id(void *handle, const int *ids, int count, int k, const uint32_t *allow_bits, long long nbits, int *out_ids,
                                      float *out_dists);
/* NEAR-DUPLICATES OF STORED ITEMS: the exact range scan for stored rows, and single-linkage groups from one scan.
 * Both run on the primary device context, take the handle exclusively and leave the resident query set as it was.
 *
 * hnsw_mi355x_exact_range_query_by_id: list i is byte for byte what hnsw_mi355x_exact_range_query returns for the vector
 * hnsw_mi355x_get_vectors gives for ids[i] with the candidates "allow_bits (NULL: every live id) minus ids[i]": ascending by
 * (distance, id), -0 and NaN as there, a NaN range gives empty lists, +inf every candidate whose distance is a number, a negative
 * range is ordinary.  The pair (query i, row ids[i]) offers no key in the scan and is not counted in hnswdev_stats.exact_evals; a
 * duplicate of the row under another id is an ordinary result at its distance.  ids may repeat and come in any order; one that is
 * not live: -1 before anything is launched, with a message that names it.  A set that holds only ids[i] gives an empty list, one
 * that does not hold ids[i] changes nothing for query i.  The allocation contract is hnsw_range_query's (hnsw_free_results); NULL
 * handle, count <= 0, nbits < 0 and the state after an error (every pointer NULL, every count 0) as hnsw_mi355x_exact_range_query.
 * Counted in hnsw_mi355x_by_id_info (calls, scanned, rows gathered, pairs skipped) and in hnsw_mi355x_exact_range_info. */
int hnsw_mi355x_exact_range_query_by_id(void *handle, const int *ids, int count, float range, const uint32_t *allow_bits, long long nbits, void **out_ids,
                                        void **out_dists, int *counts);
/* hnsw_mi355x_duplicate_groups: the MEMBERS are the live ids that allow_bits allows (NULL: every live id), ascending.  Members
 * a < b are joined when the distance measured with the stored row of a as the query -- handled as in the call above -- and row b as
 * the candidate is <= range (the float compare of hnsw_mi355x_exact_range_query: a NaN distance or a NaN range joins nothing).  The
 * groups are the connected components of that graph.  out_labels[v], v < length: the smallest member id of v's group, -1 where v is
 * no member -- unique, whatever order the device finds the pairs in.  cap: the entries of out_labels; cap < length is -1 with a
 * message.  out_info[0] members m, [1] groups, [2] pairs a < b within the range, [3] pairs measured = m (m - 1) / 2.  One scan
 * whose sink is a union-find on the device: no list is built, sorted or copied.  Fewer than two members launch nothing.  NULL
 * handle: 0, out_info zeroed.  NULL out_info, or NULL out_labels with length > 0: -1. */
int hnsw_mi355x_duplicate_groups(void *handle, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, long long cap, uint64_t out_info[4]);
/* hnsw_mi355x_density_clusters: DBSCAN over the members and the pair rule of hnsw_mi355x_duplicate_groups, which is
 * this call at min_samples = 1.  Members a < b are WITHIN when the distance with the stored row of a as the query and row b as the
 * candidate is <= range (the float compare: a NaN distance or a NaN range admits nothing).
 *   out_counts[v], v < length: the within pairs that hold v -- its neighbours; -1 where v is no member.
 *   CORE: a member with out_counts[v] + 1 >= min_samples (the item counts itself).  min_samples < 1: -1 with a message.
 *   CLUSTERS: the connected components of the core members under the within pairs whose two ends are both core; a cluster's label
 *   is its smallest core id.
 *   BORDER: a member that is not core and has a core within-neighbour; it takes the label of the one with the smallest
 *   (distance, id) -- the pair's own distance, -0 equal to +0 -- so the result is unique, where textbook DBSCAN depends on the
 *   order of its visits.
 *   NOISE: every other member; its label is -1, as is every non-member's (out_counts tells the two apart).
 * out_info[0] members m, [1] clusters, [2] core, [3] border, [4] noise, [5] pairs a < b within the range, [6] pairs measured --
 * m (m - 1) / 2 per scan --, [7] scans: 0 with fewer than two members (nothing is launched), else 1, or 2 where the pairs found did
 * not fit the device's pair arena and the scan ran once more.  out_labels == NULL: the counts alone -- one scan, and the slots that
 * need labels ([1] .. [4]) are 0.  cap: the entries of out_counts, and of out_labels where given; cap < length is -1 with a message.
 * NULL handle: 0, out_info zeroed.  NULL out_info, or NULL out_counts with length > 0: -1. */
int hnsw_mi355x_density_clusters(void *handle, float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels, int *out_counts,
                                 long long cap, uint64_t out_info[8]);
/* NEAR-DUPLICATES OVER THE GRAPH'S EDGES: the question of the two calls above asked of layer 0 of the index's graph
 * instead of every pair -- n x (at most 2 MaxEdges) distances instead of m (m - 1) / 2.  The MEMBERS are those of
 * hnsw_mi355x_duplicate_groups.  An EDGE is a pair (i, j): i a member, j in i's layer-0 list, j a member; it is directed (j listing i
 * too is a second edge).  It is WITHIN the range when the distance with the stored row of i as the query and row j as the candidate is
 * <= range: the float compare, so a NaN range or distance admits nothing, +inf every edge whose distance is a number, a negative
 * range is ordinary; the bits are those hnsw_mi355x_exact_range_query_by_id reports for j in i's list.  Both calls bring the graph
 * mirror up to date first, run on the primary device context, take the handle exclusively and leave the resident query set and
 * every other call's pending results as they were.
 *
 * hnsw_mi355x_graph_duplicate_groups: the groups are the connected components of the members under the within-edges read both ways.
 * out_labels[v], v < length: the smallest member id of v's group, -1 where v is no member -- unique, whatever order the device
 * joins in.  Where the metric's value does not depend on which of two rows is the query (DESIGN.md 3.30 says for which kinds that
 * holds bit for bit) every within-edge is a pair hnsw_mi355x_duplicate_groups joins too, so these groups are that call's groups or
 * a refinement of them: two near-duplicates with no path of within-edges between them stay apart.  cap: the entries of out_labels;
 * cap < length is -1 with a message.  out_info[0] members, [1] groups, [2] edges within the range (directed), [3] edges measured
 * (directed edges between members: the distances taken), [4] launches of the edge kernel.  Fewer than two members launch nothing.
 * NULL handle: 0, out_info zeroed.  NULL out_info, or NULL out_labels with length > 0: -1. */
int hnsw_mi355x_graph_duplicate_groups(void *handle, float range, const uint32_t *allow_bits, long long nbits, int *out_labels, long long cap,
                                       uint64_t out_info[5]);
/* hnsw_mi355x_near_edges: the within-edges themselves.  The call counts them into *out_count and keeps them in the index until
 * hnsw_mi355x_near_edges_results copies them into out_src / out_dst / out_dists (cap entries each; cap below the count kept: -1 with a
 * message, nothing written) or the next hnsw_mi355x_near_edges replaces them.  Order: ascending by src; the entries of one src
 * ascending by (distance, dst) with -0 and +0 equal -- that item's hnsw_mi355x_exact_range_query_by_id list restricted to its
 * layer-0 list, in that list's order and with its distance bits.  NULL handle: 0 and a count of 0.  NULL out_count: -1. */
int hnsw_mi355x_near_edges(void *handle, float range, const uint32_t *allow_bits, long long nbits, long long *out_count);
int hnsw_mi355x_near_edges_results(void *handle, int *out_src, int *out_dst, float *out_dists, long long cap);
/* Counters of the by-id calls since creation or hnswdev_reset_stats / hnsw_mi355x_reset_stats, summed over the device contexts:
 * out[0] knn_query_by_id / exact_knn_query_by_id calls that reached a device, out[1] queries traversed on the device, out[2] of
 * those handed back to the host traversal, out[3] queries scanned, out[4] rows gathered (get_vectors' included), out[5] pairs
 * the scan skipped because the row was the query's own.  0, or -1 for a NULL argument. */
int hnsw_mi355x_by_id_info(void *handle, uint64_t out[6]);
/* RangeQuery with a GROUP FILTER PER QUERY: the graph traversal of hnsw_mi355x_range_query_at_layer, query i
 * filtered by { j < n_row_group : row_group[j] == query_group[i] }.  Per group g the lists of the queries with query_group == g
 * are byte for byte -- ids, distance bits, the order among equal distances -- what hnsw_mi355x_range_query_at_layer returns for
 * those queries with that set as allow_bits.  One device traversal serves every group.  Where the reference pops an empty heap
 * (range < 0) the whole call fails as the filtered call does: -1, "System.InvalidOperationException: Heap is empty", every array
 * NULL and every count 0.  A query whose group holds no graph id gets an empty list without a traversal when range >= 0.
 * Group arguments and their errors as hnsw_mi355x_knn_query_grouped; arrays as hnsw_range_query (hnsw_free_results).  NULL
 * handle and count <= 0: 0, nothing written.  Takes the handle exclusively; replaces the resident query set. */
int hnsw_mi355x_range_query_grouped(void *handle, const float *vectors, int count, int dim, float range, int layer, const int *row_group,
                                    long long n_row_group, const int *query_group, int n_groups, void **out_ids, void **out_dists, int *counts);
/* Counters of hnsw_mi355x_range_query_grouped on the primary context since hnsw_mi355x_reset_stats: out[0] calls that reached the
 * context, out[1] queries launched, out[2] queries answered without a job because their group holds no graph id, out[3] lists the
 * device left to the host (closures to partition, sort or replay, and hand-backs).  0, or -1 for a NULL argument. */
int hnsw_mi355x_range_grouped_info(void *handle, uint64_t out[4]);
/* The two range families with a TAG MASK PER QUERY (row_tags, query_tags and match as for the tagged k-NN calls
 * above: the word 0, an id past row_tags, a vacant slot and the mask 0 match nothing; at most 65 536 distinct masks).
 * hnsw_mi355x_range_query_tagged: the graph traversal of hnsw_mi355x_range_query_at_layer, query i filtered by the ids whose word
 * matches query_tags[i].  Per distinct mask m the lists of the queries with query_tags == m are byte for byte -- ids, distance
 * bits, the order among equal distances -- what hnsw_mi355x_range_query_at_layer returns for those queries with that set as
 * allow_bits.  One device traversal serves every mask; only the words of graph ids count.  Where the reference pops an empty heap
 * (range < 0) the whole call fails as the filtered call does: -1, "System.InvalidOperationException: Heap is empty", every array
 * NULL and every count 0.  A query whose mask matches no graph id gets an empty list without a traversal when range >= 0 (a NaN
 * range runs).  Arrays as hnsw_range_query (hnsw_free_results).  Primary context only.  Takes the handle exclusively; replaces
 * the resident query set.
 * hnsw_mi355x_exact_range_query_tagged: the flat scan of hnsw_mi355x_exact_range_query over the same candidates -- per distinct
 * mask the counts, ids, distance bits and ascending (distance, id) order of that call with the mask's ids as allow_bits, its rules
 * for the radius (NaN, +inf, -0.0, negative), its limit of 2^27 keys per query and its allocation contract unchanged, the lists in
 * the caller's query order.  A query whose mask has no candidate gets an empty list without a scan.  Always on the primary context.
 * Both: -1 with a message, every array NULL and every count 0: vectors, out_ids, out_dists, counts or query_tags NULL, dim <= 0
 * (System.ArgumentNullException); row_tags NULL or n_row_tags < 0 (System.ArgumentException); match other than 0 and 1, more than
 * 65 536 distinct masks -- the message names the index of the first mask beyond (System.ArgumentOutOfRangeException); for the
 * traversal a layer outside 0 .. the entry point's top layer on a non-empty index (System.IndexOutOfRangeException).  NULL handle
 * and count <= 0: 0, nothing written. */
int hnsw_mi355x_range_query_tagged(void *handle, const float *vectors, int count, int dim, float range, int layer, const uint32_t *row_tags,
                                   long long n_row_tags, const uint32_t *query_tags, int match, void **out_ids, void **out_dists, int *counts);
int hnsw_mi355x_exact_range_query_tagged(void *handle, const float *vectors, int count, int dim, float range, const uint32_t *row_tags,
                                         long long n_row_tags, const uint32_t *query_tags, int match, void **out_ids, void **out_dists, int *counts);
/* Counters of hnsw_mi355x_range_query_tagged on the primary context since hnsw_mi355x_reset_stats: out[0] calls that reached the
 * context, out[1] distinct masks of those calls, out[2] queries launched, out[3] queries answered without a job because their mask
 * matches no graph id, out[4] lists the device left to the host (closures to partition, sort or replay, and hand-backs), out[5]
 * closures of more than 2 048 entries that the device finished all the same (their allowed entries fit its table and none tie).
 * 0, or -1 for a NULL argument. */
int hnsw_mi355x_range_tagged_info(void *handle, uint64_t out[6]);
/* Counters of hnsw_mi355x_exact_range_query_tagged since hnsw_mi355x_reset_stats: out[0] calls that counted candidates on the
 * device, out[1] distinct masks of those calls, out[2] queries scanned, out[3] queries answered empty without a scan, out[4] ids
 * written into candidate lists, out[5] batches of masks scanned, out[6] lists of two or more entries ordered on the device, out[7]
 * lists ordered on the host, out[8] pieces scanned again with exact capacities.  0, or -1 for a NULL argument. */
int hnsw_mi355x_exact_range_tagged_info(void *handle, uint64_t out[9]);

/* Measurement aid: hnsw_mi355x_set_queries uploads a query set (count x dim) once; every later
 * hnsw_mi355x_knn_query_resident(k) is hnsw_knn_query on that set with the inputs already in HBM
 * (out arrays: count x k). */
int hnsw_mi355x_set_queries(void *handle, const float *queries, int count, int dim);
int hnsw_mi355x_knn_query_resident(void *handle, int k, int *out_ids, float *out_dists);
/* Rows of the query set currently resident (hnsw_knn_query leaves its own queries resident, hnsw_range_query leaves
 * none): the out arrays of hnsw_mi355x_knn_query_resident must hold this many rows of k. */
int hnsw_mi355x_resident_count(void *handle);

/* Graph introspection for parity checks (reads host state only). */
int hnsw_mi355x_count(void *handle);   /* HNSWIndex.Count: live items */
int hnsw_mi355x_length(void *handle);  /* slots ever allocated (ids are < length) */
/* HNSWIndex.Ids(): the live ids in ActiveSet order; returns Count. */
int hnsw_mi355x_active_ids(void *handle, int *out, int cap);
int hnsw_mi355x_entry_point(void *handle);
/* Row length fixed by the first add (or by the loaded snapshot); 0 before that. */
int hnsw_mi355x_dim(void *handle);
int hnsw_mi355x_node_max_layer(void *handle, int id);
/* Copies up to cap out-edge ids of (id, layer); returns the edge count or -1. */
int hnsw_mi355x_get_out_edges(void *handle, int id, int layer, int *out, int cap);
uint64_t hnsw_mi355x_graph_hash(void *handle);

/* HNSWIndex.GetInfo() (src/HNSWIndex/HNSWIndex.cs:192-197): HNSWInfo.LayerInfo (HNSWInfo.cs:18-43), one per layer 0 .. top, top = the
 * entry point's MaxLayer (GraphData.GetTopLayer).  A layer's members are the live ids with MaxLayer >= layer.  Out-degrees are the
 * lengths of the members' lists on the layer; in-degrees count the list entries u -> v between members, which is what the reference's
 * InEdges[layer] hold.  avg_*: the integer sum as int64, converted to double, divided by nodes_count (LINQ's Average).  *_median:
 * Median (HNSWInfo.cs:45-51): sorted[n / 2] for an odd count, (sorted[n / 2 - 1] + sorted[n / 2]) / 2 in integer arithmetic for an
 * even one.  Without AllowRemovals the four in-edge statistics and avg_in_edges are 0 (:39-42).
 * Computed on the device from the graph mirror in HBM: the adjacency lists are not copied back to the host. */
typedef struct hnsw_mi355x_layer_info {
    int32_t layer_id, nodes_count, max_out_edges, min_out_edges, max_in_edges, min_in_edges, out_edges_median, in_edges_median;
    double avg_out_edges, avg_in_edges;
} hnsw_mi355x_layer_info; /* 48 bytes */
/* Returns top + 1 and writes min(cap, top + 1) entries (cap smaller than that is no error: read the count, call again, as with
 * hnsw_mi355x_active_ids).  A NULL handle: 0.  An index with no live item: -1 with System.IndexOutOfRangeException in the message
 * (the reference indexes Nodes[-1], GraphData.GetTopLayer).  Other errors: -1 with a message.  Takes the handle exclusively; runs on
 * the device, on the primary context, whatever hnsw_mi355x_set_device_traversal says (the mirror is brought up to date first). */
int hnsw_mi355x_get_info(void *handle, hnsw_mi355x_layer_info *out, int cap);
/* HNSWIndex.GetConnectedComponentCounts() (HNSWIndex.cs:199-205, GraphNavigator.cs:331-419): per layer 0 .. top the number of weakly
 * connected components among the layer's members; an entry u -> v between two members joins them, whichever way it points.  Returns
 * top + 1 and writes min(cap, top + 1) counts; 0 for an empty index (the reference's empty array) and for a NULL handle; -1 with a
 * message on error.  Locking, device and context as hnsw_mi355x_get_info. */
int hnsw_mi355x_connected_component_counts(void *handle, int *out, int cap);
/* Counters of the two calls above on the primary context since hnsw_mi355x_reset_stats: out[0] layers summarised, out[1] layers whose
 * components were counted, out[2] list entries read (the members' out-degrees, summed by the kernels themselves), out[3] kernel
 * launches.  0, or -1 for a NULL argument. */
int hnsw_mi355x_graph_info_counters(void *handle, uint64_t out[4]);

/* Reachability from the entry point over OUT-edges, computed on the device from the graph mirror.  Every query --
 * KnnQuery, RangeQuery, their filtered and `layer` forms, MultiLayerKnnQuery -- starts at the entry point, descends over the out-lists
 * of the layers above and expands out-lists on its target layer; weak connectivity (the call above) says nothing about that.
 * An entry u -> v counts only between two members of the layer (live ids with MaxLayer >= layer).  For a seed set S, reach_L(S) is the
 * set of members reachable from the member seeds over such entries, seeds included, and the hop count of a member is its BFS
 * distance from them.  The chain, with ep the entry point and top its MaxLayer: F_top = reach_top({ep}), F_L = reach_L(F_{L+1}) for
 * L = top - 1 .. 0.  F_L contains every node a descent can arrive at on L and every node a search on L can expand, so a member of L
 * outside F_L is never a result of any query on L -- a NECESSARY condition for being found, not a sufficient one: a member of F_L may
 * still be missed by a greedy search.  hnsw_mi355x_exact_knn_query returns such items; no traversal does. */
typedef struct hnsw_mi355x_layer_reach {
    int32_t layer_id, nodes_count, seeds, reached, max_hops; /* members of the layer; |F_{L+1}| (1 on the top layer); |F_L|; the largest hop count in F_L */
} hnsw_mi355x_layer_reach; /* 20 bytes */
/* The chain for the layers 0 .. top: returns top + 1 and writes min(cap, top + 1) entries (the whole chain is computed whatever cap
 * is).  0 for an empty index and for a NULL handle; -1 with a message on error.  Locking, device and context as hnsw_mi355x_get_info. */
int hnsw_mi355x_reachability(void *handle, hnsw_mi355x_layer_reach *out, int cap);
/* The live members of `layer` outside F_layer, ascending: returns their number and writes min(cap, number) ids.  Only the reached set's
 * bitset (length / 8 bytes) comes back from the device.  layer outside 0 .. top on a non-empty index: -1 with a message.  An empty index
 * and a NULL handle: 0. */
int hnsw_mi355x_unreachable_ids(void *handle, int layer, int *out, int cap);
/* out[id] for ids < hnsw_mi355x_length: >= 0 the hop count of id in F_layer, -1 a member of `layer` outside F_layer, -2 no member of
 * the layer (removed, or MaxLayer < layer).  Returns length and writes min(cap, length) entries.  Errors as above. */
int hnsw_mi355x_hop_counts(void *handle, int layer, int *out, int cap);
/* Counters of the three calls above on the primary context since hnsw_mi355x_reset_stats: out[0] layers walked, out[1] rounds (launches
 * of the expansion kernel: one per BFS level), out[2] list entries the expansions read (counted by the kernel: the out-degrees of the
 * reached members, each expanded once), out[3] kernel launches.  0, or -1 for a NULL argument. */
int hnsw_mi355x_graph_reach_counters(void *handle, uint64_t out[4]);

/* Repair of reachability: links the items that hnsw_mi355x_unreachable_ids reports into the lists of their nearest
 * reached members, on the device, so that the chain above reaches them.  OPT-IN, and the only call besides Add and Remove that edits
 * neighbour lists: a graph it has changed is no longer an outcome of the reference's Add.  It stays a well-formed graph -- every list
 * within MaxEdges(layer), no duplicate, no self entry, members only -- so its snapshots load everywhere.  It promises reachability,
 * not recall: a reached item can still be missed by a greedy search, and an evicted entry is an edge some search may have used.
 * Layers are processed from the entry point's top layer down; the seeds of a layer are the final reached set of the layer above.  On a
 * layer, up to max_rounds times: (1) the chain's BFS; U = the members without a hop count, ascending; none: the layer is done.  (2) For
 * each u of U the `cands` nearest REACHED members: the ids hnsw_mi355x_exact_knn_query returns for the stored row of u with k = cands
 * and this round's reached set as allow-set.  (3) For each candidate v a slot code from v's list as it stands: count(v) if the list is
 * below MaxEdges(layer) (an append); otherwise the evictable entry of largest (distance to v, slot), where entry s -> w is evictable
 * iff w is a member with 0 <= hop[w] <= hop[v] and the distance is no NaN; -1 if there is none.  (4) U ascending: u takes its first
 * candidate with a code whose list no other u has taken in this round; slot `code` of that list becomes u.  A round that applies
 * nothing ends the layer.  An evicted entry v -> w has hop[w] <= hop[v], and every reached non-seed keeps an in-edge from a node one
 * hop nearer, which is never evictable: what was reached before a round is reached after it, in no more hops. */
typedef struct hnsw_mi355x_layer_repair {
    int32_t layer_id, unreachable_before, linked, evicted, rounds, unreachable_after; /* members outside F_L at the first BFS; u linked; ... of them by an eviction; rounds that found members outside F_L; members outside F_L at the end */
} hnsw_mi355x_layer_repair; /* 24 bytes */
/* Returns top + 1 and writes min(cap, top + 1) entries (every layer is repaired whatever cap is).  cands and max_rounds: 1 .. 64 each
 * (8 and 8 are the bindings' defaults), outside that -1 with a message.  0 for an empty index and for a NULL handle; -1 with a message
 * on error; a device failure after the first list was changed fails the index, as for Remove.  Exclusive, on the primary context, on
 * the device whatever hnsw_mi355x_set_device_traversal says. */
int hnsw_mi355x_repair_reachability(void *handle, int cands, int max_rounds, hnsw_mi355x_layer_repair *out, int cap);
/* Counters of the call above on the primary context since hnsw_mi355x_reset_stats: out[0] rounds that ran the proposal kernel, out[1]
 * (u, candidate) pairs it judged, out[2] distances it measured (counted by the kernel), out[3] lists patched.  0, or -1 for a NULL argument. */
int hnsw_mi355x_graph_repair_counters(void *handle, uint64_t out[4]);

/* HNSWIndex.Serialize(filePath) / HNSWIndex.Deserialize(distFnc, filePath)
 * (src/HNSWIndex/HNSWIndex.cs:210-229): the reference's protobuf-net snapshot of
 * HNSWIndexSnapshot<float[],float> (HNSWIndexSnapshot.cs:12-16, GraphDataSnapshot.cs:13-35,
 * Node.cs:9-36, HNSWParameters.cs:12-55).  The reference's C ABI does not export these; its C#
 * API has them.  serialize: 0 / -1.  deserialize: a handle for hnsw_* calls, or 0 with the
 * message in hnsw_get_last_error_utf8; HNSW parameters come from the file, the pending
 * hnsw_mi355x_set_* backend knobs are consumed as by hnsw_create. */
int hnsw_mi355x_serialize(void *handle, const char *path_utf8);
void *hnsw_mi355x_deserialize(const char *distance_metric_utf8, const char *path_utf8);
/* Loading a graph that was built elsewhere -- by another replica of this index (multi-GPU: build once, broadcast,
 * import; hnswindex.net_amd/distributed.py::replicate_index) or by a host that owns one -- into a handle that holds
 * nothing yet.  hnsw_mi355x_import_nodes: rows (n x dim float32, id == row index), levels[i] = MaxLayer of node i
 * (Node.cs:27), the entry point (GraphData.EntryPointId); then one hnsw_mi355x_import_edges per layer 0..max(levels)
 * in the layout of hnsw_mi355x_export_edges (counts ignored where the node lacks the layer; ids in EdgeList order,
 * Node.cs:31-107).  Lists are validated (ids in range and on that layer, no duplicates, length <= MaxEdges(layer)).
 * Afterwards the index behaves as if it had inserted the n items itself: the level generator is advanced by n draws
 * (GraphData.cs:211-219), so later Adds continue exactly as on the index the graph came from.  0 / -1. */
int hnsw_mi355x_import_nodes(void *handle, const float *rows, int n, int dim, const int *levels, int entry_point);
int hnsw_mi355x_import_edges(void *handle, int layer, const int *counts, const int *edges, int stride);
/* Bulk forms: levels of nodes [0, min(count, cap)); returns count. */
int hnsw_mi355x_export_levels(void *handle, int *out, int cap);
/* counts[id] = out-degree of (id, layer), -1 where the node has no such layer;
 * edges[id*stride ..] = the ids, in adjacency order.  Returns count or -1. */
int hnsw_mi355x_export_edges(void *handle, int layer, int *counts, int *edges, int stride, int cap);

/* Counters of the index's device context (see hnswdev_stats). */
struct hnswdev_stats;
int hnsw_mi355x_get_stats(void *handle, struct hnswdev_stats *out);
int hnsw_mi355x_reset_stats(void *handle);
int hnsw_mi355x_set_profiling(void *handle, int enabled);

/* =====================================================================================
 * (B) Inner boundary: batched candidate-distance backend
 *     replaces GraphData.Distance(int, TVector) / Distance(int, int)
 *     (src/HNSWIndex/GraphData.cs:255-277) at the 14 call sites of SURVEY.md 8a.
 * ===================================================================================== */

/* 0-2: the reference's three float metrics (HNSWIndexExports.cs:47-60).  3: squared Euclidean distance on
 * int8-quantised rows with one float scale per row (BASELINE config 5; no reference counterpart) -- rows and
 * queries still cross the boundary as float32 and are quantised on the device, q = rint(x / scale), scale =
 * max|x| / 127; the distance is that of the dequantised vectors, computed from the exact int32 dot product
 * (metric name "sq_euclid_i8" for hnsw_create).  4, 5: sq_euclid / ucosine on rows STORED as IEEE binary16 ("sq_euclid_f16",
 * "ucosine_f16"): a row is rounded element by element (nearest even, subnormals kept, beyond 65504 -> inf: numpy's
 * astype(float16)) when it is uploaded, queries stay float32, and every distance is metric 0 / 2 on the rounded rows, bit for
 * bit; hnswdev_download_rows returns the rounded rows as floats, hnswdev_stats.row_bytes is 2 * dim. */
enum { HNSWDEV_SQ_EUCLID = 0, HNSWDEV_COSINE = 1, HNSWDEV_UCOSINE = 2, HNSWDEV_SQ_EUCLID_I8 = 3, HNSWDEV_SQ_EUCLID_F16 = 4, HNSWDEV_UCOSINE_F16 = 5 };

typedef struct hnswdev_stats {
    uint64_t launches;      /* distance-kernel launches */
    uint64_t evals;         /* distance evaluations (one candidate row read each) */
    uint64_t timed_launches;/* launches bracketed by HIP events (profiling on) */
    uint64_t timed_evals;   /* evaluations inside those launches */
    double kernel_ms;       /* sum of HIP-event durations of the timed launches */
    uint64_t row_bytes;     /* dim * sizeof(float) (2 * dim for the _f16 metrics): algorithmic bytes per evaluation */
    /* graph-resident search kernel (traversal on the device) */
    uint64_t search_launches;
    uint64_t search_evals;        /* distance evaluations inside those launches (device-counted) */
    uint64_t search_timed_launches;
    uint64_t search_timed_evals;
    double search_kernel_ms;      /* HIP-event durations of the timed search launches */
    uint64_t search_overflows;    /* traversals handed back to the lock-step path */
    uint64_t search_repeats;      /* traversals repeated on the device with the exact two-heap variant (equal distances) */
    /* Add's two halves, counted separately as well (they are also part of the search_* totals above):
     * graph_insert_search_kernel (descent + per-layer search + RelativeNeighborPruning) and the link half
     * (link_plan / link_offsets / link_order + graph_link_kernel: appends and PruneOverflow) */
    uint64_t insert_launches, insert_evals, insert_timed_launches, insert_timed_evals;
    double insert_kernel_ms;
    uint64_t link_launches, link_evals, link_timed_launches, link_timed_evals;
    double link_kernel_ms;
    uint64_t visited_hash_launches; /* traversal launches whose visited sets were per-wave hash tables (graphs above 4M nodes) */
    /* graph_range_kernel (RangeQuery on the device; also part of the search_* totals) */
    uint64_t range_launches, range_evals, range_timed_launches, range_timed_evals;
    double range_kernel_ms;
    uint64_t range_handbacks;       /* range traversals handed back (more results than a wave's list holds, visited table full) */
    uint64_t replica_bytes;         /* bytes this context received from another one (rows + graph mirror of a replica) */
    uint64_t tie_windows;           /* searches that met open candidates of equal distance and were shown to be order-free (no exact re-run) */
    uint64_t peer_direct_copies;    /* replica / query-set copies between contexts whose devices have peer access enabled (one device: counted here) */
    uint64_t peer_staged_copies;    /* ... and those the runtime had to stage through host memory (no peer access between the two devices) */
    uint64_t lat_launches;          /* traversal launches that ran the latency variant of their kernel (fewer jobs than its resident waves) */
    uint64_t range_device_ordered;  /* RangeQuery result lists (of two or more entries) whose ORDER the device completed: ranked, and replayed where distances tie */
    uint64_t range_host_ordered;    /* ... and those handed to the host for it (beyond 2 048 entries, a -0 distance, a replay the device gave up) */
    uint64_t insert_tie_reruns;     /* Add searches answered by the exact two-heap traversal because equal distances could show in what the insert
                                     * consumes in order (Span.Sort among equal keys, Heuristic.cs:22; heap layout at the far end of the list): the inserts
                                     * whose outcome rests on BCL tie behaviour this build restates from memory -- the "parity unpinned" exposure as a number
                                     * (also counted in search_repeats) */
    uint64_t lean_launches;         /* traversal launches that ran the lean form of their kernel (no visited sets: the default wherever lists hold <= 64 ids and rows <= 1 KB) */
    /* graph_multilayer_kernel (MultiLayerKnnQuery's chains; its launches and evaluations are also part of the search_* totals) */
    uint64_t multilayer_launches;   /* launches */
    uint64_t multilayer_jobs;       /* chains given to the device (one per query) */
    uint64_t multilayer_handbacks;  /* ... of which handed back whole (NaN / -0 distance, candidate heap full, visited table crowded) */
    /* the flat scan (hnswdev_exact_knn: exact_scan_kernel + exact_merge_kernel; no traversal, so NOT part of the search_* totals) */
    uint64_t exact_launches;        /* scan launches (one per round of queries) */
    uint64_t exact_evals;           /* (query, row) pairs measured: queries x rows that are live and allowed, exactly */
    uint64_t exact_timed_launches, exact_timed_evals;
    double exact_kernel_ms;         /* HIP-event durations of the timed rounds (scan + merge) */
} hnswdev_stats;

/* All return 0 on success, < 0 on error (message via hnswdev_ctx_last_error / hnswdev_last_error).
 * Calls on ONE context are serialised by the library (a mutex per context); different contexts
 * run concurrently. */

/* Creates a context on HIP device `device` holding up to `capacity` rows of `dim` float32
 * in one contiguous row-major HBM matrix (id == row index, GraphData.cs:95-115). */
int hnswdev_create(int device, int dim, int metric, long long capacity, void **ctx);
int hnswdev_destroy(void *ctx);
/* Grows the matrix (contents preserved); the counterpart of the doubling resize at
 * GraphData.cs:98-111. */
int hnswdev_reserve(void *ctx, long long capacity);
/* Copies rows [first_id, first_id+n) host -> HBM (and, for cosine, computes each row's
 * f32 squared norm in the reference's lane order and its double sqrt on the device). */
int hnswdev_upload_rows(void *ctx, int first_id, int n, const float *rows);
/* Reads rows back (parity checks). */
int hnswdev_download_rows(void *ctx, int first_id, int n, float *rows);

/* Uploads the query set of a batch of searches ONCE (nq x dim host floats; for cosine the norms are
 * computed on the device); records then name a query by its row index in this set.  Replaces the
 * previous resident set. */
int hnswdev_set_queries(void *ctx, const float *queries, int nq);

/* ---- the batched step, asynchronous and double-buffered ---------------------------------------
 * This is what replaces the scalar delegate inside the traversal loops (GraphNavigator.cs:70,
 * :163, :231; Heuristic.cs:34; GraphConnector.cs:233): the host advances MANY traversals together;
 * each step every live traversal states one record -- which vector (a resident query, or a stored
 * row) against which candidate rows -- and ONE launch evaluates all of them.
 *
 * The context owns two buffer sets (set = 0 | 1) in pinned host memory with an HBM mirror; they
 * are (re)allocated only when nslots grows or stride changes, never per step, and no other call
 * moves them: the pointers stay valid until the next hnswdev_step_buffers for that set that asks
 * for more (or hnswdev_destroy).  Layout of set `set`:
 *     rec [s * (stride + 2) + 0]      = cnt   number of candidate ids of slot s (0: idle slot)
 *     rec [s * (stride + 2) + 1]      = qidx  >= 0: resident query index;  < 0: ~row_id (id<->id)
 *     rec [s * (stride + 2) + 2 ...]  = ids   candidate row ids, cnt <= stride
 *     dist[s * stride + c]            = metric(row[ids[c]], that vector) after hnswdev_step_wait
 * hnswdev_step_submit enqueues ONE host->HBM copy of the used records, ONE kernel and ONE copy of
 * the distances back, on the context's stream, and returns; hnswdev_step_wait blocks until that
 * set's distances have landed.  While one set is in flight the host consumes / fills the other.
 * A record naming a row or query that was never uploaded is not dereferenced: its distances come
 * back NaN and hnswdev_step_wait returns -1. */
int hnswdev_step_buffers(void *ctx, int set, int nslots, int stride, int **rec, float **dist);
int hnswdev_step_submit(void *ctx, int set, int nslots_used);
int hnswdev_step_wait(void *ctx, int set);

/* Synchronous conveniences over the same two sets (nothing is allocated per call once they exist):
 * Distance(int a, TVector b) for many (query, candidate-list) pairs at once:
 * out[j] = metric(row[cand_ids[j]], queries[i]) for cand_offsets[i] <= j < cand_offsets[i+1].
 * queries: nq x dim host floats, uploaded as the resident set -- or NULL to use the set already
 * resident (hnswdev_set_queries), so that a batch of searches uploads its queries once;
 * cand_offsets: nq+1 ints. */
int hnswdev_dist_query_batch(void *ctx, const float *queries, int nq, const int *cand_offsets, const int *cand_ids,
                             float *out);
/* Distance(int a, int b): out[j] = metric(row[a_ids[j]], row[b_ids[j]]); synchronous. */
int hnswdev_dist_pair_batch(void *ctx, const int *a_ids, const int *b_ids, int n, float *out);

/* ---- graph-resident traversal: SearchLayerQuery + FindEntryPointQuery
 *      (src/HNSWIndex/GraphNavigator.cs:39-82,194-256) for a batch of queries in one launch ---- */

/* Describes the host graph to the context: n nodes, MaxEdges = max_edges, levels[i] = MaxLayer of
 * node i (Node.cs:27).  Then one hnswdev_graph_set_layer per layer 0..max(levels), then commit. */
int hnswdev_graph_begin(void *ctx, int n, int max_edges, const int *levels);
/* counts[i] = OutEdges[layer].Count of node i (ignored where levels[i] < layer);
 * edges[i*stride .. i*stride+counts[i]) = its ids in EdgeList order (Node.cs:31-107). */
int hnswdev_graph_set_layer(void *ctx, int layer, const int *counts, const int *edges, int stride);
/* Uploads the staged graph to HBM (replaces the previous one). */
int hnswdev_graph_commit(void *ctx);
/* KnnQuery for nq queries (nq x dim floats) from entry point `entry_point` (GraphData.EntryPoint):
 * beam width k_beam = max(MinNN, k) (HNSWIndex.cs:115), first k_out results of the stable distance
 * order (HNSWIndex.cs:121) into out_ids / out_dists (nq x k_out, padded with -1 / NaN).
 * out_flags[i] = 1: query i met a case the device path hands back (candidate heap beyond its
 * capacity, NaN or -0 distance) -- evaluate it with hnswdev_dist_query_batch instead. */
int hnswdev_knn_search(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int *out_ids,
                       float *out_dists, int *out_flags);
/* hnswdev_knn_search with an allow-set (SearchLayerQuery's filterFnc, GraphNavigator.cs:194-256): allow_bits / nbits as for
 * hnsw_mi355x_knn_query_filtered (a NULL allow_bits or nbits < 0: -1).  Runs the exact two-heap traversal with the filter
 * (graph_search_filtered_kernel); out_flags[i] = 1: handed back as above (a selective filter grows the candidate heap). */
int hnswdev_knn_search_filtered(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, const uint32_t *allow_bits,
                                long long nbits, int *out_ids, float *out_dists, int *out_flags);

/* RangeQuery for nq queries from `entry_point`: FindEntryPointQuery + SearchLayerRange at layer 0
 * (HNSWIndex.cs:144-156, GraphNavigator.cs:262-325), no filter.  out_counts[i] = results of query i, kept in the
 * context until the next range search and copied out by hnswdev_range_results: concatenated in query order, each
 * query's results in RangeQuery's order -- ascending by distance, results of EQUAL distance in the order of the
 * reference's heap array (replayed on the committed graph) -- out_ids / out_dists hold sum(out_counts) entries.
 * out_flags[i] = 1: handed back (count 0; on graphs above 4M nodes, a traversal that outgrows its visited table):
 * evaluate it with hnswdev_dist_query_batch instead. */
int hnswdev_range_search(void *ctx, const float *queries, int nq, int entry_point, float range, int *out_counts, int *out_flags);
/* hnswdev_range_search with an allow-set (the bitset of hnsw_mi355x_range_query_filtered; a NULL allow_bits or nbits < 0: -1):
 * only allowed results are counted and returned, through hnswdev_range_results, in the reference's order.  Where the reference
 * throws (range < 0, see hnsw_mi355x_range_query_filtered) it returns -1 with "System.InvalidOperationException: Heap is empty". */
int hnswdev_range_search_filtered(void *ctx, const float *queries, int nq, int entry_point, float range, const uint32_t *allow_bits,
                                  long long nbits, int *out_counts, int *out_flags);
int hnswdev_range_results(void *ctx, int *out_ids, float *out_dists);
/* The searches above on the lists of `layer` (0 .. the entry point's level; outside: -1): the descent stops above it.
 * allow_bits == NULL: no filter (nbits ignored).  A layer per call, not a setting of the context. */
int hnswdev_knn_search_at_layer(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int layer,
                                const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists, int *out_flags);
int hnswdev_range_search_at_layer(void *ctx, const float *queries, int nq, int entry_point, float range, int layer, const uint32_t *allow_bits,
                                  long long nbits, int *out_counts, int *out_flags);
/* hnswdev_knn_search_at_layer with a group filter per query (graph_search_grouped_kernel; the labels of
 * hnsw_mi355x_knn_query_grouped): query i is answered from the graph ids j < n_row_group with row_group[j] == query_group[i], row by
 * row what hnswdev_knn_search_at_layer returns for it with that group's ids as the allow-set.  A query whose group holds no graph id:
 * a padded row, flag 0, no job.  out_flags[i] = 1: handed back, as hnswdev_knn_search_filtered.  -1 with a message and no launch:
 * a NULL array, n_row_group < 0, n_groups outside 1 .. 65 536, a query_group value outside [0, n_groups), an entry point outside the
 * graph, k_out < 1 or k_beam < k_out, a layer the entry point does not have. */
int hnswdev_knn_search_grouped(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int layer, const int *row_group,
                               long long n_row_group, const int *query_group, int n_groups, int *out_ids, float *out_dists, int *out_flags);
/* out[0 .. 3] as hnsw_mi355x_knn_grouped_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_knn_grouped_info(void *ctx, uint64_t out[4]);
/* hnswdev_knn_search_at_layer with a tag mask per query (graph_search_tagged_kernel; the words, masks and match of
 * hnsw_mi355x_knn_query_tagged): query i is answered from the graph ids j < n_row_tags whose word matches query_tags[i], row by row
 * what hnswdev_knn_search_at_layer returns for it with those ids as the allow-set.  A query whose mask has no candidate: a padded
 * row, flag 0, no job.  out_flags[i] = 1: handed back, as hnswdev_knn_search_filtered.  -1 with a message and no launch: a NULL
 * array, n_row_tags < 0, match other than 0 and 1, more than 65 536 distinct masks, an entry point outside the graph, k_out < 1 or
 * k_beam < k_out, a layer the entry point does not have. */
int hnswdev_knn_search_tagged(void *ctx, const float *queries, int nq, int entry_point, int k_beam, int k_out, int layer, const uint32_t *row_tags,
                              long long n_row_tags, const uint32_t *query_tags, int match, int *out_ids, float *out_dists, int *out_flags);
/* out[0 .. 4] as hnsw_mi355x_knn_tagged_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_knn_tagged_info(void *ctx, uint64_t out[5]);
/* hnswdev_exact_knn_grouped with a tag mask per query (the words, masks and match of hnsw_mi355x_exact_knn_query_tagged) over the
 * uploaded rows j < min(n_rows, uploaded, n_row_tags); queries == NULL: the resident query set.  -1 with a message and no scan: a
 * NULL array, n_row_tags < 0, match other than 0 and 1, more than 65 536 distinct masks, k < 1 or k > 1024. */
int hnswdev_exact_knn_tagged(void *ctx, const float *queries, int nq, long long n_rows, int k, const uint32_t *row_tags, long long n_row_tags,
                             const uint32_t *query_tags, int match, int *out_ids, float *out_dists);
/* out[0 .. 5] as hnsw_mi355x_exact_tagged_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_exact_tagged_info(void *ctx, uint64_t out[6]);
/* Query by stored id on a context.
 * hnswdev_gather_rows: out[i] = the uploaded row ids[i] as dim floats, hnswdev_download_rows' values for the row kind, gathered in
 * one launch and copied back in one copy.  ids may repeat, in any order; an id outside the uploaded rows gives a row of zeros.
 * n <= 0: 0, nothing is written. */
int hnswdev_gather_rows(void *ctx, const int *ids, int n, float *out);
/* hnswdev_knn_search_at_layer whose query i is the uploaded row ids[i] -- made resident on the device as hnswdev_set_queries
 * would make hnswdev_gather_rows' row -- answered from every graph id but ids[i] (graph_search_self_kernel).  Row i is byte for
 * byte hnswdev_knn_search_filtered's at that layer with that allow-set.  out_flags as there (1: handed back).  An id that is no
 * uploaded row of a graph node is an error that names it. */
int hnswdev_knn_search_by_id(void *ctx, const int *ids, int nq, int entry_point, int k_beam, int k_out, int layer, int *out_ids, float *out_dists,
                             int *out_flags);
/* hnswdev_exact_knn whose query i is the uploaded row ids[i] and whose candidates are hnswdev_exact_knn's minus ids[i]; the scan's
 * sink drops that pair, which is not counted in exact_evals.  The resident set stays what it was.  An id that is no uploaded row is
 * an error that names it. */
int hnswdev_exact_knn_by_id(void *ctx, const int *ids, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits, int *out_ids,
                            float *out_dists);
/* hnswdev_exact_range whose query i is the uploaded row ids[i] and whose candidates are hnswdev_exact_range's minus ids[i]
 * (exact_scan_kernel's ExactRangeSelf sink); the lists are kept and fetched as there (hnswdev_exact_range_results).  The resident
 * set stays what it was.  An id that is no uploaded row is an error that names it, before any launch. */
int hnswdev_exact_range_by_id(void *ctx, const int *ids, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits,
                              int *out_counts);
/* The scan behind hnsw_mi355x_duplicate_groups: the members are the uploaded rows [0, n_rows) that allow_bits allows, out_labels
 * has min(n_rows, uploaded rows) entries, out_info as there.  Neither the resident set nor what hnswdev_exact_range_results has
 * pending is touched. */
int hnswdev_exact_range_groups(void *ctx, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels,
                               uint64_t out_info[4]);
/* The scans behind hnsw_mi355x_density_clusters: the members are the uploaded rows [0, n_rows) that allow_bits allows, out_labels
 * (NULL: the counts alone) and out_counts have min(n_rows, uploaded rows) entries, out_info as there.  min_samples < 1: -1 with a
 * message.  Neither the resident set nor what hnswdev_exact_range_results has pending is touched. */
int hnswdev_exact_range_density(void *ctx, long long n_rows, float range, int min_samples, const uint32_t *allow_bits, long long nbits, int *out_labels,
                                int *out_counts, uint64_t out_info[8]);
/* The calls behind hnsw_mi355x_graph_duplicate_groups / hnsw_mi355x_near_edges, on the context's own rows and the graph it was given
 * (hnswdev_graph_begin .. _commit): the members are the uploaded rows [0, n_rows) that allow_bits allows and that are nodes of the
 * graph; out_labels has min(n_rows, uploaded rows) entries, out_info as there.  hnswdev_graph_near_edges counts and keeps,
 * hnswdev_graph_near_edges_results fetches (cap below the count kept: -1 with a message).  No graph committed while n_rows > 0 rows
 * are uploaded: -1.  Neither the resident set nor what hnswdev_exact_range_results has pending is touched. */
int hnswdev_graph_edge_groups(void *ctx, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, int *out_labels,
                              uint64_t out_info[5]);
int hnswdev_graph_near_edges(void *ctx, long long n_rows, float range, const uint32_t *allow_bits, long long nbits, long long *out_count);
int hnswdev_graph_near_edges_results(void *ctx, int *out_src, int *out_dst, float *out_dists, long long cap);
/* out[0 .. 5] as hnsw_mi355x_by_id_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_by_id_info(void *ctx, uint64_t out[6]);
/* Measurement aid: the HIP-event time, in ms, of the tagged calls' list-building kernels (count, offsets, fill) on this context
 * while profiling is on; zeroed by hnswdev_reset_stats. */
int hnswdev_tag_list_ms(void *ctx, double *out_ms);
/* hnswdev_range_search_at_layer with a group filter per query (range_sort_grouped_kernel behind graph_range_kernel): query i is
 * answered as with the allow-set { id : row_group[id] == query_group[i] }; only the labels of graph ids count.  out_counts /
 * out_flags and the fetch with hnswdev_range_results as hnswdev_range_search_filtered; a query whose group holds no graph id gets
 * count 0, flag 0 and no job when range >= 0.  -1 with a message: a NULL array, n_row_group < 0, n_groups outside 1 .. 65 536, a
 * query_group value outside [0, n_groups), an entry point outside the graph, a layer it does not have, the empty-heap failure. */
int hnswdev_range_search_grouped(void *ctx, const float *queries, int nq, int entry_point, float range, int layer, const int *row_group,
                                 long long n_row_group, const int *query_group, int n_groups, int *out_counts, int *out_flags);
/* out[0 .. 3] as hnsw_mi355x_range_grouped_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_range_grouped_info(void *ctx, uint64_t out[4]);
/* hnswdev_range_search_at_layer with a tag mask per query (range_sort_tagged_kernel behind graph_range_kernel; the words, masks and
 * match of hnsw_mi355x_range_query_tagged): query i is answered as with the allow-set { id : row_tags[id] matches query_tags[i] };
 * only the words of graph ids count, and which masks have a candidate among them is counted on the device.  out_counts / out_flags
 * and the fetch with hnswdev_range_results as hnswdev_range_search_filtered; a query whose mask has no candidate gets count 0,
 * flag 0 and no job when range >= 0.  -1 with a message: a NULL array, n_row_tags < 0, match other than 0 and 1, more than 65 536
 * distinct masks, an entry point outside the graph, a layer it does not have, the empty-heap failure. */
int hnswdev_range_search_tagged(void *ctx, const float *queries, int nq, int entry_point, float range, int layer, const uint32_t *row_tags,
                                long long n_row_tags, const uint32_t *query_tags, int match, int *out_counts, int *out_flags);
/* out[0 .. 5] as hnsw_mi355x_range_tagged_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_range_tagged_info(void *ctx, uint64_t out[6]);
/* MultiLayerKnnQuery's chains (graph_multilayer_kernel), one job per query: layers min(top, max_layer) .. min_layer with beam k
 * (k >= 2), top = entry_point's level; semantics of hnsw_mi355x_multilayer_knn_query.  Returns the slot count min(top, max_layer) + 1
 * (0 for max_layer == -1), or -1 (max_layer < -1, min_layer < 0, layers_cap below the count).  out_ids / out_dists:
 * [nq][layers_cap][k - 1]; out_flags[i] = 1: query i was handed back whole (its slots hold nothing to rely on) -- evaluate it
 * with hnswdev_dist_query_batch instead. */
int hnswdev_multilayer_search(void *ctx, const float *queries, int nq, int entry_point, int k, int max_layer, int min_layer, int layers_cap,
                              int *out_ids, float *out_dists, int *out_flags);

int hnswdev_sync(void *ctx);
int hnswdev_set_profiling(void *ctx, int enabled);
/* The flat scan behind hnsw_mi355x_exact_knn_query: per query the k rows of smallest (distance, id) among the uploaded rows
 * [0, n_rows) that allow_bits allows (NULL: all; else nbits bits, ids >= nbits not allowed), ascending, padded with -1 / NaN.
 * No graph and no active set are involved.  n_rows and nbits beyond what was uploaded are clamped: a row that does not exist is
 * never dereferenced.  queries == NULL: the resident set (hnswdev_set_queries); otherwise the queries go to a buffer of the
 * scan's own and the resident set stays.  nbits is ignored when allow_bits is NULL.  1 <= k <= 1024.  hnswdev_stats.exact_evals is
 * counted by the scan kernel itself. */
int hnswdev_exact_knn(void *ctx, const float *queries, int nq, long long n_rows, int k, const uint32_t *allow_bits, long long nbits,
                      int *out_ids, float *out_dists);
/* The flat scan behind hnsw_mi355x_exact_range_query: hnswdev_exact_knn's candidates, queries (NULL: the resident set) and
 * distances; out_counts[i] = the candidates of query i with distance <= range.  The lists -- each ascending by (distance, id) --
 * are kept in the context, concatenated in query order, until the next hnswdev_exact_range and are copied out by
 * hnswdev_exact_range_results (out_ids / out_dists hold sum(out_counts) entries).  They live in buffers of their own: what
 * hnswdev_range_results has pending is not disturbed.  -1: every count is 0 and nothing is kept. */
int hnswdev_exact_range(void *ctx, const float *queries, int nq, long long n_rows, float range, const uint32_t *allow_bits, long long nbits,
                        int *out_counts);
int hnswdev_exact_range_results(void *ctx, int *out_ids, float *out_dists);
/* out[0 .. 3] as hnsw_mi355x_exact_range_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_exact_range_info(void *ctx, uint64_t out[4]);
/* The flat scan behind hnsw_mi355x_exact_knn_query_grouped: hnswdev_exact_knn with a candidate set per query.  The candidates of
 * query i are the uploaded rows j < min(n_rows, n_row_group) with row_group[j] == query_group[i] (n_rows and n_row_group beyond
 * what was uploaded are clamped); no active set is involved.  row_group values outside [0, n_groups) are in no group; a
 * query_group value outside it, row_group == NULL, n_row_group < 0 and n_groups outside 1 .. 65 536 are -1 with a message and
 * nothing written.  queries == NULL: the resident set, as in hnswdev_exact_knn.  The groups' id lists are built on the device from
 * row_group and are unordered; the result does not depend on their order. */
int hnswdev_exact_knn_grouped(void *ctx, const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group,
                              const int *query_group, int n_groups, int *out_ids, float *out_dists);
/* The flat scan behind hnsw_mi355x_exact_knn_query_collapsed: hnswdev_exact_knn (its candidates, allow_bits and queries == NULL)
 * with at most per_group results per value of row_group[id].  n_row_group must be at least min(n_rows, uploaded rows): every
 * candidate id needs a label; fewer, row_group == NULL, per_group outside [1, k] and k > 1024 are -1 with a message and nothing
 * written.  The labels are uploaded once per call. */
int hnswdev_exact_knn_collapsed(void *ctx, const float *queries, int nq, long long n_rows, int k, const int *row_group, long long n_row_group,
                                int per_group, const uint32_t *allow_bits, long long nbits, int *out_ids, float *out_dists);
/* out[0 .. 3] as hnsw_mi355x_exact_collapsed_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_exact_collapsed_info(void *ctx, uint64_t out[4]);
/* out[0 .. 3] as hnsw_mi355x_exact_grouped_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_exact_grouped_info(void *ctx, uint64_t out[4]);
/* Measurement aid: *out_ms = the HIP-event time, in milliseconds, of the list-building kernels (count, offsets, place) of the
 * hnswdev_exact_knn_grouped calls made while profiling was on (hnswdev_set_profiling) since hnswdev_reset_stats.  The scan and the
 * merge of those calls are in hnswdev_stats.exact_kernel_ms.  0, or -1 for a NULL argument. */
int hnswdev_exact_grouped_list_ms(void *ctx, double *out_ms);
/* The flat scan behind hnsw_mi355x_exact_range_query_grouped: hnswdev_exact_range with hnswdev_exact_knn_grouped's group arguments
 * (queries == NULL: the resident set, gathered into the call's order on the device).  out_counts[i]: query i's number of results;
 * the lists are kept like hnswdev_exact_range's, in the caller's query order, and fetched with hnswdev_exact_range_results.  The
 * list-building kernels' time counts in hnswdev_exact_grouped_list_ms.  -1: nothing is kept and every count is 0. */
int hnswdev_exact_range_grouped(void *ctx, const float *queries, int nq, long long n_rows, float range, const int *row_group, long long n_row_group,
                                const int *query_group, int n_groups, int *out_counts);
/* out[0 .. 3] as hnsw_mi355x_exact_range_grouped_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_exact_range_grouped_info(void *ctx, uint64_t out[4]);
/* The flat scan behind hnsw_mi355x_exact_range_query_tagged: hnswdev_exact_range with hnswdev_exact_knn_tagged's tag arguments and
 * batches of masks (queries == NULL: the resident set, which stays untouched).  out_counts[i]: query i's number of results; the
 * lists are kept like hnswdev_exact_range's, in the caller's query order whatever the batches were, and fetched with
 * hnswdev_exact_range_results.  When no query's mask has a candidate nothing is launched.  -1 with a message (a NULL array,
 * n_rows < 0, n_row_tags < 0, match other than 0 and 1, more than 65 536 distinct masks): nothing is kept and every count is 0. */
int hnswdev_exact_range_tagged(void *ctx, const float *queries, int nq, long long n_rows, float range, const uint32_t *row_tags, long long n_row_tags,
                               const uint32_t *query_tags, int match, int *out_counts);
/* out[0 .. 8] as hnsw_mi355x_exact_range_tagged_info, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_exact_range_tagged_info(void *ctx, uint64_t out[9]);
/* hnsw_mi355x_get_info / hnsw_mi355x_connected_component_counts for ONE layer of the committed graph mirror of a context.
 * live_bits == NULL: every node of the mirror is live; otherwise a bitset of nbits bits in the allow-sets' format, ids >= nbits not
 * live.  A layer's members are the live nodes with level >= layer; an entry that points at no member counts in its owner's out-degree
 * and is otherwise ignored (never dereferenced).  with_in_edges == 0: the in-edge fields are 0 and no in-degree pass runs.  A layer
 * with no member: nodes_count 0 and every statistic 0 (layer_id is the layer asked for), 0 components.  layer outside 0 .. the
 * mirror's top level, or no committed graph: -1. */
int hnswdev_graph_info(void *ctx, int layer, const uint32_t *live_bits, long long nbits, int with_in_edges, hnsw_mi355x_layer_info *out);
int hnswdev_graph_components(void *ctx, int layer, const uint32_t *live_bits, long long nbits, int *out_count);
/* out[0 .. 3] as hnsw_mi355x_graph_info_counters, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_graph_info_counters(void *ctx, uint64_t out[4]);
/* Reachability over out-edges (see hnsw_mi355x_layer_reach) on ONE layer of the committed graph mirror of a context, from explicit
 * seeds.  live_bits / nbits and the layer test as hnswdev_graph_info.  seed_bits: a bitset of seed_nbits bits in the allow-sets'
 * format (it may be longer than the graph); NULL is -1; seeds that are no members of the layer are ignored; an empty set is legal:
 * nothing is reached and no expansion is launched.  out_reached_bits: ceil(n / 32) words, n the mirror's nodes, or NULL.  out_hops: n
 * ints or NULL -- >= 0 the hop count, -1 a member not reached, -2 no member.  out_summary: members, member seeds, reached, largest hop. */
int hnswdev_graph_reach_layer(void *ctx, int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits,
                              uint32_t *out_reached_bits, int *out_hops, uint64_t out_summary[4]);
/* The chain from entry_point's level (top) down to min_layer: returns top + 1, fills out_layers[L] for min_layer <= L < min(cap, top + 1);
 * the two arrays (either may be NULL) describe min_layer.  The seeds of a layer are the reached set of the layer above and never leave
 * the device.  An entry point that is no member of its own level reaches nothing on any layer; so does one out of range, for which
 * top is the graph's top level.  min_layer outside 0 .. top, no committed graph: -1. */
int hnswdev_graph_reach(void *ctx, int entry_point, const uint32_t *live_bits, long long nbits, int min_layer, hnsw_mi355x_layer_reach *out_layers,
                        int cap, uint32_t *out_reached_bits, int *out_hops);
/* out[0 .. 3] as hnsw_mi355x_graph_reach_counters, of this context; zeroed by hnswdev_reset_stats. */
int hnswdev_graph_reach_counters(void *ctx, uint64_t out[4]);
/* Steps (1) - (3) of one round of hnsw_mi355x_repair_reachability on ONE layer of the committed graph mirror, from explicit seeds; the
 * graph is read, not changed.  live_bits / nbits, the layer test and seed_bits / seed_nbits as hnswdev_graph_reach_layer.  max_edges:
 * MaxEdges(layer), 1 .. what a list of the mirror holds.  cands: 1 .. 64.  *out_n = |U|; min(cap, |U|) rows are written: out_ids[i] the
 * i-th unreached member ascending, out_cands[i * cands + j] its j-th nearest reached member (-1: padding), out_codes[i * cands + j] the
 * slot code of that pair (0-based position in the candidate's list, -1: none).  Every node of the graph needs an uploaded row. */
int hnswdev_graph_repair_propose(void *ctx, int layer, const uint32_t *live_bits, long long nbits, const uint32_t *seed_bits, long long seed_nbits, int cands,
                                 int max_edges, int *out_n, int *out_ids, int *out_cands, int *out_codes, int cap);
/* out[0 .. 3] as hnsw_mi355x_graph_repair_counters, of this context (out[3]: lists patched through it); zeroed by hnswdev_reset_stats. */
int hnswdev_graph_repair_counters(void *ctx, uint64_t out[4]);
int hnswdev_get_stats(void *ctx, hnswdev_stats *out);
int hnswdev_reset_stats(void *ctx);
/* Last error, process-wide (creation failures have no context yet) ... */
int hnswdev_last_error(char *buf, int buf_len);
/* ... and of one context: calls on different contexts never overwrite each other's message.
 * Both copy at most buf_len-1 bytes, NUL-terminate and return the byte count needed. */
int hnswdev_ctx_last_error(void *ctx, char *buf, int buf_len);
/* Number of visible HIP devices (>= 0), or < 0 on error. */
int hnswdev_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* HNSW_MI355X_H */
