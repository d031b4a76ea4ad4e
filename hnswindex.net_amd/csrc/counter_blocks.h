// counter_blocks.h -- the blocks of uint64_t counters a Device keeps beside hnswdev_stats, one row each:
// X(name, scope, slot names in order).  `name` is what follows hnswdev_ and hnsw_mi355x_ in the two getters of the block (both
// generated from this table: device_backend.hip, exports.cpp; declared by hand in include/hnsw_mi355x.h).  `scope` says what
// HnswIndex::counters reports: `summed` over every context, or the `primary` context's alone (the call runs there only).  The slot
// names are the keys of the dicts that bindings.py returns (its COUNTER_BLOCKS; tests/test_counter_blocks.py holds the two copies
// together), and the number of names is the length of the ABI's out[] array.  A new block is one row here and one there.
//
// What the slots count, since reset_stats, on one context:
//   knn_grouped_info          search_grouped: calls, queries launched, queries padded for an empty group, queries handed back
//   knn_tagged_info           search_tagged: calls, distinct masks, queries launched, queries padded for a mask without a candidate, handed back
//   by_id_info                search_self / exact_knn_by_id calls, queries traversed on the device, hand-backs, queries scanned, rows
//                             gathered, pairs the scan skipped as the query's own
//   range_grouped_info        grouped range calls that reached the context, queries launched, queries skipped for a group without graph
//                             ids, lists the device left to the host (closures to partition / sort / replay, and hand-backs)
//   range_tagged_info         the same of the tagged range calls, with their distinct masks; and closures above kRangeSortMax entries
//                             that the device finished
//   exact_range_info          lists of >= 2 entries ordered on the device, lists ordered on the host, rounds repeated with exact
//                             capacities, results returned
//   exact_grouped_info        grouped calls that launched, groups scanned (a query and a candidate each), scan blocks launched, ids placed
//                             in group lists (all four count the calls that launched a scan only)
//   exact_collapsed_info      collapsed calls that scanned, queries they scanned, keys the cap dropped at an insert, entries evicted by a
//                             nearer key of their label (the last two depend on the order the keys arrived in)
//   exact_tagged_info         calls that counted candidates, distinct masks, queries scanned, queries padded for a mask without a
//                             candidate, list entries built, batches of masks scanned
//   exact_range_grouped_info  grouped range calls that launched a scan, lists of >= 2 entries ordered on the device, lists ordered on the
//                             host, pieces scanned again with exact capacities
//   exact_range_tagged_info   exact_tagged_info's six of the tagged range scan, then exact_range_grouped_info's last three
//   graph_info_counters       layers summarised, layers whose components were counted, list entries read (counted by the kernels), launches
//   graph_reach_counters      layers walked, rounds (expansion launches), list entries the expansions read, kernel launches
//   graph_repair_counters     rounds that ran the proposal kernel, (u, candidate) pairs it judged, distances it measured, lists patched
#pragma once
#include <cstdint>

#define HNSW_FOR_EACH_COUNTER_BLOCK(X)                                                                                     \
    X(knn_grouped_info, summed, calls, launched, skipped, handbacks)                                                      \
    X(knn_tagged_info, summed, calls, masks, launched, skipped, handbacks)                                                \
    X(by_id_info, summed, calls, traversed, handbacks, scanned, rows_gathered, self_skipped)                              \
    X(range_grouped_info, primary, calls, launched, skipped, host_finished)                                               \
    X(range_tagged_info, primary, calls, masks, launched, skipped, host_finished, long_finished)                          \
    X(exact_range_info, primary, device_sorted, host_sorted, repeated_rounds, results)                                    \
    X(exact_grouped_info, primary, calls, groups_scanned, scan_blocks, ids_listed)                                        \
    X(exact_collapsed_info, primary, calls, queries, dropped, evicted)                                                    \
    X(exact_tagged_info, primary, calls, masks, scanned, skipped, ids_listed, batches)                                    \
    X(exact_range_grouped_info, primary, calls, device_sorted, host_sorted, repeated_pieces)                              \
    X(exact_range_tagged_info, primary, calls, masks, scanned, skipped, ids_listed, batches, device_sorted, host_sorted, repeated_pieces) \
    X(graph_info_counters, primary, info_layers, component_layers, entries, launches)                                     \
    X(graph_reach_counters, primary, layers, rounds, entries, launches)                                                   \
    X(graph_repair_counters, primary, rounds, pairs, distances, lists_patched)

namespace hnsw {

enum class CounterScope { primary, summed };

// The blocks in table order; kCounterBlocks of them.
#define HNSW_COUNTER_BLOCK_ID(NAME, SCOPE, ...) NAME,
enum class CounterBlock : int { HNSW_FOR_EACH_COUNTER_BLOCK(HNSW_COUNTER_BLOCK_ID) };
#undef HNSW_COUNTER_BLOCK_ID

// A block's slots by name: slot::knn_grouped_info::launched is the index of `launched` in that block, ::kCount the block's length.
namespace slot {
#define HNSW_COUNTER_BLOCK_SLOTS(NAME, SCOPE, ...) \
    struct NAME { enum : int { __VA_ARGS__, kCount }; static constexpr CounterBlock kBlock = CounterBlock::NAME; };
HNSW_FOR_EACH_COUNTER_BLOCK(HNSW_COUNTER_BLOCK_SLOTS)
#undef HNSW_COUNTER_BLOCK_SLOTS
} // namespace slot

#define HNSW_COUNTER_BLOCK_COUNT(NAME, SCOPE, ...) slot::NAME::kCount,
constexpr int kCounterSlots[] = {HNSW_FOR_EACH_COUNTER_BLOCK(HNSW_COUNTER_BLOCK_COUNT)};
#undef HNSW_COUNTER_BLOCK_COUNT
#define HNSW_COUNTER_BLOCK_SCOPE(NAME, SCOPE, ...) CounterScope::SCOPE,
constexpr CounterScope kCounterScope[] = {HNSW_FOR_EACH_COUNTER_BLOCK(HNSW_COUNTER_BLOCK_SCOPE)};
#undef HNSW_COUNTER_BLOCK_SCOPE
constexpr int kCounterBlocks = (int)(sizeof(kCounterSlots) / sizeof(kCounterSlots[0]));
constexpr int max_counter_slots()
{
    int m = 0;
    for (int i = 0; i < kCounterBlocks; ++i) m = kCounterSlots[i] > m ? kCounterSlots[i] : m;
    return m;
}
constexpr int kMaxCounterSlots = max_counter_slots();

// Helpers that fill either of two blocks through a pointer rely on the two agreeing where they write:
// exact_tag_batches on the first six slots of the two tagged scans' blocks ...
static_assert(slot::exact_tagged_info::kCount == 6 && (int)slot::exact_range_tagged_info::calls == slot::exact_tagged_info::calls &&
                  (int)slot::exact_range_tagged_info::masks == slot::exact_tagged_info::masks &&
                  (int)slot::exact_range_tagged_info::scanned == slot::exact_tagged_info::scanned &&
                  (int)slot::exact_range_tagged_info::skipped == slot::exact_tagged_info::skipped &&
                  (int)slot::exact_range_tagged_info::ids_listed == slot::exact_tagged_info::ids_listed &&
                  (int)slot::exact_range_tagged_info::batches == slot::exact_tagged_info::batches,
              "exact_range_tagged_info begins with exact_tagged_info's slots");
// ... and exact_range_finish on the two sort counters of exact_range_info, which exact_range_grouped_scan's block holds by the
// same names (that scan also fills a local block of this shape, which exact_range_tagged folds into its own by name).

} // namespace hnsw
