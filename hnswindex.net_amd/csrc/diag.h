// diag.h -- the one door for test hooks and A/B switches.  NOT product surface: the product's knobs are the seven fields of
// hnsw_mi355x_options (include/hnsw_mi355x.h); everything here exists so that the test tiers can force a code path that the
// defaults would pick by themselves only on other inputs (the exact two-heap traversal, the latency variants, the hashed
// visited sets, spills and hand-backs, ...) and so that a measurement can be repeated with one mechanism switched off.
// Until round 4 these were 27 separate HNSW_MI355X_* environment variables, some read once and some per call; now:
//   * a list "name=value,name=value" -- hnsw_mi355x_options::diagnostics (process-wide, hnsw_mi355x_set_options) or, when
//     that is unset, the environment variable HNSW_MI355X_DIAG -- read on EVERY use, so a test that changes it between two
//     calls gets what it asked for;
//   * names (defaults in brackets; DESIGN.md 4.1 says what each is for):
//       lat [1]  novis [2]  novis_insert [1]  sorted_top [1]  shadow [1]  overlap [1]  mfma [1]  vis_hash [-1 = by graph size]
//       vis_hash_cap [0]  cand_cap [0]  spill_cap [-1]  link_plan [1]  concurrent_queries [1]  stream_queries [1]
//       xw_dry [1]  xw_stage [1]  trace [0]  lean [1]  exact_chunk [0 = the picker's]  exact_qtile [0 = the picker's]
//       exact_range_cap [0 = the picker's]  exact_range_sort [0 = 4096]  exact_range_arena [0 = 1 GiB of keys]
//       exact_union_round [0 = 65 536 members are the queries of one launch of duplicate_groups' scan]
//       density_pair_cap [0 = 2^24 records (256 MiB) in the pair arena of density_clusters; fewer within pairs fit: one scan, more: two]
//       edge_round [0 = 65 536 members are the owners of one launch of graph_duplicate_groups' / near_edges' edge kernel]
//       tag_list_cap [0 = 2^28 ids in the candidate lists of one batch of masks of exact_knn_tagged]
//       range_sort_long [1; 0 = range_sort_tagged_kernel hands a closure beyond its table to the host as the other two sorts do]
//       graph_unchecked [0]  row_prefilter [1 = the library chooses the shadow width; 0 = off, nothing allocated;
//       2 = the f16 forms, kept on after a launch that re-read most rows; 3 = the 8-bit form, where built (row length 128), kept on likewise]
//       pf_fixed_dim [1; 0 = the row prefilter's run-time-length kernel form also where the row length is the compiled-in one]
#pragma once
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

namespace hnsw {

inline std::string &diag_override() { static std::string s; return s; }
inline bool &diag_override_set() { static bool b = false; return b; }
inline std::mutex &diag_mutex() { static std::mutex m; return m; }

inline void set_diag_string(const char *s) // nullptr: back to the environment variable
{
    std::lock_guard<std::mutex> lk(diag_mutex());
    diag_override_set() = s != nullptr;
    diag_override() = s ? s : "";
}

inline int diag(const char *name, int dflt)
{
    std::string held;
    const char *list;
    {
        std::lock_guard<std::mutex> lk(diag_mutex());
        if (diag_override_set()) { held = diag_override(); list = held.c_str(); }
        else list = std::getenv("HNSW_MI355X_DIAG");
    }
    if (!list || !*list) return dflt;
    const size_t n = std::strlen(name);
    for (const char *p = list; *p;) {
        while (*p == ',' || *p == ' ') ++p;
        if (std::strncmp(p, name, n) == 0 && p[n] == '=') return std::atoi(p + n + 1);
        while (*p && *p != ',') ++p;
    }
    return dflt;
}

} // namespace hnsw
