"""
ctypes bindings over the C-ABI library -- the host-side mirror of the reference's Python
interface (/root/reference/bindings/bindings.py): same `Index` class, method names, argument
meaning, dtypes/shapes and error behaviour (RuntimeError carrying the native last-error
string on a negative status).  `DeviceBackend` exposes the inner hnswdev_* boundary.
"""
import ctypes as ct
import os
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import numpy.typing as npt

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "artifacts" / "native" / "linux-x64" / "HNSWIndex.Native.so"  # bindings.py:27-41


def _load_lib():
    # torch ships its own libamdhip64.so.7; load it first so that this process holds ONE
    # HIP runtime (the library's DT_NEEDED then resolves to the copy already mapped).
    if os.environ.get("HNSW_MI355X_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch absent: /opt/rocm's runtime is used
            pass
    override = os.environ.get("HNSW_MI355X_LIB")  # diagnostic builds only (e.g. the phase-clock variant, tools/)
    if override:
        return ct.CDLL(override)
    if not LIB_PATH.exists():
        raise FileNotFoundError(
            f"Native library missing {LIB_PATH}: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); there is no pure-Python or CPU fallback")
    return ct.CDLL(str(LIB_PATH))


lib = _load_lib()

_F = ct.POINTER(ct.c_float)
_I = ct.POINTER(ct.c_int)


class Stats(ct.Structure):
    """The FIRST PART of hnswdev_stats (include/hnsw_mi355x.h): the counters up to multilayer_handbacks.  NOT large enough to
    pass to hnswdev_get_stats / hnsw_mi355x_get_stats, which write the whole C struct: pass a DeviceStats (below), as every
    call in this module does -- the argtypes of the three get_stats functions take POINTER(DeviceStats), so ctypes refuses
    byref(Stats()) with an ArgumentError instead of letting the library write 40 bytes past it."""
    _fields_ = [("launches", ct.c_uint64), ("evals", ct.c_uint64), ("timed_launches", ct.c_uint64),
                ("timed_evals", ct.c_uint64), ("kernel_ms", ct.c_double), ("row_bytes", ct.c_uint64),
                ("search_launches", ct.c_uint64), ("search_evals", ct.c_uint64), ("search_timed_launches", ct.c_uint64),
                ("search_timed_evals", ct.c_uint64), ("search_kernel_ms", ct.c_double), ("search_overflows", ct.c_uint64),
                ("search_repeats", ct.c_uint64),
                ("insert_launches", ct.c_uint64), ("insert_evals", ct.c_uint64), ("insert_timed_launches", ct.c_uint64),
                ("insert_timed_evals", ct.c_uint64), ("insert_kernel_ms", ct.c_double),
                ("link_launches", ct.c_uint64), ("link_evals", ct.c_uint64), ("link_timed_launches", ct.c_uint64),
                ("link_timed_evals", ct.c_uint64), ("link_kernel_ms", ct.c_double), ("visited_hash_launches", ct.c_uint64),
                ("range_launches", ct.c_uint64), ("range_evals", ct.c_uint64), ("range_timed_launches", ct.c_uint64),
                ("range_timed_evals", ct.c_uint64), ("range_kernel_ms", ct.c_double), ("range_handbacks", ct.c_uint64),
                ("replica_bytes", ct.c_uint64),
                ("tie_windows", ct.c_uint64), ("peer_direct_copies", ct.c_uint64), ("peer_staged_copies", ct.c_uint64), ("lat_launches", ct.c_uint64),
                ("range_device_ordered", ct.c_uint64), ("range_host_ordered", ct.c_uint64), ("insert_tie_reruns", ct.c_uint64), ("lean_launches", ct.c_uint64),
                ("multilayer_launches", ct.c_uint64), ("multilayer_jobs", ct.c_uint64), ("multilayer_handbacks", ct.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for c in reversed(type(self).__mro__) for k, _ in c.__dict__.get("_fields_", ())}


class DeviceStats(Stats):
    """The whole of hnswdev_stats: `Stats` (the struct as it stood before the flat scan; its layout is pinned) followed by the
    counters appended to the C struct since -- a ctypes subclass lays its own fields out behind its base's, as the header
    appends them.  Every get_stats call of this module fills one of these."""
    _fields_ = [("exact_launches", ct.c_uint64), ("exact_evals", ct.c_uint64), ("exact_timed_launches", ct.c_uint64),
                ("exact_timed_evals", ct.c_uint64), ("exact_kernel_ms", ct.c_double)]

    @classmethod
    def field_names(cls):
        return [k for c in reversed(cls.__mro__) for k, _ in c.__dict__.get("_fields_", ())]


# ---- (A) the reference's 16 exports: bindings.py:45-119 ---------------------------------
lib.hnsw_create.restype = ct.c_void_p
lib.hnsw_create.argtypes = [ct.c_char_p]
lib.hnsw_free.restype = None
lib.hnsw_free.argtypes = [ct.c_void_p]
lib.hnsw_add.restype = ct.c_int
lib.hnsw_add.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, _I]
lib.hnsw_remove.restype = ct.c_int
lib.hnsw_remove.argtypes = [ct.c_void_p, _I, ct.c_int]
lib.hnsw_knn_query.restype = ct.c_int
lib.hnsw_knn_query.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, _I, _F]
lib.hnsw_range_query.restype = ct.c_int
lib.hnsw_range_query.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.POINTER(ct.c_void_p),
                                 ct.POINTER(ct.c_void_p), _I]
lib.hnsw_free_results.restype = None
lib.hnsw_free_results.argtypes = [ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_void_p), ct.c_int]
for _name in ("hnsw_set_collection_size", "hnsw_set_max_edges", "hnsw_set_max_candidates",
              "hnsw_set_remove_max_candidates", "hnsw_set_random_seed", "hnsw_set_min_nn",
              "hnsw_mi355x_set_device", "hnsw_mi355x_set_insert_batch", "hnsw_mi355x_set_remove_batch", "hnsw_mi355x_set_search_slots",
              "hnsw_mi355x_set_host_threads", "hnsw_mi355x_set_device_traversal", "hnsw_mi355x_set_devices"):
    getattr(lib, _name).restype = ct.c_int
    getattr(lib, _name).argtypes = [ct.c_int]
lib.hnsw_set_distribution_rate.restype = ct.c_int
lib.hnsw_set_distribution_rate.argtypes = [ct.c_float]
lib.hnsw_set_allow_removals.restype = ct.c_int
lib.hnsw_set_allow_removals.argtypes = [ct.c_bool]
lib.hnsw_get_last_error_utf8.restype = ct.c_int
lib.hnsw_get_last_error_utf8.argtypes = [ct.c_void_p, ct.c_int]

# ---- additions ---------------------------------------------------------------------------
for _name in ("hnsw_mi355x_count", "hnsw_mi355x_length", "hnsw_mi355x_entry_point", "hnsw_mi355x_reset_stats", "hnsw_mi355x_resident_count"):
    getattr(lib, _name).restype = ct.c_int
    getattr(lib, _name).argtypes = [ct.c_void_p]
lib.hnsw_mi355x_set_queries.restype = ct.c_int
lib.hnsw_mi355x_set_queries.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int]
lib.hnsw_mi355x_knn_query_resident.restype = ct.c_int
lib.hnsw_mi355x_knn_query_resident.argtypes = [ct.c_void_p, ct.c_int, _I, _F]
_U32 = ct.POINTER(ct.c_uint32)
lib.hnsw_mi355x_knn_query_filtered.restype = ct.c_int
lib.hnsw_mi355x_knn_query_filtered.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnsw_mi355x_exact_knn_query.restype = ct.c_int
lib.hnsw_mi355x_exact_knn_query.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnsw_mi355x_exact_range_query.restype = ct.c_int
lib.hnsw_mi355x_exact_range_query.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, _U32, ct.c_longlong, ct.POINTER(ct.c_void_p),
                                              ct.POINTER(ct.c_void_p), _I]
lib.hnsw_mi355x_exact_range_query_grouped.restype = ct.c_int
lib.hnsw_mi355x_exact_range_query_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, _I, ct.c_longlong, _I, ct.c_int,
                                                      ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int)]
lib.hnsw_mi355x_exact_knn_query_grouped.restype = ct.c_int
lib.hnsw_mi355x_exact_knn_query_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, _I, ct.c_longlong, _I, ct.c_int, _I, _F]
lib.hnsw_mi355x_exact_knn_query_collapsed.restype = ct.c_int
lib.hnsw_mi355x_exact_knn_query_collapsed.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, _I, ct.c_longlong, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnsw_mi355x_knn_query_collapsed.restype = ct.c_int
lib.hnsw_mi355x_knn_query_collapsed.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, ct.c_longlong, ct.c_int, ct.c_int, _U32, ct.c_longlong,
                                                _I, _F]
_TAG_MATCH = {"any": 0, "all": 1}   # the `match` argument of the tagged calls
lib.hnsw_mi355x_knn_query_tagged.restype = ct.c_int
lib.hnsw_mi355x_knn_query_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_int, _I, _F]
lib.hnsw_mi355x_exact_knn_query_tagged.restype = ct.c_int
lib.hnsw_mi355x_exact_knn_query_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_int, _I, _F]
# query by stored id
_BY_ID_CHUNK = 65536   # ids per call of Index.exact_knn_graph: bounds the gathered query set
lib.hnsw_mi355x_get_vectors.restype = ct.c_int
lib.hnsw_mi355x_get_vectors.argtypes = [ct.c_void_p, _I, ct.c_int, _F]
lib.hnsw_mi355x_knn_query_by_id.restype = ct.c_int
lib.hnsw_mi355x_knn_query_by_id.argtypes = [ct.c_void_p, _I, ct.c_int, ct.c_int, ct.c_int, _I, _F]
lib.hnsw_mi355x_exact_knn_query_by_id.restype = ct.c_int
lib.hnsw_mi355x_exact_knn_query_by_id.argtypes = [ct.c_void_p, _I, ct.c_int, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnsw_mi355x_exact_range_query_by_id.restype = ct.c_int
lib.hnsw_mi355x_exact_range_query_by_id.argtypes = [ct.c_void_p, _I, ct.c_int, ct.c_float, _U32, ct.c_longlong, ct.POINTER(ct.c_void_p),
                                                    ct.POINTER(ct.c_void_p), _I]
lib.hnsw_mi355x_duplicate_groups.restype = ct.c_int
lib.hnsw_mi355x_duplicate_groups.argtypes = [ct.c_void_p, ct.c_float, _U32, ct.c_longlong, _I, ct.c_longlong, ct.POINTER(ct.c_uint64)]
_GROUPS_INFO = ("members", "groups", "pairs_within", "pairs_measured")   # out_info[0 .. 3] of hnsw_mi355x_duplicate_groups
lib.hnsw_mi355x_density_clusters.restype = ct.c_int
lib.hnsw_mi355x_density_clusters.argtypes = [ct.c_void_p, ct.c_float, ct.c_int, _U32, ct.c_longlong, _I, _I, ct.c_longlong, ct.POINTER(ct.c_uint64)]
_DENSITY_INFO = ("members", "clusters", "core", "border", "noise", "pairs_within", "pairs_measured", "scans")   # out_info[0 .. 7] of hnsw_mi355x_density_clusters
lib.hnsw_mi355x_graph_duplicate_groups.restype = ct.c_int
lib.hnsw_mi355x_graph_duplicate_groups.argtypes = [ct.c_void_p, ct.c_float, _U32, ct.c_longlong, _I, ct.c_longlong, ct.POINTER(ct.c_uint64)]
lib.hnsw_mi355x_near_edges.restype = ct.c_int
lib.hnsw_mi355x_near_edges.argtypes = [ct.c_void_p, ct.c_float, _U32, ct.c_longlong, ct.POINTER(ct.c_longlong)]
lib.hnsw_mi355x_near_edges_results.restype = ct.c_int
lib.hnsw_mi355x_near_edges_results.argtypes = [ct.c_void_p, _I, _I, _F, ct.c_longlong]
_EDGE_GROUPS_INFO = ("members", "groups", "edges_within", "edges_measured", "launches")   # out_info[0 .. 4] of hnsw_mi355x_graph_duplicate_groups
lib.hnsw_mi355x_knn_query_grouped.restype = ct.c_int
lib.hnsw_mi355x_knn_query_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, ct.c_longlong, _I, ct.c_int, _I, _F]
lib.hnsw_mi355x_range_query_grouped.restype = ct.c_int
lib.hnsw_mi355x_range_query_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.c_int, _I, ct.c_longlong, _I, ct.c_int,
                                                ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int)]
lib.hnsw_mi355x_range_query_tagged.restype = ct.c_int
lib.hnsw_mi355x_range_query_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_int,
                                               ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int)]
lib.hnsw_mi355x_exact_range_query_tagged.restype = ct.c_int
lib.hnsw_mi355x_exact_range_query_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, _U32, ct.c_longlong, _U32, ct.c_int,
                                                     ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int)]


class LayerInfo(ct.Structure):
    """hnsw_mi355x_layer_info: HNSWInfo.LayerInfo (HNSWInfo.cs:18-29) of one layer."""
    _fields_ = [(n, ct.c_int32) for n in ("layer_id", "nodes_count", "max_out_edges", "min_out_edges", "max_in_edges", "min_in_edges",
                                          "out_edges_median", "in_edges_median")] + [("avg_out_edges", ct.c_double), ("avg_in_edges", ct.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


lib.hnsw_mi355x_get_info.restype = ct.c_int
lib.hnsw_mi355x_get_info.argtypes = [ct.c_void_p, ct.POINTER(LayerInfo), ct.c_int]
lib.hnsw_mi355x_connected_component_counts.restype = ct.c_int
lib.hnsw_mi355x_connected_component_counts.argtypes = [ct.c_void_p, _I, ct.c_int]
lib.hnswdev_graph_info.restype = ct.c_int
lib.hnswdev_graph_info.argtypes = [ct.c_void_p, ct.c_int, _U32, ct.c_longlong, ct.c_int, ct.POINTER(LayerInfo)]
lib.hnswdev_graph_components.restype = ct.c_int
lib.hnswdev_graph_components.argtypes = [ct.c_void_p, ct.c_int, _U32, ct.c_longlong, _I]


class LayerReach(ct.Structure):
    """hnsw_mi355x_layer_reach: one layer of the reachability chain from the entry point."""
    _fields_ = [(n, ct.c_int32) for n in ("layer_id", "nodes_count", "seeds", "reached", "max_hops")]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


_GRAPH_REACH_SUMMARY = ("nodes_count", "seeds", "reached", "max_hops")   # hnswdev_graph_reach_layer's out_summary[0 .. 3]
lib.hnsw_mi355x_reachability.restype = ct.c_int
lib.hnsw_mi355x_reachability.argtypes = [ct.c_void_p, ct.POINTER(LayerReach), ct.c_int]
lib.hnsw_mi355x_unreachable_ids.restype = ct.c_int
lib.hnsw_mi355x_unreachable_ids.argtypes = [ct.c_void_p, ct.c_int, _I, ct.c_int]
lib.hnsw_mi355x_hop_counts.restype = ct.c_int
lib.hnsw_mi355x_hop_counts.argtypes = [ct.c_void_p, ct.c_int, _I, ct.c_int]
lib.hnswdev_graph_reach_layer.restype = ct.c_int
lib.hnswdev_graph_reach_layer.argtypes = [ct.c_void_p, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_longlong, _U32, _I, ct.POINTER(ct.c_uint64)]
lib.hnswdev_graph_reach.restype = ct.c_int
lib.hnswdev_graph_reach.argtypes = [ct.c_void_p, ct.c_int, _U32, ct.c_longlong, ct.c_int, ct.POINTER(LayerReach), ct.c_int, _U32, _I]


class LayerRepair(ct.Structure):
    """hnsw_mi355x_layer_repair: what repair_reachability did on one layer."""
    _fields_ = [(n, ct.c_int32) for n in ("layer_id", "unreachable_before", "linked", "evicted", "rounds", "unreachable_after")]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


lib.hnsw_mi355x_repair_reachability.restype = ct.c_int
lib.hnsw_mi355x_repair_reachability.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(LayerRepair), ct.c_int]
lib.hnswdev_graph_repair_propose.restype = ct.c_int
lib.hnswdev_graph_repair_propose.argtypes = [ct.c_void_p, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_longlong, ct.c_int, ct.c_int, _I, _I, _I, _I, ct.c_int]
lib.hnsw_mi355x_range_query_filtered.restype = ct.c_int
lib.hnsw_mi355x_range_query_filtered.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, _U32, ct.c_longlong, ct.POINTER(ct.c_void_p),
                                                 ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int)]
lib.hnsw_mi355x_active_ids.restype = ct.c_int
lib.hnsw_mi355x_knn_query_at_layer.restype = ct.c_int
lib.hnsw_mi355x_knn_query_at_layer.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnsw_mi355x_range_query_at_layer.restype = ct.c_int
lib.hnsw_mi355x_range_query_at_layer.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.c_int, _U32, ct.c_longlong, ct.POINTER(ct.c_void_p),
                                                 ct.POINTER(ct.c_void_p), ct.POINTER(ct.c_int)]
lib.hnsw_mi355x_multilayer_knn_query.restype = ct.c_int
lib.hnsw_mi355x_multilayer_knn_query.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, _F]
lib.hnsw_mi355x_active_ids.argtypes = [ct.c_void_p, _I, ct.c_int]
lib.hnsw_mi355x_node_max_layer.restype = ct.c_int
lib.hnsw_mi355x_node_max_layer.argtypes = [ct.c_void_p, ct.c_int]
lib.hnsw_mi355x_get_out_edges.restype = ct.c_int
lib.hnsw_mi355x_get_out_edges.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, _I, ct.c_int]
lib.hnsw_mi355x_export_levels.restype = ct.c_int
lib.hnsw_mi355x_export_levels.argtypes = [ct.c_void_p, _I, ct.c_int]
lib.hnsw_mi355x_export_edges.restype = ct.c_int
lib.hnsw_mi355x_export_edges.argtypes = [ct.c_void_p, ct.c_int, _I, _I, ct.c_int, ct.c_int]
lib.hnsw_mi355x_dim.restype = ct.c_int
lib.hnsw_mi355x_dim.argtypes = [ct.c_void_p]
lib.hnsw_mi355x_serialize.restype = ct.c_int
lib.hnsw_mi355x_serialize.argtypes = [ct.c_void_p, ct.c_char_p]
lib.hnsw_mi355x_deserialize.restype = ct.c_void_p
lib.hnsw_mi355x_deserialize.argtypes = [ct.c_char_p, ct.c_char_p]
lib.hnsw_mi355x_graph_hash.restype = ct.c_uint64
lib.hnsw_mi355x_graph_hash.argtypes = [ct.c_void_p]
lib.hnsw_mi355x_get_stats.restype = ct.c_int
lib.hnsw_mi355x_get_stats.argtypes = [ct.c_void_p, ct.POINTER(DeviceStats)]
lib.hnsw_mi355x_set_profiling.restype = ct.c_int
lib.hnsw_mi355x_set_profiling.argtypes = [ct.c_void_p, ct.c_int]
lib.hnsw_mi355x_index_set_insert_batch.restype = ct.c_int
lib.hnsw_mi355x_index_set_insert_batch.argtypes = [ct.c_void_p, ct.c_int]
lib.hnsw_mi355x_index_insert_batch.restype = ct.c_int
lib.hnsw_mi355x_index_insert_batch.argtypes = [ct.c_void_p]
lib.hnsw_mi355x_host_parallelism.restype = ct.c_int
lib.hnsw_mi355x_host_parallelism.argtypes = []
lib.hnsw_mi355x_device_count.restype = ct.c_int
lib.hnsw_mi355x_device_count.argtypes = [ct.c_void_p]
lib.hnsw_mi355x_get_stats_at.restype = ct.c_int
lib.hnsw_mi355x_get_stats_at.argtypes = [ct.c_void_p, ct.c_int, ct.POINTER(DeviceStats)]
lib.hnsw_mi355x_build_id.restype = ct.c_char_p
lib.hnsw_mi355x_build_id.argtypes = []
lib.hnsw_mi355x_exact_window_stats.restype = ct.c_int
lib.hnsw_mi355x_exact_window_stats.argtypes = [ct.c_void_p, ct.POINTER(ct.c_uint64)]
lib.hnsw_mi355x_row_prefilter_stats.restype = ct.c_int
lib.hnsw_mi355x_row_prefilter_stats.argtypes = [ct.c_void_p, ct.POINTER(ct.c_uint64)]
lib.hnsw_mi355x_row_prefilter_form_stats.restype = ct.c_int
lib.hnsw_mi355x_row_prefilter_form_stats.argtypes = [ct.c_void_p, ct.POINTER(ct.c_uint64)]
lib.hnsw_mi355x_row_prefilter8_stats.restype = ct.c_int
lib.hnsw_mi355x_row_prefilter8_stats.argtypes = [ct.c_void_p, ct.POINTER(ct.c_uint64)]
lib.hnsw_mi355x_row_prefilter8_peek.restype = ct.c_int
lib.hnsw_mi355x_row_prefilter8_peek.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_uint8)]
lib.hnsw_mi355x_row_prefilter_peek.restype = ct.c_int
lib.hnsw_mi355x_row_prefilter_peek.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, ct.POINTER(ct.c_uint64), ct.POINTER(ct.c_float)]

# ---- (B) hnswdev_* -------------------------------------------------------------------------
lib.hnsw_mi355x_import_nodes.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, _I, ct.c_int]
lib.hnsw_mi355x_import_edges.argtypes = [ct.c_void_p, ct.c_int, _I, _I, ct.c_int]
lib.hnswdev_device_count.restype = ct.c_int
lib.hnswdev_create.restype = ct.c_int
lib.hnswdev_create.argtypes = [ct.c_int, ct.c_int, ct.c_int, ct.c_longlong, ct.POINTER(ct.c_void_p)]
lib.hnswdev_destroy.argtypes = [ct.c_void_p]
lib.hnswdev_reserve.argtypes = [ct.c_void_p, ct.c_longlong]
lib.hnswdev_upload_rows.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, _F]
lib.hnswdev_download_rows.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, _F]
lib.hnswdev_dist_query_batch.argtypes = [ct.c_void_p, _F, ct.c_int, _I, _I, _F]
lib.hnswdev_dist_pair_batch.argtypes = [ct.c_void_p, _I, _I, ct.c_int, _F]
lib.hnswdev_graph_begin.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, _I]
lib.hnswdev_graph_set_layer.argtypes = [ct.c_void_p, ct.c_int, _I, _I, ct.c_int]
lib.hnswdev_graph_commit.argtypes = [ct.c_void_p]
lib.hnswdev_knn_search.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, _F, _I]
lib.hnswdev_knn_search_filtered.restype = ct.c_int
lib.hnswdev_knn_search_filtered.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _I, _F, _I]
lib.hnswdev_range_search.restype = ct.c_int
lib.hnswdev_range_search.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, _I, _I]
lib.hnswdev_exact_knn.restype = ct.c_int
lib.hnswdev_exact_knn.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnswdev_range_search_filtered.restype = ct.c_int
lib.hnswdev_range_search_filtered.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, _U32, ct.c_longlong, _I, _I]
lib.hnswdev_exact_range.restype = ct.c_int
lib.hnswdev_exact_range.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_float, _U32, ct.c_longlong, _I]
lib.hnswdev_exact_range_results.restype = ct.c_int
lib.hnswdev_exact_range_results.argtypes = [ct.c_void_p, _I, _F]
lib.hnswdev_exact_range_grouped.restype = ct.c_int
lib.hnswdev_exact_range_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_float, _I, ct.c_longlong, _I, ct.c_int, _I]
lib.hnswdev_exact_knn_grouped.restype = ct.c_int
lib.hnswdev_exact_knn_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_int, _I, ct.c_longlong, _I, ct.c_int, _I, _F]
lib.hnswdev_exact_knn_collapsed.restype = ct.c_int
lib.hnswdev_exact_knn_collapsed.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_int, _I, ct.c_longlong, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnswdev_exact_grouped_list_ms.restype = ct.c_int
lib.hnswdev_exact_grouped_list_ms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_double)]
lib.hnswdev_knn_search_tagged.restype = ct.c_int
lib.hnswdev_knn_search_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_int, _I, _F, _I]
lib.hnswdev_exact_knn_tagged.restype = ct.c_int
lib.hnswdev_exact_knn_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_int, _I, _F]
lib.hnswdev_gather_rows.restype = ct.c_int
lib.hnswdev_gather_rows.argtypes = [ct.c_void_p, _I, ct.c_int, _F]
lib.hnswdev_knn_search_by_id.restype = ct.c_int
lib.hnswdev_knn_search_by_id.argtypes = [ct.c_void_p, _I, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, _F, _I]
lib.hnswdev_exact_knn_by_id.restype = ct.c_int
lib.hnswdev_exact_knn_by_id.argtypes = [ct.c_void_p, _I, ct.c_int, ct.c_longlong, ct.c_int, _U32, ct.c_longlong, _I, _F]
lib.hnswdev_exact_range_by_id.restype = ct.c_int
lib.hnswdev_exact_range_by_id.argtypes = [ct.c_void_p, _I, ct.c_int, ct.c_longlong, ct.c_float, _U32, ct.c_longlong, _I]
lib.hnswdev_exact_range_groups.restype = ct.c_int
lib.hnswdev_exact_range_groups.argtypes = [ct.c_void_p, ct.c_longlong, ct.c_float, _U32, ct.c_longlong, _I, ct.POINTER(ct.c_uint64)]
lib.hnswdev_exact_range_density.restype = ct.c_int
lib.hnswdev_exact_range_density.argtypes = [ct.c_void_p, ct.c_longlong, ct.c_float, ct.c_int, _U32, ct.c_longlong, _I, _I, ct.POINTER(ct.c_uint64)]
lib.hnswdev_graph_edge_groups.restype = ct.c_int
lib.hnswdev_graph_edge_groups.argtypes = [ct.c_void_p, ct.c_longlong, ct.c_float, _U32, ct.c_longlong, _I, ct.POINTER(ct.c_uint64)]
lib.hnswdev_graph_near_edges.restype = ct.c_int
lib.hnswdev_graph_near_edges.argtypes = [ct.c_void_p, ct.c_longlong, ct.c_float, _U32, ct.c_longlong, ct.POINTER(ct.c_longlong)]
lib.hnswdev_graph_near_edges_results.restype = ct.c_int
lib.hnswdev_graph_near_edges_results.argtypes = [ct.c_void_p, _I, _I, _F, ct.c_longlong]
lib.hnswdev_tag_list_ms.restype = ct.c_int
lib.hnswdev_tag_list_ms.argtypes = [ct.c_void_p, ct.POINTER(ct.c_double)]
lib.hnswdev_knn_search_grouped.restype = ct.c_int
lib.hnswdev_knn_search_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, ct.c_longlong, _I, ct.c_int, _I, _F, _I]
lib.hnswdev_range_search_grouped.restype = ct.c_int
lib.hnswdev_range_search_grouped.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.c_int, _I, ct.c_longlong, _I, ct.c_int, _I, _I]
lib.hnswdev_range_search_tagged.restype = ct.c_int
lib.hnswdev_range_search_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.c_int, _U32, ct.c_longlong, _U32, ct.c_int, _I, _I]
lib.hnswdev_exact_range_tagged.restype = ct.c_int
lib.hnswdev_exact_range_tagged.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_longlong, ct.c_float, _U32, ct.c_longlong, _U32, ct.c_int, _I]
lib.hnswdev_range_results.restype = ct.c_int
lib.hnswdev_range_results.argtypes = [ct.c_void_p, _I, _F]
lib.hnswdev_knn_search_at_layer.restype = ct.c_int
lib.hnswdev_knn_search_at_layer.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _U32, ct.c_longlong, _I, _F, _I]
lib.hnswdev_range_search_at_layer.restype = ct.c_int
lib.hnswdev_range_search_at_layer.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_float, ct.c_int, _U32, ct.c_longlong, _I, _I]
lib.hnswdev_multilayer_search.restype = ct.c_int
lib.hnswdev_multilayer_search.argtypes = [ct.c_void_p, _F, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, ct.c_int, _I, _F, _I]
lib.hnswdev_sync.argtypes = [ct.c_void_p]
lib.hnswdev_set_profiling.argtypes = [ct.c_void_p, ct.c_int]
lib.hnswdev_get_stats.argtypes = [ct.c_void_p, ct.POINTER(DeviceStats)]
lib.hnswdev_reset_stats.argtypes = [ct.c_void_p]
lib.hnswdev_last_error.argtypes = [ct.c_char_p, ct.c_int]
lib.hnswdev_ctx_last_error.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_int]
lib.hnswdev_set_queries.argtypes = [ct.c_void_p, _F, ct.c_int]
lib.hnswdev_step_buffers.argtypes = [ct.c_void_p, ct.c_int, ct.c_int, ct.c_int, ct.POINTER(_I), ct.POINTER(_F)]
lib.hnswdev_step_submit.argtypes = [ct.c_void_p, ct.c_int, ct.c_int]
lib.hnswdev_step_wait.argtypes = [ct.c_void_p, ct.c_int]
lib.hnswdev_test_sqrt_rn.argtypes = [ct.c_int, ct.POINTER(ct.c_double), ct.POINTER(ct.c_double), ct.c_int]

# ---- (C) the counter blocks ----------------------------------------------------------------
# One row per block, in the order and with the slot names of csrc/counter_blocks.h (tests/test_counter_blocks.py holds the two
# tables together): name -> (slot names, docstring).  hnsw_mi355x_<name> and hnswdev_<name> fill an array of one uint64 per slot;
# Index.<name>() and DeviceBackend.<name>() return it as a dict keyed by the slot names (_install_counter_methods, below the
# classes).  A new block is one row here and one there.
COUNTER_BLOCKS = {
    "knn_grouped_info": (("calls", "launched", "skipped", "handbacks"),
        """Counters of knn_query_grouped's device launches since reset_stats (hnsw_mi355x_knn_grouped_info): calls that reached a
        context, queries launched, queries skipped because their group holds no graph id, queries handed back to the host."""),
    "knn_tagged_info": (("calls", "masks", "launched", "skipped", "handbacks"),
        """Counters of knn_query_tagged's device launches since reset_stats (hnsw_mi355x_knn_tagged_info): calls that reached a
        context, their distinct masks, queries launched, queries skipped because their mask has no candidate, queries handed back."""),
    "by_id_info": (("calls", "traversed", "handbacks", "scanned", "rows_gathered", "self_skipped"),
        """Counters of the by-id calls since reset_stats (hnsw_mi355x_by_id_info): calls that reached a device, queries traversed on
        the device, of those handed back to the host, queries scanned, rows gathered, pairs the scan skipped as the query's own."""),
    "range_grouped_info": (("calls", "launched", "skipped", "host_finished"),
        """Counters of range_query_grouped since reset_stats (hnsw_mi355x_range_grouped_info): calls that reached the context, queries
        launched, queries skipped because their group holds no graph id, lists the device left to the host."""),
    "range_tagged_info": (("calls", "masks", "launched", "skipped", "host_finished", "long_finished"),
        """Counters of range_query_tagged since reset_stats (hnsw_mi355x_range_tagged_info): calls that reached the context, their
        distinct masks, queries launched, queries skipped because their mask matches no graph id, lists the device left to the host,
        closures beyond the device's table that it finished all the same."""),
    "exact_range_info": (("device_sorted", "host_sorted", "repeated_rounds", "results"),
        """Counters of exact_range_query since reset_stats (hnsw_mi355x_exact_range_info)."""),
    "exact_grouped_info": (("calls", "groups_scanned", "scan_blocks", "ids_listed"),
        """Counters of exact_knn_query_grouped since reset_stats (hnsw_mi355x_exact_grouped_info)."""),
    "exact_collapsed_info": (("calls", "queries", "dropped", "evicted"),
        """Counters of exact_knn_query_collapsed since reset_stats (hnsw_mi355x_exact_collapsed_info): calls that scanned, queries
        scanned, keys dropped by the cap at a list, list entries evicted by a nearer key of their label."""),
    "exact_tagged_info": (("calls", "masks", "scanned", "skipped", "ids_listed", "batches"),
        """Counters of exact_knn_query_tagged since reset_stats (hnsw_mi355x_exact_tagged_info): calls, their distinct masks, queries
        scanned, queries skipped because their mask has no candidate, ids written into candidate lists, batches of masks."""),
    "exact_range_grouped_info": (("calls", "device_sorted", "host_sorted", "repeated_pieces"),
        """Counters of exact_range_query_grouped since reset_stats (hnsw_mi355x_exact_range_grouped_info)."""),
    "exact_range_tagged_info": (("calls", "masks", "scanned", "skipped", "ids_listed", "batches", "device_sorted", "host_sorted", "repeated_pieces"),
        """Counters of exact_range_query_tagged since reset_stats (hnsw_mi355x_exact_range_tagged_info)."""),
    "graph_info_counters": (("info_layers", "component_layers", "entries", "launches"),
        """Counters of get_info / connected_component_counts since reset_stats (hnsw_mi355x_graph_info_counters)."""),
    "graph_reach_counters": (("layers", "rounds", "entries", "launches"),
        """Counters of reachability / unreachable_ids / hop_counts since reset_stats (hnsw_mi355x_graph_reach_counters)."""),
    "graph_repair_counters": (("rounds", "pairs", "distances", "lists_patched"),
        """Counters of repair_reachability since reset_stats (hnsw_mi355x_graph_repair_counters)."""),
}
for _name in COUNTER_BLOCKS:
    for _sym in ("hnsw_mi355x_" + _name, "hnswdev_" + _name):
        getattr(lib, _sym).restype = ct.c_int
        getattr(lib, _sym).argtypes = [ct.c_void_p, ct.POINTER(ct.c_uint64)]

METRICS = {"sq_euclid": 0,"cosine": 1, "ucosine": 2, "sq_euclid_i8": 3, "sq_euclid_f16": 4, "ucosine_f16": 5}


class Options(ct.Structure):
    """hnsw_mi355x_options, version 1 (include/hnsw_mi355x.h): every knob of the backend."""
    _fields_ = [("struct_size", ct.c_uint32), ("device", ct.c_int32), ("devices", ct.c_int32), ("insert_batch", ct.c_int32),
                ("remove_batch", ct.c_int32), ("host_threads", ct.c_int32), ("search_slots", ct.c_int32), ("device_traversal", ct.c_int32),
                ("diagnostics", ct.c_char_p)]


lib.hnsw_mi355x_default_options.restype = ct.c_int
lib.hnsw_mi355x_default_options.argtypes = [ct.POINTER(Options)]
lib.hnsw_mi355x_set_options.restype = ct.c_int
lib.hnsw_mi355x_set_options.argtypes = [ct.POINTER(Options)]


def default_options() -> Options:
    o = Options()
    if lib.hnsw_mi355x_default_options(ct.byref(o)) != 0:
        raise RuntimeError("hnsw_mi355x_default_options failed")
    return o


def set_options(**knobs) -> None:
    """Sets the pending backend knobs for the next Index (defaults for whatever is not named): device, devices, insert_batch,
    remove_batch, host_threads, search_slots, device_traversal, diagnostics (str or None)."""
    o = default_options()
    for k, v in knobs.items():
        if k not in dict(Options._fields_) or k == "struct_size":
            raise TypeError(f"unknown option {k!r}")
        setattr(o, k, v.encode() if isinstance(v, str) else v)
    if lib.hnsw_mi355x_set_options(ct.byref(o)) != 0:
        raise RuntimeError(last_error())


def host_parallelism() -> int:
    """Hardware threads this process may run on = the default cap of Add's snapshot batches (include/hnsw_mi355x.h)."""
    return int(lib.hnsw_mi355x_host_parallelism())


def _group_args(row_group, query_group, n_groups, nq):
    """(row_group, query_group, n_groups) as the grouped scans take them: contiguous int32 arrays, query_group of nq entries;
    n_groups None: the largest value in either array plus one, at least 1."""
    rg = np.ascontiguousarray(np.asarray(row_group).reshape(-1), dtype=np.int32)
    qg = np.ascontiguousarray(np.asarray(query_group).reshape(-1), dtype=np.int32)
    if qg.shape[0] != nq:
        raise ValueError(f"query_group has {qg.shape[0]} entries for {nq} queries")
    if n_groups is None:
        n_groups = max(int(rg.max(initial=-1)), int(qg.max(initial=-1))) + 1
        n_groups = max(n_groups, 1)
    return rg, qg, int(n_groups)


def _collapse_args(row_group, k, per_group, n_ids, k_limit=1024):
    """row_group as the collapsed scan takes it -- a contiguous int32 array with a label for each of the n_ids ids -- after the checks
    of k and per_group.  Every breach is a ValueError here, before anything native runs."""
    k, per_group = int(k), int(per_group)
    if k_limit is not None and k > k_limit:
        raise ValueError(f"k = {k} is above the limit of {k_limit}")
    if k >= 1 and not 1 <= per_group <= k:
        raise ValueError(f"per_group = {per_group} is outside [1, k = {k}]")
    rg = np.asarray(row_group).reshape(-1)
    if rg.size and rg.dtype.kind not in "iu":
        raise ValueError(f"row_group must hold integers (int32 labels), not {rg.dtype}")
    if rg.size and (int(rg.min()) < -2 ** 31 or int(rg.max()) > 2 ** 31 - 1):
        raise ValueError("row_group holds a value outside the int32 range")   # (wrapped, two labels could become one)
    if rg.shape[0] < n_ids:
        raise ValueError(f"row_group has {rg.shape[0]} entries, the index's length is {n_ids}")
    return np.ascontiguousarray(rg, dtype=np.int32)


def _tag_words(values, name):
    """A tag array as the C ABI takes it: contiguous uint32, one word per entry.  Integers outside 0 .. 2^32 - 1 are an error, not
    wrapped."""
    a = np.asarray(values).reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integers (uint32 tag words), not {a.dtype}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise ValueError(f"{name} holds a value outside 0 .. 2^32 - 1")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _tag_args(row_tags, query_tags, match, nq):
    """(row_tags, query_tags, match) as the tagged calls take them: uint32 arrays, query_tags of nq entries with at most 65 536
    distinct values, match "any" -> 0 / "all" -> 1.  Every breach is a ValueError here, before anything native runs."""
    if match not in _TAG_MATCH:
        raise ValueError(f"match = {match!r} is neither 'any' nor 'all'")
    rt = _tag_words(row_tags, "row_tags")
    qt = _tag_words(query_tags, "query_tags")
    if qt.shape[0] != nq:
        raise ValueError(f"query_tags has {qt.shape[0]} entries for {nq} queries")
    distinct = int(np.unique(qt).size)
    if distinct > 65536:
        raise ValueError(f"query_tags holds {distinct} distinct masks, more than 65536")
    return rt, qt, _TAG_MATCH[match]


def _take_lists(ids_pp, dists_pp, counts, n):
    """The per-query arrays a range export handed out, copied into numpy arrays and released (hnsw_free_results)."""
    ids, dists = [], []
    try:
        for i in range(n):
            m = counts[i]
            if m == 0:
                ids.append(np.empty(0, dtype=np.int32))
                dists.append(np.empty(0, dtype=np.float32))
                continue
            ids.append(np.ctypeslib.as_array(ct.cast(ids_pp[i], _I), shape=(m,)).copy())
            dists.append(np.ctypeslib.as_array(ct.cast(dists_pp[i], _F), shape=(m,)).copy())
    finally:
        lib.hnsw_free_results(ids_pp, dists_pp, n)
    return ids, dists


def last_error() -> str:
    """The library's last error message (what the reference's `_last_error` returns, bindings.py:122-128):
    hnsw_get_last_error_utf8 reports the byte count it needs when asked with no buffer."""
    need = int(lib.hnsw_get_last_error_utf8(None, 0))
    if need < 1:
        return ""
    raw = (ct.c_char * (need + 1))()
    lib.hnsw_get_last_error_utf8(raw, need + 1)
    return bytes(raw).split(b"\0", 1)[0].decode("utf-8", "replace")


def _dev_error() -> str:
    buf = ct.create_string_buffer(1024)
    lib.hnswdev_last_error(buf, len(buf))
    return buf.value.decode("utf-8", "replace")


def allow_bits(allowed) -> Tuple[npt.NDArray[np.uint32], int]:
    """An allow-set in the C ABI's form (hnsw_mi355x_knn_query_filtered): (words, nbits), bit i = bit (i & 31) of word (i >> 5),
    ids >= nbits not allowed.  `allowed` is a bool mask indexed by id (ids past its end are not allowed) or an integer array of
    allowed ids (negative ids are an error)."""
    a = np.asarray(allowed)
    if a.dtype == np.bool_:
        mask = a.ravel()
    elif a.size == 0 or np.issubdtype(a.dtype, np.integer):
        ids = a.astype(np.int64).ravel()
        if ids.size and ids.min() < 0:
            raise ValueError("allowed ids must be >= 0")
        mask = np.zeros(int(ids.max()) + 1 if ids.size else 0, dtype=np.bool_)
        mask[ids] = True
    else:
        raise TypeError("allowed must be a bool mask indexed by id or an integer array of ids")
    nbits = int(mask.size)
    padded = np.zeros((nbits + 31) // 32 * 32, dtype=np.bool_)
    padded[:nbits] = mask
    words = np.packbits(padded.reshape(-1, 32), axis=1, bitorder="little").view("<u4").ravel().astype(np.uint32)
    return np.ascontiguousarray(words), nbits


def _id_list(ids) -> npt.NDArray[np.int32]:
    """The id list of a by-id call: a contiguous int32 vector (a scalar is a list of one)."""
    a = np.asarray(ids)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError("ids must be integers")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int32)


def _words_arg(words):
    """A pointer the C ABI accepts even for an empty set (NULL is an error there)."""
    if words.size == 0:
        words = np.zeros(1, dtype=np.uint32)
    return words, words.ctypes.data_as(ct.POINTER(ct.c_uint32))


def _as_2d_f32(x: npt.ArrayLike, dim_expected=None):
    """One vector or a batch of them as a C-contiguous float32 matrix (n, dim) -- the input contract of the
    reference's wrapper (bindings.py:131-139): a single vector becomes a batch of one, anything else that is not
    two-dimensional or has the wrong row length is a ValueError."""
    m = np.atleast_2d(np.asarray(x, dtype=np.float32))
    if m.ndim > 2 or np.ndim(x) == 0:
        raise ValueError("expected a 2D array of shape (n, dim) or a 1D vector")
    if dim_expected is not None and m.shape[1] != dim_expected:
        raise ValueError(f"expected dim={dim_expected}, got {m.shape[1]}")
    return np.require(m, dtype=np.float32, requirements="C")


class Index:
    """
    Python binding for the native HNSW index -- drop-in for the reference's `Index`
    (bindings/bindings.py:142-597) on the float32 add / knn_query path.

    The native index is created lazily on first insertion; configuration setters must be
    called before it (they mutate the process-global pending parameters that the next
    `hnsw_create` consumes, exactly as in the reference).
    """

    def __init__(self, dim: int, metric="sq_euclid"):
        self.dim = dim
        self.metric = metric
        self._initialized = False
        self._h = None

    def __del__(self):
        if getattr(self, "_h", None):
            lib.hnsw_free(self._h)
            self._h = None

    def _initialize(self):
        h = lib.hnsw_create(self.metric.encode("utf-8"))
        if not h:
            raise RuntimeError("hnsw_create failed: " + last_error())
        self._h = h
        self._initialized = True

    @staticmethod
    def _check(status):
        if status < 0:
            raise RuntimeError(last_error())

    # ---- the reference's setters (bindings.py:200-398) ----
    def set_collection_size(self, init_size: int):
        self._check(lib.hnsw_set_collection_size(init_size))

    def set_max_edges(self, max_conn: int):
        self._check(lib.hnsw_set_max_edges(max_conn))

    def set_max_candidates(self, max_candidates: int):
        self._check(lib.hnsw_set_max_candidates(max_candidates))

    def set_remove_max_candidates(self, rem_max_candidates: int):
        self._check(lib.hnsw_set_remove_max_candidates(rem_max_candidates))

    def set_distribution_rate(self, dist_rate: float):
        self._check(lib.hnsw_set_distribution_rate(dist_rate))

    def set_random_seed(self, random_seed: int):
        self._check(lib.hnsw_set_random_seed(random_seed))

    def set_min_nn(self, min_nn: int):
        self._check(lib.hnsw_set_min_nn(min_nn))

    def set_allow_removals(self, allow_removals: bool):
        self._check(lib.hnsw_set_allow_removals(allow_removals))

    # ---- backend knobs (not in the reference) ----
    def set_device(self, device: int):
        self._check(lib.hnsw_mi355x_set_device(device))

    def set_devices(self, n: int):
        """Device contexts of the index: knn_query shards its queries over n GPUs inside this process (include/hnsw_mi355x.h)."""
        self._check(lib.hnsw_mi355x_set_devices(n))

    def stats_at(self, context: int):
        st = DeviceStats()
        if not self._h or lib.hnsw_mi355x_get_stats_at(self._h, context, ct.byref(st)) != 0:
            raise RuntimeError(last_error() or "no such device context")
        return st.as_dict()

    def set_insert_batch(self, max_batch: int):
        """Cap of Add's snapshot batches.  0 (default) = the host's hardware threads: what the reference's Parallel.For can hold
        in flight here; 1 = strictly sequential inserts (HNSWIndex.Add(item)); -W = the same graph built through speculative
        windows of W items; larger caps (65536: rounds 1-4's schedule) are opt-in (see include/hnsw_mi355x.h)."""
        self._check(lib.hnsw_mi355x_set_insert_batch(max_batch))

    def set_insert_batch_live(self, max_batch: int):
        """The insert-batch knob on the index as it stands (pending like the others while nothing has been added)."""
        if not self._h:
            return self.set_insert_batch(max_batch)
        self._check(lib.hnsw_mi355x_index_set_insert_batch(self._h, max_batch))

    @property
    def insert_batch_cap(self) -> int:
        """The cap this index's Add runs under (the resolved default when nothing was set)."""
        return int(lib.hnsw_mi355x_index_insert_batch(self._h)) if self._h else host_parallelism()

    def exact_window_stats(self):
        """Counters of the exact-window Add: rounds, searches run, items inserted alone, items linked through windows."""
        out = (ct.c_uint64 * 4)()
        if not self._h or lib.hnsw_mi355x_exact_window_stats(self._h, out) != 0:
            return {"rounds": 0, "searches": 0, "alone": 0, "linked": 0}
        return {"rounds": int(out[0]), "searches": int(out[1]), "alone": int(out[2]), "linked": int(out[3])}

    def row_prefilter_stats(self):
        """Counters of KnnQuery's half-precision row prefilter: launches with it, rows measured on the shadow, rows re-read in f32,
        shadow rows packed."""
        out = (ct.c_uint64 * 4)()
        if not self._h or lib.hnsw_mi355x_row_prefilter_stats(self._h, out) != 0:
            return {"launches": 0, "rows_on_shadow": 0, "rows_reread": 0, "rows_packed": 0}
        return {"launches": int(out[0]), "rows_on_shadow": int(out[1]), "rows_reread": int(out[2]), "rows_packed": int(out[3])}

    def row_prefilter_form_stats(self):
        """Which kernel form the row prefilter's launches took: the one that reads the row length at run time, the one with it compiled in."""
        out = (ct.c_uint64 * 2)()
        if not self._h or lib.hnsw_mi355x_row_prefilter_form_stats(self._h, out) != 0:
            return {"runtime_dim": 0, "fixed_dim": 0}
        return {"runtime_dim": int(out[0]), "fixed_dim": int(out[1])}

    def row_prefilter_peek(self, first_id: int = 0, count: int = 0):
        """The row prefilter's shadow as it stands, read only: {"packed": the watermark (shadow rows [0, packed) are current),
        "e_bits": the 32 bits of E, "e": E as a float32, "rows": the shadow rows [first_id, first_id + count) widened to f32}.
        An index without a shadow has packed 0; a range that is not below the watermark is an error."""
        out = (ct.c_uint64 * 2)()
        rows = np.zeros((max(int(count), 0), self.dim), dtype=np.float32)
        if not self._h:
            if count > 0:
                raise RuntimeError("row_prefilter_peek: the index has no shadow rows")
            return {"packed": 0, "e_bits": 0, "e": np.float32(0), "rows": rows}
        self._check(lib.hnsw_mi355x_row_prefilter_peek(self._h, int(first_id), int(count), out, rows.ctypes.data_as(ct.POINTER(ct.c_float))))
        bits = int(out[1]) & 0xffffffff
        return {"packed": int(out[0]), "e_bits": bits, "e": np.array([bits], dtype=np.uint32).view(np.float32)[0], "rows": rows}

    def row_prefilter8_stats(self):
        """Counters of the 8-bit shadow of KnnQuery's row prefilter (dim 128): launches on it, rows packed into it, rows measured on it,
        rows re-read in f32, full packs (a fresh grid each), switches to the half-precision prefilter."""
        names = ("launches", "rows_packed", "rows_on_shadow", "rows_reread", "full_packs", "fallbacks_to_f16")
        out = (ct.c_uint64 * 6)()
        if not self._h or lib.hnsw_mi355x_row_prefilter8_stats(self._h, out) != 0:
            return dict.fromkeys(names, 0)
        return {name: int(v) for name, v in zip(names, out)}

    def row_prefilter8_peek(self, first_id: int = 0, count: int = 0):
        """The 8-bit shadow as it stands, read only: {"packed": the watermark, "lo", "step": the grid (float32; code c stands for
        fmaf(step, c, lo)), "e_bits" / "e": E8, "codes": the code bytes of rows [first_id, first_id + count), uint8 (count, 128)}."""
        out = (ct.c_uint64 * 4)()
        codes = np.zeros((max(int(count), 0), 128), dtype=np.uint8)
        f32 = lambda v: np.array([int(v) & 0xffffffff], dtype=np.uint32).view(np.float32)[0]
        if not self._h:
            if count > 0:
                raise RuntimeError("row_prefilter8_peek: the index has no 8-bit shadow rows")
            return {"packed": 0, "lo": np.float32(0), "step": np.float32(0), "e_bits": 0, "e": np.float32(0), "codes": codes}
        self._check(lib.hnsw_mi355x_row_prefilter8_peek(self._h, int(first_id), int(count), out, codes.ctypes.data_as(ct.POINTER(ct.c_uint8))))
        return {"packed": int(out[0]), "lo": f32(out[1]), "step": f32(out[2]), "e_bits": int(out[3]) & 0xffffffff, "e": f32(out[3]), "codes": codes}

    def set_remove_batch(self, max_batch: int):
        """1 (default): remove() takes the ids one after the other; B > 1: removals with disjoint neighbourhoods together."""
        self._check(lib.hnsw_mi355x_set_remove_batch(max_batch))

    def set_search_slots(self, slots: int):
        self._check(lib.hnsw_mi355x_set_search_slots(slots))

    def set_host_threads(self, threads: int):
        self._check(lib.hnsw_mi355x_set_host_threads(threads))

    def set_device_traversal(self, enabled: bool):
        """True (default): knn_query traverses on the device; False: host lock-step traversal."""
        self._check(lib.hnsw_mi355x_set_device_traversal(int(enabled)))

    # ---- data path ----
    def add(self, vecs: npt.ArrayLike) -> npt.NDArray[np.int32]:
        """bindings.py:400-441."""
        if not self._initialized:
            self._initialize()
        a = _as_2d_f32(vecs, self.dim)
        n, d = a.shape
        out_ids = np.empty(n, dtype=np.int32)
        rc = lib.hnsw_add(self._h, a.ctypes.data_as(_F), int(n), int(d), out_ids.ctypes.data_as(_I))
        if rc < 0:
            raise RuntimeError(last_error())
        return out_ids[:rc].copy()

    def remove(self, ids: npt.ArrayLike) -> None:
        """bindings.py:443-472."""
        arr = np.asarray(ids, dtype=np.int32).ravel()
        if arr.size == 0:
            return
        result = lib.hnsw_remove(self._h, arr.ctypes.data_as(_I), int(arr.size))
        if result < 0:
            raise RuntimeError(last_error())

    def knn_query(self, queries: npt.ArrayLike, k: int, allowed=None, layer: int = 0) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """bindings.py:474-521.  allowed (not in the reference's Python class; its C# KnnQuery takes a filterFnc): a bool mask
        indexed by id or an integer array of allowed ids -- only those ids are results (hnsw_mi355x_knn_query_filtered).
        layer (the C# KnnQuery's `layer`): search that layer's nodes only (hnsw_mi355x_knn_query_at_layer); outside
        0 .. top_layer() on a non-empty index: RuntimeError."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        ids = np.empty((n, k), dtype=np.int32)
        dists = np.empty((n, k), dtype=np.float32)
        if layer != 0:
            ids.fill(-1)          # (an index nothing was added to has no native handle yet: padding, as an empty index answers)
            dists.fill(np.nan)
            words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
            words, wp = _words_arg(words) if allowed is not None else (None, None)
            status = lib.hnsw_mi355x_knn_query_at_layer(self._h, q.ctypes.data_as(_F), n, self.dim, k, int(layer), wp, nbits, ids.ctypes.data_as(_I),
                                                        dists.ctypes.data_as(_F))
            if status < 0:
                raise RuntimeError(last_error())
            return ids, dists
        if allowed is not None:
            words, nbits = allow_bits(allowed)
            words, wp = _words_arg(words)
            status = lib.hnsw_mi355x_knn_query_filtered(self._h, q.ctypes.data_as(_F), n, self.dim, k, wp, nbits, ids.ctypes.data_as(_I),
                                                        dists.ctypes.data_as(_F))
            if status < 0:
                raise RuntimeError(last_error())
            return ids, dists
        status = lib.hnsw_knn_query(self._h, q.ctypes.data_as(_F), n, self.dim, k, ids.ctypes.data_as(_I),
                                    dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists  # freshly allocated above (the reference returns copies of equally fresh arrays, bindings.py:521)

    def exact_knn_query(self, queries: npt.ArrayLike, k: int, allowed=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """The k live (and, with `allowed`, allowed) ids of smallest distance per query, ascending by (distance, id), from a flat
        scan on the device (hnsw_mi355x_exact_knn_query): exact, independent of the graph.  allowed: as for knn_query.
        1 <= k <= 1024; rows that run out of candidates are padded with -1 / NaN."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        status = lib.hnsw_mi355x_exact_knn_query(self._h, q.ctypes.data_as(_F), n, self.dim, k, wp, nbits, ids.ctypes.data_as(_I),
                                                 dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    def exact_knn_query_grouped(self, queries: npt.ArrayLike, k: int, row_group, query_group,
                                n_groups=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """exact_knn_query with a candidate group per query, every group in one scan (hnsw_mi355x_exact_knn_query_grouped):
        row_group[id] is the group of an id (a value outside 0 .. n_groups - 1, or an id past the array's end: no group),
        query_group[i] the group query i is answered from.  n_groups None: the largest value in either array plus one.  Per
        group the rows equal exact_knn_query(queries[query_group == g], k, allowed=(row_group == g))."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        status = lib.hnsw_mi355x_exact_knn_query_grouped(self._h, q.ctypes.data_as(_F), n, self.dim, k, rg.ctypes.data_as(_I), rg.shape[0],
                                                         qg.ctypes.data_as(_I), ng, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    def exact_knn_query_collapsed(self, queries: npt.ArrayLike, k: int, row_group, per_group: int = 1,
                                  allowed=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """exact_knn_query with at most per_group results per label (hnsw_mi355x_exact_knn_query_collapsed): row_group[id] is the
        label of an id -- the document a chunk belongs to -- and needs an entry for every id below length().  Per query the live
        (allowed) ids are walked in exact_knn_query's order, ascending (distance, id); an id is kept while fewer than per_group
        kept ids have its label, until k are kept; rows that run out are padded with -1 / NaN.  Labels are compared for equality
        (negative values are labels like any).  Exact, in one scan; per_group == k returns exact_knn_query's rows byte for byte.
        1 <= per_group <= k <= 1024."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rg = _collapse_args(row_group, k, per_group, self.length)
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        status = lib.hnsw_mi355x_exact_knn_query_collapsed(self._h, q.ctypes.data_as(_F), n, self.dim, k, rg.ctypes.data_as(_I), rg.shape[0], int(per_group),
                                                           wp, nbits, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    def knn_query_collapsed(self, queries: npt.ArrayLike, k: int, row_group, per_group: int = 1, beam=None, allowed=None,
                            layer: int = 0) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """The traversal form of exact_knn_query_collapsed (hnsw_mi355x_knn_query_collapsed): per query the first k survivors of the
        same walk -- an id is kept while fewer than per_group kept ids have its label row_group[id] -- over the row that
        knn_query(q, beam, allowed=allowed, layer=layer) returns, in that row's own order, padding skipped; byte for byte.  beam
        defaults to 4 * k and may be any value >= k that knn_query accepts as k.  Approximate exactly as far as knn_query at that
        beam is: what the traversal does not reach at width beam is not in the result, and a label with many near rows uses up
        beam entries -- exact_knn_query_collapsed is the exact call.  Where the traversal runs on the device the rows are
        collapsed there and only k columns come back."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        beam = 4 * int(k) if beam is None else int(beam)
        if k >= 1 and beam < k:
            raise ValueError(f"beam = {beam} is below k = {k}")
        rg = _collapse_args(row_group, k, per_group, self.length, k_limit=None)   # (k and beam: whatever knn_query accepts)
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        status = lib.hnsw_mi355x_knn_query_collapsed(self._h, q.ctypes.data_as(_F), n, self.dim, k, beam, rg.ctypes.data_as(_I), rg.shape[0], int(per_group),
                                                     int(layer), wp, nbits, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    def knn_query_grouped(self, queries: npt.ArrayLike, k: int, row_group, query_group, n_groups=None,
                          layer: int = 0) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """knn_query with a group filter per query, every group in one device traversal (hnsw_mi355x_knn_query_grouped):
        row_group[id] is the group of an id (a value outside 0 .. n_groups - 1, or an id past the array's end: no group),
        query_group[i] the group query i is answered from.  n_groups None: the largest value in either array plus one.  Per
        group the rows equal knn_query(queries[query_group == g], k, allowed=(row_group == g), layer=layer), ids and distance
        bits; a query whose group holds no id of the graph gets a padded row."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        status = lib.hnsw_mi355x_knn_query_grouped(self._h, q.ctypes.data_as(_F), n, self.dim, k, int(layer), rg.ctypes.data_as(_I), rg.shape[0],
                                                   qg.ctypes.data_as(_I), ng, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    def knn_query_tagged(self, queries: npt.ArrayLike, k: int, row_tags, query_tags, match: str = "any",
                         layer: int = 0) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """knn_query with a tag mask per query, every mask in one device traversal (hnsw_mi355x_knn_query_tagged): row_tags[id] is
        a uint32 with one bit per tag (an id past the array's end, or the word 0: no tag), query_tags[i] the mask of query i.
        match "any": id is a candidate of query i when row_tags[id] & query_tags[i] != 0; "all": when query_tags[i] != 0 and
        row_tags[id] & query_tags[i] == query_tags[i].  Per distinct mask m the rows equal
        knn_query(queries[query_tags == m], k, allowed=<the ids that match m>, layer=layer), ids and distance bits; a query whose mask
        has no candidate gets a padded row."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        status = lib.hnsw_mi355x_knn_query_tagged(self._h, q.ctypes.data_as(_F), n, self.dim, k, int(layer), rt.ctypes.data_as(_U32), rt.shape[0],
                                                  qt.ctypes.data_as(_U32), mode, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    def exact_knn_query_tagged(self, queries: npt.ArrayLike, k: int, row_tags, query_tags,
                               match: str = "any") -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """exact_knn_query with knn_query_tagged's tag mask per query (hnsw_mi355x_exact_knn_query_tagged): per distinct mask m the rows
        equal exact_knn_query(queries[query_tags == m], k, allowed=<the ids that match m>).  1 <= k <= 1024."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        ids = np.full((n, max(k, 0)), -1, dtype=np.int32)   # (an index nothing was added to has no native handle yet: padding)
        dists = np.full((n, max(k, 0)), np.nan, dtype=np.float32)
        status = lib.hnsw_mi355x_exact_knn_query_tagged(self._h, q.ctypes.data_as(_F), n, self.dim, k, rt.ctypes.data_as(_U32), rt.shape[0],
                                                        qt.ctypes.data_as(_U32), mode, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if status < 0:
            raise RuntimeError(last_error())
        return ids, dists

    # ---- query by stored id ----
    def _by_id_list(self, ids, who: str) -> npt.NDArray[np.int32]:
        a = _id_list(ids)
        if a.size and not self._h:   # (an index nothing was added to has no native handle yet, and no live id)
            raise RuntimeError(f"System.Collections.Generic.KeyNotFoundException: {who}: ids[0] = {int(a[0])} is not a live id")
        return a

    def get_vectors(self, ids) -> npt.NDArray[np.float32]:
        """float32[n, dim]: the stored rows of `ids` (hnsw_mi355x_get_vectors), gathered on the device -- the values distances are
        measured on: float32 rows as added, half-precision rows rounded and widened, int8 rows q * scale.  ids may repeat and come
        in any order; one that is not live: RuntimeError naming it."""
        a = self._by_id_list(ids, "hnsw_mi355x_get_vectors")
        out = np.empty((a.size, self.dim), dtype=np.float32)
        if a.size and lib.hnsw_mi355x_get_vectors(self._h, a.ctypes.data_as(_I), a.size, out.ctypes.data_as(_F)) < 0:
            raise RuntimeError(last_error())
        return out

    def items(self) -> npt.NDArray[np.float32]:
        """HNSWIndex.Items(): the stored rows of every live id, in ids() order (get_vectors(ids()))."""
        return self.get_vectors(self.ids())

    def knn_query_by_id(self, ids, k: int, layer: int = 0) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """"What is near item i": knn_query for the stored rows of `ids`, each answered from every id but its own, without a vector
        crossing the host boundary (hnsw_mi355x_knn_query_by_id).  Row i is byte for byte
        knn_query(get_vectors([ids[i]]), k, allowed=<every id except ids[i]>, layer=layer); a duplicate of the row under another id is
        an ordinary candidate.  An id that is not live: RuntimeError naming it."""
        a = self._by_id_list(ids, "hnsw_mi355x_knn_query_by_id")
        out_ids = np.full((a.size, max(k, 0)), -1, dtype=np.int32)
        dists = np.full((a.size, max(k, 0)), np.nan, dtype=np.float32)
        if a.size and lib.hnsw_mi355x_knn_query_by_id(self._h, a.ctypes.data_as(_I), a.size, k, int(layer), out_ids.ctypes.data_as(_I),
                                                      dists.ctypes.data_as(_F)) < 0:
            raise RuntimeError(last_error())
        return out_ids, dists

    def exact_knn_query_by_id(self, ids, k: int, allowed=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """exact_knn_query for the stored rows of `ids` (hnsw_mi355x_exact_knn_query_by_id): row i equals
        exact_knn_query(get_vectors([ids[i]]), k, allowed=<allowed, or every live id, minus ids[i]>) -- ascending by (distance, id),
        padded where the candidates run out (n live items give at most n - 1 results).  1 <= k <= 1024."""
        a = self._by_id_list(ids, "hnsw_mi355x_exact_knn_query_by_id")
        out_ids = np.full((a.size, max(k, 0)), -1, dtype=np.int32)
        dists = np.full((a.size, max(k, 0)), np.nan, dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        if a.size and lib.hnsw_mi355x_exact_knn_query_by_id(self._h, a.ctypes.data_as(_I), a.size, k, wp, nbits, out_ids.ctypes.data_as(_I),
                                                            dists.ctypes.data_as(_F)) < 0:
            raise RuntimeError(last_error())
        return out_ids, dists

    def exact_knn_graph(self, k: int, ids=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """The exact k-NN graph of the index: exact_knn_query_by_id over `ids` (None: every live id ascending), (int32[n, k],
        float32[n, k]).  Row i never holds ids[i].  The ids go down in pieces of 65 536, so the gathered query set stays bounded;
        inside a piece the scan picks its rounds as for any call."""
        a = np.sort(self.ids()) if ids is None else _id_list(ids)
        out_ids = np.full((a.size, max(k, 0)), -1, dtype=np.int32)
        dists = np.full((a.size, max(k, 0)), np.nan, dtype=np.float32)
        for lo in range(0, a.size, _BY_ID_CHUNK):
            out_ids[lo:lo + _BY_ID_CHUNK], dists[lo:lo + _BY_ID_CHUNK] = self.exact_knn_query_by_id(a[lo:lo + _BY_ID_CHUNK], k)
        return out_ids, dists

    # ---- near-duplicates of stored items ----
    def exact_range_query_by_id(self, ids, radius: float,
                                allowed=None) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """"Which stored items lie within `radius` of item i": exact_range_query for the stored rows of `ids`
        (hnsw_mi355x_exact_range_query_by_id).  List i is byte for byte
        exact_range_query(get_vectors([ids[i]]), radius, allowed=<allowed, or every live id, minus ids[i]>): ascending by (distance, id);
        a duplicate of the row under another id is an ordinary result.  ids may repeat and come in any order; one that is not live:
        RuntimeError naming it."""
        a = self._by_id_list(ids, "hnsw_mi355x_exact_range_query_by_id")
        n = int(a.size)
        ids_pp = (ct.c_void_p * max(n, 1))()
        dists_pp = (ct.c_void_p * max(n, 1))()
        counts = (ct.c_int * max(n, 1))()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        if n and lib.hnsw_mi355x_exact_range_query_by_id(self._h, a.ctypes.data_as(_I), n, radius, wp, nbits, ids_pp, dists_pp, counts) < 0:
            raise RuntimeError(last_error())
        out_ids, dists = [], []
        try:
            for i in range(n):
                m = counts[i]
                out_ids.append(np.ctypeslib.as_array(ct.cast(ids_pp[i], _I), shape=(m,)).copy() if m else np.empty(0, dtype=np.int32))
                dists.append(np.ctypeslib.as_array(ct.cast(dists_pp[i], _F), shape=(m,)).copy() if m else np.empty(0, dtype=np.float32))
        finally:
            if n:
                lib.hnsw_free_results(ids_pp, dists_pp, n)
        return out_ids, dists

    def exact_radius_graph(self, radius: float, ids=None) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """The exact radius graph of the index: exact_range_query_by_id over `ids` (None: every live id ascending), the lists
        concatenated.  List i never holds ids[i].  The ids go down in pieces of 65 536, as exact_knn_graph's."""
        a = np.sort(self.ids()) if ids is None else _id_list(ids)
        out_ids, dists = [], []
        for lo in range(0, a.size, _BY_ID_CHUNK):
            got_ids, got_d = self.exact_range_query_by_id(a[lo:lo + _BY_ID_CHUNK], radius)
            out_ids += got_ids
            dists += got_d
        return out_ids, dists

    def duplicate_groups(self, radius: float, allowed=None) -> Tuple[npt.NDArray[np.int32], dict]:
        """Groups of near-duplicates (hnsw_mi355x_duplicate_groups): (int32[length], info).  The members are the live ids `allowed`
        allows (None: every live id); members a < b are joined when the distance from the stored row of a, taken as the query, to
        row b is <= radius, and the groups are the connected components.  labels[v]: the smallest member id of v's group, -1 where v
        is no member.  info: members, groups, pairs_within (a < b within the radius), pairs_measured (= m (m - 1) / 2).  One scan on
        the device with a union-find as its sink: no list is built or copied."""
        n = int(self.length)
        labels = np.full(n, -1, dtype=np.int32)
        info = (ct.c_uint64 * 4)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        if self._h and lib.hnsw_mi355x_duplicate_groups(self._h, radius, wp, nbits, labels.ctypes.data_as(_I), n, info) < 0:
            raise RuntimeError(last_error())
        return labels, {name: int(info[i]) for i, name in enumerate(_GROUPS_INFO)}

    # ---- density clusters ----
    def _density(self, radius, min_samples, allowed, want_labels):
        if int(min_samples) < 1:    # (said here as well: an index that holds nothing yet has no handle to say it)
            raise ValueError("density_clusters: min_samples = %d is below 1" % int(min_samples))
        n = int(self.length)
        labels = np.full(n, -1, dtype=np.int32) if want_labels else None
        counts = np.full(n, -1, dtype=np.int32)
        info = (ct.c_uint64 * 8)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        lp = labels.ctypes.data_as(_I) if want_labels else None
        if self._h and lib.hnsw_mi355x_density_clusters(self._h, radius, int(min_samples), wp, nbits, lp, counts.ctypes.data_as(_I), n, info) < 0:
            raise RuntimeError(last_error())
        return labels, counts, {name: int(info[i]) for i, name in enumerate(_DENSITY_INFO)}

    def density_clusters(self, radius: float, min_samples: int, allowed=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.int32], dict]:
        """DBSCAN over the stored rows (hnsw_mi355x_density_clusters): (labels int32[length], counts int32[length], info).  The
        members and the pair rule are duplicate_groups', which is this call at min_samples = 1: members a < b are within when the
        distance from the stored row of a, taken as the query, to row b is <= radius.  counts[v]: the within pairs that hold v, -1
        where v is no member.  A member is core when counts[v] + 1 >= min_samples.  The clusters are the connected components of the
        core members under the within pairs between two of them; labels[v] of a core member is the smallest core id of its cluster.
        A member that is not core takes the label of its core within-neighbour of smallest (distance, id) -- a border -- or -1 -- noise;
        a non-member has -1 as well.  info: members, clusters, core, border, noise, pairs_within, pairs_measured (m (m - 1) / 2 per
        scan), scans (1, or 2 where the within pairs did not fit the device's pair arena; 0 with fewer than two members)."""
        return self._density(radius, min_samples, allowed, True)

    def neighbor_counts(self, radius: float, allowed=None) -> npt.NDArray[np.int32]:
        """The local density alone (hnsw_mi355x_density_clusters with no labels): int32[length], counts[v] the members within
        `radius` of member v -- density_clusters' counts -- and -1 where v is no member.  One scan; no pair is kept, nothing is joined."""
        return self._density(radius, 1, allowed, False)[1]

    # ---- near-duplicates over the graph's edges ----
    def graph_duplicate_groups(self, radius: float, allowed=None) -> Tuple[npt.NDArray[np.int32], dict]:
        """duplicate_groups asked of the graph (hnsw_mi355x_graph_duplicate_groups): (int32[length], info).  The members are
        duplicate_groups'; what joins two of them is a layer-0 edge (i, j) -- j in i's list -- whose distance, the stored row of i
        taken as the query, is <= radius; the groups are the connected components, labelled with their smallest member id, -1
        where v is no member.  n x (at most 2 MaxEdges) distances instead of m (m - 1) / 2: duplicate_groups' grouping or a
        refinement of it -- near-duplicates that no path of such edges connects stay apart.  info: members, groups, edges_within and
        edges_measured (directed), launches (of the edge kernel)."""
        n = int(self.length)
        labels = np.full(n, -1, dtype=np.int32)
        info = (ct.c_uint64 * 5)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        if self._h and lib.hnsw_mi355x_graph_duplicate_groups(self._h, radius, wp, nbits, labels.ctypes.data_as(_I), n, info) < 0:
            raise RuntimeError(last_error())
        return labels, {name: int(info[i]) for i, name in enumerate(_EDGE_GROUPS_INFO)}

    def near_edges(self, radius: float, allowed=None) -> Tuple[npt.NDArray[np.int32], npt.NDArray[np.int32], npt.NDArray[np.float32]]:
        """The layer-0 edges between members that lie within `radius` (hnsw_mi355x_near_edges + _results): (src, dst, dist), ascending
        by src and, inside one src, by (distance, dst) -- that item's exact_range_query_by_id list restricted to its adjacency list,
        with that list's distance bits.  Directed: two items that list each other appear twice."""
        count = ct.c_longlong(0)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        if self._h and lib.hnsw_mi355x_near_edges(self._h, radius, wp, nbits, ct.byref(count)) < 0:
            raise RuntimeError(last_error())
        n = int(count.value)
        src, dst, d = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
        if n and lib.hnsw_mi355x_near_edges_results(self._h, src.ctypes.data_as(_I), dst.ctypes.data_as(_I), d.ctypes.data_as(_F), n) < 0:
            raise RuntimeError(last_error())
        return src, dst, d

    def exact_range_query(self, queries: npt.ArrayLike, radius: float,
                          allowed=None) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """Per query every live (and, with `allowed`, allowed) id whose distance is <= radius, ascending by (distance, id), from
        the flat scan on the device (hnsw_mi355x_exact_range_query): exact, independent of the graph, of any length.  allowed: as
        for knn_query.  The shape range_query returns."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        ids_pp = (ct.c_void_p * n)()
        dists_pp = (ct.c_void_p * n)()
        counts = (ct.c_int * n)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        status = lib.hnsw_mi355x_exact_range_query(self._h, q.ctypes.data_as(_F), n, self.dim, radius, wp, nbits, ids_pp, dists_pp, counts)
        if status < 0:
            raise RuntimeError(last_error())
        ids, dists = [], []
        try:
            for i in range(n):
                m = counts[i]
                if m == 0:
                    ids.append(np.empty(0, dtype=np.int32))
                    dists.append(np.empty(0, dtype=np.float32))
                    continue
                ids.append(np.ctypeslib.as_array(ct.cast(ids_pp[i], _I), shape=(m,)).copy())
                dists.append(np.ctypeslib.as_array(ct.cast(dists_pp[i], _F), shape=(m,)).copy())
        finally:
            lib.hnsw_free_results(ids_pp, dists_pp, n)
        return ids, dists

    def exact_range_query_grouped(self, queries: npt.ArrayLike, radius: float, row_group, query_group,
                                  n_groups=None) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """exact_range_query with a candidate group per query, every group in one scan (hnsw_mi355x_exact_range_query_grouped):
        row_group / query_group / n_groups as for exact_knn_query_grouped.  Per group the lists equal
        exact_range_query(queries[query_group == g], radius, allowed=(row_group == g)); they come back in the caller's order."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        ids_pp = (ct.c_void_p * n)()
        dists_pp = (ct.c_void_p * n)()
        counts = (ct.c_int * n)()
        status = lib.hnsw_mi355x_exact_range_query_grouped(self._h, q.ctypes.data_as(_F), n, self.dim, radius, rg.ctypes.data_as(_I), rg.shape[0],
                                                           qg.ctypes.data_as(_I), ng, ids_pp, dists_pp, counts)
        if status < 0:
            raise RuntimeError(last_error())
        ids, dists = [], []
        try:
            for i in range(n):
                m = counts[i]
                if m == 0:
                    ids.append(np.empty(0, dtype=np.int32))
                    dists.append(np.empty(0, dtype=np.float32))
                    continue
                ids.append(np.ctypeslib.as_array(ct.cast(ids_pp[i], _I), shape=(m,)).copy())
                dists.append(np.ctypeslib.as_array(ct.cast(dists_pp[i], _F), shape=(m,)).copy())
        finally:
            lib.hnsw_free_results(ids_pp, dists_pp, n)
        return ids, dists

    def range_query(self, queries: npt.ArrayLike, radius: float,
                    allowed=None, layer: int = 0) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """bindings.py:523-597.  allowed: as for knn_query -- only those ids are results (hnsw_mi355x_range_query_filtered); where
        the reference throws on an empty heap (radius < 0) RuntimeError carries its message.  layer: as for knn_query
        (hnsw_mi355x_range_query_at_layer)."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        ids_pp = (ct.c_void_p * n)()
        dists_pp = (ct.c_void_p * n)()
        counts = (ct.c_int * n)()
        if layer != 0:
            words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
            words, wp = _words_arg(words) if allowed is not None else (None, None)
            status = lib.hnsw_mi355x_range_query_at_layer(self._h, q.ctypes.data_as(_F), n, self.dim, radius, int(layer), wp, nbits, ids_pp, dists_pp, counts)
        elif allowed is not None:
            words, nbits = allow_bits(allowed)
            words, wp = _words_arg(words)
            status = lib.hnsw_mi355x_range_query_filtered(self._h, q.ctypes.data_as(_F), n, self.dim, radius, wp, nbits, ids_pp, dists_pp, counts)
        else:
            status = lib.hnsw_range_query(self._h, q.ctypes.data_as(_F), n, self.dim, radius, ids_pp, dists_pp, counts)
        if status < 0:
            raise RuntimeError(last_error())
        ids, dists = [], []
        try:
            for i in range(n):
                m = counts[i]
                if m == 0:
                    ids.append(np.empty(0, dtype=np.int32))
                    dists.append(np.empty(0, dtype=np.float32))
                    continue
                ids.append(np.ctypeslib.as_array(ct.cast(ids_pp[i], _I), shape=(m,)).copy())
                dists.append(np.ctypeslib.as_array(ct.cast(dists_pp[i], _F), shape=(m,)).copy())
        finally:
            lib.hnsw_free_results(ids_pp, dists_pp, n)
        return ids, dists

    def range_query_grouped(self, queries: npt.ArrayLike, radius: float, row_group, query_group, n_groups=None,
                            layer: int = 0) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """range_query with a group filter per query, every group in one device traversal (hnsw_mi355x_range_query_grouped):
        row_group / query_group / n_groups as for knn_query_grouped.  Per group the lists equal
        range_query(queries[query_group == g], radius, allowed=(row_group == g), layer=layer), the order among equal distances
        included; where the reference throws on an empty heap (radius < 0) RuntimeError carries its message."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        ids_pp = (ct.c_void_p * n)()
        dists_pp = (ct.c_void_p * n)()
        counts = (ct.c_int * n)()
        status = lib.hnsw_mi355x_range_query_grouped(self._h, q.ctypes.data_as(_F), n, self.dim, radius, int(layer), rg.ctypes.data_as(_I), rg.shape[0],
                                                     qg.ctypes.data_as(_I), ng, ids_pp, dists_pp, counts)
        if status < 0:
            raise RuntimeError(last_error())
        ids, dists = [], []
        try:
            for i in range(n):
                m = counts[i]
                if m == 0:
                    ids.append(np.empty(0, dtype=np.int32))
                    dists.append(np.empty(0, dtype=np.float32))
                    continue
                ids.append(np.ctypeslib.as_array(ct.cast(ids_pp[i], _I), shape=(m,)).copy())
                dists.append(np.ctypeslib.as_array(ct.cast(dists_pp[i], _F), shape=(m,)).copy())
        finally:
            lib.hnsw_free_results(ids_pp, dists_pp, n)
        return ids, dists

    def range_query_tagged(self, queries: npt.ArrayLike, radius: float, row_tags, query_tags, match: str = "any",
                           layer: int = 0) -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """range_query with a tag mask per query, every mask in one device traversal (hnsw_mi355x_range_query_tagged): row_tags /
        query_tags / match as for knn_query_tagged.  Per distinct mask m the lists equal
        range_query(queries[query_tags == m], radius, allowed=<the ids that match m>, layer=layer), the order among equal distances
        included; where the reference throws on an empty heap (radius < 0) RuntimeError carries its message."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        ids_pp = (ct.c_void_p * n)()
        dists_pp = (ct.c_void_p * n)()
        counts = (ct.c_int * n)()
        status = lib.hnsw_mi355x_range_query_tagged(self._h, q.ctypes.data_as(_F), n, self.dim, radius, int(layer), rt.ctypes.data_as(_U32), rt.shape[0],
                                                    qt.ctypes.data_as(_U32), mode, ids_pp, dists_pp, counts)
        if status < 0:
            raise RuntimeError(last_error())
        return _take_lists(ids_pp, dists_pp, counts, n)

    def exact_range_query_tagged(self, queries: npt.ArrayLike, radius: float, row_tags, query_tags,
                                 match: str = "any") -> Tuple[List[npt.NDArray[np.int32]], List[npt.NDArray[np.float32]]]:
        """exact_range_query with a tag mask per query (hnsw_mi355x_exact_range_query_tagged): row_tags / query_tags / match as for
        knn_query_tagged.  Per distinct mask m the lists equal
        exact_range_query(queries[query_tags == m], radius, allowed=<the ids that match m>); they come back in the caller's order."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        ids_pp = (ct.c_void_p * n)()
        dists_pp = (ct.c_void_p * n)()
        counts = (ct.c_int * n)()
        status = lib.hnsw_mi355x_exact_range_query_tagged(self._h, q.ctypes.data_as(_F), n, self.dim, radius, rt.ctypes.data_as(_U32), rt.shape[0],
                                                          qt.ctypes.data_as(_U32), mode, ids_pp, dists_pp, counts)
        if status < 0:
            raise RuntimeError(last_error())
        return _take_lists(ids_pp, dists_pp, counts, n)

    # ---- measurement aid: query set resident in HBM across calls ----
    def set_resident_queries(self, queries: npt.ArrayLike):
        q = _as_2d_f32(queries, self.dim)
        if lib.hnsw_mi355x_set_queries(self._h, q.ctypes.data_as(_F), int(q.shape[0]), self.dim) < 0:
            raise RuntimeError(last_error())

    def multilayer_knn_query(self, queries: npt.ArrayLike, k: int, max_layer=None, min_layer: int = 0):
        """The C# MultiLayerKnnQuery for a batch of independent queries (hnsw_mi355x_multilayer_knn_query): (ids, dists) of shape
        [nq, nlayers, k - 1], nlayers = min(top_layer(), max_layer) + 1 -- slot L holds layer L's neighbours in distance order without
        the nearest one (it is the entry point of the layer below), -1 / NaN where a layer has fewer and in slots below min_layer."""
        q = _as_2d_f32(queries, self.dim)
        n = int(q.shape[0])
        cap = max(self.top_layer() + 1, 1)
        per = max(int(k) - 1, 0)
        ids = np.full((n, cap, per), -1, dtype=np.int32)
        dists = np.full((n, cap, per), np.nan, dtype=np.float32)
        nl = lib.hnsw_mi355x_multilayer_knn_query(self._h, q.ctypes.data_as(_F), n, self.dim, int(k), 2 ** 31 - 1 if max_layer is None else int(max_layer),
                                                  int(min_layer), cap, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F))
        if nl < 0:
            raise RuntimeError(last_error())
        return np.ascontiguousarray(ids[:, :nl]), np.ascontiguousarray(dists[:, :nl])

    def top_layer(self) -> int:
        """max_layer(entry_point): the highest layer of the graph (-1: empty index)."""
        ep = self.entry_point
        return self.max_layer(ep) if ep >= 0 else -1

    def knn_query_resident(self, k: int):
        n = int(lib.hnsw_mi355x_resident_count(self._h)) if self._h else 0  # asked, not remembered: knn_query / range_query replace the set
        if n <= 0:
            raise RuntimeError("no resident query set: call set_resident_queries first (range_query discards it)")
        ids = np.empty((n, k), dtype=np.int32)
        dists = np.empty((n, k), dtype=np.float32)
        if lib.hnsw_mi355x_knn_query_resident(self._h, k, ids.ctypes.data_as(_I), dists.ctypes.data_as(_F)) < 0:
            raise RuntimeError(last_error())
        return ids, dists

    # ---- introspection (parity checks, measurement) ----
    @property
    def count(self) -> int:
        return lib.hnsw_mi355x_count(self._h) if self._h else 0

    @property
    def entry_point(self) -> int:
        return lib.hnsw_mi355x_entry_point(self._h) if self._h else -1

    def max_layer(self, i: int) -> int:
        return lib.hnsw_mi355x_node_max_layer(self._h, int(i))

    @property
    def length(self) -> int:
        """Slots ever allocated; every id is < length (removed slots are reused by later adds)."""
        return lib.hnsw_mi355x_length(self._h) if self._h else 0

    def ids(self):
        """HNSWIndex.Ids(): live ids."""
        out = np.empty(max(1, self.count), dtype=np.int32)
        n = lib.hnsw_mi355x_active_ids(self._h, out.ctypes.data_as(_I), out.size) if self._h else 0
        return out[:n].copy()

    def levels(self):
        out = np.empty(self.length, dtype=np.int32)
        if out.size:
            lib.hnsw_mi355x_export_levels(self._h, out.ctypes.data_as(_I), out.size)
        return out

    def export_edges(self, layer: int, stride: int):
        """(counts[n], edges[n, stride]) of one layer; counts == -1 where the node is absent."""
        n = self.length
        counts = np.empty(n, dtype=np.int32)
        edges = np.zeros((n, stride), dtype=np.int32)
        if n and lib.hnsw_mi355x_export_edges(self._h, int(layer), counts.ctypes.data_as(_I), edges.ctypes.data_as(_I),
                                              int(stride), n) < 0:
            raise RuntimeError("export_edges: stride too small")
        return counts, edges

    def edges(self, i: int, layer: int):
        buf = np.empty(4096, dtype=np.int32)
        n = lib.hnsw_mi355x_get_out_edges(self._h, int(i), int(layer), buf.ctypes.data_as(_I), buf.size)
        if n < 0:
            raise IndexError((i, layer))
        return buf[:n].copy()

    # ---- HNSWIndex.GetInfo / GetConnectedComponentCounts (src/HNSWIndex/HNSWIndex.cs:192-205) ----
    def get_info(self) -> List[dict]:
        """HNSWIndex.GetInfo(): one dict per layer 0 .. top with the fields of hnsw_mi355x_layer_info (HNSWInfo.LayerInfo), computed
        on the device from the graph mirror.  An index with no items raises, as the reference does (IndexOutOfRangeException)."""
        if not self._initialized:
            self._initialize()
        cap = 16
        while True:
            out = (LayerInfo * cap)()
            n = lib.hnsw_mi355x_get_info(self._h, out, cap)
            if n < 0:
                raise RuntimeError(last_error())
            if n <= cap:
                return [out[i].as_dict() for i in range(n)]
            cap = n

    def connected_component_counts(self) -> npt.NDArray[np.int32]:
        """HNSWIndex.GetConnectedComponentCounts(): weakly connected components per layer 0 .. top, counted on the device from the
        graph mirror; an empty array for an empty index."""
        if not self._initialized:
            self._initialize()
        out = np.zeros(16, dtype=np.int32)
        while True:
            n = lib.hnsw_mi355x_connected_component_counts(self._h, out.ctypes.data_as(_I), out.size)
            if n < 0:
                raise RuntimeError(last_error())
            if n <= out.size:
                return out[:n].copy()
            out = np.zeros(n, dtype=np.int32)

    # ---- reachability from the entry point over out-edges ----
    def reachability(self) -> List[dict]:
        """One dict per layer 0 .. top with the fields of hnsw_mi355x_layer_reach: the layer's members, the seeds that arrive from the
        layer above (the entry point on the top layer), how many members a traversal from them can reach over out-edges, and the
        largest hop count.  Computed on the device from the graph mirror; an empty list for an empty index."""
        if not self._initialized:
            self._initialize()
        cap = 16
        while True:
            out = (LayerReach * cap)()
            n = lib.hnsw_mi355x_reachability(self._h, out, cap)
            if n < 0:
                raise RuntimeError(last_error())
            if n <= cap:
                return [out[i].as_dict() for i in range(n)]
            cap = n

    def unreachable_ids(self, layer: int = 0) -> npt.NDArray[np.int32]:
        """The live members of `layer` that no query on that layer can return, ascending: they are outside everything the entry
        point reaches over out-edges (a necessary condition for being found, not a sufficient one).  exact_knn_query returns them."""
        if not self._initialized:
            self._initialize()
        out = np.zeros(max(1, self.count), dtype=np.int32)   # room for every live id: one call, one walk of the chain
        n = lib.hnsw_mi355x_unreachable_ids(self._h, int(layer), out.ctypes.data_as(_I), out.size)
        if n < 0:
            raise RuntimeError(last_error())
        return out[:n].copy()

    def hop_counts(self, layer: int = 0) -> npt.NDArray[np.int32]:
        """Per id < length: the hop count at which the chain from the entry point first reaches it on `layer` (>= 0), -1 for a member
        of the layer that is not reached, -2 for an id that is no member (removed, or below the layer)."""
        if not self._initialized:
            self._initialize()
        out = np.zeros(max(1, self.length), dtype=np.int32)
        n = lib.hnsw_mi355x_hop_counts(self._h, int(layer), out.ctypes.data_as(_I), out.size)
        if n < 0:
            raise RuntimeError(last_error())
        return out[:n].copy()

    # ---- repair of reachability ----
    def repair_reachability(self, cands: int = 8, max_rounds: int = 8) -> List[dict]:
        """Links the items that unreachable_ids() reports into the lists of their nearest reached members, on the device, layer by
        layer from the top; one dict per layer 0 .. top with the fields of hnsw_mi355x_layer_repair.  Opt-in: it edits neighbour
        lists, so the graph is no longer an outcome of the reference's Add (it stays well formed, and its snapshots load).  It
        promises reachability, not recall.  cands, max_rounds: 1 .. 64.  An empty list for an empty index."""
        if not self._initialized:
            self._initialize()
        cap = max(1, self.top_layer() + 1)   # one call: a second one would report what it found left to do, which is nothing
        out = (LayerRepair * cap)()
        n = lib.hnsw_mi355x_repair_reachability(self._h, int(cands), int(max_rounds), out, cap)
        if n < 0:
            raise RuntimeError(last_error())
        return [out[i].as_dict() for i in range(min(n, cap))]

    # ---- HNSWIndex.Serialize / Deserialize (src/HNSWIndex/HNSWIndex.cs:210-229) ----
    def serialize(self, path) -> None:
        """Write the reference's protobuf-net snapshot of this index to `path`."""
        if not self._initialized:
            self._initialize()
        self._check(lib.hnsw_mi355x_serialize(self._h, os.fsencode(path)))

    @classmethod
    def deserialize(cls, path, metric="sq_euclid") -> "Index":
        """Reconstruct an index from a snapshot written by `serialize` or by the reference."""
        h = lib.hnsw_mi355x_deserialize(metric.encode("utf-8"), os.fsencode(path))
        if not h:
            raise RuntimeError("deserialize failed: " + last_error())
        ix = cls(0, metric)
        ix._h = h
        ix._initialized = True
        ix.dim = int(lib.hnsw_mi355x_dim(h))
        return ix

    def import_graph(self, rows, levels, entry_point: int, layers):
        """Load a graph built elsewhere into this (still empty) index: rows [n, dim], levels [n], the entry point and per
        layer a (counts[n], edges[n, stride]) pair as `export_edges` returns them.  Afterwards the index answers and
        grows exactly like the one the graph came from."""
        if not self._initialized:
            self._initialize()
        a = _as_2d_f32(rows, self.dim)
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        self._check(lib.hnsw_mi355x_import_nodes(self._h, a.ctypes.data_as(_F), int(a.shape[0]), int(a.shape[1]),
                                                 lv.ctypes.data_as(_I), int(entry_point)))
        for layer, (counts, edges) in enumerate(layers):
            c = np.ascontiguousarray(counts, dtype=np.int32)
            e = np.ascontiguousarray(edges, dtype=np.int32)
            self._check(lib.hnsw_mi355x_import_edges(self._h, layer, c.ctypes.data_as(_I), e.ctypes.data_as(_I), int(e.shape[1])))

    def graph_hash(self) -> int:
        return int(lib.hnsw_mi355x_graph_hash(self._h))

    def set_profiling(self, on: bool):
        if not self._initialized:
            self._initialize()
        lib.hnsw_mi355x_set_profiling(self._h, int(on))

    def stats(self) -> dict:
        s = DeviceStats()
        if self._h:
            lib.hnsw_mi355x_get_stats(self._h, ct.byref(s))
        return s.as_dict()

    def reset_stats(self):
        if self._h:
            lib.hnsw_mi355x_reset_stats(self._h)


class DeviceBackend:
    """The inner boundary (hnswdev_*): HBM-resident row matrix + batched distance calls."""

    def __init__(self, dim: int, metric="sq_euclid", capacity=1024, device=0):
        self.dim, self.metric = dim, metric
        ctx = ct.c_void_p()
        if lib.hnswdev_create(device, dim, METRICS[metric], capacity, ct.byref(ctx)) != 0:
            raise RuntimeError("hnswdev_create failed: " + _dev_error())
        self._ctx = ctx
        self._graph_n = 0   # nodes of the committed graph (set_graph)
        self._graph_m = 0   # ... and its max_edges

    def __del__(self):
        if getattr(self, "_ctx", None):
            lib.hnswdev_destroy(self._ctx)
            self._ctx = None

    def last_error(self) -> str:
        """This context's own last error (hnswdev_ctx_last_error)."""
        buf = ct.create_string_buffer(4096)
        lib.hnswdev_ctx_last_error(self._ctx, buf, len(buf))
        return buf.value.decode("utf-8", "replace")

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.last_error())

    def reserve(self, capacity: int):
        self._check(lib.hnswdev_reserve(self._ctx, capacity))

    def upload_rows(self, first_id: int, rows):
        a = _as_2d_f32(rows, self.dim)
        self._check(lib.hnswdev_upload_rows(self._ctx, first_id, a.shape[0], a.ctypes.data_as(_F)))

    def download_rows(self, first_id: int, n: int):
        out = np.empty((n, self.dim), dtype=np.float32)
        self._check(lib.hnswdev_download_rows(self._ctx, first_id, n, out.ctypes.data_as(_F)))
        return out

    def gather_rows(self, ids):
        """hnswdev_gather_rows: float32[n, dim], the uploaded rows of `ids` in the order asked (download_rows' values); an id outside
        the uploaded rows gives zeros."""
        a = _id_list(ids)
        out = np.empty((a.size, self.dim), dtype=np.float32)
        self._check(lib.hnswdev_gather_rows(self._ctx, a.ctypes.data_as(_I), a.size, out.ctypes.data_as(_F)))
        return out

    def knn_search_by_id(self, ids, entry_point: int, k_beam: int, k_out: int, layer: int = 0):
        """hnswdev_knn_search_by_id: knn_search whose query i is the uploaded row ids[i], answered from every graph id but ids[i].
        (ids, dists, flags)."""
        a = _id_list(ids)
        out_ids = np.empty((a.size, k_out), dtype=np.int32)
        d = np.empty((a.size, k_out), dtype=np.float32)
        flags = np.empty(a.size, dtype=np.int32)
        self._check(lib.hnswdev_knn_search_by_id(self._ctx, a.ctypes.data_as(_I), a.size, int(entry_point), int(k_beam), int(k_out), int(layer),
                                                 out_ids.ctypes.data_as(_I), d.ctypes.data_as(_F), flags.ctypes.data_as(_I)))
        return out_ids, d, flags

    def exact_knn_by_id(self, ids, k: int, n_rows=None, allowed=None):
        """hnswdev_exact_knn_by_id: exact_knn whose query i is the uploaded row ids[i] and whose candidates are exact_knn's minus
        ids[i].  (ids, dists)."""
        a = _id_list(ids)
        out_ids = np.empty((a.size, k), dtype=np.int32)
        d = np.empty((a.size, k), dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_knn_by_id(self._ctx, a.ctypes.data_as(_I), a.size, (1 << 62) if n_rows is None else int(n_rows), int(k), wp, nbits,
                                                out_ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        return out_ids, d

    def exact_range_by_id(self, ids, radius: float, n_rows=None, allowed=None):
        """hnswdev_exact_range_by_id: exact_range whose query i is the uploaded row ids[i] and whose candidates are exact_range's
        minus ids[i].  (list of ids, list of dists)."""
        a = _id_list(ids)
        if a.size == 0:
            return [], []
        counts = np.zeros(a.size, dtype=np.int32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_range_by_id(self._ctx, a.ctypes.data_as(_I), a.size, (1 << 62) if n_rows is None else int(n_rows), float(radius), wp,
                                                  nbits, counts.ctypes.data_as(_I)))
        counts = counts[:a.size]
        total = int(counts.sum(dtype=np.int64))
        out_ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_exact_range_results(self._ctx, out_ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts, dtype=np.int64)[:-1]
        return np.split(out_ids[:total], cuts), np.split(d[:total], cuts)

    def exact_range_groups(self, radius: float, n_rows: int, allowed=None):
        """hnswdev_exact_range_groups: (int32[n_rows] labels, info dict) -- the single-linkage groups of the uploaded rows of
        [0, n_rows) that `allowed` allows, as Index.duplicate_groups returns them; an id that is no uploaded row is no member (-1)."""
        labels = np.full(int(n_rows), -1, dtype=np.int32)
        info = (ct.c_uint64 * 4)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_range_groups(self._ctx, int(n_rows), float(radius), wp, nbits, labels.ctypes.data_as(_I), info))
        return labels, {name: int(info[i]) for i, name in enumerate(_GROUPS_INFO)}

    def exact_range_density(self, radius: float, min_samples: int, n_rows: int, allowed=None, labels=True):
        """hnswdev_exact_range_density: (int32[n_rows] labels or None, int32[n_rows] counts, info dict) -- Index.density_clusters on the
        uploaded rows of [0, n_rows) that `allowed` allows; labels=False: the counts alone (one scan, the label slots of info 0)."""
        out_labels = np.full(int(n_rows), -1, dtype=np.int32) if labels else None
        counts = np.full(int(n_rows), -1, dtype=np.int32)
        info = (ct.c_uint64 * 8)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_range_density(self._ctx, int(n_rows), float(radius), int(min_samples), wp, nbits,
                                                    out_labels.ctypes.data_as(_I) if labels else None, counts.ctypes.data_as(_I), info))
        return out_labels, counts, {name: int(info[i]) for i, name in enumerate(_DENSITY_INFO)}

    def graph_edge_groups(self, radius: float, n_rows: int, allowed=None):
        """hnswdev_graph_edge_groups: (int32[n_rows] labels, info dict) -- Index.graph_duplicate_groups on the uploaded rows of
        [0, n_rows) that `allowed` allows and the graph set_graph committed."""
        labels = np.full(int(n_rows), -1, dtype=np.int32)
        info = (ct.c_uint64 * 5)()
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_graph_edge_groups(self._ctx, int(n_rows), float(radius), wp, nbits, labels.ctypes.data_as(_I), info))
        return labels, {name: int(info[i]) for i, name in enumerate(_EDGE_GROUPS_INFO)}

    def graph_near_edges(self, radius: float, n_rows: int, allowed=None):
        """hnswdev_graph_near_edges + _results: (src, dst, dist) as Index.near_edges returns them, on the uploaded rows of [0, n_rows)."""
        count = ct.c_longlong(0)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_graph_near_edges(self._ctx, int(n_rows), float(radius), wp, nbits, ct.byref(count)))
        n = int(count.value)
        src, dst, d = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float32)
        if n:
            self._check(lib.hnswdev_graph_near_edges_results(self._ctx, src.ctypes.data_as(_I), dst.ctypes.data_as(_I), d.ctypes.data_as(_F), n))
        return src, dst, d

    def set_queries(self, queries):
        """Uploads the query set of a batch of searches once; records name queries by row index."""
        q = _as_2d_f32(queries, self.dim)
        self._check(lib.hnswdev_set_queries(self._ctx, q.ctypes.data_as(_F), q.shape[0]))

    def dist_query_batch(self, queries, cand_offsets, cand_ids):
        """queries=None: measure against the resident set (set_queries), nothing is re-uploaded."""
        off = np.ascontiguousarray(cand_offsets, dtype=np.int32)
        ids = np.ascontiguousarray(cand_ids, dtype=np.int32)
        out = np.empty(ids.size, dtype=np.float32)
        if queries is None:
            qp, nq = None, off.size - 1
        else:
            q = _as_2d_f32(queries, self.dim)
            assert off.size == q.shape[0] + 1
            qp, nq = q.ctypes.data_as(_F), q.shape[0]
        self._check(lib.hnswdev_dist_query_batch(self._ctx, qp, nq, off.ctypes.data_as(_I), ids.ctypes.data_as(_I),
                                                 out.ctypes.data_as(_F)))
        return out

    def step_buffers(self, which: int, nslots: int, stride: int):
        """The context's pinned step-buffer set `which` (0 | 1) as numpy views: records
        [nslots, stride + 2] = (cnt, qidx, ids...) and distances [nslots, stride]."""
        rec, dist = _I(), _F()
        self._check(lib.hnswdev_step_buffers(self._ctx, which, nslots, stride, ct.byref(rec), ct.byref(dist)))
        r = np.ctypeslib.as_array(rec, shape=(nslots, stride + 2))
        d = np.ctypeslib.as_array(dist, shape=(nslots, stride))
        return r, d

    def step_submit(self, which: int, nslots_used: int):
        self._check(lib.hnswdev_step_submit(self._ctx, which, nslots_used))

    def step_wait(self, which: int):
        self._check(lib.hnswdev_step_wait(self._ctx, which))

    def dist_pair_batch(self, a_ids, b_ids):
        a = np.ascontiguousarray(a_ids, dtype=np.int32)
        b = np.ascontiguousarray(b_ids, dtype=np.int32)
        assert a.size == b.size
        out = np.empty(a.size, dtype=np.float32)
        self._check(lib.hnswdev_dist_pair_batch(self._ctx, a.ctypes.data_as(_I), b.ctypes.data_as(_I), a.size,
                                                out.ctypes.data_as(_F)))
        return out

    def set_graph(self, levels, layers, max_edges: int):
        """layers: per layer a (counts[n], edges[n, stride]) pair, EdgeList order (as Index.export_edges)."""
        lv = np.ascontiguousarray(levels, dtype=np.int32)
        self._graph_n = 0
        self._check(lib.hnswdev_graph_begin(self._ctx, lv.size, int(max_edges), lv.ctypes.data_as(_I)))
        for layer, (counts, edges) in enumerate(layers):
            c = np.ascontiguousarray(counts, dtype=np.int32)
            e = np.ascontiguousarray(edges, dtype=np.int32)
            self._check(lib.hnswdev_graph_set_layer(self._ctx, layer, c.ctypes.data_as(_I), e.ctypes.data_as(_I), e.shape[1]))
        self._check(lib.hnswdev_graph_commit(self._ctx))
        self._graph_n = int(lv.size)
        self._graph_m = int(max_edges)

    @staticmethod
    def _live_arg(live):
        """live: None (every node of the mirror) or a bool mask / id list as the allowed= arguments take it."""
        if live is None:
            return None, None, 0
        words, nbits = allow_bits(live)
        words, wp = _words_arg(words)
        return words, wp, nbits

    def graph_info(self, layer: int, live=None, with_in_edges: bool = True) -> dict:
        """hnswdev_graph_info: HNSWInfo.LayerInfo of one layer of the committed graph, as a dict of hnsw_mi355x_layer_info's fields."""
        words, wp, nbits = self._live_arg(live)
        out = LayerInfo()
        self._check(lib.hnswdev_graph_info(self._ctx, int(layer), wp, nbits, int(bool(with_in_edges)), ct.byref(out)))
        return out.as_dict()

    def graph_components(self, layer: int, live=None) -> int:
        """hnswdev_graph_components: weakly connected components among the members of one layer of the committed graph."""
        words, wp, nbits = self._live_arg(live)
        out = ct.c_int(0)
        self._check(lib.hnswdev_graph_components(self._ctx, int(layer), wp, nbits, ct.byref(out)))
        return int(out.value)

    def _reach_out(self):
        """(n, reached words, hops) for a reachability call on the committed graph."""
        n = int(self._graph_n)
        return n, np.zeros((n + 31) // 32, dtype=np.uint32), np.zeros(n, dtype=np.int32)

    @staticmethod
    def _reached_mask(words, n):
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(np.bool_)

    def graph_reach_layer(self, layer: int, seeds, live=None):
        """hnswdev_graph_reach_layer: what the members of one layer of the committed graph that are in `seeds` (a bool mask or an id
        list, as `live`) reach over out-edges.  (reached mask[n], hops[n], summary dict)."""
        _, wp, nbits = self._live_arg(live)
        swords, snbits = allow_bits(seeds)
        swords, sp = _words_arg(swords)
        n, words, hops = self._reach_out()
        summary = (ct.c_uint64 * 4)()
        self._check(lib.hnswdev_graph_reach_layer(self._ctx, int(layer), wp, nbits, sp, snbits, words.ctypes.data_as(_U32), hops.ctypes.data_as(_I), summary))
        return self._reached_mask(words, n), hops, dict(zip(_GRAPH_REACH_SUMMARY, (int(v) for v in summary)))

    def graph_reach(self, entry_point: int, live=None, min_layer: int = 0):
        """hnswdev_graph_reach: the chain from the entry point's level down to min_layer.  (per-layer dicts for min_layer .. top,
        reached mask[n] and hops[n] of min_layer)."""
        _, wp, nbits = self._live_arg(live)
        n, words, hops = self._reach_out()
        cap = 16
        while True:
            out = (LayerReach * cap)()
            got = lib.hnswdev_graph_reach(self._ctx, int(entry_point), wp, nbits, int(min_layer), out, cap, words.ctypes.data_as(_U32), hops.ctypes.data_as(_I))
            if got < 0:
                raise RuntimeError(self.last_error())
            if got <= cap:
                return [out[i].as_dict() for i in range(int(min_layer), got)], self._reached_mask(words, n), hops
            cap = got

    def graph_repair_propose(self, layer: int, seeds, live=None, cands: int = 8, max_edges: Optional[int] = None):
        """hnswdev_graph_repair_propose: steps 1 - 3 of one repair round on one layer of the committed graph (read, not changed), from
        `seeds` (a bool mask or an id list, as `live`).  (U[n_u] ascending, cands[n_u, cands], codes[n_u, cands]).  max_edges:
        MaxEdges(layer); None: 2 M on layer 0 and M above, M the max_edges given to set_graph."""
        _, wp, nbits = self._live_arg(live)
        swords, snbits = allow_bits(seeds)
        swords, sp = _words_arg(swords)
        if max_edges is None:
            max_edges = self._graph_m * (2 if int(layer) == 0 else 1)
        n, c = int(self._graph_n), int(cands)
        n_u = ct.c_int(0)
        ids = np.zeros(max(n, 1), dtype=np.int32)
        cd = np.zeros((max(n, 1), max(c, 1)), dtype=np.int32)
        code = np.zeros((max(n, 1), max(c, 1)), dtype=np.int32)
        self._check(lib.hnswdev_graph_repair_propose(self._ctx, int(layer), wp, nbits, sp, snbits, c, int(max_edges), ct.byref(n_u), ids.ctypes.data_as(_I),
                                                     cd.ctypes.data_as(_I), code.ctypes.data_as(_I), n))
        k = int(n_u.value)
        return ids[:k].copy(), cd[:k].copy(), code[:k].copy()

    def knn_search(self, queries, entry_point: int, k_beam: int, k_out: int, allowed=None, layer: int = 0):
        """allowed: as for Index.knn_query (hnswdev_knn_search_filtered); None runs hnswdev_knn_search.  layer != 0:
        hnswdev_knn_search_at_layer."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        ids = np.empty((n, k_out), dtype=np.int32)
        d = np.empty((n, k_out), dtype=np.float32)
        flags = np.empty(n, dtype=np.int32)
        if layer != 0:
            words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
            words, wp = _words_arg(words) if allowed is not None else (None, None)
            self._check(lib.hnswdev_knn_search_at_layer(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), int(k_beam), int(k_out), int(layer), wp, nbits,
                                                        ids.ctypes.data_as(_I), d.ctypes.data_as(_F), flags.ctypes.data_as(_I)))
            return ids, d, flags
        if allowed is not None:
            words, nbits = allow_bits(allowed)
            words, wp = _words_arg(words)
            self._check(lib.hnswdev_knn_search_filtered(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), int(k_beam), int(k_out), wp, nbits,
                                                        ids.ctypes.data_as(_I), d.ctypes.data_as(_F), flags.ctypes.data_as(_I)))
            return ids, d, flags
        self._check(lib.hnswdev_knn_search(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), int(k_beam), int(k_out),
                                           ids.ctypes.data_as(_I), d.ctypes.data_as(_F), flags.ctypes.data_as(_I)))
        return ids, d, flags

    def knn_search_grouped(self, queries, entry_point: int, k_beam: int, k_out: int, row_group, query_group, n_groups=None, layer: int = 0):
        """hnswdev_knn_search_grouped: knn_search with a group filter per query -- query i is answered from the graph ids j with
        row_group[j] == query_group[i].  (ids, dists, flags); n_groups None: the largest value in either array plus one."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        ids = np.empty((n, k_out), dtype=np.int32)
        d = np.empty((n, k_out), dtype=np.float32)
        flags = np.empty(n, dtype=np.int32)
        self._check(lib.hnswdev_knn_search_grouped(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), int(k_beam), int(k_out), int(layer),
                                                   rg.ctypes.data_as(_I), rg.shape[0], qg.ctypes.data_as(_I), ng, ids.ctypes.data_as(_I),
                                                   d.ctypes.data_as(_F), flags.ctypes.data_as(_I)))
        return ids, d, flags

    def knn_search_tagged(self, queries, entry_point: int, k_beam: int, k_out: int, row_tags, query_tags, match: str = "any", layer: int = 0):
        """hnswdev_knn_search_tagged: knn_search with a tag mask per query -- query i is answered from the graph ids j whose word
        row_tags[j] matches query_tags[i] (Index.knn_query_tagged's rule).  (ids, dists, flags)."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        ids = np.empty((n, k_out), dtype=np.int32)
        d = np.empty((n, k_out), dtype=np.float32)
        flags = np.empty(n, dtype=np.int32)
        self._check(lib.hnswdev_knn_search_tagged(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), int(k_beam), int(k_out), int(layer),
                                                  rt.ctypes.data_as(_U32), rt.shape[0], qt.ctypes.data_as(_U32), mode, ids.ctypes.data_as(_I),
                                                  d.ctypes.data_as(_F), flags.ctypes.data_as(_I)))
        return ids, d, flags

    def exact_knn_tagged(self, queries, k: int, row_tags, query_tags, match: str = "any", n_rows=None):
        """hnswdev_exact_knn_tagged: exact_knn with a tag mask per query -- query i is answered from the uploaded rows j of [0, n_rows)
        (None: all) whose word row_tags[j] matches query_tags[i].  queries None: the resident set (len(query_tags) of its rows)."""
        q = None if queries is None else _as_2d_f32(queries, self.dim)
        n = int(np.asarray(query_tags).size) if q is None else int(q.shape[0])
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        ids = np.empty((n, k), dtype=np.int32)
        d = np.empty((n, k), dtype=np.float32)
        self._check(lib.hnswdev_exact_knn_tagged(self._ctx, None if q is None else q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows),
                                                 int(k), rt.ctypes.data_as(_U32), rt.shape[0], qt.ctypes.data_as(_U32), mode, ids.ctypes.data_as(_I),
                                                 d.ctypes.data_as(_F)))
        return ids, d

    def tag_list_ms(self) -> float:
        """HIP-event milliseconds of the tagged calls' list-building kernels while profiling was on, since reset_stats."""
        out = ct.c_double(0.0)
        self._check(lib.hnswdev_tag_list_ms(self._ctx, ct.byref(out)))
        return float(out.value)

    def exact_knn(self, queries, k: int, n_rows=None, allowed=None):
        """hnswdev_exact_knn: (ids, dists) of shape [nq, k], per query the k uploaded rows of smallest (distance, id) among rows
        [0, n_rows) (None: every uploaded row) that `allowed` allows (as for Index.knn_query; None: all).  A flat scan: no graph."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        ids = np.empty((n, k), dtype=np.int32)
        d = np.empty((n, k), dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_knn(self._ctx, q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows), int(k), wp, nbits,
                                          ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        return ids, d

    def exact_knn_grouped(self, queries, k: int, row_group, query_group, n_groups=None, n_rows=None):
        """hnswdev_exact_knn_grouped: exact_knn with a candidate group per query -- query i is answered from the uploaded rows j of
        [0, n_rows) (None: all) with row_group[j] == query_group[i].  queries None: the resident set (len(query_group) of its rows).
        n_groups None: the largest value in either array plus one."""
        q = None if queries is None else _as_2d_f32(queries, self.dim)
        n = int(np.asarray(query_group).size) if q is None else int(q.shape[0])
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        ids = np.empty((n, k), dtype=np.int32)
        d = np.empty((n, k), dtype=np.float32)
        self._check(lib.hnswdev_exact_knn_grouped(self._ctx, None if q is None else q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows),
                                                  int(k), rg.ctypes.data_as(_I), rg.shape[0], qg.ctypes.data_as(_I), ng, ids.ctypes.data_as(_I),
                                                  d.ctypes.data_as(_F)))
        return ids, d

    def exact_knn_collapsed(self, queries, k: int, row_group, per_group: int = 1, n_rows=None, allowed=None):
        """hnswdev_exact_knn_collapsed: exact_knn with at most per_group results per label row_group[id]; row_group needs an entry
        for every uploaded row below n_rows (the context checks that: a RuntimeError with both numbers)."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        rg = _collapse_args(row_group, k, per_group, 0)   # (the rows uploaded are the context's to know: it checks the length)
        ids = np.empty((n, k), dtype=np.int32)
        d = np.empty((n, k), dtype=np.float32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_knn_collapsed(self._ctx, q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows), int(k),
                                                    rg.ctypes.data_as(_I), rg.shape[0], int(per_group), wp, nbits, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        return ids, d

    def exact_grouped_list_ms(self) -> float:
        """HIP-event milliseconds of exact_knn_grouped's list-building kernels while profiling was on, since reset_stats."""
        out = ct.c_double(0.0)
        self._check(lib.hnswdev_exact_grouped_list_ms(self._ctx, ct.byref(out)))
        return float(out.value)

    def exact_range(self, queries, radius: float, n_rows=None, allowed=None):
        """hnswdev_exact_range: (list of ids, list of dists), per query every uploaded row of [0, n_rows) (None: all) that `allowed`
        allows with distance <= radius, ascending by (distance, id).  A flat scan: no graph."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        counts = np.zeros(n, dtype=np.int32)
        words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
        words, wp = _words_arg(words) if allowed is not None else (None, None)
        self._check(lib.hnswdev_exact_range(self._ctx, q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows), float(radius), wp, nbits,
                                            counts.ctypes.data_as(_I)))
        total = int(counts.sum(dtype=np.int64))
        ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_exact_range_results(self._ctx, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts, dtype=np.int64)[:-1]
        return np.split(ids[:total], cuts), np.split(d[:total], cuts)

    def exact_range_grouped(self, queries, radius: float, row_group, query_group, n_groups=None, n_rows=None):
        """hnswdev_exact_range_grouped: exact_range with a candidate group per query -- (list of ids, list of dists) in the caller's
        query order, query i answered from the uploaded rows j of [0, n_rows) (None: all) with row_group[j] == query_group[i].
        queries None: the resident set (len(query_group) of its rows).  n_groups None: the largest value in either array plus one."""
        q = None if queries is None else _as_2d_f32(queries, self.dim)
        n = int(np.asarray(query_group).size) if q is None else int(q.shape[0])
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        counts = np.zeros(n, dtype=np.int32)
        self._check(lib.hnswdev_exact_range_grouped(self._ctx, None if q is None else q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows),
                                                    float(radius), rg.ctypes.data_as(_I), rg.shape[0], qg.ctypes.data_as(_I), ng,
                                                    counts.ctypes.data_as(_I)))
        total = int(counts.sum(dtype=np.int64))
        ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_exact_range_results(self._ctx, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts, dtype=np.int64)[:-1]
        return np.split(ids[:total], cuts), np.split(d[:total], cuts)

    def multilayer_search(self, queries, entry_point: int, k: int, max_layer=None, min_layer: int = 0, layers_cap=None):
        """hnswdev_multilayer_search: (ids, dists, flags), ids / dists of shape [nq, nlayers, k - 1] as Index.multilayer_knn_query;
        flags[i] = 1: query i was handed back."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        cap = 64 if layers_cap is None else int(layers_cap)
        per = max(int(k) - 1, 0)
        ids = np.full((n, cap, per), -1, dtype=np.int32)
        d = np.full((n, cap, per), np.nan, dtype=np.float32)
        flags = np.zeros(n, dtype=np.int32)
        nl = lib.hnswdev_multilayer_search(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), int(k), 2 ** 31 - 1 if max_layer is None else int(max_layer),
                                           int(min_layer), cap, ids.ctypes.data_as(_I), d.ctypes.data_as(_F), flags.ctypes.data_as(_I))
        self._check(min(nl, 0))
        return np.ascontiguousarray(ids[:, :nl]), np.ascontiguousarray(d[:, :nl]), flags

    def range_search(self, queries, entry_point: int, radius: float, allowed=None, layer: int = 0):
        """Per query the ids / distances within `radius`, ascending by distance; flags[i] = 1: handed back (empty).
        allowed: as for Index.knn_query (hnswdev_range_search_filtered); None runs hnswdev_range_search.  layer != 0:
        hnswdev_range_search_at_layer."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        counts = np.zeros(n, dtype=np.int32)
        flags = np.zeros(n, dtype=np.int32)
        if layer != 0:
            words, nbits = allow_bits(allowed) if allowed is not None else (None, 0)
            words, wp = _words_arg(words) if allowed is not None else (None, None)
            self._check(lib.hnswdev_range_search_at_layer(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), float(radius), int(layer), wp, nbits,
                                                          counts.ctypes.data_as(_I), flags.ctypes.data_as(_I)))
        elif allowed is not None:
            words, nbits = allow_bits(allowed)
            words, wp = _words_arg(words)
            self._check(lib.hnswdev_range_search_filtered(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), float(radius), wp, nbits,
                                                          counts.ctypes.data_as(_I), flags.ctypes.data_as(_I)))
        else:
            self._check(lib.hnswdev_range_search(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), float(radius),
                                                 counts.ctypes.data_as(_I), flags.ctypes.data_as(_I)))
        total = int(counts.sum())
        ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_range_results(self._ctx, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts)[:-1]
        return np.split(ids[:total], cuts), np.split(d[:total], cuts), flags

    def range_search_grouped(self, queries, entry_point: int, radius: float, row_group, query_group, n_groups=None, layer: int = 0):
        """hnswdev_range_search_grouped: range_search with a group filter per query -- (ids, dists, flags) as range_search returns
        them, query i filtered by row_group == query_group[i]."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        rg, qg, ng = _group_args(row_group, query_group, n_groups, n)
        counts = np.zeros(n, dtype=np.int32)
        flags = np.zeros(n, dtype=np.int32)
        self._check(lib.hnswdev_range_search_grouped(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), float(radius), int(layer), rg.ctypes.data_as(_I),
                                                     rg.shape[0], qg.ctypes.data_as(_I), ng, counts.ctypes.data_as(_I), flags.ctypes.data_as(_I)))
        total = int(counts.sum())
        ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_range_results(self._ctx, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts)[:-1]
        return np.split(ids[:total], cuts), np.split(d[:total], cuts), flags

    def range_search_tagged(self, queries, entry_point: int, radius: float, row_tags, query_tags, match: str = "any", layer: int = 0):
        """hnswdev_range_search_tagged: range_search with a tag mask per query -- (ids, dists, flags) as range_search returns them,
        query i filtered by the ids whose word row_tags[id] matches query_tags[i]."""
        q = _as_2d_f32(queries, self.dim)
        n = q.shape[0]
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        counts = np.zeros(n, dtype=np.int32)
        flags = np.zeros(n, dtype=np.int32)
        self._check(lib.hnswdev_range_search_tagged(self._ctx, q.ctypes.data_as(_F), n, int(entry_point), float(radius), int(layer), rt.ctypes.data_as(_U32),
                                                    rt.shape[0], qt.ctypes.data_as(_U32), mode, counts.ctypes.data_as(_I), flags.ctypes.data_as(_I)))
        total = int(counts.sum())
        ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_range_results(self._ctx, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts)[:-1]
        return np.split(ids[:total], cuts), np.split(d[:total], cuts), flags

    def exact_range_tagged(self, queries, radius: float, row_tags, query_tags, match: str = "any", n_rows=None):
        """hnswdev_exact_range_tagged: exact_range with a tag mask per query -- (list of ids, list of dists) in the caller's query
        order, query i answered from the uploaded rows j of [0, n_rows) (None: all) whose word row_tags[j] matches query_tags[i].
        queries None: the resident set (len(query_tags) of its rows)."""
        q = None if queries is None else _as_2d_f32(queries, self.dim)
        n = int(np.asarray(query_tags).size) if q is None else int(q.shape[0])
        rt, qt, mode = _tag_args(row_tags, query_tags, match, n)
        counts = np.zeros(n, dtype=np.int32)
        self._check(lib.hnswdev_exact_range_tagged(self._ctx, None if q is None else q.ctypes.data_as(_F), n, (1 << 62) if n_rows is None else int(n_rows),
                                                   float(radius), rt.ctypes.data_as(_U32), rt.shape[0], qt.ctypes.data_as(_U32), mode,
                                                   counts.ctypes.data_as(_I)))
        total = int(counts.sum(dtype=np.int64))
        ids = np.empty(max(total, 1), dtype=np.int32)
        d = np.empty(max(total, 1), dtype=np.float32)
        self._check(lib.hnswdev_exact_range_results(self._ctx, ids.ctypes.data_as(_I), d.ctypes.data_as(_F)))
        cuts = np.cumsum(counts, dtype=np.int64)[:-1]
        return np.split(ids[:total], cuts), np.split(d[:total], cuts)

    def set_profiling(self, on: bool):
        self._check(lib.hnswdev_set_profiling(self._ctx, int(on)))

    def stats(self) -> dict:
        s = DeviceStats()
        self._check(lib.hnswdev_get_stats(self._ctx, ct.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._check(lib.hnswdev_reset_stats(self._ctx))


def _install_counter_methods(name, slots, doc):
    """Index.<name>() and DeviceBackend.<name>() of one row of COUNTER_BLOCKS: the block as a dict keyed by its slot names.
    Index: all zero while there is no native handle, and it never raises.  DeviceBackend: a failure raises, as every call of it."""
    def index_block(self) -> dict:
        out = (ct.c_uint64 * len(slots))()
        if self._h:
            getattr(lib, "hnsw_mi355x_" + name)(self._h, out)
        return dict(zip(slots, (int(v) for v in out)))

    def backend_block(self) -> dict:
        out = (ct.c_uint64 * len(slots))()
        self._check(getattr(lib, "hnswdev_" + name)(self._ctx, out))
        return dict(zip(slots, (int(v) for v in out)))

    index_block.__doc__ = doc
    backend_block.__doc__ = f"This context's counters of that block since reset_stats (hnswdev_{name}): the slots of Index.{name}."
    for cls, fn in ((Index, index_block), (DeviceBackend, backend_block)):
        fn.__name__, fn.__qualname__ = name, f"{cls.__name__}.{name}"
        setattr(cls, name, fn)


for _name, (_slots, _doc) in COUNTER_BLOCKS.items():
    _install_counter_methods(_name, _slots, _doc)


def device_sqrt_rn(x, device=0):
    """Test hook: the device's correctly rounded double sqrt (cosine epilogue)."""
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(a)
    rc = lib.hnswdev_test_sqrt_rn(device, a.ctypes.data_as(ct.POINTER(ct.c_double)),
                                  out.ctypes.data_as(ct.POINTER(ct.c_double)), a.size)
    if rc != 0:
        raise RuntimeError(_dev_error())
    return out
