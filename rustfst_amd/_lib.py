"""ctypes binding of libwfst_amd.so (include/wfst.h).  Fails loudly when the library is missing:
there is no CPU fallback anywhere in this package."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libwfst_amd.so")

TR_DTYPE = np.dtype([("ilabel", "<u4"), ("olabel", "<u4"), ("weight", "<f4"), ("nextstate", "<u4")])


class WfstError(RuntimeError):
    """KO status from the C-ABI; carries the thread-local error text (rustfst-ffi/src/lib.rs:58-76)."""


class ComposeConfig(C.Structure):
    _fields_ = [("compose_filter", C.c_uint32), ("connect", C.c_uint32)]


class MatcherConfig(C.Structure):  # wfst_matcher_config
    _fields_ = [("sigma_label", C.c_uint32), ("rewrite_mode", C.c_uint32), ("sigma_allowed_matches", C.POINTER(C.c_uint32)),
                ("n_allowed", C.c_size_t)]


class ShortestPathConfig(C.Structure):
    _fields_ = [("delta", C.c_float), ("nshortest", C.c_uint64), ("unique", C.c_uint32)]


class ShortestDistanceConfig(C.Structure):
    _fields_ = [("reverse", C.c_uint32), ("delta", C.c_float)]


class PushWeightsConfig(C.Structure):
    _fields_ = [("delta", C.c_float), ("remove_total_weight", C.c_uint32)]


class DeterminizeConfig(C.Structure):
    _fields_ = [("delta", C.c_float), ("det_type", C.c_uint32)]


class MinimizeConfig(C.Structure):
    _fields_ = [("delta", C.c_float), ("allow_nondet", C.c_uint32)]


class IsomorphicConfig(C.Structure):  # wfst_isomorphic_config
    _fields_ = [("delta", C.c_float)]


TIES_UNKNOWN = (1 << 64) - 1  # WFST_TIES_UNKNOWN


class LabelFstPair(C.Structure):
    _fields_ = [("label", C.c_uint32), ("fst", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("relax_launches", C.c_uint64), ("relax_ms", C.c_double), ("relax_arcs", C.c_uint64),
                ("relax_states", C.c_uint64), ("sweeps", C.c_uint64), ("compose_states", C.c_uint64),
                ("compose_arcs", C.c_uint64), ("compose_retries", C.c_uint64), ("compose_ms", C.c_double),
                ("string_problems", C.c_uint64), ("relax_kernel", C.c_uint64), ("nbest_device_problems", C.c_uint64),
                ("resident_aborts", C.c_uint64), ("tied_choices", C.c_uint64)]


# The route counters: family -> (getter, the names of its uint64_t* parameters behind ctx, in order).  The one statement of
# the names on this side; include/wfst.h and the family's struct in csrc/common.h say the same (tests/test_host.py).
_BATCH = ("launches", "items_in_kernel", "items_single")
COUNTERS = {
    "rm_epsilon": ("wfst_ctx_get_rm_epsilon_stats",
                   ("batches", "thread_launches", "wave_launches", "states_thread", "states_wave", "max_closure_cap")),
    "rm_epsilon_batch": ("wfst_ctx_get_rm_epsilon_batch_stats", _BATCH),
    "rearm": ("wfst_ctx_get_rearm_stats", ("armed", "adopted", "dropped")),
    "small_path": ("wfst_ctx_get_small_path_stats",
                   ("n1_in_kernel", "n1_staged", "n1_handed_back", "nbest_in_kernel", "nbest_tree_full", "nbest_out_full",
                    "nbest_tree_capacity")),
    "compose_path": ("wfst_ctx_get_compose_path_stats",
                     ("string_answered", "string_handed_back", "wave_first", "relaunch_states", "relaunch_arcs",
                      "relaunch_hash", "relaunch_path", "switched_wide", "two_step", "caps_states", "caps_arcs", "caps_hash")),
    "string_run": ("wfst_ctx_get_string_run_stats", ("run_levels", "runs")),
    "determinize": ("wfst_ctx_get_determinize_stats",
                    ("levels", "wide_levels", "narrow_launches", "exit_wide_states", "exit_wide_cands", "exit_budget",
                     "exit_need", "exit_done", "wide_need", "grow_states", "grow_elts", "grow_arcs", "grow_cands", "rehashes",
                     "cap_states", "cap_elts", "cap_arcs", "cap_cands", "rounds_max")),
    "determinize_batch": ("wfst_ctx_get_determinize_batch_stats", _BATCH),
    "minimize": ("wfst_ctx_get_minimize_stats",
                 ("check_levels", "check_wide_levels", "check_narrow_launches", "check_exit_wide", "check_exit_done", "levels",
                  "wide_levels", "narrow_launches", "exit_wide", "exit_done", "branch", "wave_states", "unequal_compares")),
    "minimize_batch": ("wfst_ctx_get_minimize_batch_stats", _BATCH),
    "push": ("wfst_ctx_get_push_stats",
             ("searches", "rounds", "reads", "rounds_max", "bfs_blocks", "arcs_blocks", "total_blocks", "structural",
              "start_branch", "removed")),
    "tr_sum_batch": ("wfst_ctx_get_tr_sum_batch_stats", _BATCH),
    "replace": ("wfst_ctx_get_replace_stats",
                ("levels", "states", "arcs", "prefixes", "max_depth", "call_arcs", "dropped_calls", "return_arcs", "arena_grows",
                 "prefix_reruns", "level_launches")),
    "top_sort": ("wfst_ctx_get_top_sort_stats",
                 ("levels", "narrow_launches", "wide_launches", "narrow_levels", "max_level_width", "max_tree_depth", "lift_rows",
                  "states_compared", "wave_states", "cyclic")),
    "lookahead": ("wfst_ctx_get_lookahead_stats",
                  ("items", "items_no_start", "wave_answered", "handed_over_states", "handed_over_width", "overflow_arcs",
                   "overflow_states", "wide_items", "wave_regrows", "wide_grows", "wide_hinted", "hint_fallbacks", "one_limits")),
}

# wfst_ctx_get_top_sort_batch_counters: the uint64_t* parameters behind ctx, in order: a one-workgroup-per-item batch family
# like the *_batch entries above, its getter outside the table of the *_stats families
TOP_SORT_BATCH_COUNTERS = _BATCH

# wfst_ctx_get_compose_batch_counters: the same driver's three counts, then what the list form of compose adds to them
COMPOSE_BATCH_COUNTERS = _BATCH + ("items_no_start", "regrown_states", "regrown_arcs", "regrown_hash")

# wfst_ctx_get_compose_sigma_counters: the uint64_t* parameters behind ctx, in order (outside the table of the *_stats families)
COMPOSE_SIGMA_COUNTERS = ("levels", "states", "arcs", "require1_states", "require2_states", "exact_items", "sigma_items",
                          "sigma_arcs", "refused_items", "arena_grows", "level_launches")

# wfst_ctx_get_sigma_batch_counters: the same, for the fused batch with matcher configs
SIGMA_BATCH_COUNTERS = ("launches", "items_in_kernel", "items_handed_back", "items_loop", "exact_items", "sigma_items", "sigma_arcs",
                        "refused_items", "max_level_width")

# wfst_ctx_get_isomorphic_counters: the same, for the level search of isomorphic
ISOMORPHIC_COUNTERS = ("levels", "narrow_launches", "wide_launches", "narrow_levels", "max_level_width", "pairs", "events",
                       "wave_pairs", "big_states_sorted", "nondet_marks")

# wfst_ctx_get_paths_counters: the same, for the last count_paths / paths / paths_batch call
PATHS_COUNTERS = ("launches", "items_in_kernel", "items_single", "levels", "paths", "max_path_arcs", "saturated")

# wfst_ctx_get_string_pair_counts: the same, for the pair levels of the string kernel
STRING_PAIR_COUNTS = ("pair_levels", "pair_splits")

# wfst_ctx_get_string_placement: the same, for where the waves of the last string launch sat
STRING_PLACEMENT = ("waves_per_workgroup", "slice_states", "workgroups", "packed_for_resident", "forced")

# wfst_ctx_get_solo_query: the same, for the one-launch route of a repeated bounded shortest-path query
SOLO_QUERY = ("attempts", "answered", "aborted", "last_abort", "cleaned")
SOLO_ABORTS = ("", "BAND", "GREW", "LOG", "OTHER")  # last_abort, by value

# every symbol include/wfst.h declares: (name, restype, argtypes)
_vp, _u32, _u64, _i64, _f32, _sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64, C.c_float, C.c_size_t
_P = C.POINTER
SYMBOLS = [(symbol, C.c_int, [_vp] + [_P(_u64)] * len(names)) for symbol, names in COUNTERS.values()] + [
    ("wfst_ctx_get_compose_sigma_counters", C.c_int, [_vp] + [_P(_u64)] * len(COMPOSE_SIGMA_COUNTERS)),
    ("wfst_ctx_get_sigma_batch_counters", C.c_int, [_vp] + [_P(_u64)] * len(SIGMA_BATCH_COUNTERS)),
    ("wfst_ctx_get_top_sort_batch_counters", C.c_int, [_vp] + [_P(_u64)] * len(TOP_SORT_BATCH_COUNTERS)),
    ("wfst_ctx_get_compose_batch_counters", C.c_int, [_vp] + [_P(_u64)] * len(COMPOSE_BATCH_COUNTERS)),
    ("wfst_ctx_get_isomorphic_counters", C.c_int, [_vp] + [_P(_u64)] * len(ISOMORPHIC_COUNTERS)),
    ("wfst_ctx_get_paths_counters", C.c_int, [_vp] + [_P(_u64)] * len(PATHS_COUNTERS)),
    ("wfst_ctx_get_string_pair_counts", C.c_int, [_vp] + [_P(_u64)] * len(STRING_PAIR_COUNTS)),
    ("wfst_ctx_get_string_placement", C.c_int, [_vp] + [_P(_u64)] * len(STRING_PLACEMENT)),
    ("wfst_ctx_get_solo_query", C.c_int, [_vp] + [_P(_u64)] * len(SOLO_QUERY)),
    ("wfst_ctx_parked_key_check", C.c_int, [_vp, _P(_u64)]),
    ("wfst_last_error", C.c_int, [_P(C.c_char_p)]),
    ("wfst_string_destroy", C.c_int, [C.c_char_p]),
    ("wfst_abi_version", _u32, []),
    ("wfst_ctx_create", C.c_int, [C.c_int, _P(_vp)]),
    ("wfst_ctx_create_on_stream", C.c_int, [C.c_int, _vp, _P(_vp)]),
    ("wfst_ctx_create_with_cu_mask", C.c_int, [C.c_int, _vp, _u32, _P(_vp)]),
    ("wfst_ctx_destroy", C.c_int, [_vp]),
    ("wfst_ctx_synchronize", C.c_int, [_vp]),
    ("wfst_ctx_stream", C.c_int, [_vp, _P(_vp)]),
    ("wfst_fst_upload", C.c_int, [_vp, _u32, _i64, _vp, _vp, _vp, _u64, _P(_vp)]),
    ("wfst_fst_upload_device", C.c_int, [_vp, _u32, _i64, _vp, _vp, _vp, _u64, _P(_vp)]),
    ("wfst_fst_upload_many", C.c_int, [_vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _P(_vp)]),
    ("wfst_fst_from_openfst_bytes", C.c_int, [_vp, C.c_char_p, _sz, _P(_vp)]),
    ("wfst_fst_to_openfst_bytes", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("wfst_fst_to_openfst_const_bytes", C.c_int, [_vp, _P(_vp), _P(_sz)]),
    ("wfst_bytes_destroy", C.c_int, [_vp]),
    ("wfst_fst_info", C.c_int, [_vp, _P(_u32), _P(_u64), _P(_i64), _P(_u64)]),
    ("wfst_fst_download", C.c_int, [_vp, _vp, _vp, _vp]),
    ("wfst_fst_destroy", C.c_int, [_vp]),
    ("wfst_fst_destroy_many", C.c_int, [_P(_vp), _sz]),
    ("wfst_compose", C.c_int, [_vp, _vp, _vp, _P(ComposeConfig), _P(_vp)]),
    ("wfst_compose_batch", C.c_int, [_vp, _P(_vp), _sz, _P(_vp), _sz, _P(ComposeConfig), _P(_vp), _vp]),
    ("wfst_compose_with_matchers", C.c_int, [_vp, _vp, _vp, _P(ComposeConfig), _P(MatcherConfig), _P(MatcherConfig), _P(_vp)]),
    ("wfst_shortest_path", C.c_int, [_vp, _vp, _P(ShortestPathConfig), _P(_vp)]),
    ("wfst_connect", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_rm_epsilon", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_rm_epsilon_batch", C.c_int, [_vp, _P(_vp), _sz, _P(_vp), _vp]),
    ("wfst_ctx_get_bounded_stats", C.c_int, [_vp, _P(_u64), _P(_u64), _P(C.c_char_p)]),
    ("wfst_ctx_trim_pool", C.c_int, [_vp]),
    ("wfst_fst_project", C.c_int, [_vp, _vp, C.c_int]),
    ("wfst_fst_invert", C.c_int, [_vp, _vp]),
    ("wfst_isomorphic", C.c_int, [_vp, _vp, _vp, _P(IsomorphicConfig), _P(C.c_int)]),
    ("wfst_fst_count_paths", C.c_int, [_vp, _vp, _P(_u64)]),
    ("wfst_fst_paths", C.c_int, [_vp, _vp, _u64, _P(_vp)]),
    ("wfst_fst_paths_batch", C.c_int, [_vp, _P(_vp), _sz, _u64, _P(_vp), _vp]),
    ("wfst_paths_info", C.c_int, [_vp, _P(_u64), _P(_u64), _P(_u64), _P(_u64)]),
    ("wfst_paths_download", C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("wfst_paths_destroy", C.c_int, [_vp]),
    ("wfst_lookahead_create", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_lookahead_relabel", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_lookahead_fst1", C.c_int, [_vp, _P(_vp)]),
    ("wfst_compose_lookahead", C.c_int, [_vp, _vp, _vp, _P(_vp)]),
    ("wfst_compose_lookahead_batch", C.c_int, [_vp, _vp, _P(_vp), _sz, _P(_vp)]),
    ("wfst_lookahead_destroy", C.c_int, [_vp]),
    ("wfst_lookahead_info", C.c_int, [_vp, _P(_u32), _P(_u64), _P(_u32), _P(_u32)]),
    ("wfst_lookahead_download", C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    ("wfst_label_reachable_compute", C.c_int, [_u32, _vp, _vp, _vp, C.c_int, _P(_vp)]),
    ("wfst_ctx_set_tie_order", C.c_int, [_vp, C.c_int]),
    ("wfst_ctx_set_resident_share", C.c_int, [_vp, _u32]),
    ("wfst_shortest_path_batch", C.c_int, [_vp, _P(_vp), _sz, _P(ShortestPathConfig), _P(_vp)]),
    ("wfst_shortest_path_begin", C.c_int, [_vp, _vp, _P(ShortestPathConfig), _P(_vp)]),
    ("wfst_shortest_path_end", C.c_int, [_vp, _P(_vp)]),
    ("wfst_shortest_distance", C.c_int, [_vp, _vp, _vp, _vp]),
    ("wfst_shortest_distance_with_config", C.c_int, [_vp, _vp, _P(ShortestDistanceConfig), _vp, _P(_u32)]),
    ("wfst_push_weights", C.c_int, [_vp, _vp, _u32, _P(PushWeightsConfig), _P(_vp)]),
    ("wfst_reweight", C.c_int, [_vp, _vp, _vp, _u64, _u32, _P(_vp)]),
    ("wfst_determinize", C.c_int, [_vp, _vp, _P(DeterminizeConfig), _P(_vp)]),
    ("wfst_determinize_batch", C.c_int, [_vp, _P(_vp), _sz, _P(DeterminizeConfig), _P(_vp), _vp]),
    ("wfst_determinize_with_distance", C.c_int, [_vp, _vp, _vp, _u64, _f32, _P(_vp), _P(_vp), _P(_u64)]),
    ("wfst_determinize_with_distance_batch", C.c_int,
     [_vp, _P(_vp), _sz, _P(_vp), _P(_u64), _f32, _P(_vp), _P(_vp), _P(_u64), _vp]),
    ("wfst_minimize", C.c_int, [_vp, _vp, _P(MinimizeConfig), _P(_vp)]),
    ("wfst_minimize_batch", C.c_int, [_vp, _P(_vp), _sz, _P(MinimizeConfig), _P(_vp), _vp]),
    ("wfst_tr_sum", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_tr_unique", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_optimize", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_tr_sum_batch", C.c_int, [_vp, _P(_vp), _sz, _P(_vp), _vp]),
    ("wfst_tr_unique_batch", C.c_int, [_vp, _P(_vp), _sz, _P(_vp), _vp]),
    ("wfst_optimize_batch", C.c_int, [_vp, _P(_vp), _sz, _P(_vp), _vp]),
    ("wfst_ctx_get_optimize_batch_stats", C.c_int, [_vp, _P(_u64), _P(_u64), _P(_u64), _P(_u64)]),
    ("wfst_union", C.c_int, [_vp, _vp, _vp, _P(_vp)]),
    ("wfst_concat", C.c_int, [_vp, _vp, _vp, _P(_vp)]),
    ("wfst_closure", C.c_int, [_vp, _vp, _u32, _P(_vp)]),
    ("wfst_union_list", C.c_int, [_vp, _P(_vp), _sz, _P(_vp)]),
    ("wfst_concat_list", C.c_int, [_vp, _P(_vp), _sz, _P(_vp)]),
    ("wfst_replace", C.c_int, [_vp, _u32, _P(LabelFstPair), _sz, _u32, _P(_vp)]),
    ("wfst_rational_check_sizes", C.c_int, [_u32, _vp, _vp, _sz]),
    ("wfst_state_sort", C.c_int, [_vp, _vp, _vp, _sz, _P(_vp)]),
    ("wfst_top_sort", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_top_sort_batch", C.c_int, [_vp, _P(_vp), _sz, _P(_vp), _vp]),
    ("wfst_compose_shortest_path_batch", C.c_int,
     [_vp, _P(_vp), _sz, _vp, _P(ComposeConfig), _P(ShortestPathConfig), _P(_vp), _P(_u64)]),
    ("wfst_compose_shortest_path_batch_with_matchers", C.c_int,
     [_vp, _P(_vp), _sz, _vp, _P(ComposeConfig), _P(MatcherConfig), _P(MatcherConfig), _P(ShortestPathConfig), _P(_vp), _P(_u64)]),
    ("wfst_compose_shortest_path_batch_begin", C.c_int,
     [_vp, _P(_vp), _sz, _vp, _P(ComposeConfig), _P(ShortestPathConfig), _P(_vp)]),
    ("wfst_compose_shortest_path_batch_end", C.c_int, [_vp, _P(_vp), _P(_u64)]),
    ("wfst_fst_pack_paths", C.c_int, [_P(_vp), _sz, _u32, _vp]),
    ("wfst_compose_shortest_path_batch_packed", C.c_int,
     [_vp, _P(_vp), _sz, _vp, _P(ComposeConfig), _P(ShortestPathConfig), _u32, _vp, _P(_u64)]),
    ("wfst_comm_unique_id", C.c_int, [_vp]),
    ("wfst_comm_create", C.c_int, [_vp, _vp, _u32, _u32, _P(_vp)]),
    ("wfst_comm_create_host", C.c_int, [_u32, _u32, _vp, _vp, _P(_vp)]),
    ("wfst_gather_records_begin", C.c_int, [_vp, _vp, _sz, _u32]),
    ("wfst_comm_info", C.c_int, [_vp, _P(_u32), _P(_u32)]),
    ("wfst_comm_destroy", C.c_int, [_vp]),
    ("wfst_comm_order_after", C.c_int, [_vp, _vp]),
    ("wfst_gather_paths_begin", C.c_int, [_vp, _P(_vp), _sz, _u32]),
    ("wfst_gather_paths_end", C.c_int, [_vp, _vp]),
    ("wfst_comm_allgather_begin", C.c_int, [_vp, _vp, _sz]),
    ("wfst_comm_allgather_end", C.c_int, [_vp, _vp]),
    ("wfst_comm_allgatherv", C.c_int, [_vp, _vp, _sz, _vp, _P(_vp), _P(_sz)]),
    ("wfst_fst_tr_sort", C.c_int, [_vp, _vp, C.c_int]),
    ("wfst_fst_set_start", C.c_int, [_vp, _vp, C.c_uint32]),
    ("wfst_reverse", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_vec_fst_new", C.c_int, [_P(_vp)]),
    ("wfst_vec_fst_destroy", C.c_int, [_vp]),
    ("wfst_vec_fst_copy", C.c_int, [_vp, _P(_vp)]),
    ("wfst_vec_fst_add_state", C.c_int, [_vp, _P(_u32)]),
    ("wfst_vec_fst_add_tr", C.c_int, [_vp, _u32, _vp]),
    ("wfst_vec_fst_set_start", C.c_int, [_vp, _u32]),
    ("wfst_vec_fst_set_final", C.c_int, [_vp, _u32, _f32]),
    ("wfst_vec_fst_del_final_weight", C.c_int, [_vp, _u32]),
    ("wfst_vec_fst_num_states", C.c_int, [_vp, _P(_u32)]),
    ("wfst_vec_fst_start", C.c_int, [_vp, _P(_i64)]),
    ("wfst_vec_fst_final_weight", C.c_int, [_vp, _u32, _P(_f32), _P(C.c_int)]),
    ("wfst_vec_fst_num_trs", C.c_int, [_vp, _u32, _P(_u64)]),
    ("wfst_vec_fst_get_trs", C.c_int, [_vp, _u32, _vp, _u64, _P(_u64)]),
    ("wfst_vec_fst_properties", C.c_int, [_vp, _P(_u64)]),
    ("wfst_vec_fst_tr_sort", C.c_int, [_vp, C.c_int]),
    ("wfst_vec_fst_equals", C.c_int, [_vp, _vp, _P(C.c_int)]),
    ("wfst_vec_fst_to_device", C.c_int, [_vp, _vp, _P(_vp)]),
    ("wfst_vec_fst_from_device", C.c_int, [_vp, _P(_vp)]),
    ("wfst_ctx_set_profiling", C.c_int, [_vp, C.c_int]),
    ("wfst_ctx_get_stats", C.c_int, [_vp, _P(Stats)]),
    ("wfst_ctx_reset_stats", C.c_int, [_vp]),
    ("wfst_ctx_get_sweep_trace", C.c_int, [_vp, _vp, _vp, _vp, _sz, _P(_sz)]),
    ("wfst_ctx_get_sweep_modes", C.c_int, [_vp, _vp, _sz, _P(_sz)]),
]

_lib = None


def lib():
    """Loads libwfst_amd.so. Raises if it has not been built (python -m rustfst_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m rustfst_amd.build` "
                "(hipcc --offload-arch=gfx950). rustfst_amd has no CPU fallback.")
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64 (same SONAME
        # libamdhip64.so.7, requested by file name).  If the system copy were loaded first, torch would load
        # a second runtime and then see no GPU; loaded in this order the dynamic linker resolves our
        # NEEDED libamdhip64.so.7 to the copy torch already mapped.
        if os.environ.get("WFST_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        # (experiments only: WFST_LIB_PATH points tools/ A/B scripts at another build of the same ABI)
        L = C.CDLL(os.environ.get("WFST_LIB_PATH") or LIB_PATH)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name, None)
            if fn is None and os.environ.get("WFST_LIB_PATH"):
                continue  # (an older build of the same ABI version: what it lacks cannot be called)
            if fn is None:
                raise AttributeError(f"{LIB_PATH} does not export {name}: rebuild it (python -m rustfst_amd.build)")
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, what=""):
    """check_ffi_error (rustfst-python/rustfst/ffi_utils.py): raise with the library's message."""
    if status != 0:
        msg = C.c_char_p()
        L = lib()
        text = "unknown error"
        if L.wfst_last_error(C.byref(msg)) == 0 and msg.value is not None:
            text = msg.value.decode(errors="replace")
            L.wfst_string_destroy(msg)
        raise WfstError(f"{what}: {text}" if what else text)
