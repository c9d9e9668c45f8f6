"""ctypes binding of libeirgrid_hip.so (the C ABI declared in include/eirgrid_hip.h).

The library is built in-tree (eirgrid_amd/libeirgrid_hip.so) by `eirgrid_amd.build.build()`; importing this module
fails loudly if it is missing — there is no Python or CPU implementation to fall back to.
"""
from __future__ import annotations

import ctypes as C
import os

YEARS, N_ACTIONS, N_DEFICIT, N_COUNTS, N_TYPES = 26, 61, 15, 21, 15
GRID, CELLS, YEARLY_FIELDS = 51, 2601, 21
MAX_GENS, MAX_OFFSETS, RUN_CAP, DEF_CAP, ACT_CAP, ONCHIP_GENS = 4096, 4096, 4096, 4096, 4096, 512
TOPK_MAX = 64      # EG_TOPK_MAX: entries a top-K archive holds at most
PARETO_MAX = 256   # EG_PARETO_MAX: entries a Pareto archive holds at most
PARETO_KEEP_SPREAD = 0x100   # EG_PARETO_KEEP_SPREAD: OR-ed into an archive's mode, the capacity rule "keep spread"
STATS_LEN = 8 + 2 * YEARS * N_ACTIONS + YEARS * N_DEFICIT
CANDIDATE_BYTES = 8 + 8 + 32 + 4 * YEARS + 4 * YEARS + RUN_CAP + DEF_CAP
PACKET_BYTES = 8 * STATS_LEN + CANDIDATE_BYTES

EG_OK, EG_ERR_NO_DEVICE, EG_ERR_BAD_ARG, EG_ERR_HIP, EG_ERR_UNSUPPORTED, EG_ERR_NOMEM, EG_ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6
EG_EP_OK, EG_EP_OVERFLOW, EG_EP_NO_LOCATION, EG_EP_INTERNAL, EG_EP_INFEASIBLE = 0, -1, -2, -3, -4

# EIRGRID_LIB selects another build of the same library (only used for the -DEG_STAMPS diagnostic build)
LIB_PATH = os.environ.get("EIRGRID_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libeirgrid_hip.so")

_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)
_u16p = C.POINTER(C.c_uint16)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)


class EgWorld(C.Structure):
    _fields_ = [("n_settlements", C.c_int32), ("settlement_x", _dp), ("settlement_y", _dp), ("settlement_pop", _u32p),
                ("n_existing", C.c_int32), ("existing_x", _dp), ("existing_y", _dp), ("existing_type", _i32p),
                ("existing_capacity_mw", _dp), ("n_coast", C.c_int32), ("coast_x", _dp), ("coast_y", _dp),
                ("existing_operational_at_start", C.c_int32)]


class EgOpts(C.Structure):
    _fields_ = [("enable_energy_sales", C.c_int32), ("enable_construction_delays", C.c_int32), ("write_yearly", C.c_int32)]


class EgPolicySnapshot(C.Structure):
    _fields_ = [("weights", _dp), ("deficit_weights", _dp), ("count_weights", _dp),
                ("learning_rate", C.c_double), ("exploration_rate", C.c_double),
                ("iterations_without_improvement", C.c_uint32), ("has_best", C.c_int32),
                ("best_metrics", C.c_double * 4),
                ("best_count", _i32p), ("best_actions", _u8p), ("best_deficit_count", _i32p), ("best_deficit_actions", _u8p)]


class EgEpisodeOut(C.Structure):
    _fields_ = [("metrics", _dp), ("yearly", _dp), ("status", _i32p), ("n_run", _i32p), ("n_def", _i32p), ("n_act", _i32p),
                ("run_log", _u8p), ("def_log", _u8p), ("act_log", _u8p), ("n_gens", _i32p), ("gen_cell", _u16p),
                ("gen_pack", _u16p), ("n_offsets", _i32p), ("off_pack", _u16p), ("n_draws", _u64p), ("bytes_moved", _dp),
                ("n_chunks", _u32p)]


class EgPlanSet(C.Structure):
    _fields_ = [("n_plans", C.c_int32), ("best_count", _i32p), ("best_actions", _u8p), ("best_deficit_count", _i32p),
                ("best_deficit_actions", _u8p), ("best_actions_len", C.c_int64), ("best_deficit_actions_len", C.c_int64),
                ("names", C.POINTER(C.c_char_p))]


class EgPlanEdit(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("list", C.c_uint8), ("year", C.c_uint16), ("pos", C.c_uint32), ("action", C.c_uint8)]


class EgRefineOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("max_rounds", C.c_int32), ("n_replace", C.c_int32), ("replace_with", _u8p),
                ("n_append", C.c_int32), ("append_with", _u8p)]


class EgRefineStep(C.Structure):
    _fields_ = [("edit", EgPlanEdit), ("variant", C.c_int32), ("n_variants", C.c_int32), ("n_failed", C.c_int32), ("score", C.c_double),
                ("metrics", C.c_double * 4)]


class EgPlanMove(C.Structure):
    _fields_ = [("list", C.c_uint8), ("to_year", C.c_uint8), ("year", C.c_uint16), ("pos", C.c_uint32), ("to_pos", C.c_uint32)]


class EgRefineMoveOpts(C.Structure):
    _fields_ = [("max_shift", C.c_int32)]


class EgRefineMoveStep(C.Structure):
    _fields_ = [("is_move", C.c_int32), ("edit", EgPlanEdit), ("move", EgPlanMove), ("variant", C.c_int32), ("n_variants", C.c_int32),
                ("n_failed", C.c_int32), ("score", C.c_double), ("metrics", C.c_double * 4)]


class EgRepairStep(C.Structure):
    _fields_ = [("is_move", C.c_int32), ("edit", EgPlanEdit), ("move", EgPlanMove), ("variant", C.c_int32), ("n_variants", C.c_int32),
                ("n_failed", C.c_int32), ("n_feasible", C.c_int32), ("violated", C.c_uint32), ("violation", C.c_double), ("score", C.c_double),
                ("metrics", C.c_double * 4)]


class EgPlanCross(C.Structure):
    _fields_ = [("a", C.c_uint16), ("b", C.c_uint16), ("from_year", C.c_uint8), ("to_year", C.c_uint8)]


class EgBreedOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("objectives", C.c_int32), ("cap", C.c_int32), ("max_generations", C.c_int32), ("n_cuts", C.c_int32),
                ("cuts", _u8p), ("launch_variants", C.c_int32)]


class EgBreedGeneration(C.Structure):
    _fields_ = [("n_parents", C.c_int32), ("n_skipped", C.c_int32), ("n_kept", C.c_int32), ("n_children_kept", C.c_int32),
                ("n_variants", C.c_int64), ("n_valid", C.c_int64), ("n_dropped", C.c_int64)]


class EgActionMap(C.Structure):
    _fields_ = [("to", C.c_uint8 * N_ACTIONS)]


class EgPlanRewrite(C.Structure):
    _fields_ = [("plan", C.c_uint16), ("map", C.c_uint16), ("from_year", C.c_uint8), ("to_year", C.c_uint8), ("lists", C.c_uint8), ("pad", C.c_uint8)]


class EgBreedMember(C.Structure):
    _fields_ = [("cross", EgPlanCross), ("variant", C.c_int32), ("score", C.c_double), ("metrics", C.c_double * 4)]


class EgExploreOpts(C.Structure):
    _fields_ = [("mode", C.c_int32), ("objectives", C.c_int32), ("cap", C.c_int32), ("max_generations", C.c_int32), ("n_replace", C.c_int32),
                ("replace_with", _u8p), ("n_append", C.c_int32), ("append_with", _u8p), ("max_shift", C.c_int32), ("launch_variants", C.c_int32),
                ("max_variants", C.c_int64)]


class EgExploreGeneration(C.Structure):
    _fields_ = [("n_frontier", C.c_int32), ("n_held", C.c_int32), ("n_new", C.c_int32), ("pad", C.c_int32),
                ("n_variants", C.c_int64), ("n_valid", C.c_int64), ("n_dropped", C.c_int64)]


class EgExploreMember(C.Structure):
    _fields_ = [("parent", C.c_int64), ("is_move", C.c_int32), ("edit", EgPlanEdit), ("move", EgPlanMove), ("number", C.c_int64),
                ("score", C.c_double), ("metrics", C.c_double * 4)]


class EgPlanConstraint(C.Structure):
    _fields_ = [("column", C.c_uint8), ("aggregate", C.c_uint8), ("op", C.c_uint8), ("from_year", C.c_uint8), ("to_year", C.c_uint8), ("pad", C.c_uint8 * 3),
                ("bound", C.c_double)]


BUILD_CLASSES, BUILD_SPEC_MAX = 19, 1024      # EG_BUILD_CLASSES, EG_BUILD_SPEC_MAX
# the build classes in index order: the generator types (models/generator.rs order), then the four offsets
BUILD_CLASS_NAMES = ("OnshoreWind", "OffshoreWind", "DomesticSolar", "CommercialSolar", "UtilitySolar", "Nuclear", "CoalPlant", "GasCombinedCycle",
                     "GasPeaker", "Biomass", "HydroDam", "PumpedStorage", "BatteryStorage", "TidalGenerator", "WaveEnergy",
                     "Forest", "Wetland", "ActiveCapture", "CarbonCredit")


class EgBuildConstraint(C.Structure):
    _fields_ = [("aggregate", C.c_uint8), ("op", C.c_uint8), ("from_year", C.c_uint8), ("to_year", C.c_uint8), ("pad", C.c_uint8 * 4),
                ("bound", C.c_double), ("weight", C.c_double * BUILD_CLASSES)]


STREAMS_MAX = 64      # EG_STREAMS_MAX: draw streams a plan batch is judged over at most


class EgEnsembleRow(C.Structure):      # eg_ensemble_row: what k_ensemble_commit leaves per variant of a batch under plan streams
    _fields_ = [("nominal", C.c_double * 4), ("committed", C.c_double * 4), ("score_min", C.c_double), ("score_max", C.c_double),
                ("score_sum", C.c_double), ("n_ok", C.c_int32), ("n_infeasible", C.c_int32), ("n_failed", C.c_int32), ("worst_stream", C.c_int32),
                ("status", C.c_int32), ("pad", C.c_int32 * 5)]


assert C.sizeof(EgEnsembleRow) == 128
assert C.sizeof(EgPlanConstraint) == 16 and C.sizeof(EgBuildConstraint) == 168
assert C.sizeof(EgPlanMove) == 12 and C.sizeof(EgPlanCross) == 6
assert C.sizeof(EgActionMap) == 61 and C.sizeof(EgPlanRewrite) == 8
assert C.sizeof(EgExploreOpts) == 64 and C.sizeof(EgExploreGeneration) == 40 and C.sizeof(EgExploreMember) == 88
assert C.sizeof(EgBreedOpts) == 40 and C.sizeof(EgBreedGeneration) == 40 and C.sizeof(EgBreedMember) == 56

EDIT_NONE, EDIT_DELETE, EDIT_REPLACE, EDIT_INSERT = 0, 1, 2, 3
REFINE_LOCAL_OPTIMUM, REFINE_MAX_ROUNDS, REFINE_BASE_FAILED = 0, 1, 2
REPAIR_FEASIBLE, REPAIR_MAX_ROUNDS, REPAIR_BASE_FAILED, REPAIR_STUCK = 0, 1, 2, 3      # EG_REPAIR_*
REFINE_MAX_VARIANTS = 16384      # EG_REFINE_MAX_VARIANTS
REFINE_MAX_PLANS = 256           # EG_REFINE_MAX_PLANS
CROSS_MAX_PARENTS = 256          # EG_CROSS_MAX_PARENTS
CROSS_MAX_VARIANTS = 16384       # EG_CROSS_MAX_VARIANTS
REWRITE_DROP = 0xFF              # EG_REWRITE_DROP
REWRITE_MAX_MAPS = 256           # EG_REWRITE_MAX_MAPS
REWRITE_MAX_VARIANTS = 16384     # EG_REWRITE_MAX_VARIANTS
CONSTRAINTS_MAX, CONSTRAINT_SPEC_MAX = 32, 96      # EG_CONSTRAINTS_MAX, EG_CONSTRAINT_SPEC_MAX
AGG_EVERY, AGG_SUM, OP_LE, OP_GE = 0, 1, 0, 1      # EG_AGG_*, EG_OP_*
# the lower-case EG_Y_* names, in column order: what eg_plan_constraint_parse reads as COLUMN
YEARLY_COLUMNS = ("year", "pop", "usage", "gen", "balance", "opinion", "yearly_capital", "total_capital", "inflation", "co2", "offset", "net_co2",
                  "yearly_credit", "total_credit", "yearly_sales", "total_sales", "active_gens", "upgrade_costs", "closure_costs", "yearly_total_cost",
                  "total_cost")
BREED_CONVERGED, BREED_MAX_GENERATIONS, BREED_EMPTY = 0, 1, 2      # EG_BREED_*
EXPLORE_EXPLORED, EXPLORE_MAX_GENERATIONS, EXPLORE_EMPTY, EXPLORE_BUDGET = 0, 1, 2, 3      # EG_EXPLORE_*
PLAN_BLOCK_BYTES = 8832      # EG_PLAN_BLOCK_BYTES
DEBUG_LIST_LEN, DEBUG_FOLD_BEST_RESULT, DEBUG_FOLD_TOP_K = 8, 1, 2      # EG_DEBUG_*
# the crafted-generation hooks (eg_debug_breed_*): the canary byte, the multiplier of a block's tag, the two turnovers, and the layouts
DEBUG_BREED_CANARY, DEBUG_BREED_TAG_MUL = 0xC5, 0x9E3779B97F4A7C15                # EG_DEBUG_BREED_CANARY, EG_DEBUG_BREED_TAG_MUL
DEBUG_TURNOVER_BREED, DEBUG_TURNOVER_EXPLORE = 1, 2                               # EG_DEBUG_TURNOVER_*
DEBUG_PARETO_ENTRY_BYTES = 56                                                     # EG_DEBUG_PARETO_ENTRY_BYTES
DEBUG_PARETO_STATE_BYTES = 32 + PARETO_MAX * DEBUG_PARETO_ENTRY_BYTES             # EG_DEBUG_PARETO_STATE_BYTES
DEBUG_BREED_HEADER_BYTES, DEBUG_BREED_ROW_BYTES = 32, 288                         # EG_DEBUG_BREED_HEADER_BYTES, EG_DEBUG_BREED_ROW_BYTES
DEBUG_BREED_READBACK_BYTES = DEBUG_BREED_HEADER_BYTES + PARETO_MAX * DEBUG_BREED_ROW_BYTES      # EG_DEBUG_BREED_READBACK_BYTES
DEBUG_BREED_BLOCK_OFFSETS = 416                                                   # EG_DEBUG_BREED_BLOCK_OFFSETS


class EgUpdateCandidate(C.Structure):      # the candidate record of an update packet (CANDIDATE_BYTES)
    _fields_ = [("score", C.c_double), ("index", C.c_int64), ("metrics", C.c_double * 4), ("n_run", C.c_int32 * YEARS), ("n_def", C.c_int32 * YEARS),
                ("run_log", C.c_uint8 * RUN_CAP), ("def_log", C.c_uint8 * DEF_CAP)]


class EgDebugRefineEntry(C.Structure):      # eg_debug_refine_pick's step entry (EG_DEBUG_REFINE_ENTRY_BYTES)
    _fields_ = [("winner", C.c_int32), ("n_failed", C.c_int32), ("edit", C.c_uint32 * 2), ("score", C.c_double), ("metrics", C.c_double * 4),
                ("off26", C.c_int32), ("offd26", C.c_int32), ("base_ok", C.c_int32), ("n", C.c_int32), ("base_score", C.c_double),
                ("base_metrics", C.c_double * 4)]


class EgDebugRepairEntry(C.Structure):      # eg_debug_repair_pick_many's entry (EG_DEBUG_REPAIR_ENTRY_BYTES)
    _fields_ = [("winner", C.c_int32), ("n_failed", C.c_int32), ("edit", C.c_uint32 * 2), ("violation", C.c_double), ("score", C.c_double),
                ("metrics", C.c_double * 4), ("violated", C.c_uint32), ("n_feasible", C.c_int32), ("off26", C.c_int32), ("offd26", C.c_int32),
                ("base_ok", C.c_int32), ("n", C.c_int32), ("base_violation", C.c_double), ("base_score", C.c_double), ("base_violated", C.c_uint32),
                ("pad", C.c_uint32)]


assert C.sizeof(EgUpdateCandidate) == CANDIDATE_BYTES and C.sizeof(EgDebugRefineEntry) == 112
assert C.sizeof(EgRepairStep) == 96 and C.sizeof(EgDebugRepairEntry) == 112

# every symbol include/eirgrid_hip.h declares
EXPORTS = [
    "eg_build_hash", "eg_last_error", "eg_device_count", "eg_create", "eg_destroy", "eg_rollout_batch", "eg_upload_snapshot",
    "eg_rollout_launch", "eg_rollout_launch_update", "eg_sync", "eg_last_batch_size", "eg_policy_hold", "eg_policy_rewind", "eg_replay_hoist", "eg_replay_hoist_stats", "eg_debug_hoist_stamps", "eg_fetch", "eg_timing_reset", "eg_timing_read", "eg_timing_read_grids", "eg_memory_report", "eg_update_stats", "eg_fetch_scores",
    "eg_fetch_episode_lists", "eg_fetch_record", "eg_fetch_best_run", "eg_best_result_track", "eg_fetch_best_result", "eg_evaluate_action_impact", "eg_place", "eg_find_suitable_location", "eg_debug_fill_lds", "eg_debug_occupy", "eg_policy_apply_reduced", "eg_policy_apply_packet", "eg_train_step",
    "eg_policy_push", "eg_device_rollout", "eg_device_apply", "eg_device_step", "eg_policy_pull",
    "eg_group_create", "eg_group_destroy", "eg_group_rank", "eg_group_push", "eg_group_step", "eg_group_pull", "eg_group_replay_hoist",
    "eg_group_best_result_track", "eg_group_fetch_best_result", "eg_top_k_track", "eg_fetch_top_k", "eg_rank_score",
    "eg_pareto_track", "eg_pareto_fold_last_batch", "eg_fetch_pareto", "eg_debug_pareto_fold",
    "eg_debug_load_batch", "eg_debug_fold_last_batch", "eg_debug_pick_best", "eg_debug_refine_pick",
    "eg_group_top_k_track", "eg_group_fetch_top_k", "eg_plans_validate", "eg_evaluate_plans", "eg_plans_load", "eg_plans_free",
    "eg_plan_edits_validate", "eg_evaluate_plan_edits", "eg_debug_fetch_plan_block", "eg_plans_save", "eg_refine_validate", "eg_refine_plan",
    "eg_refine_plans_validate", "eg_refine_plans", "eg_debug_refine_pick_many",
    "eg_debug_breed_begin", "eg_debug_breed_chunk", "eg_debug_breed_turnover", "eg_debug_breed_fetch", "eg_debug_tiles_refresh",
    "eg_plan_moves_validate", "eg_evaluate_plan_moves", "eg_refine_plans_moves_validate", "eg_refine_plans_moves",
    "eg_plan_crosses_validate", "eg_evaluate_plan_crosses", "eg_plan_rewrites_validate", "eg_evaluate_plan_rewrites",
    "eg_breed_validate", "eg_breed_plans", "eg_explore_validate", "eg_explore_neighbourhood", "eg_explore_plans",
    "eg_plan_constraints_validate", "eg_plan_constraints_set", "eg_fetch_plan_feasibility", "eg_last_batch_constraints", "eg_plan_constraint_parse", "eg_plan_constraint_format",
    "eg_debug_load_yearly", "eg_debug_constrain_last_batch",
    "eg_build_constraints_validate", "eg_build_constraints_set", "eg_last_batch_build_constraints", "eg_build_constraint_parse", "eg_build_constraint_format",
    "eg_debug_load_built",
    "eg_repair_plans_validate", "eg_repair_plans", "eg_debug_repair_pick_many",
    "eg_plan_streams_validate", "eg_plan_streams_set", "eg_last_batch_streams", "eg_fetch_plan_ensemble", "eg_fetch_plan_streams",
    "eg_debug_ensemble_keep", "eg_debug_ensemble_commit",
    "eg_host_tables_create", "eg_host_tables_free", "eg_host_tables_f64", "eg_host_tables_i32",
    "eg_policy_new", "eg_policy_free", "eg_policy_snapshot_view", "eg_policy_get_tables", "eg_policy_set_tables",
    "eg_policy_get_scalar", "eg_policy_set_scalar", "eg_policy_get_list", "eg_policy_apply_episode", "eg_score_metrics",
    "eg_policy_save_json", "eg_policy_load_json", "eg_policy_append_weight_history", "eg_policy_export_improvement_csv", "eg_export_summary_csv", "eg_export_run_details",
]

_lib = None


def source_hash() -> str:
    """The hash csrc/Makefile stamps into the library (eg_build_hash): sha256 over the sources it is built from, in the
    Makefile's order (make's $(sort) = byte order of the relative paths)."""
    import glob
    import hashlib
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    rel = [os.path.basename(f) for pat in ("*.hip", "*.cpp", "*.h") for f in glob.glob(os.path.join(csrc, pat))]
    rel += ["../../include/" + os.path.basename(f) for f in glob.glob(os.path.join(csrc, "..", "..", "include", "*.h"))]
    rel = sorted(set(rel + ["Makefile"]) - {"eg_build_hash.cpp"}, key=lambda r: r.encode())
    h = hashlib.sha256()
    for r in rel:
        h.update(open(os.path.join(csrc, r), "rb").read())
    return h.hexdigest()[:16]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950).  eirgrid_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    L.eg_build_hash.restype = C.c_char_p
    if not os.environ.get("EIRGRID_LIB"):      # a stale or mixed binary (e.g. a prebuilt .so shipped next to edited sources) fails loudly
        built, tree = L.eg_build_hash().decode(), source_hash()
        if built != tree:
            raise ImportError(f"{LIB_PATH} was built from other sources (library {built}, tree {tree}): run `make -C eirgrid_amd/csrc`")
    L.eg_last_error.restype = C.c_char_p
    L.eg_device_count.restype = C.c_int32
    L.eg_create.restype = C.c_void_p
    L.eg_create.argtypes = [C.c_int32, C.POINTER(EgWorld)]
    L.eg_destroy.argtypes = [C.c_void_p]
    L.eg_rollout_batch.restype = C.c_int32
    L.eg_rollout_batch.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.c_uint64, C.c_uint64,
                                   C.c_uint32, _u8p, C.POINTER(EgEpisodeOut)]
    L.eg_upload_snapshot.restype = C.c_int32
    L.eg_upload_snapshot.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts)]
    L.eg_rollout_launch.restype = C.c_int32
    L.eg_rollout_launch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, _u8p]
    L.eg_rollout_launch_update.restype = C.c_int32
    L.eg_rollout_launch_update.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, _u8p, C.c_void_p]
    L.eg_sync.restype = C.c_int32
    L.eg_sync.argtypes = [C.c_void_p]
    L.eg_last_batch_size.restype = C.c_uint32
    for f in (L.eg_policy_hold, L.eg_policy_rewind):
        f.restype = C.c_int32; f.argtypes = [C.c_void_p]
    L.eg_last_batch_size.argtypes = [C.c_void_p]
    if hasattr(L, "eg_replay_hoist") or not os.environ.get("EIRGRID_LIB"):      # (EIRGRID_LIB: an A/B build may predate it)
        L.eg_replay_hoist.restype = C.c_int32
        L.eg_replay_hoist.argtypes = [C.c_void_p, C.c_int32]
        L.eg_replay_hoist_stats.restype = C.c_int32
        L.eg_replay_hoist_stats.argtypes = [C.c_void_p, _u64p, _i32p]
        L.eg_debug_hoist_stamps.restype = C.c_int32
        L.eg_debug_hoist_stamps.argtypes = [C.c_void_p, _u64p]
    L.eg_fetch.restype = C.c_int32
    L.eg_fetch.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut)]
    L.eg_timing_reset.restype = C.c_int32
    L.eg_timing_reset.argtypes = [C.c_void_p]
    L.eg_timing_read.restype = C.c_int32
    L.eg_timing_read.argtypes = [C.c_void_p, _dp, _i32p]
    if hasattr(L, "eg_memory_report") or not os.environ.get("EIRGRID_LIB"):      # (EIRGRID_LIB: an A/B build may predate it)
        L.eg_memory_report.restype = C.c_int32
        L.eg_memory_report.argtypes = [C.c_void_p, _u64p, _u64p, _u64p]
    L.eg_timing_read_grids.restype = C.c_int32
    L.eg_timing_read_grids.argtypes = [C.c_void_p, _dp, _dp, _i32p]
    L.eg_update_stats.restype = C.c_int32
    L.eg_update_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.eg_fetch_scores.restype = C.c_int32
    L.eg_fetch_scores.argtypes = [C.c_void_p, _dp]
    L.eg_fetch_episode_lists.restype = C.c_int32
    L.eg_fetch_episode_lists.argtypes = [C.c_void_p, C.c_uint32, _dp, _i32p, _u8p, _i32p, _u8p]
    L.eg_policy_apply_reduced.restype = C.c_int32
    L.eg_policy_apply_reduced.argtypes = [C.c_void_p, C.POINTER(C.c_int64), _dp, _i32p, _u8p, _i32p, _u8p, C.c_uint64]
    L.eg_policy_apply_packet.restype = C.c_int32
    L.eg_policy_apply_packet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64]
    L.eg_train_step.restype = C.c_int32
    L.eg_train_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, _u8p, C.c_uint64]
    L.eg_policy_push.restype = C.c_int32
    L.eg_policy_push.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.eg_device_rollout.restype = C.c_int32
    L.eg_device_rollout.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]
    L.eg_device_apply.restype = C.c_int32
    L.eg_device_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint64]
    L.eg_device_step.restype = C.c_int32
    L.eg_device_step.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    L.eg_policy_pull.restype = C.c_int32
    L.eg_policy_pull.argtypes = [C.c_void_p, C.c_void_p]
    L.eg_group_create.restype = C.c_void_p
    L.eg_group_create.argtypes = [_i32p, C.c_int32, C.POINTER(EgWorld)]
    L.eg_group_destroy.restype = None
    L.eg_group_destroy.argtypes = [C.c_void_p]
    L.eg_group_rank.restype = C.c_void_p
    L.eg_group_rank.argtypes = [C.c_void_p, C.c_int32]
    L.eg_group_push.restype = C.c_int32
    L.eg_group_push.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.eg_group_step.restype = C.c_int32
    L.eg_group_step.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
    L.eg_group_pull.restype = C.c_int32
    L.eg_group_pull.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.eg_group_replay_hoist.restype = C.c_int32
    L.eg_group_replay_hoist.argtypes = [C.c_void_p, C.c_int32]
    L.eg_group_best_result_track.restype = C.c_int32
    L.eg_group_best_result_track.argtypes = [C.c_void_p, C.c_int32]
    L.eg_group_fetch_best_result.restype = C.c_int32
    L.eg_group_fetch_best_result.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.eg_policy_append_weight_history.restype = C.c_int32
    L.eg_policy_append_weight_history.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
    L.eg_policy_export_improvement_csv.restype = C.c_int32
    L.eg_export_summary_csv.restype = C.c_int32
    L.eg_export_summary_csv.argtypes = [C.POINTER(EgEpisodeOut), C.c_char_p, C.c_char_p]
    L.eg_export_run_details.restype = C.c_int32
    L.eg_export_run_details.argtypes = [C.POINTER(EgWorld), C.POINTER(C.c_char_p), C.POINTER(EgEpisodeOut), C.c_char_p, C.c_uint64]
    L.eg_fetch_record.restype = C.c_int32
    L.eg_fetch_record.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(EgEpisodeOut)]
    L.eg_best_result_track.restype = C.c_int32
    L.eg_best_result_track.argtypes = [C.c_void_p, C.c_int32]
    L.eg_fetch_best_result.restype = C.c_int32
    L.eg_fetch_best_result.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.eg_top_k_track.restype = C.c_int32
    L.eg_top_k_track.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.eg_fetch_top_k.restype = C.c_int32
    L.eg_fetch_top_k.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut), C.POINTER(C.c_int32), _dp, C.POINTER(C.c_int64)]
    L.eg_group_top_k_track.restype = C.c_int32
    L.eg_group_top_k_track.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.eg_group_fetch_top_k.restype = C.c_int32
    L.eg_group_fetch_top_k.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut), C.POINTER(C.c_int32), _dp, C.POINTER(C.c_int64)]
    L.eg_plans_validate.restype = C.c_int32
    L.eg_plans_validate.argtypes = [C.POINTER(EgPlanSet)]
    L.eg_evaluate_plans.restype = C.c_int32
    L.eg_evaluate_plans.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.c_uint64, C.c_uint64,
                                    C.POINTER(EgEpisodeOut)]
    # EIRGRID_LIB names another build of the library for an A/B measurement (scripts/plan_edit_probe.py times the host path of a build of
    # the parent commit, which has no plan edits): such a build may lack these symbols and still loads.  The shipped library must have them.
    if hasattr(L, "eg_evaluate_plan_edits") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plan_edits_validate.restype = C.c_int32
        L.eg_plan_edits_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgPlanEdit), C.c_int32]
        L.eg_debug_fetch_plan_block.restype = C.c_int32
        L.eg_debug_fetch_plan_block.argtypes = [C.c_void_p, C.c_uint32, _u8p]
        L.eg_evaluate_plan_edits.restype = C.c_int32
        L.eg_evaluate_plan_edits.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgPlanEdit),
                                             C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(EgEpisodeOut)]
    # (likewise: scripts/refine_probe.py times the Python loop on a build of the parent commit, which has no refinement)
    if hasattr(L, "eg_refine_plan") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plans_save.restype = C.c_int32
        L.eg_plans_save.argtypes = [C.POINTER(EgPlanSet), C.c_char_p]
        L.eg_refine_validate.restype = C.c_int32
        L.eg_refine_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts)]
        L.eg_refine_plan.restype = C.c_int32
        L.eg_refine_plan.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts),
                                     C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(EgPlanSet)), C.POINTER(EgRefineStep), _i32p, _i32p, _dp,
                                     C.POINTER(EgEpisodeOut)]
    # (likewise: scripts/refine_many_probe.py may load a build of the parent commit, which refines one plan a call)
    if hasattr(L, "eg_refine_plans") or not os.environ.get("EIRGRID_LIB"):
        L.eg_refine_plans_validate.restype = C.c_int32
        L.eg_refine_plans_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts)]
        L.eg_refine_plans.restype = C.c_int32
        L.eg_refine_plans.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts),
                                      C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(EgPlanSet)), C.POINTER(EgRefineStep), _i32p, _i32p, _dp,
                                      C.POINTER(EgEpisodeOut)]
        L.eg_debug_refine_pick_many.restype = C.c_int32
        L.eg_debug_refine_pick_many.argtypes = [C.c_void_p, C.c_int32, _u32p, _u32p, C.c_int32, C.c_void_p, _u8p]
    # (likewise: a probe may load a build of the parent commit, which has no plan moves)
    if hasattr(L, "eg_evaluate_plan_moves") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plan_moves_validate.restype = C.c_int32
        L.eg_plan_moves_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgPlanMove), C.c_int32]
        L.eg_evaluate_plan_moves.restype = C.c_int32
        L.eg_evaluate_plan_moves.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgPlanMove),
                                             C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(EgEpisodeOut)]
        L.eg_refine_plans_moves_validate.restype = C.c_int32
        L.eg_refine_plans_moves_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts), C.POINTER(EgRefineMoveOpts)]
        L.eg_refine_plans_moves.restype = C.c_int32
        L.eg_refine_plans_moves.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts),
                                            C.POINTER(EgRefineMoveOpts), C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(EgPlanSet)), C.POINTER(EgRefineMoveStep),
                                            _i32p, _i32p, _dp, C.POINTER(EgEpisodeOut)]
    # (likewise: a probe may load a build of the parent commit, which has no plan crosses)
    if hasattr(L, "eg_evaluate_plan_crosses") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plan_crosses_validate.restype = C.c_int32
        L.eg_plan_crosses_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgPlanCross), C.c_int32]
        L.eg_evaluate_plan_crosses.restype = C.c_int32
        L.eg_evaluate_plan_crosses.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgPlanCross),
                                               C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(EgEpisodeOut)]
    # (likewise: scripts/rewrite_probe.py may load a build of the parent commit, which has no plan rewrites)
    if hasattr(L, "eg_evaluate_plan_rewrites") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plan_rewrites_validate.restype = C.c_int32
        L.eg_plan_rewrites_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgActionMap), C.c_int32, C.POINTER(EgPlanRewrite), C.c_int32]
        L.eg_evaluate_plan_rewrites.restype = C.c_int32
        L.eg_evaluate_plan_rewrites.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgActionMap), C.c_int32,
                                                C.POINTER(EgPlanRewrite), C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(EgEpisodeOut)]
    # (likewise: scripts/breed_probe.py may load a build of the parent commit, which crosses one generation a call)
    if hasattr(L, "eg_breed_plans") or not os.environ.get("EIRGRID_LIB"):
        L.eg_breed_validate.restype = C.c_int32
        L.eg_breed_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgBreedOpts)]
        L.eg_breed_plans.restype = C.c_int32
        L.eg_breed_plans.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgBreedOpts),
                                     C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(EgPlanSet)), C.POINTER(EgBreedGeneration), C.POINTER(EgBreedMember),
                                     _i32p, _i32p, C.POINTER(EgEpisodeOut)]
    # (likewise: a probe may load a build of the parent commit, which does not explore)
    if hasattr(L, "eg_explore_plans") or not os.environ.get("EIRGRID_LIB"):
        L.eg_explore_validate.restype = C.c_int32
        L.eg_explore_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgExploreOpts)]
        L.eg_explore_neighbourhood.restype = C.c_int32
        L.eg_explore_neighbourhood.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgExploreOpts), C.POINTER(C.c_int64)]
        L.eg_explore_plans.restype = C.c_int32
        L.eg_explore_plans.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgExploreOpts),
                                       C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(EgPlanSet)), C.POINTER(EgExploreGeneration),
                                       C.POINTER(EgExploreMember), C.POINTER(C.c_int64), _i32p, _i32p, C.POINTER(EgEpisodeOut)]
    # (likewise: an A/B build named by EIRGRID_LIB may predate plan constraints)
    if hasattr(L, "eg_plan_constraints_set") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plan_constraints_validate.restype = C.c_int32
        L.eg_plan_constraints_validate.argtypes = [C.POINTER(EgPlanConstraint), C.c_int32]
        L.eg_plan_constraints_set.restype = C.c_int32
        L.eg_plan_constraints_set.argtypes = [C.c_void_p, C.POINTER(EgPlanConstraint), C.c_int32]
        L.eg_fetch_plan_feasibility.restype = C.c_int32
        L.eg_fetch_plan_feasibility.argtypes = [C.c_void_p, _u32p, _dp]
        L.eg_last_batch_constraints.restype = C.c_int32
        L.eg_last_batch_constraints.argtypes = [C.c_void_p, C.POINTER(EgPlanConstraint)]
        L.eg_plan_constraint_parse.restype = C.c_int32
        L.eg_plan_constraint_parse.argtypes = [C.c_char_p, C.POINTER(EgPlanConstraint)]
        L.eg_plan_constraint_format.restype = C.c_int32
        L.eg_plan_constraint_format.argtypes = [C.POINTER(EgPlanConstraint), C.c_char_p, C.c_int32]
        L.eg_debug_load_yearly.restype = C.c_int32
        L.eg_debug_load_yearly.argtypes = [C.c_void_p, _dp, C.c_uint32]
        L.eg_debug_constrain_last_batch.restype = C.c_int32
        L.eg_debug_constrain_last_batch.argtypes = [C.c_void_p]
    # (likewise: scripts/build_constraint_probe.py may load a build of the parent commit, which has no build constraints)
    if hasattr(L, "eg_build_constraints_set") or not os.environ.get("EIRGRID_LIB"):
        L.eg_build_constraints_validate.restype = C.c_int32
        L.eg_build_constraints_validate.argtypes = [C.POINTER(EgBuildConstraint), C.c_int32]
        L.eg_build_constraints_set.restype = C.c_int32
        L.eg_build_constraints_set.argtypes = [C.c_void_p, C.POINTER(EgBuildConstraint), C.c_int32]
        L.eg_last_batch_build_constraints.restype = C.c_int32
        L.eg_last_batch_build_constraints.argtypes = [C.c_void_p, C.POINTER(EgBuildConstraint)]
        L.eg_build_constraint_parse.restype = C.c_int32
        L.eg_build_constraint_parse.argtypes = [C.c_char_p, C.POINTER(EgBuildConstraint)]
        L.eg_build_constraint_format.restype = C.c_int32
        L.eg_build_constraint_format.argtypes = [C.POINTER(EgBuildConstraint), C.c_char_p, C.c_int32]
        L.eg_debug_load_built.restype = C.c_int32
        L.eg_debug_load_built.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.c_uint32]
    # (likewise: scripts/repair_probe.py may load a build of the parent commit, which has no repair)
    if hasattr(L, "eg_repair_plans") or not os.environ.get("EIRGRID_LIB"):
        L.eg_repair_plans_validate.restype = C.c_int32
        L.eg_repair_plans_validate.argtypes = [C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts), C.POINTER(EgRefineMoveOpts), _dp, C.c_int32]
        L.eg_repair_plans.restype = C.c_int32
        L.eg_repair_plans.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot), C.POINTER(EgOpts), C.POINTER(EgPlanSet), C.POINTER(EgRefineOpts),
                                      C.POINTER(EgRefineMoveOpts), _dp, C.c_uint64, C.c_uint64, C.POINTER(C.POINTER(EgPlanSet)), C.POINTER(EgRepairStep),
                                      _i32p, _i32p, _dp, _dp, C.POINTER(EgEpisodeOut)]
        L.eg_debug_repair_pick_many.restype = C.c_int32
        L.eg_debug_repair_pick_many.argtypes = [C.c_void_p, C.c_int32, _dp, _u32p, _u32p, C.c_int32, C.c_void_p, _u8p]
    # (likewise: scripts/ensemble_probe.py may load a build of the parent commit, which has no plan streams)
    if hasattr(L, "eg_plan_streams_set") or not os.environ.get("EIRGRID_LIB"):
        L.eg_plan_streams_validate.restype = C.c_int32
        L.eg_plan_streams_validate.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.eg_plan_streams_set.restype = C.c_int32
        L.eg_plan_streams_set.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.eg_last_batch_streams.restype = C.c_int32
        L.eg_last_batch_streams.argtypes = [C.c_void_p, _i32p, _i32p]
        L.eg_fetch_plan_ensemble.restype = C.c_int32
        L.eg_fetch_plan_ensemble.argtypes = [C.c_void_p, C.POINTER(EgEnsembleRow)]
        L.eg_fetch_plan_streams.restype = C.c_int32
        L.eg_fetch_plan_streams.argtypes = [C.c_void_p, _dp, _i32p]
        L.eg_debug_ensemble_keep.restype = C.c_int32
        L.eg_debug_ensemble_keep.argtypes = [C.c_void_p, C.c_int32]
        L.eg_debug_ensemble_commit.restype = C.c_int32
        L.eg_debug_ensemble_commit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    if hasattr(L, "eg_pareto_track") or not os.environ.get("EIRGRID_LIB"):
        L.eg_pareto_track.restype = C.c_int32
        L.eg_pareto_track.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.eg_pareto_fold_last_batch.restype = C.c_int32
        L.eg_pareto_fold_last_batch.argtypes = [C.c_void_p]
        L.eg_fetch_pareto.restype = C.c_int32
        L.eg_fetch_pareto.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut), _i32p, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64)]
        L.eg_debug_pareto_fold.restype = C.c_int32
        L.eg_debug_pareto_fold.argtypes = [C.c_void_p, _dp, _i32p, C.c_uint32, C.c_uint64]
    if hasattr(L, "eg_debug_load_batch") or not os.environ.get("EIRGRID_LIB"):      # (likewise: the crafted-batch test hooks)
        L.eg_debug_load_batch.restype = C.c_int32
        L.eg_debug_load_batch.argtypes = [C.c_void_p, _dp, _i32p, _i32p, _u8p, _dp, C.c_uint32, C.c_uint64]
        L.eg_debug_fold_last_batch.restype = C.c_int32
        L.eg_debug_fold_last_batch.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.eg_debug_pick_best.restype = C.c_int32
        L.eg_debug_pick_best.argtypes = [C.c_void_p, C.c_void_p]
        L.eg_debug_refine_pick.restype = C.c_int32
        L.eg_debug_refine_pick.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, _u8p]
    if hasattr(L, "eg_debug_breed_begin") or not os.environ.get("EIRGRID_LIB"):      # (likewise: the crafted-generation test hooks)
        L.eg_debug_breed_begin.restype = C.c_int32
        L.eg_debug_breed_begin.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.eg_debug_breed_chunk.restype = C.c_int32
        L.eg_debug_breed_chunk.argtypes = [C.c_void_p, _dp, _i32p, C.c_uint32, C.c_uint64]
        L.eg_debug_breed_turnover.restype = C.c_int32
        L.eg_debug_breed_turnover.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64]
        L.eg_debug_breed_fetch.restype = C.c_int32
        L.eg_debug_breed_fetch.argtypes = [C.c_void_p, C.c_void_p, _u8p, _u8p, _u8p, _u8p, C.c_void_p, _u64p]
    if hasattr(L, "eg_debug_tiles_refresh") or not os.environ.get("EIRGRID_LIB"):      # (likewise: the lazy field's catch-up on one wave)
        L.eg_debug_tiles_refresh.restype = C.c_int32
        L.eg_debug_tiles_refresh.argtypes = [C.c_void_p, _u16p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp, _i32p]
    L.eg_plans_load.restype = C.POINTER(EgPlanSet)
    L.eg_plans_load.argtypes = [C.c_char_p]
    L.eg_plans_free.argtypes = [C.POINTER(EgPlanSet)]
    L.eg_rank_score.restype = C.c_double
    L.eg_rank_score.argtypes = [_dp, C.c_int32]
    L.eg_evaluate_action_impact.restype = C.c_double
    L.eg_evaluate_action_impact.argtypes = [_dp, _dp, C.c_int32]
    L.eg_fetch_best_run.restype = C.c_int32
    L.eg_fetch_best_run.argtypes = [C.c_void_p, C.POINTER(EgEpisodeOut), C.POINTER(C.c_int32)]
    L.eg_policy_export_improvement_csv.argtypes = [C.c_void_p, C.c_char_p]
    L.eg_find_suitable_location.restype = C.c_int32
    L.eg_find_suitable_location.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _dp, _dp, C.c_int32, C.c_float, _dp, _dp, _i32p, _dp]
    L.eg_place.restype = C.c_int32
    L.eg_debug_fill_lds.restype = C.c_int32
    L.eg_debug_fill_lds.argtypes = [C.c_void_p, C.c_uint32]
    if hasattr(L, "eg_debug_occupy") or not os.environ.get("EIRGRID_LIB"):
        L.eg_debug_occupy.restype = C.c_int32
        L.eg_debug_occupy.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
    L.eg_place.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _u16p, C.c_int32, _i32p, _dp]
    L.eg_host_tables_create.restype = C.c_void_p
    L.eg_host_tables_create.argtypes = [C.POINTER(EgWorld)]
    L.eg_host_tables_free.argtypes = [C.c_void_p]
    L.eg_host_tables_f64.restype = C.c_int32
    L.eg_host_tables_f64.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(_dp), C.POINTER(C.c_int64)]
    L.eg_host_tables_i32.restype = C.c_int32
    L.eg_host_tables_i32.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(_i32p), C.POINTER(C.c_int64)]
    L.eg_policy_new.restype = C.c_void_p
    L.eg_policy_free.argtypes = [C.c_void_p]
    L.eg_policy_snapshot_view.restype = C.c_int32
    L.eg_policy_snapshot_view.argtypes = [C.c_void_p, C.POINTER(EgPolicySnapshot)]
    L.eg_policy_get_tables.restype = C.c_int32
    L.eg_policy_get_tables.argtypes = [C.c_void_p, _dp, _dp, _dp]
    L.eg_policy_set_tables.restype = C.c_int32
    L.eg_policy_set_tables.argtypes = [C.c_void_p, _dp, _dp, _dp]
    L.eg_policy_get_scalar.restype = C.c_double
    L.eg_policy_get_scalar.argtypes = [C.c_void_p, C.c_int32]
    L.eg_policy_set_scalar.restype = C.c_int32
    L.eg_policy_set_scalar.argtypes = [C.c_void_p, C.c_int32, C.c_double]
    L.eg_policy_get_list.restype = C.c_int32
    L.eg_policy_get_list.argtypes = [C.c_void_p, C.c_int32, C.c_int32, _u8p, C.c_int32]
    L.eg_policy_apply_episode.restype = C.c_int32
    L.eg_policy_apply_episode.argtypes = [C.c_void_p, _dp, _i32p, _u8p, _i32p, _u8p, C.c_uint64]
    L.eg_policy_save_json.restype = C.c_int32
    L.eg_policy_save_json.argtypes = [C.c_void_p, C.c_char_p]
    L.eg_policy_load_json.restype = C.c_void_p
    L.eg_policy_load_json.argtypes = [C.c_char_p]
    L.eg_score_metrics.restype = C.c_double
    L.eg_score_metrics.argtypes = [_dp, C.c_int32]
    _lib = L
    return L


class EirgridError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    if rc != EG_OK:
        msg = lib().eg_last_error()
        raise EirgridError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
