"""The C ABI of include/mcl_hip_engine.h (libmcl_hip_engine.so), stated once for Python: its constants, its structures, the
numpy record views of its result types, one signature per exported function, and the loader that applies them.

A new export is one line of SIGNATURES (plus a structure, if it brings one); tests/test_abi_table.py holds every line, every
layout and every constant here to the header.  There is no fallback -- if the shared library is missing, load_library raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MCL_LIB: another build of the same library, for A/B runs on one box -- a development aid, never set by the product or the tests)
LIB_PATH = os.environ.get("MCL_LIB") or os.path.join(_HERE, "libmcl_hip_engine.so")
LEGACY_LIB_PATH = os.path.join(_HERE, "libmcl_hip_engine_legacy.so")

# ---- constants (each MCL_<name> of the header; tests/test_abi_table.py compares the values) ---------------------------------------
MCL_OK = 0
MCL_ERR_INVALID_ARG = -1
MCL_ERR_NOT_READY = -2
MCL_ERR_UNSUPPORTED = -5
MCL_ERR_PEER = -6          # sharded update: another rank reported a failure; the update is void on every rank
MCL_ERR_TIMEOUT = -7       # sharded update: a collective did not finish in time; the communicator was aborted
RESAMPLE_MULTINOMIAL, RESAMPLE_SYSTEMATIC = 0, 1
WEIGHT_LOG, WEIGHT_PRODUCT = 0, 1
RAYS_AUTO, RAYS_MARCH, RAYS_SKIP, RAYS_QUAD, RAYS_CELL, RAYS_SWEEP = 0, 1, 2, 3, 4, 5
RAYS_DESKEW = 6            # reported only: the kernel of an update with per-beam sensor offsets on (Engine.set_beam_offsets)
BUF_X, BUF_Y, BUF_THETA, BUF_QWEIGHT, BUF_LOGW, BUF_SCALARS = range(6)
MOTION_REFERENCE, MOTION_DIFF, MOTION_OMNI = 0, 1, 2
MOTION_MODELS = {"reference": MOTION_REFERENCE, "diff": MOTION_DIFF, "omni": MOTION_OMNI}
WEDGES = 16                      # MCL_WEDGES
MAX_SEARCH_SCANS = 16            # MCL_SEARCH_MAX_SCANS
MAX_REFINE_SEQ_ROWS = 1 << 21    # MCL_REFINE_SEQ_MAX_ROWS
# limits the header states in the comments of its calls only -- no macro to compare with:
MAX_QUERY_POSES = 65536
MAX_SEARCH_HITS = 65536
MAX_REFINE_SEEDS, MAX_REFINE_WINDOW = 4096, 32768
# mcl_get_map_table: name -> (selector MCL_MAP_TABLE_<NAME>, dtype); the header names QUADRANT0 and leaves 4 .. 6 to a comment
MAP_TABLES = {"grid": (0, np.int8), "skip": (1, np.uint8), "skip_nibbles": (2, np.uint8), "quadrant0": (3, np.uint8), "quadrant1": (4, np.uint8),
              "quadrant2": (5, np.uint8), "quadrant3": (6, np.uint8), "free_cells": (7, np.uint32)}


# ---- structures (_c_name_: the header's type; tests/test_abi_table.py compares every size and offset) -----------------------------
class Config(C.Structure):
    _c_name_ = "mcl_config_t"
    _fields_ = [
        ("max_particles", C.c_int64), ("device", C.c_int32), ("seed", C.c_uint64), ("max_range_m", C.c_double),
        ("z_hit", C.c_double), ("z_short", C.c_double), ("z_max", C.c_double), ("z_rand", C.c_double),
        ("sigma_hit", C.c_double), ("squash_factor", C.c_double), ("motion_dispersion_x", C.c_double),
        ("motion_dispersion_y", C.c_double), ("motion_dispersion_theta", C.c_double), ("resample_mode", C.c_int32),
        ("weight_mode", C.c_int32), ("ray_kernel", C.c_int32), ("keep_ray_steps", C.c_int32),
        ("debug_force_exact", C.c_int32), ("debug_count_probes", C.c_int32), ("rays_per_lane", C.c_int32),
        ("resample_neff_permille", C.c_int32), ("graph_mode", C.c_int32), ("reserved", C.c_int32 * 3),
    ]


class KldConfig(C.Structure):
    """mcl_kld_config_t: KLD-adaptive particle count (Engine.set_kld)."""
    _c_name_ = "mcl_kld_config_t"
    _fields_ = [
        ("min_particles", C.c_int64), ("max_particles", C.c_int64), ("err", C.c_double), ("z", C.c_double),
        ("bin_x_m", C.c_double), ("bin_y_m", C.c_double), ("n_theta_bins", C.c_int32), ("round_to", C.c_int32),
        ("shrink_permille", C.c_int32), ("reserved", C.c_int32),
    ]


class RecoveryConfig(C.Structure):
    """mcl_recovery_config_t: recovery by random-particle injection (Engine.set_recovery)."""
    _c_name_ = "mcl_recovery_config_t"
    _fields_ = [("alpha_slow", C.c_double), ("alpha_fast", C.c_double), ("per_beam", C.c_int32), ("reserved", C.c_int32)]


class LikelihoodFieldConfig(C.Structure):
    """mcl_likelihood_field_config_t: the likelihood-field sensor model (Engine.set_likelihood_field)."""
    _c_name_ = "mcl_likelihood_field_config_t"
    _fields_ = [("z_hit", C.c_double), ("z_rand", C.c_double), ("sigma_hit_m", C.c_double), ("max_occ_dist_m", C.c_double),
                ("reserved", C.c_int32 * 2)]


class BeamSkipConfig(C.Structure):
    """mcl_beam_skip_config_t: beam skipping for the likelihood field (Engine.set_beam_skip)."""
    _c_name_ = "mcl_beam_skip_config_t"
    _fields_ = [("distance_m", C.c_double), ("threshold", C.c_double), ("error_threshold", C.c_double), ("reserved", C.c_int32 * 2)]


class BeamSkipState(C.Structure):
    """mcl_beam_skip_state_t: what the last update with beam skipping decided (Engine.beam_skip_state, rule BS6)."""
    _c_name_ = "mcl_beam_skip_state_t"
    _fields_ = [("n_particles", C.c_int64), ("min_count", C.c_int64), ("n_used", C.c_int32), ("n_kept", C.c_int32),
                ("n_skipped", C.c_int32), ("min_skipped", C.c_int32), ("integrate_all", C.c_int32), ("ka", C.c_int32)]


class MotionConfig(C.Structure):
    """mcl_motion_config_t: the odometry motion models (Engine.set_motion_model)."""
    _c_name_ = "mcl_motion_config_t"
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("alpha1", C.c_double), ("alpha2", C.c_double),
                ("alpha3", C.c_double), ("alpha4", C.c_double), ("alpha5", C.c_double), ("floor_trans_m", C.c_double),
                ("floor_rot_rad", C.c_double)]


class ClusterConfig(C.Structure):
    """mcl_cluster_config_t: the bins of the pose clustering (Engine.pose_clusters)."""
    _c_name_ = "mcl_cluster_config_t"
    _fields_ = [("bin_x_m", C.c_double), ("bin_y_m", C.c_double), ("n_theta_bins", C.c_int32), ("reserved", C.c_int32)]


class Cluster(C.Structure):
    """mcl_cluster_t: one pose hypothesis."""
    _c_name_ = "mcl_cluster_t"
    _fields_ = [
        ("weight_q", C.c_uint64), ("weight", C.c_double), ("n_particles", C.c_int64), ("n_bins", C.c_int64),
        ("first_bin", C.c_int64), ("mean", C.c_double * 3), ("cov", C.c_double * 9),
    ]


class PoseScore(C.Structure):
    """mcl_pose_score_t: how well a scan supports one pose (Engine.score_poses)."""
    _c_name_ = "mcl_pose_score_t"
    _fields_ = [("log_likelihood", C.c_double), ("n_valid", C.c_int32), ("n_agree", C.c_int32), ("n_miss", C.c_int32),
                ("reserved", C.c_int32)]


class SearchConfig(C.Structure):
    """mcl_search_config_t: the lattice of the global search (Engine.global_search)."""
    _c_name_ = "mcl_search_config_t"
    _fields_ = [("stride_cells", C.c_int32), ("n_headings", C.c_int32), ("beam_stride", C.c_int32), ("nms", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class SearchStreamConfig(C.Structure):
    """mcl_search_stream_config_t: the memory budget and the slab of a streamed search (Engine.global_search_streamed)."""
    _c_name_ = "mcl_search_stream_config_t"
    _fields_ = [("budget_bytes", C.c_uint64), ("slab_headings", C.c_int32), ("reserved", C.c_int32 * 5)]


class SearchPruneConfig(C.Structure):
    """mcl_search_prune_config_t: the block side and the first round of a pruned search (Engine.global_search_pruned)."""
    _c_name_ = "mcl_search_prune_config_t"
    _fields_ = [("block", C.c_int32), ("first_pairs", C.c_int32), ("reserved", C.c_int32 * 6)]


class RefineConfig(C.Structure):
    """mcl_refine_config_t: the window of the pose refinement (Engine.refine_poses)."""
    _c_name_ = "mcl_refine_config_t"
    _fields_ = [("half_xy", C.c_int32), ("half_theta", C.c_int32), ("step_xy_cells", C.c_double), ("step_theta_rad", C.c_double),
                ("beam_stride", C.c_int32), ("reserved", C.c_int32 * 3)]


class MapPatchStats(C.Structure):
    """mcl_map_patch_stats_t: what a map patch changed (Engine.update_map_region)."""
    _c_name_ = "mcl_map_patch_stats_t"
    _fields_ = [("changed_cells", C.c_int32), ("changed_stop_cells", C.c_int32), ("window", C.c_int32 * 4), ("lf_window", C.c_int32 * 4),
                ("free_cells", C.c_int64), ("ms", C.c_double)]


# ---- numpy views of arrays of the header's result records -------------------------------------------------------------------------
CLUSTER_DTYPE = np.dtype([("weight_q", np.uint64), ("weight", np.float64), ("n_particles", np.int64), ("n_bins", np.int64),
                          ("first_bin", np.int64), ("mean", np.float64, (3,)), ("cov", np.float64, (3, 3))])           # Engine.pose_clusters
POSE_SCORE_DTYPE = np.dtype([("log_likelihood", np.float64), ("n_valid", np.int32), ("n_agree", np.int32), ("n_miss", np.int32),
                             ("reserved", np.int32)])                                                                   # Engine.score_poses
SEARCH_HIT_DTYPE = np.dtype([("pose", np.float64, (3,)), ("log_likelihood", np.float64), ("index", np.int64)])          # Engine.global_search
REFINE_DTYPE = np.dtype([("best", np.float64, (3,)), ("best_log_likelihood", np.float64), ("seed_log_likelihood", np.float64),
                         ("best_index", np.int64), ("mean", np.float64, (3,)), ("cov", np.float64, (3, 3)),
                         ("weight_sum", np.float64)])                                                                   # Engine.refine_poses
RECORD_DTYPES = {"mcl_cluster_t": CLUSTER_DTYPE, "mcl_pose_score_t": POSE_SCORE_DTYPE, "mcl_search_hit_t": SEARCH_HIT_DTYPE,
                 "mcl_refine_result_t": REFINE_DTYPE}


# ---- errors -------------------------------------------------------------------------------------------------------------------------
class EngineError(RuntimeError):
    """A call through the C ABI returned a negative mcl_status; `.status` holds it."""

    def __init__(self, msg, status=None):
        super().__init__(msg)
        self.status = status


class ShardedUpdateError(EngineError):
    """An update of a SHARDED set is void on every rank: this rank failed locally (`.local` is True, the message says how) or
    another rank did (MCL_ERR_PEER), or a collective ran out of time and the communicator was aborted (MCL_ERR_TIMEOUT).  Every
    rank raises from the same update; the particle set must be set or initialised again on every rank before the next one."""

    def __init__(self, msg, status=None, local=False):
        super().__init__(msg, status)
        self.local = local


# ---- signatures: name -> (restype, argtypes), every function of the header in the header's order -----------------------------------
# A scalar is the ctypes class of its C type.  A pointer is vp (it takes None, byref(...), ctypes arrays, integers and what
# host._p returns) unless it is one of the typed pointers below, which take byref / an instance of exactly that type.
i32, u32, i64, u64, sz, f32, f64, cint, vp, P = (C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_size_t, C.c_float, C.c_double,
                                                 C.c_int, C.c_void_p, C.POINTER)
SIGNATURES = {
    "mcl_default_config": (None, [P(Config)]),
    "mcl_abi_version": (cint, []),
    # ---- lifetime
    "mcl_create": (cint, [P(Config), P(vp)]),
    "mcl_destroy": (None, [vp]),
    "mcl_last_error": (C.c_char_p, [vp]),
    # ---- map + sensor table
    "mcl_set_map": (cint, [vp, vp, u32, u32, f32, f64, f64]),
    "mcl_get_max_range_px": (cint, [vp, vp]),
    "mcl_get_sensor_table": (cint, [vp, vp, sz]),
    # ---- beam geometry
    "mcl_set_beam_angles": (cint, [vp, vp, i32]),
    # ---- particle state
    "mcl_set_particles": (cint, [vp, vp, vp, i64]),
    "mcl_set_particles_shard": (cint, [vp, vp, vp, i64, f64]),
    "mcl_init_particles_pose": (cint, [vp, vp, i64, i64, i64]),
    "mcl_init_global": (cint, [vp, i64, i64, i64]),
    "mcl_get_particles": (cint, [vp, vp, i64]),
    "mcl_get_weights": (cint, [vp, vp, i64]),
    "mcl_sample_particles": (cint, [vp, i32, vp, vp]),
    "mcl_particle_mean": (cint, [vp, vp]),
    # ---- the update
    "mcl_update": (cint, [vp, vp, vp, i32, vp, vp]),
    "mcl_update_scan": (cint, [vp, vp, vp, i32, i32]),
    "mcl_sensor_update": (cint, [vp, vp, i32]),
    # ---- expected_pose()
    "mcl_expected_pose": (cint, [vp, vp]),
    # ---- TimingStats mirror
    "mcl_get_stage_timings": (cint, [vp, vp]),
    # ---- parity / diagnostics
    "mcl_get_resample_indices": (cint, [vp, vp, i64]),
    "mcl_get_ray_steps": (cint, [vp, vp, sz]),
    "mcl_get_ray_steps16": (cint, [vp, vp, sz]),
    "mcl_get_log_weights": (cint, [vp, vp, i64]),
    "mcl_get_counters": (cint, [vp, vp]),
    "mcl_get_compact_list": (cint, [vp, vp, vp]),
    "mcl_set_debug_count_probes": (cint, [vp, i32]),
    "mcl_set_debug_force_exact": (cint, [vp, i32]),
    "mcl_get_ray_kernel_ms": (cint, [vp, vp]),
    "mcl_get_ray_kernel_id": (cint, [vp, vp]),
    "mcl_get_ray_kernel_variant": (cint, [vp, vp]),
    "mcl_get_planned_ray_kernel": (cint, [vp, i64, vp, vp]),
    "mcl_get_effective_sample_size": (cint, [vp, vp, vp]),
    # ---- KLD-adaptive particle count
    "mcl_default_kld_config": (None, [P(KldConfig)]),
    "mcl_set_kld": (cint, [vp, P(KldConfig)]),
    "mcl_get_particle_count": (cint, [vp, P(i64)]),
    "mcl_get_kld_state": (cint, [vp, P(i64), P(i64)]),
    "mcl_host_kld_bins": (cint, [vp, vp, vp, i64, u32, u32, f32, f64, f64, P(KldConfig), P(i64)]),
    "mcl_host_kld_target": (cint, [P(KldConfig), i64, i64, P(i64)]),
    # ---- pose hypotheses
    "mcl_default_cluster_config": (None, [P(ClusterConfig)]),
    "mcl_pose_clusters": (cint, [vp, P(ClusterConfig), i32, vp, P(i64), P(u64)]),
    "mcl_get_cluster_labels": (cint, [vp, vp, i64]),
    # ---- pose query
    "mcl_query_scans": (cint, [vp, vp, i32, vp, vp]),
    "mcl_score_poses": (cint, [vp, vp, i32, vp, i32, i32, vp]),
    "mcl_get_query_counters": (cint, [vp, vp]),
    # ---- global search
    "mcl_default_search_config": (None, [P(SearchConfig)]),
    "mcl_global_search": (cint, [vp, P(SearchConfig), vp, i32, i32, vp, P(i64), vp]),
    "mcl_get_search_scores": (cint, [vp, vp, sz]),
    "mcl_get_search_bytes": (cint, [vp, P(u64)]),
    "mcl_host_search_lattice": (cint, [P(SearchConfig), vp, u32, u32, f32, f64, f64, vp, vp, sz, P(i64)]),
    "mcl_host_search_headings": (cint, [P(SearchConfig), vp, sz]),
    # ---- global search over a scan sequence joined by odometry
    "mcl_global_search_sequence": (cint, [vp, P(SearchConfig), vp, vp, i32, i32, i32, vp, P(i64), vp]),
    "mcl_host_search_sequence_offsets": (cint, [P(SearchConfig), vp, i32, vp, sz]),
    "mcl_host_relative_poses": (cint, [vp, i32, i32, vp]),
    # ---- global search in heading slabs
    "mcl_default_search_stream_config": (None, [P(SearchStreamConfig)]),
    "mcl_global_search_streamed": (cint, [vp, P(SearchConfig), P(SearchStreamConfig), vp, vp, i32, i32, i32, vp, P(i64), vp]),
    "mcl_host_search_slabs": (cint, [P(SearchConfig), P(SearchStreamConfig), i64, i32, P(i32), P(i32), P(u64)]),
    # ---- global search under the beam model
    "mcl_global_search_beam": (cint, [vp, P(SearchConfig), vp, i32, u64, i32, vp, P(i64), vp]),
    "mcl_host_search_beam_grid": (cint, [vp, i32, i32, P(i32), P(i32), P(f64), P(f64), vp, sz]),
    "mcl_get_search_beam_table": (cint, [vp, vp, sz, P(i64), P(i64)]),
    # ---- global search with exact pruning
    "mcl_default_search_prune_config": (None, [P(SearchPruneConfig)]),
    "mcl_global_search_pruned": (cint, [vp, P(SearchConfig), P(SearchPruneConfig), vp, i32, i32, vp, P(i64), vp]),
    "mcl_get_search_bounds": (cint, [vp, vp, sz]),
    "mcl_host_search_blocks": (cint, [P(SearchConfig), P(SearchPruneConfig), vp, u32, u32, P(i32), P(i32), P(i32), P(i32), vp, sz]),
    "mcl_host_lf_pool": (cint, [vp, u32, u32, i32, i32, vp, sz]),
    "mcl_host_search_bound_table": (cint, [vp, i32, vp]),
    "mcl_host_search_prune_next": (cint, [P(SearchPruneConfig), i64, i64, i64, P(i64)]),
    # ---- global search over a scan sequence with exact pruning
    "mcl_global_search_sequence_pruned": (cint, [vp, P(SearchConfig), P(SearchPruneConfig), vp, vp, i32, i32, i32, vp, P(i64), vp]),
    # ---- pose refinement
    "mcl_default_refine_config": (None, [P(RefineConfig)]),
    "mcl_refine_poses": (cint, [vp, P(RefineConfig), vp, i32, vp, i32, vp, vp]),
    "mcl_get_refine_scores": (cint, [vp, vp, sz]),
    "mcl_get_refine_bytes": (cint, [vp, P(u64)]),
    "mcl_host_refine_window": (cint, [P(RefineConfig), vp, f32, vp, sz]),
    "mcl_host_refine_reduce": (cint, [P(RefineConfig), vp, f32, vp, sz, vp]),
    # ---- pose refinement under the beam model
    "mcl_refine_poses_beam": (cint, [vp, P(RefineConfig), vp, i32, vp, i32, vp, vp]),
    # ---- pose refinement over a scan sequence joined by odometry
    "mcl_refine_poses_sequence": (cint, [vp, P(RefineConfig), vp, i32, vp, vp, i32, i32, vp, vp]),
    "mcl_host_refine_sequence_offsets": (cint, [P(RefineConfig), vp, i32, vp, i32, vp, sz]),
    # ---- recovery by random-particle injection
    "mcl_default_recovery_config": (None, [P(RecoveryConfig)]),
    "mcl_set_recovery": (cint, [vp, P(RecoveryConfig)]),
    "mcl_get_recovery_state": (cint, [vp, vp, P(i64)]),
    "mcl_set_recovery_state": (cint, [vp, vp]),
    "mcl_host_recovery_step": (cint, [P(RecoveryConfig), vp, i32, f64, f64, f64, i32, vp, P(f64)]),
    "mcl_set_recovery_proposal": (cint, [vp, i32, vp, vp, vp]),
    "mcl_get_recovery_proposal": (cint, [vp, P(i32), vp, vp]),
    "mcl_host_recovery_proposal": (cint, [i32, vp, vp, vp, vp, vp]),
    # ---- likelihood-field
    "mcl_default_likelihood_field_config": (None, [P(LikelihoodFieldConfig)]),
    "mcl_set_likelihood_field": (cint, [vp, P(LikelihoodFieldConfig)]),
    "mcl_get_likelihood_field": (cint, [vp, vp, sz]),
    "mcl_get_likelihood_table": (cint, [vp, vp, sz, P(i32)]),
    "mcl_host_likelihood_field": (cint, [vp, u32, u32, f32, P(LikelihoodFieldConfig), vp, sz]),
    "mcl_host_likelihood_table": (cint, [P(Config), P(LikelihoodFieldConfig), f32, vp, sz, P(i32)]),
    # ---- beam skipping for the likelihood field
    "mcl_default_beam_skip_config": (None, [P(BeamSkipConfig)]),
    "mcl_set_beam_skip": (cint, [vp, P(BeamSkipConfig)]),
    "mcl_get_beam_skip_state": (cint, [vp, vp, vp, sz, P(BeamSkipState)]),
    "mcl_host_beam_skip_thresholds": (cint, [P(BeamSkipConfig), f32, i64, i32, P(i32), P(i64), P(i32)]),
    "mcl_host_beam_skip_plan": (cint, [P(BeamSkipConfig), vp, i32, i64, vp, P(i32), P(i32)]),
    # ---- sensor mount
    "mcl_set_sensor_mount": (cint, [vp, vp]),
    "mcl_get_sensor_mount": (cint, [vp, vp]),
    "mcl_mount_poses": (cint, [vp, vp, i64, vp]),
    "mcl_get_sensor_poses": (cint, [vp, vp, i64]),
    "mcl_sensor_update_fuse": (cint, [vp, vp, i32]),
    "mcl_host_sensor_mount": (cint, [vp, vp, i64, vp]),
    "mcl_host_sensor_unmount": (cint, [vp, vp, i64, vp]),
    "mcl_host_sensor_mount_cov": (cint, [vp, vp, vp, cint, vp]),
    # ---- scan de-skew
    "mcl_set_beam_offsets": (cint, [vp, vp, i32]),
    "mcl_get_beam_offsets": (cint, [vp, vp, vp, i32, vp]),
    "mcl_beam_origins": (cint, [vp, vp, i64, vp]),
    "mcl_host_scan_motion_offsets": (cint, [vp, vp, vp, f64, i32, vp]),
    "mcl_host_beam_offset_table": (cint, [vp, vp, i32, vp, vp]),
    "mcl_host_beam_offset_pairs": (cint, [vp, vp, vp, i32, f64, vp]),
    # ---- odometry motion models and covariance-based pose initialisation
    "mcl_default_motion_config": (None, [P(MotionConfig)]),
    "mcl_set_motion_model": (cint, [vp, P(MotionConfig)]),
    "mcl_get_motion_model": (cint, [vp, P(MotionConfig)]),
    "mcl_host_motion_scalars": (cint, [P(MotionConfig), vp, vp]),
    "mcl_host_motion_sample": (cint, [P(MotionConfig), vp, vp, vp, i64, vp]),
    "mcl_init_particles_gaussian": (cint, [vp, vp, vp, i64, i64, i64]),
    "mcl_host_gaussian_factor": (cint, [vp, vp]),
    "mcl_init_particles_mixture": (cint, [vp, i32, vp, vp, vp, i64, i64, i64]),
    # ---- host-side precomputation
    "mcl_host_sensor_table": (cint, [vp, i32, vp, sz]),
    "mcl_host_skip_field": (cint, [vp, u32, u32, vp, sz]),
    "mcl_host_skip_field_dir": (cint, [vp, u32, u32, i32, vp, sz]),
    "mcl_host_skip_field_wedge": (cint, [vp, u32, u32, i32, vp, sz]),
    "mcl_host_skip_field_wedge_tight": (cint, [vp, u32, u32, i32, vp, sz]),
    "mcl_host_wedge_tight_table": (cint, [i32, vp, vp, sz]),
    "mcl_host_sweep_global_layout": (cint, [u32, u32, i32, P(i64)]),
    # ---- the tables under the ray stage
    "mcl_get_wedge_fields": (cint, [vp, vp, sz, P(i32)]),
    "mcl_get_ring_fields": (cint, [vp, vp, sz]),
    "mcl_get_sweep_table": (cint, [vp, vp, sz, P(i32)]),
    # ---- the order the ray stage worked in
    "mcl_host_sort_key": (cint, [vp, vp, i32, u32, u32, vp, vp, vp, i64, i64, i32, vp]),
    "mcl_get_sort_order": (cint, [vp, vp, vp, sz, vp, vp, sz, P(i64), P(i32)]),
    "mcl_get_sort_record_form": (cint, [vp, vp]),
    # ---- the guide of the compact parent list
    "mcl_host_compact_guide": (cint, [vp, i64, u64, i32, vp, sz, P(i32), P(u32), P(i64)]),
    "mcl_host_compact_search": (cint, [vp, i64, vp, sz, i32, u32, vp, i64, vp]),
    "mcl_get_compact_guide": (cint, [vp, vp, sz, vp, sz, vp]),
    # ---- multi-GPU staging
    "mcl_device_ptr": (cint, [vp, i32, vp]),
    "mcl_export_state": (cint, [vp, vp, vp, vp, vp]),
    "mcl_get_scalars": (cint, [vp, vp]),
    "mcl_get_host_scalars": (cint, [vp, vp]),
    "mcl_stage_propagate": (cint, [vp, vp, vp, vp, vp, i64, u64, i64, i64, vp, vp, i32]),
    "mcl_stage_resample": (cint, [vp, vp, vp, vp, vp, i64, u64, i64, i64, vp]),
    "mcl_export_records": (cint, [vp, vp]),
    "mcl_stage_resample_records": (cint, [vp, vp, vp, i64, u64, i64, i64, vp]),
    "mcl_stage_distinct_parents": (cint, [vp, vp, i64, i64, vp, vp, vp]),
    "mcl_export_records_at": (cint, [vp, vp, i64, vp]),
    "mcl_stage_resample_indices": (cint, [vp, vp, i64, u64, i64, i64, vp]),
    "mcl_stage_motion_records": (cint, [vp, vp, i64, vp, i64, i64, vp]),
    "mcl_compact_chunk_bytes": (cint, [i64, vp]),
    "mcl_export_compact": (cint, [vp, vp, i64]),
    "mcl_stage_resample_compact": (cint, [vp, vp, i32, i64, vp, vp, i64, i32, i64, i64, vp]),
    "mcl_stage_rays": (cint, [vp, vp, i32]),
    "mcl_set_reserved_cus": (cint, [vp, i32]),
    "mcl_stage_weights": (cint, [vp, f64]),
    "mcl_stage_finish": (cint, [vp, vp]),
    # ---- the same stages ORDERED ON THE DEVICE
    "mcl_stage_keep": (cint, [vp, i64, i64, vp]),
    "mcl_stream_wait_external": (cint, [vp, vp]),
    "mcl_external_wait_stream": (cint, [vp, vp]),
    "mcl_export_compact_async": (cint, [vp, vp, i64]),
    "mcl_stage_resample_compact_async": (cint, [vp, vp, i32, i64, vp, vp, i64, i32, i64, i64, vp]),
    "mcl_stage_rays_async": (cint, [vp, vp, i32, vp]),
    "mcl_stage_weights_async": (cint, [vp, vp, vp, i32, i32]),
    "mcl_stage_complete": (cint, [vp, vp, vp]),
    # ---- one process per GPU
    "mcl_comm_available": (cint, [vp]),
    "mcl_comm_unique_id": (cint, [vp]),
    "mcl_comm_create": (cint, [vp, vp, i32, i32]),
    "mcl_comm_selftest": (cint, [vp]),
    "mcl_comm_destroy": (cint, [vp]),
    "mcl_comm_set_lists": (cint, [vp, vp, vp]),
    "mcl_comm_update": (cint, [vp, vp, vp, i32, vp]),
    "mcl_comm_get_vector": (cint, [vp, vp, i32]),
    "mcl_comm_stats": (cint, [vp, vp, vp, vp]),
    "mcl_comm_last_exchange": (cint, [vp, vp, vp, vp]),
    "mcl_scan_weights": (cint, [vp, vp, vp, i64, u64]),
    # ---- several GPUs behind one handle
    "mcl_group_create": (cint, [P(Config), vp, i32, P(vp)]),
    "mcl_group_destroy": (None, [vp]),
    "mcl_group_last_error": (C.c_char_p, [vp]),
    "mcl_group_size": (i32, [vp]),
    "mcl_group_engine": (cint, [vp, i32, vp]),
    "mcl_group_set_map": (cint, [vp, vp, u32, u32, f32, f64, f64]),
    "mcl_group_set_beam_angles": (cint, [vp, vp, i32]),
    "mcl_group_set_particles": (cint, [vp, vp, vp, i64]),
    "mcl_group_init_particles_pose": (cint, [vp, vp, i64]),
    "mcl_group_init_global": (cint, [vp, i64]),
    "mcl_group_init_particles_gaussian": (cint, [vp, vp, vp, i64]),
    "mcl_group_set_motion_model": (cint, [vp, P(MotionConfig)]),
    "mcl_group_set_sensor_mount": (cint, [vp, vp]),
    "mcl_group_update": (cint, [vp, vp, vp, i32]),
    "mcl_group_expected_pose": (cint, [vp, vp]),
    "mcl_group_get_particles": (cint, [vp, vp, i64]),
    "mcl_group_get_weights": (cint, [vp, vp, i64]),
    "mcl_group_get_resample_indices": (cint, [vp, vp, i64]),
    "mcl_group_get_stage_timings": (cint, [vp, vp]),
    "mcl_group_exchange_bytes": (cint, [vp, vp]),
    "mcl_group_exchanged_lists": (i32, [vp]),
    # ---- map patches
    "mcl_update_map_region": (cint, [vp, vp, u32, u32, u32, u32, u32, P(MapPatchStats)]),
    "mcl_host_map_patch_plan": (cint, [u32, u32, P(i32), i32, P(i32), P(i32)]),
    "mcl_get_map_table": (cint, [vp, i32, vp, sz, P(sz)]),
    "mcl_group_update_map_region": (cint, [vp, vp, u32, u32, u32, u32, u32]),
}
del i32, u32, i64, u64, sz, f32, f64, cint, vp, P
EXPORTS = list(SIGNATURES)

_libs = {}


def load_library(legacy=False):
    """Loads libmcl_hip_engine.so (built by __graft_entry__.build()); raises if absent.  legacy=True: the same sources built with
    -DMCL_LEGACY_RAY_KERNELS (libmcl_hip_engine_legacy.so), which also holds k_rays_quad / k_rays_cell -- the predecessors of the
    windowed ray kernel, kept as two more implementations to test it against; an Engine asks for it only when its configuration
    names one of them (ray_kernel = RAYS_QUAD / RAYS_CELL)."""
    path = LEGACY_LIB_PATH if legacy else LIB_PATH
    _lib = _libs.get(path)
    if _lib is None:
        # PyTorch-ROCm wheels bundle their own copies of the ROCm runtime under the same sonames as /opt/rocm's
        # (libamdhip64.so.7, libhsa-runtime64.so.1).  A process that uses both must load torch's first: if this library pulls
        # in /opt/rocm's copies before `import torch`, torch ends up on a runtime it was not built with and reports
        # "No HIP GPUs are available".  So when torch is installed and not imported yet, import it here (dist.py and
        # bench.py need it anyway); without torch the library simply uses /opt/rocm's runtime.
        import importlib.util
        import sys
        if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        if not os.path.exists(path):
            raise EngineError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        lib = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            if hasattr(lib, name):          # (a build from before an export, loaded through MCL_LIB for an A/B run, lacks it)
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        _libs[path] = _lib = lib
    return _lib
