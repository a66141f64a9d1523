"""ctypes binding of the C ABI in include/mcl_hip_engine.h (libmcl_hip_engine.so).

This is plumbing only: every numeric step runs in the HIP library.  There is no fallback — if the
shared library is missing or no gfx950 device is visible the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MCL_LIB: another build of the same library, for A/B runs on one box -- a development aid, never set by the product or the tests)
LIB_PATH = os.environ.get("MCL_LIB") or os.path.join(_HERE, "libmcl_hip_engine.so")

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

EXPORTS = [
    "mcl_abi_version", "mcl_default_config", "mcl_create", "mcl_destroy", "mcl_last_error", "mcl_set_map",
    "mcl_get_max_range_px", "mcl_get_sensor_table", "mcl_set_beam_angles", "mcl_set_particles",
    "mcl_get_particles", "mcl_get_weights", "mcl_sample_particles", "mcl_particle_mean", "mcl_update",
    "mcl_sensor_update", "mcl_expected_pose", "mcl_get_stage_timings", "mcl_get_resample_indices",
    "mcl_get_ray_steps", "mcl_get_log_weights", "mcl_get_counters", "mcl_get_ray_kernel_ms", "mcl_device_ptr",
    "mcl_stage_propagate", "mcl_stage_weights", "mcl_stage_finish", "mcl_scan_weights", "mcl_export_state",
    "mcl_get_scalars", "mcl_host_sensor_table", "mcl_host_skip_field", "mcl_init_particles_pose", "mcl_init_global",
    "mcl_update_scan", "mcl_get_ray_kernel_id", "mcl_host_skip_field_dir", "mcl_host_skip_field_wedge", "mcl_export_records", "mcl_get_effective_sample_size", "mcl_get_host_scalars", "mcl_stage_resample_records", "mcl_stage_resample", "mcl_stage_rays",
    "mcl_set_reserved_cus", "mcl_stage_resample_indices", "mcl_stage_motion_records", "mcl_stage_distinct_parents", "mcl_export_records_at",
    "mcl_group_create", "mcl_group_destroy", "mcl_group_last_error", "mcl_group_size", "mcl_group_engine", "mcl_group_set_map",
    "mcl_group_set_beam_angles", "mcl_group_set_particles", "mcl_group_init_particles_pose", "mcl_group_init_global",
    "mcl_group_update", "mcl_group_expected_pose", "mcl_group_get_particles", "mcl_group_get_weights",
    "mcl_group_get_resample_indices", "mcl_group_get_stage_timings", "mcl_group_exchange_bytes",
    "mcl_set_debug_count_probes", "mcl_set_debug_force_exact", "mcl_set_particles_shard", "mcl_get_compact_list", "mcl_compact_chunk_bytes", "mcl_export_compact",
    "mcl_stage_resample_compact", "mcl_group_exchanged_lists", "mcl_get_ray_steps16", "mcl_get_planned_ray_kernel",
    "mcl_stream_wait_external", "mcl_external_wait_stream", "mcl_export_compact_async", "mcl_stage_resample_compact_async",
    "mcl_stage_rays_async", "mcl_stage_weights_async", "mcl_stage_complete", "mcl_stage_keep",
    "mcl_comm_available", "mcl_comm_unique_id", "mcl_comm_create", "mcl_comm_destroy", "mcl_comm_update", "mcl_comm_stats", "mcl_comm_set_lists", "mcl_comm_get_vector", "mcl_comm_last_exchange", "mcl_comm_selftest",
    "mcl_host_sweep_global_layout", "mcl_get_ray_kernel_variant", "mcl_host_skip_field_wedge_tight", "mcl_host_wedge_tight_table",
    "mcl_get_wedge_fields", "mcl_get_ring_fields", "mcl_get_sweep_table", "mcl_host_sort_key", "mcl_get_sort_order", "mcl_get_sort_record_form",
    "mcl_default_kld_config", "mcl_set_kld", "mcl_get_particle_count", "mcl_get_kld_state", "mcl_host_kld_bins", "mcl_host_kld_target",
    "mcl_default_cluster_config", "mcl_pose_clusters", "mcl_get_cluster_labels",
    "mcl_query_scans", "mcl_score_poses", "mcl_get_query_counters",
    "mcl_default_search_config", "mcl_global_search", "mcl_get_search_scores", "mcl_get_search_bytes", "mcl_host_search_lattice",
    "mcl_host_search_headings", "mcl_init_particles_mixture",
    "mcl_global_search_sequence", "mcl_host_search_sequence_offsets", "mcl_host_relative_poses",
    "mcl_default_search_stream_config", "mcl_global_search_streamed", "mcl_host_search_slabs",
    "mcl_global_search_beam", "mcl_host_search_beam_grid", "mcl_get_search_beam_table",
    "mcl_default_search_prune_config", "mcl_global_search_pruned", "mcl_get_search_bounds", "mcl_host_search_blocks", "mcl_host_lf_pool",
    "mcl_host_search_bound_table", "mcl_host_search_prune_next", "mcl_global_search_sequence_pruned",
    "mcl_default_refine_config", "mcl_refine_poses", "mcl_refine_poses_beam", "mcl_get_refine_scores", "mcl_get_refine_bytes", "mcl_host_refine_window",
    "mcl_host_refine_reduce", "mcl_refine_poses_sequence", "mcl_host_refine_sequence_offsets",
    "mcl_default_recovery_config", "mcl_set_recovery", "mcl_get_recovery_state", "mcl_set_recovery_state", "mcl_host_recovery_step",
    "mcl_set_recovery_proposal", "mcl_get_recovery_proposal", "mcl_host_recovery_proposal",
    "mcl_default_likelihood_field_config", "mcl_set_likelihood_field", "mcl_get_likelihood_field", "mcl_get_likelihood_table",
    "mcl_host_likelihood_field", "mcl_host_likelihood_table",
    "mcl_default_beam_skip_config", "mcl_set_beam_skip", "mcl_get_beam_skip_state", "mcl_host_beam_skip_thresholds",
    "mcl_host_beam_skip_plan",
    "mcl_default_motion_config", "mcl_set_motion_model", "mcl_get_motion_model", "mcl_host_motion_scalars", "mcl_host_motion_sample",
    "mcl_init_particles_gaussian", "mcl_host_gaussian_factor", "mcl_group_set_motion_model", "mcl_group_init_particles_gaussian",
    "mcl_set_sensor_mount", "mcl_get_sensor_mount", "mcl_mount_poses", "mcl_get_sensor_poses", "mcl_sensor_update_fuse",
    "mcl_group_set_sensor_mount", "mcl_host_sensor_mount", "mcl_host_sensor_unmount", "mcl_host_sensor_mount_cov",
    "mcl_set_beam_offsets", "mcl_get_beam_offsets", "mcl_beam_origins", "mcl_host_scan_motion_offsets", "mcl_host_beam_offset_table",
    "mcl_host_beam_offset_pairs",
    "mcl_update_map_region", "mcl_host_map_patch_plan", "mcl_get_map_table", "mcl_group_update_map_region",
    "mcl_host_compact_guide", "mcl_host_compact_search", "mcl_get_compact_guide",
]
MOTION_REFERENCE, MOTION_DIFF, MOTION_OMNI = 0, 1, 2
MOTION_MODELS = {"reference": MOTION_REFERENCE, "diff": MOTION_DIFF, "omni": MOTION_OMNI}


class Config(C.Structure):
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
    _fields_ = [
        ("min_particles", C.c_int64), ("max_particles", C.c_int64), ("err", C.c_double), ("z", C.c_double),
        ("bin_x_m", C.c_double), ("bin_y_m", C.c_double), ("n_theta_bins", C.c_int32), ("round_to", C.c_int32),
        ("shrink_permille", C.c_int32), ("reserved", C.c_int32),
    ]


class RecoveryConfig(C.Structure):
    """mcl_recovery_config_t: recovery by random-particle injection (Engine.set_recovery)."""
    _fields_ = [("alpha_slow", C.c_double), ("alpha_fast", C.c_double), ("per_beam", C.c_int32), ("reserved", C.c_int32)]


class LikelihoodFieldConfig(C.Structure):
    """mcl_likelihood_field_config_t: the likelihood-field sensor model (Engine.set_likelihood_field)."""
    _fields_ = [("z_hit", C.c_double), ("z_rand", C.c_double), ("sigma_hit_m", C.c_double), ("max_occ_dist_m", C.c_double),
                ("reserved", C.c_int32 * 2)]


class BeamSkipConfig(C.Structure):
    """mcl_beam_skip_config_t: beam skipping for the likelihood field (Engine.set_beam_skip)."""
    _fields_ = [("distance_m", C.c_double), ("threshold", C.c_double), ("error_threshold", C.c_double), ("reserved", C.c_int32 * 2)]


class BeamSkipState(C.Structure):
    """mcl_beam_skip_state_t: what the last update with beam skipping decided (Engine.beam_skip_state, rule BS6)."""
    _fields_ = [("n_particles", C.c_int64), ("min_count", C.c_int64), ("n_used", C.c_int32), ("n_kept", C.c_int32),
                ("n_skipped", C.c_int32), ("min_skipped", C.c_int32), ("integrate_all", C.c_int32), ("ka", C.c_int32)]


assert C.sizeof(BeamSkipConfig) == 32 and C.sizeof(BeamSkipState) == 40


class MotionConfig(C.Structure):
    """mcl_motion_config_t: the odometry motion models (Engine.set_motion_model)."""
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("alpha1", C.c_double), ("alpha2", C.c_double),
                ("alpha3", C.c_double), ("alpha4", C.c_double), ("alpha5", C.c_double), ("floor_trans_m", C.c_double),
                ("floor_rot_rad", C.c_double)]


class ClusterConfig(C.Structure):
    """mcl_cluster_config_t: the bins of the pose clustering (Engine.pose_clusters)."""
    _fields_ = [("bin_x_m", C.c_double), ("bin_y_m", C.c_double), ("n_theta_bins", C.c_int32), ("reserved", C.c_int32)]


class Cluster(C.Structure):
    """mcl_cluster_t: one pose hypothesis."""
    _fields_ = [
        ("weight_q", C.c_uint64), ("weight", C.c_double), ("n_particles", C.c_int64), ("n_bins", C.c_int64),
        ("first_bin", C.c_int64), ("mean", C.c_double * 3), ("cov", C.c_double * 9),
    ]


# the numpy view of an array of mcl_cluster_t (Engine.pose_clusters)
CLUSTER_DTYPE = np.dtype([("weight_q", np.uint64), ("weight", np.float64), ("n_particles", np.int64), ("n_bins", np.int64),
                          ("first_bin", np.int64), ("mean", np.float64, (3,)), ("cov", np.float64, (3, 3))])
assert CLUSTER_DTYPE.itemsize == C.sizeof(Cluster)


class PoseScore(C.Structure):
    """mcl_pose_score_t: how well a scan supports one pose (Engine.score_poses)."""
    _fields_ = [("log_likelihood", C.c_double), ("n_valid", C.c_int32), ("n_agree", C.c_int32), ("n_miss", C.c_int32),
                ("reserved", C.c_int32)]


# the numpy view of an array of mcl_pose_score_t (Engine.score_poses)
POSE_SCORE_DTYPE = np.dtype([("log_likelihood", np.float64), ("n_valid", np.int32), ("n_agree", np.int32), ("n_miss", np.int32),
                             ("reserved", np.int32)])
assert POSE_SCORE_DTYPE.itemsize == C.sizeof(PoseScore) == 24
MAX_QUERY_POSES = 65536


class SearchConfig(C.Structure):
    """mcl_search_config_t: the lattice of the global search (Engine.global_search)."""
    _fields_ = [("stride_cells", C.c_int32), ("n_headings", C.c_int32), ("beam_stride", C.c_int32), ("nms", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class SearchStreamConfig(C.Structure):
    """mcl_search_stream_config_t: the memory budget and the slab of a streamed search (Engine.global_search_streamed)."""
    _fields_ = [("budget_bytes", C.c_uint64), ("slab_headings", C.c_int32), ("reserved", C.c_int32 * 5)]


class SearchPruneConfig(C.Structure):
    """mcl_search_prune_config_t: the block side and the first round of a pruned search (Engine.global_search_pruned)."""
    _fields_ = [("block", C.c_int32), ("first_pairs", C.c_int32), ("reserved", C.c_int32 * 6)]


# the numpy view of an array of mcl_search_hit_t (Engine.global_search)
SEARCH_HIT_DTYPE = np.dtype([("pose", np.float64, (3,)), ("log_likelihood", np.float64), ("index", np.int64)])
assert SEARCH_HIT_DTYPE.itemsize == 40
MAX_SEARCH_HITS = 65536
MAX_SEARCH_SCANS = 16            # MCL_SEARCH_MAX_SCANS


class RefineConfig(C.Structure):
    """mcl_refine_config_t: the window of the pose refinement (Engine.refine_poses)."""
    _fields_ = [("half_xy", C.c_int32), ("half_theta", C.c_int32), ("step_xy_cells", C.c_double), ("step_theta_rad", C.c_double),
                ("beam_stride", C.c_int32), ("reserved", C.c_int32 * 3)]


# the numpy view of an array of mcl_refine_result_t (Engine.refine_poses)
REFINE_DTYPE = np.dtype([("best", np.float64, (3,)), ("best_log_likelihood", np.float64), ("seed_log_likelihood", np.float64),
                         ("best_index", np.int64), ("mean", np.float64, (3,)), ("cov", np.float64, (3, 3)),
                         ("weight_sum", np.float64)])
assert REFINE_DTYPE.itemsize == 152 and C.sizeof(RefineConfig) == 40
MAX_REFINE_SEEDS, MAX_REFINE_WINDOW = 4096, 32768
MAX_REFINE_SEQ_ROWS = 1 << 21    # MCL_REFINE_SEQ_MAX_ROWS


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


_libs = {}
LEGACY_LIB_PATH = os.path.join(_HERE, "libmcl_hip_engine_legacy.so")


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
        lib.mcl_last_error.restype = C.c_char_p
        lib.mcl_last_error.argtypes = [C.c_void_p]
        lib.mcl_create.argtypes = [C.POINTER(Config), C.POINTER(C.c_void_p)]
        lib.mcl_destroy.argtypes = [C.c_void_p]
        lib.mcl_destroy.restype = None
        lib.mcl_default_config.argtypes = [C.POINTER(Config)]
        lib.mcl_default_config.restype = None
        lib.mcl_group_last_error.restype = C.c_char_p
        lib.mcl_group_last_error.argtypes = [C.c_void_p]
        lib.mcl_group_create.argtypes = [C.POINTER(Config), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        lib.mcl_group_destroy.argtypes = [C.c_void_p]
        lib.mcl_group_destroy.restype = None
        lib.mcl_default_kld_config.argtypes = [C.POINTER(KldConfig)]
        lib.mcl_default_kld_config.restype = None
        lib.mcl_set_kld.argtypes = [C.c_void_p, C.POINTER(KldConfig)]
        lib.mcl_get_particle_count.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        lib.mcl_get_kld_state.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.mcl_host_kld_bins.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_uint32, C.c_float,
                                          C.c_double, C.c_double, C.POINTER(KldConfig), C.POINTER(C.c_int64)]
        lib.mcl_host_kld_target.argtypes = [C.POINTER(KldConfig), C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        lib.mcl_default_cluster_config.argtypes = [C.POINTER(ClusterConfig)]
        lib.mcl_default_cluster_config.restype = None
        lib.mcl_pose_clusters.argtypes = [C.c_void_p, C.POINTER(ClusterConfig), C.c_int32, C.c_void_p, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_uint64)]
        lib.mcl_get_cluster_labels.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.mcl_query_scans.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        lib.mcl_score_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.mcl_get_query_counters.argtypes = [C.c_void_p, C.c_void_p]
        lib.mcl_default_search_config.argtypes = [C.POINTER(SearchConfig)]
        lib.mcl_default_search_config.restype = None
        lib.mcl_global_search.argtypes = [C.c_void_p, C.POINTER(SearchConfig), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                          C.POINTER(C.c_int64), C.c_void_p]
        lib.mcl_get_search_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mcl_get_search_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mcl_host_search_lattice.argtypes = [C.POINTER(SearchConfig), C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_double,
                                                C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64)]
        lib.mcl_host_search_headings.argtypes = [C.POINTER(SearchConfig), C.c_void_p, C.c_size_t]
        lib.mcl_global_search_sequence.argtypes = [C.c_void_p, C.POINTER(SearchConfig), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                                   C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        lib.mcl_host_search_sequence_offsets.argtypes = [C.POINTER(SearchConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t]
        lib.mcl_host_relative_poses.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        lib.mcl_default_search_stream_config.argtypes = [C.POINTER(SearchStreamConfig)]
        lib.mcl_default_search_stream_config.restype = None
        lib.mcl_global_search_streamed.argtypes = [C.c_void_p, C.POINTER(SearchConfig), C.POINTER(SearchStreamConfig), C.c_void_p, C.c_void_p,
                                                   C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        lib.mcl_host_search_slabs.argtypes = [C.POINTER(SearchConfig), C.POINTER(SearchStreamConfig), C.c_int64, C.c_int32,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
        lib.mcl_global_search_beam.argtypes = [C.c_void_p, C.POINTER(SearchConfig), C.c_void_p, C.c_int32, C.c_uint64, C.c_int32, C.c_void_p,
                                               C.POINTER(C.c_int64), C.c_void_p]
        lib.mcl_host_search_beam_grid.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_size_t]
        lib.mcl_get_search_beam_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        lib.mcl_default_search_prune_config.argtypes = [C.POINTER(SearchPruneConfig)]
        lib.mcl_default_search_prune_config.restype = None
        lib.mcl_global_search_pruned.argtypes = [C.c_void_p, C.POINTER(SearchConfig), C.POINTER(SearchPruneConfig), C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        lib.mcl_get_search_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mcl_global_search_sequence_pruned.argtypes = [C.c_void_p, C.POINTER(SearchConfig), C.POINTER(SearchPruneConfig), C.c_void_p,
                                                          C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int64),
                                                          C.c_void_p]
        lib.mcl_host_search_blocks.argtypes = [C.POINTER(SearchConfig), C.POINTER(SearchPruneConfig), C.c_void_p, C.c_uint32, C.c_uint32,
                                               C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                               C.c_void_p, C.c_size_t]
        lib.mcl_host_lf_pool.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
        lib.mcl_host_search_bound_table.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.mcl_host_search_prune_next.argtypes = [C.POINTER(SearchPruneConfig), C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]
        lib.mcl_default_refine_config.argtypes = [C.POINTER(RefineConfig)]
        lib.mcl_default_refine_config.restype = None
        lib.mcl_refine_poses.argtypes = [C.c_void_p, C.POINTER(RefineConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_void_p, C.c_void_p]
        lib.mcl_refine_poses_beam.argtypes = list(lib.mcl_refine_poses.argtypes)
        lib.mcl_get_refine_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mcl_get_refine_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mcl_host_refine_window.argtypes = [C.POINTER(RefineConfig), C.c_void_p, C.c_float, C.c_void_p, C.c_size_t]
        lib.mcl_host_refine_reduce.argtypes = [C.POINTER(RefineConfig), C.c_void_p, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mcl_refine_poses_sequence.argtypes = [C.c_void_p, C.POINTER(RefineConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        lib.mcl_host_refine_sequence_offsets.argtypes = [C.POINTER(RefineConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                         C.c_size_t]
        lib.mcl_init_particles_mixture.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                                   C.c_int64]
        lib.mcl_default_recovery_config.argtypes = [C.POINTER(RecoveryConfig)]
        lib.mcl_default_recovery_config.restype = None
        lib.mcl_set_recovery.argtypes = [C.c_void_p, C.POINTER(RecoveryConfig)]
        lib.mcl_get_recovery_state.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        lib.mcl_set_recovery_state.argtypes = [C.c_void_p, C.c_void_p]
        lib.mcl_host_recovery_step.argtypes = [C.POINTER(RecoveryConfig), C.c_void_p, C.c_int32, C.c_double, C.c_double,
                                               C.c_double, C.c_int32, C.c_void_p, C.POINTER(C.c_double)]
        lib.mcl_set_recovery_proposal.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mcl_get_recovery_proposal.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
        lib.mcl_host_recovery_proposal.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.mcl_default_likelihood_field_config.argtypes = [C.POINTER(LikelihoodFieldConfig)]
        lib.mcl_default_likelihood_field_config.restype = None
        lib.mcl_set_likelihood_field.argtypes = [C.c_void_p, C.POINTER(LikelihoodFieldConfig)]
        lib.mcl_get_likelihood_field.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mcl_get_wedge_fields.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        lib.mcl_update_map_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.POINTER(MapPatchStats)]
        lib.mcl_group_update_map_region.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
        lib.mcl_host_map_patch_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int32)]
        lib.mcl_get_map_table.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.mcl_get_ring_fields.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        lib.mcl_get_sweep_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        lib.mcl_host_sweep_global_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_int64)]
        lib.mcl_host_sort_key.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
        lib.mcl_get_sort_order.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        if hasattr(lib, "mcl_get_compact_guide"):          # (a build from before the guide, loaded through MCL_LIB for an A/B run, has none of the three)
            lib.mcl_host_compact_guide.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32),
                                                   C.POINTER(C.c_uint32), C.POINTER(C.c_int64)]
            lib.mcl_host_compact_search.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_int32, C.c_uint32, C.c_void_p, C.c_int64,
                                                    C.c_void_p]
            lib.mcl_get_compact_guide.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        lib.mcl_get_likelihood_table.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)]
        lib.mcl_host_likelihood_field.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(LikelihoodFieldConfig),
                                                  C.c_void_p, C.c_size_t]
        lib.mcl_host_likelihood_table.argtypes = [C.POINTER(Config), C.POINTER(LikelihoodFieldConfig), C.c_float, C.c_void_p,
                                                  C.c_size_t, C.POINTER(C.c_int32)]
        lib.mcl_default_beam_skip_config.argtypes = [C.POINTER(BeamSkipConfig)]
        lib.mcl_default_beam_skip_config.restype = None
        lib.mcl_set_beam_skip.argtypes = [C.c_void_p, C.POINTER(BeamSkipConfig)]
        lib.mcl_get_beam_skip_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(BeamSkipState)]
        lib.mcl_host_beam_skip_thresholds.argtypes = [C.POINTER(BeamSkipConfig), C.c_float, C.c_int64, C.c_int32, C.POINTER(C.c_int32),
                                                      C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.mcl_host_beam_skip_plan.argtypes = [C.POINTER(BeamSkipConfig), C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.mcl_default_motion_config.argtypes = [C.POINTER(MotionConfig)]
        lib.mcl_default_motion_config.restype = None
        lib.mcl_set_motion_model.argtypes = [C.c_void_p, C.POINTER(MotionConfig)]
        lib.mcl_get_motion_model.argtypes = [C.c_void_p, C.POINTER(MotionConfig)]
        lib.mcl_host_motion_scalars.argtypes = [C.POINTER(MotionConfig), C.c_void_p, C.c_void_p]
        lib.mcl_host_motion_sample.argtypes = [C.POINTER(MotionConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.mcl_init_particles_gaussian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
        lib.mcl_host_gaussian_factor.argtypes = [C.c_void_p, C.c_void_p]
        lib.mcl_group_set_motion_model.argtypes = [C.c_void_p, C.POINTER(MotionConfig)]
        lib.mcl_group_init_particles_gaussian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        lib.mcl_set_sensor_mount.argtypes = [C.c_void_p, C.c_void_p]
        lib.mcl_get_sensor_mount.argtypes = [C.c_void_p, C.c_void_p]
        lib.mcl_mount_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.mcl_get_sensor_poses.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        lib.mcl_sensor_update_fuse.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.mcl_group_set_sensor_mount.argtypes = [C.c_void_p, C.c_void_p]
        lib.mcl_host_sensor_mount.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.mcl_host_sensor_unmount.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.mcl_host_sensor_mount_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.mcl_set_beam_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        lib.mcl_get_beam_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        lib.mcl_beam_origins.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        lib.mcl_host_scan_motion_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]
        lib.mcl_host_beam_offset_table.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        lib.mcl_host_beam_offset_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p]
        _libs[path] = _lib = lib
    return _lib


def default_config(**over) -> Config:
    cfg = Config()
    load_library().mcl_default_config(C.byref(cfg))
    for k, v in over.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def default_kld_config(**over) -> KldConfig:
    """mcl_default_kld_config, with fields overridden by keyword."""
    k = KldConfig()
    load_library().mcl_default_kld_config(C.byref(k))
    for name, v in over.items():
        if name not in dict(KldConfig._fields_):
            raise AttributeError(name)
        setattr(k, name, v)
    return k


def default_recovery_config(**over) -> RecoveryConfig:
    """mcl_default_recovery_config, with fields overridden by keyword."""
    c = RecoveryConfig()
    load_library().mcl_default_recovery_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(RecoveryConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, v)
    return c


def host_recovery_step(cfg: RecoveryConfig, S, F, reset, max_logw, sum_w, denom, n_beams):
    """One update of the recovery averages on the host (mcl_host_recovery_step; no device needed): (S, F, p of the next
    update) after folding in the likelihood of an update with SCALARS max_logw, sum_w and denominator denom (N, or the previous
    update's sum_w for a kept update); NaN = unset."""
    st, out, p = (C.c_double * 2)(S, F), (C.c_double * 2)(), C.c_double()
    rc = load_library().mcl_host_recovery_step(C.byref(cfg), st, C.c_int32(1 if reset else 0), C.c_double(max_logw),
                                               C.c_double(sum_w), C.c_double(denom), C.c_int32(int(n_beams)), out, C.byref(p))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_recovery_step rc={rc}", rc)
    return out[0], out[1], p.value


def _proposal_arrays(means, covs, weights):
    """(M, means, covs, weights or None) as the C calls take them; ValueError for shapes that are not (M, 3) / (M, 3, 3) or (M, 9) / (M,)"""
    m = _c(np.atleast_2d(np.asarray(means, np.float64)), np.float64)
    c = _c(covs, np.float64)
    if m.ndim != 2 or m.shape[1] != 3 or c.size != 9 * m.shape[0]:
        raise ValueError("means must be (M, 3) and covs (M, 3, 3)")
    w = None
    if weights is not None:
        w = _c(weights, np.float64).ravel()
        if w.size != m.shape[0]:
            raise ValueError("weights must have one entry per component")
    return m.shape[0], m, c, w


def host_recovery_proposal(means, covs, weights=None):
    """What Engine.set_recovery_proposal uploads for a mixture (mcl_host_recovery_proposal, rules P1 / P2; no device needed):
    (thresholds, factors) -- M uint64 and (M, 9) doubles (mean x, y, theta, L00 L10 L11 L20 L21 L22).  A refused mixture raises
    EngineError; the message names the first component that is refused on its own."""
    M, m, c, w = _proposal_arrays(means, covs, weights)
    thr, fac = np.zeros(M, np.uint64), np.zeros((M, 9), np.float64)
    lib = load_library()
    rc = lib.mcl_host_recovery_proposal(C.c_int32(M), _p(m) if M else None, _p(c) if M else None, _p(w) if w is not None else None,
                                        _p(thr) if M else None, _p(fac) if M else None)
    if rc != MCL_OK:
        c9 = c.reshape(M, 9) if M else c
        one = np.ones(1)
        for k in range(M if M <= 4096 else 0):
            wk = _c([w[k]], np.float64) if w is not None and w[k] != 0.0 else one     # (a zero weight alone is only an empty sum)
            mk, ck = _c(m[k], np.float64), _c(c9[k], np.float64)
            if lib.mcl_host_recovery_proposal(C.c_int32(1), _p(mk), _p(ck), _p(wk), None, None) != MCL_OK:
                raise EngineError(f"mcl_host_recovery_proposal rc={rc}: component {k} is refused", rc)
        raise EngineError(f"mcl_host_recovery_proposal rc={rc}: n_components or the sum of the weights is refused", rc)
    return thr, fac


def default_likelihood_field_config(**over) -> LikelihoodFieldConfig:
    """mcl_default_likelihood_field_config (AMCL's defaults), with fields overridden by keyword."""
    c = LikelihoodFieldConfig()
    load_library().mcl_default_likelihood_field_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(LikelihoodFieldConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, (C.c_int32 * 2)(*v) if name == "reserved" else v)
    return c


def host_likelihood_field(grid, resolution, **fields) -> np.ndarray:
    """The likelihood field D of a map (mcl_host_likelihood_field; no device needed): shape (H, W), uint16."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H, W), np.uint16)
    c = default_likelihood_field_config(**fields)
    rc = load_library().mcl_host_likelihood_field(_p(g), W, H, np.float32(resolution), C.byref(c), _p(out), out.size)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_likelihood_field rc={rc}", rc)
    return out


def host_likelihood_table(resolution, cfg: Config | None = None, **fields) -> np.ndarray:
    """The table Lf (K + 1 float32 entries) of the likelihood field (mcl_host_likelihood_table; no device needed); cfg supplies
    max_range_m and squash_factor (default: mcl_default_config's)."""
    cfg = cfg or default_config()
    c = default_likelihood_field_config(**fields)
    lib, K = load_library(), C.c_int32()
    rc = lib.mcl_host_likelihood_table(C.byref(cfg), C.byref(c), np.float32(resolution), None, 0, C.byref(K))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_likelihood_table rc={rc}", rc)
    out = np.empty(K.value + 1, np.float32)
    rc = lib.mcl_host_likelihood_table(C.byref(cfg), C.byref(c), np.float32(resolution), _p(out), out.size, None)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_likelihood_table rc={rc}", rc)
    return out


def default_beam_skip_config(**over) -> BeamSkipConfig:
    """mcl_default_beam_skip_config (AMCL's defaults), with fields overridden by keyword."""
    c = BeamSkipConfig()
    load_library().mcl_default_beam_skip_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(BeamSkipConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, (C.c_int32 * 2)(*v) if name == "reserved" else v)
    return c


def _mount3(mount):
    m = np.ascontiguousarray(np.zeros(3) if mount is None else mount, np.float64).reshape(-1)
    if m.size != 3:
        raise ValueError("a sensor mount is (mx, my, mtheta)")
    return m


def _host_mount_call(name, mount, poses):
    m = _mount3(mount)
    p = np.ascontiguousarray(poses, np.float64)
    if p.ndim == 1 and p.size == 3:
        p = p.reshape(3, 1)
    if p.ndim != 2 or p.shape[0] != 3:
        raise ValueError("poses must be (3, n): the rows x, y, theta")
    out = np.empty_like(p)
    rc = getattr(load_library(), name)(_p(m), _p(p), C.c_int64(p.shape[1]), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"{name} rc={rc}", rc)
    return out


def host_sensor_mount(mount, poses):
    """The sensor poses (3, n) of the base poses (3, n) under `mount` = (mx, my, mtheta) (mcl_host_sensor_mount: rule SM2 of
    DESIGN.md §4.25 with the host's libm; no device needed)."""
    return _host_mount_call("mcl_host_sensor_mount", mount, poses)


def host_sensor_unmount(mount, poses):
    """The base poses (3, n) of the sensor poses (3, n): the inverse composition (mcl_host_sensor_unmount; no device needed)."""
    return _host_mount_call("mcl_host_sensor_unmount", mount, poses)


def host_sensor_mount_cov(mount, pose, cov, to_base=False):
    """J cov J^T (3, 3) with the Jacobian of SM2 at the base pose `pose`, or (to_base=True) of its inverse at the sensor pose `pose`
    (mcl_host_sensor_mount_cov; no device needed)."""
    m = _mount3(mount)
    p = np.ascontiguousarray(pose, np.float64).reshape(-1)
    c = np.ascontiguousarray(cov, np.float64).reshape(-1)
    if p.size != 3 or c.size != 9:
        raise ValueError("pose is (x, y, theta), cov 3 x 3")
    out = np.empty((3, 3), np.float64)
    rc = load_library().mcl_host_sensor_mount_cov(_p(m), _p(p), _p(c), C.c_int(1 if to_base else 0), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_sensor_mount_cov rc={rc}", rc)
    return out


def host_scan_motion_offsets(motion, n_beams, t=None, t_ref=1.0, mount=None):
    """The (3, n_beams) table of per-beam sensor offsets (rows ox, oy, dtheta) of a scan taken under a constant twist
    (mcl_host_scan_motion_offsets, rules DM1 / DM2 of DESIGN.md §4.26; no device needed).  motion = (u, v, w): the base's body-frame
    twist integrated over the scan's unit of t (the odometry twist times the sweep duration); t: one stamp per beam (None:
    j / (B - 1)); t_ref: the time at which the particles are the robot's pose (1.0: the end of the sweep); mount: the sensor mount."""
    mo = np.ascontiguousarray(motion, np.float64).reshape(-1)
    if mo.size != 3:
        raise ValueError("motion is (u, v, w)")
    m = None if mount is None else _mount3(mount)
    tt = None if t is None else np.ascontiguousarray(t, np.float64).reshape(-1)
    if tt is not None and tt.size != int(n_beams):
        raise ValueError("t holds one stamp per beam")
    out = np.empty((3, max(int(n_beams), 0)), np.float64)
    rc = load_library().mcl_host_scan_motion_offsets(_p(mo), _p(m), _p(tt), C.c_double(float(t_ref)), C.c_int32(int(n_beams)), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_scan_motion_offsets rc={rc}", rc)
    return out


def _offsets3(offsets, n_beams=None):
    o = np.ascontiguousarray(offsets, np.float64)
    if o.ndim != 2 or o.shape[0] != 3 or (n_beams is not None and o.shape[1] != n_beams):
        raise ValueError("beam offsets are (3, n_beams): the rows ox, oy, dtheta")
    return o


def host_beam_offset_table(angles, offsets):
    """(effective float angles a' (B,), their direction pairs (2, B): cos, sin) of rule DS1, as Engine.set_beam_offsets forms them
    (mcl_host_beam_offset_table; no device needed)."""
    a = _c(angles, np.float32).reshape(-1)
    o = _offsets3(offsets, a.size)
    eff, dirs = np.empty(a.size, np.float32), np.empty((2, a.size), np.float64)
    rc = load_library().mcl_host_beam_offset_table(_p(a), _p(o), C.c_int32(a.size), _p(eff), _p(dirs))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_beam_offset_table rc={rc}", rc)
    return eff, dirs


def host_beam_offset_pairs(ranges, offsets, dirs, resolution):
    """The likelihood field's pair (2, B), in cells, of every beam of `ranges` under rule DS5 (mcl_host_beam_offset_pairs; no device
    needed); dirs as host_beam_offset_table returns them."""
    r = _c(ranges, np.float32).reshape(-1)
    o = _offsets3(offsets, r.size)
    d = np.ascontiguousarray(dirs, np.float64)
    if d.shape != (2, r.size):
        raise ValueError("dirs is (2, B)")
    out = np.empty((2, r.size), np.float64)
    rc = load_library().mcl_host_beam_offset_pairs(_p(r), _p(o), _p(d), C.c_int32(r.size), C.c_double(float(np.float32(resolution))), _p(out))      # (the map's float resolution, widened: set_map)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_beam_offset_pairs rc={rc}", rc)
    return out


def host_beam_skip_thresholds(resolution, n_particles, n_used, **fields):
    """(ka, min_count, min_skipped) of an update of n_particles particles with n_used used beams (mcl_host_beam_skip_thresholds,
    rules BS1, BS3, BS4; no device needed): the integers the engine itself forms for its kernels."""
    c = default_beam_skip_config(**fields)
    ka, mc, ms = C.c_int32(), C.c_int64(), C.c_int32()
    rc = load_library().mcl_host_beam_skip_thresholds(C.byref(c), np.float32(resolution), C.c_int64(int(n_particles)),
                                                      C.c_int32(int(n_used)), C.byref(ka), C.byref(mc), C.byref(ms))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_beam_skip_thresholds rc={rc}", rc)
    return ka.value, mc.value, ms.value


def host_beam_skip_plan(counts_used, n_particles, **fields):
    """(kept_used, n_skipped, integrate_all) for the agreement counts of the used beams (mcl_host_beam_skip_plan, rules BS3, BS4; no
    device needed): kept_used is uint8 per used beam, 1 summed, 2 skipped."""
    c = default_beam_skip_config(**fields)
    cnt = _c(counts_used, np.uint32).ravel()
    kept = np.zeros(cnt.size, np.uint8)
    ns, ia = C.c_int32(), C.c_int32()
    rc = load_library().mcl_host_beam_skip_plan(C.byref(c), _p(cnt) if cnt.size else None, C.c_int32(cnt.size),
                                                C.c_int64(int(n_particles)), _p(kept) if cnt.size else None, C.byref(ns), C.byref(ia))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_beam_skip_plan rc={rc}", rc)
    return kept, ns.value, ia.value


def default_motion_config(**over) -> MotionConfig:
    """mcl_default_motion_config (DIFF, AMCL's alphas), with fields overridden by keyword; `model` may be a name
    ("reference", "diff", "omni")."""
    c = MotionConfig()
    load_library().mcl_default_motion_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(MotionConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, MOTION_MODELS[v] if name == "model" and isinstance(v, str) else v)
    return c


def host_motion_scalars(cfg: MotionConfig, action) -> np.ndarray:
    """The per-update scalars of an odometry model (mcl_host_motion_scalars; no device needed): 8 doubles."""
    a, out = _c(action, np.float64), np.empty(8)
    assert a.size == 3
    rc = load_library().mcl_host_motion_scalars(C.byref(cfg), _p(a), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_motion_scalars rc={rc}", rc)
    return out


def host_motion_sample(cfg: MotionConfig, action, xyz_colmajor, normals_nx3) -> np.ndarray:
    """The children of the poses (3, n) under an odometry model with the normals (n, 3) (mcl_host_motion_sample; no device)."""
    a, p, nrm = _c(action, np.float64), _c(xyz_colmajor, np.float64), _c(normals_nx3, np.float64)
    assert a.size == 3 and p.ndim == 2 and p.shape[0] == 3 and nrm.size == 3 * p.shape[1]
    out = np.empty_like(p)
    rc = load_library().mcl_host_motion_sample(C.byref(cfg), _p(a), _p(p), _p(nrm), C.c_int64(p.shape[1]), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_motion_sample rc={rc}", rc)
    return out


def host_gaussian_factor(cov) -> np.ndarray:
    """The lower Cholesky factor init_particles_gaussian draws with (mcl_host_gaussian_factor; no device needed), 3 x 3."""
    c, L = _c(cov, np.float64), np.empty(6)
    assert c.size == 9
    rc = load_library().mcl_host_gaussian_factor(_p(c), _p(L))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_gaussian_factor rc={rc}", rc)
    return np.array([[L[0], 0.0, 0.0], [L[1], L[2], 0.0], [L[3], L[4], L[5]]])


def default_search_config(**over) -> SearchConfig:
    """mcl_default_search_config (stride 2, 72 headings, every beam, local maxima), with fields overridden by keyword."""
    c = SearchConfig()
    load_library().mcl_default_search_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(SearchConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, (C.c_int32 * 4)(*v) if name == "reserved" else v)
    return c


def search_stream_config(budget_bytes=0, slab_headings=0, reserved=(0, 0, 0, 0, 0)) -> SearchStreamConfig:
    """mcl_search_stream_config_t: 0 bytes is the default budget (1 GiB), 0 headings the largest slab that fits it."""
    c = SearchStreamConfig()
    load_library().mcl_default_search_stream_config(C.byref(c))
    c.budget_bytes, c.slab_headings, c.reserved = int(budget_bytes), int(slab_headings), (C.c_int32 * 5)(*reserved)
    return c


def host_search_slabs(n_positions, n_scans=1, budget_bytes=0, slab_headings=0, stream_reserved=(0, 0, 0, 0, 0), **fields):
    """The plan of a streamed search (mcl_host_search_slabs, rules ST4 / ST5; no device needed): (G, n_slabs, bytes) -- the headings
    per slab, the number of slabs, the device bytes of the slab buffers.  `fields` override mcl_default_search_config."""
    c = default_search_config(**fields)
    sc = search_stream_config(budget_bytes, slab_headings, stream_reserved)
    G, ns, b = C.c_int32(), C.c_int32(), C.c_uint64()
    rc = load_library().mcl_host_search_slabs(C.byref(c), C.byref(sc), C.c_int64(int(n_positions)), C.c_int32(int(n_scans)), C.byref(G),
                                              C.byref(ns), C.byref(b))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_slabs rc={rc}", rc)
    return int(G.value), int(ns.value), int(b.value)


def search_prune_config(block=0, first_pairs=0, reserved=(0, 0, 0, 0, 0, 0)) -> SearchPruneConfig:
    """mcl_search_prune_config_t: block 0 is the default block side (mcl_default_search_prune_config's), first_pairs 0 the default
    first round (max(1024, pairs / 64))."""
    c = SearchPruneConfig()
    load_library().mcl_default_search_prune_config(C.byref(c))
    if block:
        c.block = int(block)
    c.first_pairs = int(first_pairs)
    c.reserved[:] = [int(v) for v in reserved]
    return c


def host_search_blocks(grid, block=0, **fields) -> dict:
    """The block plan of a pruned search over a map (mcl_host_search_blocks, rules P1 / P2; no device needed): {n_blocks, w, nbx,
    nby, blocks} -- the live blocks, the window of the pooled field, the block grid, and per live block (bx, by, positions in it)
    in the order of the pair numbering: pair = k * n_blocks + b.  `fields` override mcl_default_search_config."""
    g = _c(grid, np.int8)
    H, W = g.shape
    c, pc = default_search_config(**fields), search_prune_config(block)
    lib = load_library()
    n, w, nbx, nby = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    args = (C.byref(c), C.byref(pc), _p(g), W, H, C.byref(n), C.byref(w), C.byref(nbx), C.byref(nby))
    rc = lib.mcl_host_search_blocks(*args, None, 0)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_blocks rc={rc}", rc)
    blocks = np.empty((n.value, 3), np.int32)
    if n.value:
        rc = lib.mcl_host_search_blocks(*args, _p(blocks), n.value)
        if rc != MCL_OK:
            raise EngineError(f"mcl_host_search_blocks rc={rc}", rc)
    return dict(n_blocks=n.value, w=w.value, nbx=nbx.value, nby=nby.value, blocks=blocks)


def host_lf_pool(D, K, w) -> np.ndarray:
    """The pooled field Dp of a likelihood field D (mcl_host_lf_pool, rule P2; no device needed): shape (H + w - 1, W + w - 1),
    uint16; out[y + w - 1, x + w - 1] is the minimum over the w x w window with low corner (x, y), cells off the map counting K."""
    d = _c(D, np.uint16)
    H, W = d.shape
    out = np.empty((H + int(w) - 1, W + int(w) - 1), np.uint16)
    rc = load_library().mcl_host_lf_pool(_p(d), W, H, C.c_int32(int(K)), C.c_int32(int(w)), _p(out), out.size)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_lf_pool rc={rc}", rc)
    return out


def host_search_bound_table(lf) -> np.ndarray:
    """Ub[k] = max over j >= k of Lf[j] (mcl_host_search_bound_table, rule P2; no device needed): K + 1 float32 entries."""
    t = _c(lf, np.float32)
    out = np.empty_like(t)
    rc = load_library().mcl_host_search_bound_table(_p(t), C.c_int32(t.size - 1), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_bound_table rc={rc}", rc)
    return out


def host_search_prune_next(pairs, n_scored, first_below_c=0, first_pairs=0) -> int:
    """The round schedule of a pruned search (mcl_host_search_prune_next, rule P4; no device needed): how many ranks have scores
    after the next round; n_scored = 0 gives the first round."""
    pc, out = search_prune_config(0, first_pairs), C.c_int64()
    rc = load_library().mcl_host_search_prune_next(C.byref(pc), C.c_int64(int(pairs)), C.c_int64(int(n_scored)),
                                                   C.c_int64(int(first_below_c)), C.byref(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_prune_next rc={rc}", rc)
    return out.value


def host_search_lattice(grid, resolution, origin_x, origin_y, **fields):
    """The positions of the global search's lattice over a map (mcl_host_search_lattice, rule S1; no device needed): (cells, xy) --
    the linear map cell of every position (uint32) and its pose coordinates, shape (n_positions, 2)."""
    g = _c(grid, np.int8)
    H, W = g.shape
    c = default_search_config(**fields)
    lib, n = load_library(), C.c_int64()
    args = (C.byref(c), _p(g), W, H, np.float32(resolution), float(origin_x), float(origin_y))
    rc = lib.mcl_host_search_lattice(*args, None, None, 0, C.byref(n))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_lattice rc={rc}", rc)
    cells, xy = np.empty(n.value, np.uint32), np.empty((n.value, 2), np.float64)
    if n.value:
        rc = lib.mcl_host_search_lattice(*args, _p(cells), _p(xy), n.value, C.byref(n))
        if rc != MCL_OK:
            raise EngineError(f"mcl_host_search_lattice rc={rc}", rc)
    return cells, xy


def host_search_headings(**fields) -> np.ndarray:
    """The headings of the global search (mcl_host_search_headings, rule S2; no device needed): n_headings doubles."""
    c = default_search_config(**fields)
    out = np.empty(max(int(c.n_headings), 0), np.float64)
    rc = load_library().mcl_host_search_headings(C.byref(c), _p(out), out.size)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_headings rc={rc}", rc)
    return out


def host_search_beam_grid(angles, n_headings=72) -> dict:
    """The angle grid of a search under the beam model (mcl_host_search_beam_grid, rule B1; no device needed): {M, heading_step,
    delta, max_dev, phi} -- the grid angles per turn, the grid steps between two headings, the grid's increment, the worst
    deviation of a beam angle from its grid angle, and the M grid angles.  Raises EngineError (with .max_dev where it was
    measured) when the scan and the heading count do not share a grid."""
    a = _c(angles, np.float32)
    lib = load_library()
    M, s, d, dev = C.c_int32(), C.c_int32(), C.c_double(), C.c_double(float("nan"))
    rc = lib.mcl_host_search_beam_grid(_p(a) if a.size else None, C.c_int32(a.size), C.c_int32(int(n_headings)), C.byref(M), C.byref(s),
                                       C.byref(d), C.byref(dev), None, 0)
    if rc != MCL_OK:
        err = EngineError(f"mcl_host_search_beam_grid rc={rc}", rc)
        err.max_dev = dev.value
        raise err
    phi = np.empty(M.value, np.float64)
    rc = lib.mcl_host_search_beam_grid(_p(a), C.c_int32(a.size), C.c_int32(int(n_headings)), None, None, None, None, _p(phi), phi.size)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_beam_grid rc={rc}", rc)
    return dict(M=int(M.value), heading_step=int(s.value), delta=d.value, max_dev=dev.value, phi=phi)


def _rel_rows(rel) -> np.ndarray:
    """(S, 3) rows of (dx, dy, dtheta), or one such row, C-contiguous float64"""
    r = np.asarray(rel, np.float64)
    if r.ndim == 1:
        r = r.reshape(1, -1)
    if r.ndim != 2 or r.shape[1] != 3:
        raise ValueError("expected (S, 3) rows of three values, or one row")
    return _c(r, np.float64)


def host_search_sequence_offsets(rel, **fields) -> np.ndarray:
    """The table a search over a scan sequence uploads (mcl_host_search_sequence_offsets, rule SQ1; no device needed): shape
    (n_headings, S, 3), [k, s] = (ax_ks, ay_ks, theta_ks) -- scan s's displacement from the anchor in the map frame at heading k,
    and its heading.  `rel`: (S, 3) rows of (dx, dy, dtheta) in the anchor's frame."""
    c = default_search_config(**fields)
    r = _rel_rows(rel)
    S = r.shape[0]
    out = np.empty((max(int(c.n_headings), 0), S, 3), np.float64)
    rc = load_library().mcl_host_search_sequence_offsets(C.byref(c), _p(r) if S else None, C.c_int32(S), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_search_sequence_offsets rc={rc}", rc)
    return out


def relative_poses(odom, anchor=-1) -> np.ndarray:
    """Absolute odometry poses, (S, 3) rows of (x, y, theta), as poses relative to the one at `anchor` (mcl_host_relative_poses):
    the `rel` of Engine.global_search_sequence.  anchor = -1, the default: the latest pose."""
    o = _rel_rows(odom)
    S = o.shape[0]
    a = int(anchor) + S if int(anchor) < 0 else int(anchor)
    out = np.empty((S, 3), np.float64)
    rc = load_library().mcl_host_relative_poses(_p(o) if S else None, C.c_int32(S), C.c_int32(a), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_relative_poses rc={rc}", rc)
    return out


def default_refine_config(**over) -> RefineConfig:
    """mcl_default_refine_config (a 9 x 9 x 21 window: +-2 cells in steps of half a cell, +-5 degrees in steps of half a degree,
    every beam), with fields overridden by keyword."""
    c = RefineConfig()
    load_library().mcl_default_refine_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(RefineConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, (C.c_int32 * 3)(*v) if name == "reserved" else v)
    return c


def refine_window_size(c: RefineConfig) -> int:
    """n_win of a config (rule R1), in Python's integers"""
    return (2 * int(c.half_xy) + 1) ** 2 * (2 * int(c.half_theta) + 1)


def host_refine_window(seed, resolution, **fields) -> np.ndarray:
    """The window poses around `seed` (mcl_host_refine_window, rule R1; no device needed): (n_win, 3) rows of (x, y, theta) in
    window-index order, ix fastest.  `fields` override mcl_default_refine_config."""
    c = default_refine_config(**fields)
    s = _c(seed, np.float64).ravel()
    assert s.size == 3
    n = refine_window_size(c)
    out = np.empty((n if 0 < n <= MAX_REFINE_WINDOW else 1, 3), np.float64)
    rc = load_library().mcl_host_refine_window(C.byref(c), _p(s), np.float32(resolution), _p(out), C.c_size_t(out.shape[0]))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_refine_window rc={rc}", rc)
    return out


def host_refine_reduce(seed, resolution, scores, **fields) -> np.ndarray:
    """What Engine.refine_poses reports for one seed whose window scored `scores` (mcl_host_refine_reduce, rules R3 / R4; no device
    needed): one REFINE_DTYPE record."""
    c = default_refine_config(**fields)
    s, v = _c(seed, np.float64).ravel(), _c(scores, np.float64).ravel()
    assert s.size == 3
    out = np.zeros(1, REFINE_DTYPE)
    rc = load_library().mcl_host_refine_reduce(C.byref(c), _p(s), np.float32(resolution), _p(v), C.c_size_t(v.size), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_refine_reduce rc={rc}", rc)
    return out[0]


def host_refine_sequence_offsets(seeds, rel, **fields) -> np.ndarray:
    """The table a refinement over a scan sequence uploads (mcl_host_refine_sequence_offsets, rule RS1; no device needed): shape
    (M, nt, S, 3), [m, it, s] = (ax, ay, theta_s) -- scan s's displacement from the anchor in the map frame at window heading it
    of seed m, and its heading.  `seeds`: (M, 3) rows of (x, y, theta), or one; `rel`: (S, 3) rows of (dx, dy, dtheta) in the
    anchor's frame.  `fields` override mcl_default_refine_config."""
    c = default_refine_config(**fields)
    p = _rel_rows(seeds)
    r = _rel_rows(rel)
    M, S, nt = p.shape[0], r.shape[0], 2 * int(c.half_theta) + 1
    rows = M * nt * S
    if rows > MAX_REFINE_SEQ_ROWS:                            # (RS1's cap, here too: such a table is never allocated)
        raise EngineError(f"mcl_host_refine_sequence_offsets rc={MCL_ERR_INVALID_ARG}: {rows} rows, more than {MAX_REFINE_SEQ_ROWS}",
                          MCL_ERR_INVALID_ARG)
    # an empty table (no seed, no scan, a refused half_theta) still goes to the C call, which names the refusal by its status
    out = np.empty((M, nt, S, 3) if rows > 0 else (1, 1, 1, 3), np.float64)
    pc = _c(p.T, np.float64)                                  # column-major, as the refinement takes its seeds
    rc = load_library().mcl_host_refine_sequence_offsets(C.byref(c), _p(pc) if M else None, C.c_int32(M), _p(r) if S else None,
                                                         C.c_int32(S), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_refine_sequence_offsets rc={rc}", rc)
    return out


def seed_counts(log_likelihoods, n) -> np.ndarray:
    """How many of n particles each hit of a global search seeds (the counts of Engine.init_particles_mixture): shares
    proportional to exp(ll - max ll), the floors of the exact shares first, the particles left over to the largest remainders,
    ties to the earlier hit.  A hit at -inf gets none.  Pure Python (exact rationals), int64."""
    import math
    from fractions import Fraction
    ll = [float(v) for v in np.asarray(log_likelihoods, np.float64).ravel()]
    n = int(n)
    if not ll or n < 0 or any(math.isnan(v) or v == math.inf for v in ll):
        raise ValueError("seed_counts: needs at least one hit, n >= 0 and scores below +inf")
    top = max(ll)
    if top == -math.inf:
        raise ValueError("seed_counts: every hit is at -inf")
    w = [Fraction(math.exp(v - top)) for v in ll]            # (exp(-inf) = 0; the best hit weighs exactly 1)
    total = sum(w)
    share = [n * v / total for v in w]
    counts = [int(v) for v in share]                         # floors (the shares are >= 0)
    order = sorted(range(len(ll)), key=lambda i: (-(share[i] - counts[i]), i))
    for i in order[:n - sum(counts)]:
        counts[i] += 1
    return np.array(counts, np.int64)


def default_cluster_config(**over) -> ClusterConfig:
    """mcl_default_cluster_config, with fields overridden by keyword."""
    c = ClusterConfig()
    load_library().mcl_default_cluster_config(C.byref(c))
    for name, v in over.items():
        if name not in dict(ClusterConfig._fields_):
            raise AttributeError(name)
        setattr(c, name, v)
    return c


def host_kld_bins(x, y, th, width, height, resolution, origin_x, origin_y, kld: KldConfig) -> int:
    """Pose-space bins the poses (x, y, th) occupy under the KLD bin rule (mcl_host_kld_bins; no device needed)."""
    x, y, th = _c(x, np.float64), _c(y, np.float64), _c(th, np.float64)
    assert x.size == y.size == th.size
    out = C.c_int64()
    rc = load_library().mcl_host_kld_bins(_p(x), _p(y), _p(th), x.size, width, height, np.float32(resolution), origin_x, origin_y,
                                          C.byref(kld), C.byref(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_kld_bins rc={rc}", rc)
    return out.value


def host_kld_target(kld: KldConfig, bins: int, n_current: int) -> int:
    """The particle count the update after one that counted `bins` with n_current particles draws (mcl_host_kld_target)."""
    out = C.c_int64()
    rc = load_library().mcl_host_kld_target(C.byref(kld), int(bins), int(n_current), C.byref(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_kld_target rc={rc}", rc)
    return out.value


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def host_sensor_table(P: int, cfg: Config | None = None) -> np.ndarray:
    """The engine's host-side sensor table (no device needed); returned as T[d, r]."""
    cfg = cfg or default_config()
    out = np.empty((P + 1) * (P + 1), np.float64)
    rc = load_library().mcl_host_sensor_table(C.byref(cfg), C.c_int32(P), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_sensor_table rc={rc}")
    return out.reshape(P + 1, P + 1)


def host_skip_field(grid) -> np.ndarray:
    """The engine's padded skip-distance field (no device needed): shape (H+1, W+1), uint8."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    rc = load_library().mcl_host_skip_field(_p(g), C.c_uint32(W), C.c_uint32(H), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_skip_field rc={rc}")
    return out


WEDGES = 16


def host_skip_field_wedge(grid, wedge: int) -> np.ndarray:
    """Skip field for rays whose direction angle lies in sector `wedge` of WEDGES equal sectors of the turn."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    rc = load_library().mcl_host_skip_field_wedge(_p(g), C.c_uint32(W), C.c_uint32(H), C.c_int32(wedge), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_skip_field_wedge rc={rc}")
    return out


def host_sweep_global_layout(width: int, height: int, max_range_px: int) -> dict:
    """mcl_host_sweep_global_layout: {ok, pitch, rows, stride, alloc, max_offset} of the ringed copies of the wedge fields."""
    out = (C.c_int64 * 6)()
    rc = load_library().mcl_host_sweep_global_layout(C.c_uint32(width), C.c_uint32(height), C.c_int32(max_range_px), out)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_sweep_global_layout rc={rc}", rc)
    return dict(ok=bool(out[0]), pitch=int(out[1]), rows=int(out[2]), stride=int(out[3]), alloc=int(out[4]), max_offset=int(out[5]))


def host_skip_field_wedge_tight(grid, wedge: int) -> np.ndarray:
    """The wedge field under the tight rule (jumps bounded by the distance travelled inside the wedge): what set_map builds."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    rc = load_library().mcl_host_skip_field_wedge_tight(_p(g), C.c_uint32(W), C.c_uint32(H), C.c_int32(wedge), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_skip_field_wedge_tight rc={rc}")
    return out


SORT_KEY_LOG2, SORT_MAX_FINE = 22, 10      # bits of the coarse ordering key, and the most fine bits below it (csrc/mcl_sort_key.h)


def sort_fine_code(fine: int, fine_sub: int | None = None) -> int:
    """the fine setting as the one word the C calls take: the bits, and the sub-cell bits per axis where they are not the rule's"""
    if not 0 <= int(fine) <= SORT_MAX_FINE or (fine_sub is not None and not 0 <= 2 * int(fine_sub) <= int(fine)):
        raise EngineError(f"sort key: fine={fine} fine_sub={fine_sub} (0 .. {SORT_MAX_FINE} bits, at most half of them per axis)", MCL_ERR_INVALID_ARG)
    return int(fine) | ((int(fine_sub) + 1) << 4 if fine_sub is not None else 0)


def sort_tile_grid(width: int, height: int):
    """(tiles per row, rows of tiles) of the 32 x 32-cell tiles over the padded map: the shape of an ordering tile map."""
    return (int(width) >> 5) + 1, (int(height) >> 5) + 1


def host_sort_key(bbox, tilemap, width: int, height: int, px, py, theta, fine: int = 0, n_layout: int | None = None,
                  fine_sub: int | None = None) -> np.ndarray:
    """mcl_host_sort_key: the ordering keys (uint32) of particles at pixel coordinates (px, py) with headings theta, under the
    layout words `bbox` (7 int32) and the tile map (None when bbox[5] == 0), with `fine` bits below the coarse 22 -- the code
    the device runs, on the CPU.  n_layout: the size of the set the layout is for (its density decides the split of the bits);
    default: the number of particles given.  fine_sub: how many of the fine bits, per axis, are sub-cell bits (default: the
    rule, max(fine - 2, 0) // 4)."""
    bb = _c(np.asarray(bbox).reshape(-1)[:7], np.int32)
    x, y, t = _c(px, np.float64), _c(py, np.float64), _c(theta, np.float64)
    if bb.size != 7 or not (x.shape == y.shape == t.shape) or x.ndim != 1:
        raise ValueError("host_sort_key: bbox has 7 words; px, py, theta are 1-D and of one length")
    ntx, nty = sort_tile_grid(width, height)
    tm = None
    if tilemap is not None:
        tm = _c(tilemap, np.int32)
        if tm.size != ntx * nty:
            raise ValueError(f"host_sort_key: the tile map has {ntx} x {nty} entries for this map")
    out = np.empty(x.size, np.uint32)
    rc = load_library().mcl_host_sort_key(_p(bb), _p(tm) if tm is not None else None, C.c_int32(ntx), C.c_uint32(width), C.c_uint32(height),
                                          _p(x), _p(y), _p(t), C.c_int64(x.size), C.c_int64(x.size if n_layout is None else n_layout),
                                          C.c_int32(sort_fine_code(fine, fine_sub)), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_sort_key rc={rc}", rc)
    return out


def host_compact_guide(ccdf, m: int, fill=None):
    """mcl_host_compact_guide: the guide of a compact parent list with the strictly increasing CDF column `ccdf` (uint64; its last
    entry is the total) for 2^m buckets, by the rule the scan kernel follows.  Returns (guide, s, bmax, words written): guide has
    bmax + 2 uint32 words, 0 .. bmax written and the last one left at `fill` (default 0xffffffff) -- the word the search's pair
    fetch touches and never uses."""
    c = _c(ccdf, np.uint64)
    if c.ndim != 1 or c.size == 0:
        raise ValueError("host_compact_guide: ccdf is 1-D and not empty")
    lib = load_library()
    s, bmax, nw = C.c_int32(), C.c_uint32(), C.c_int64()
    q = C.c_uint64(int(c[-1]))
    rc = lib.mcl_host_compact_guide(_p(c), C.c_int64(c.size), q, C.c_int32(m), None, C.c_size_t(0), C.byref(s), C.byref(bmax), None)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_compact_guide rc={rc}", rc)
    guide = np.full(bmax.value + 2, 0xffffffff if fill is None else fill, np.uint32)
    rc = lib.mcl_host_compact_guide(_p(c), C.c_int64(c.size), q, C.c_int32(m), _p(guide), C.c_size_t(bmax.value + 1), C.byref(s), C.byref(bmax),
                                    C.byref(nw))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_compact_guide rc={rc}", rc)
    return guide, s.value, bmax.value, nw.value


def host_compact_search(ccdf, guide, s: int, bmax: int, thr) -> np.ndarray:
    """mcl_host_compact_search: for every threshold the list position the resampling kernel selects -- the first entry with
    ccdf > thr, searched between the two guide words of the threshold's bucket, clamped to the last entry (int64).  guide: the
    bmax + 2 words of host_compact_guide."""
    c, g, t = _c(ccdf, np.uint64), _c(guide, np.uint32), _c(thr, np.uint64)
    out = np.empty(t.size, np.int64)
    rc = load_library().mcl_host_compact_search(_p(c), C.c_int64(c.size), _p(g), C.c_size_t(g.size), C.c_int32(s), C.c_uint32(bmax), _p(t),
                                                C.c_int64(t.size), _p(out))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_compact_search rc={rc}", rc)
    return out


WEDGE_R = 255


def host_wedge_tight_table(wedge: int):
    """(values, reachable), each (511, 511) indexed [oy + 255, ox + 255]: the uncapped skip a stop cell at that offset allows
    under the tight rule, and whether the field search counts the offset as reachable in this wedge."""
    S = 2 * WEDGE_R + 1
    val, reach = np.empty((S, S), np.int32), np.empty((S, S), np.uint8)
    rc = load_library().mcl_host_wedge_tight_table(C.c_int32(wedge), _p(val), _p(reach), C.c_size_t(val.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_wedge_tight_table rc={rc}")
    return val, reach.astype(bool)


class MapPatchStats(C.Structure):
    _fields_ = [("changed_cells", C.c_int32), ("changed_stop_cells", C.c_int32), ("window", C.c_int32 * 4), ("lf_window", C.c_int32 * 4),
                ("free_cells", C.c_int64), ("ms", C.c_double)]


# mcl_get_map_table: name -> (selector, dtype)
MAP_TABLES = {"grid": (0, np.int8), "skip": (1, np.uint8), "skip_nibbles": (2, np.uint8), "quadrant0": (3, np.uint8), "quadrant1": (4, np.uint8),
              "quadrant2": (5, np.uint8), "quadrant3": (6, np.uint8), "free_cells": (7, np.uint32)}


def host_map_patch_plan(width: int, height: int, stop_bbox, lf_reach: int = 0):
    """mcl_host_map_patch_plan: (window, lf_window), each (x0, y0, x1, y1) inclusive (x1 < x0: none) -- the padded-grid cells of the
    skip fields, and the grid cells of a likelihood field of reach lf_reach, that a stop-bit change inside the box stop_bbox
    (grid cells, inclusive) of a width x height map can alter.  EngineError INVALID_ARG for an inverted box or one outside the map."""
    box = (C.c_int32 * 4)(*[int(v) for v in stop_bbox])
    win, lfw = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    rc = load_library().mcl_host_map_patch_plan(C.c_uint32(width), C.c_uint32(height), box, C.c_int32(lf_reach), win, lfw)
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_map_patch_plan rc={rc}", rc)
    return tuple(win), tuple(lfw)


def _patch_cells(cells2d):
    c = np.asarray(cells2d, np.int8)
    if c.ndim != 2:
        raise ValueError("update_map_region: cells must be a 2-D array (rows, columns)")
    if c.strides[1] != 1 or c.strides[0] < c.shape[1]:       # (a view whose rows are contiguous is passed as it is, with its row stride)
        c = np.ascontiguousarray(c, np.int8)
    return c


def host_skip_field_dir(grid, quadrant: int) -> np.ndarray:
    """Directional skip field for rays of one direction quadrant (0:+x+y 1:-x+y 2:-x-y 3:+x-y)."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    rc = load_library().mcl_host_skip_field_dir(_p(g), C.c_uint32(W), C.c_uint32(H), C.c_int32(quadrant), _p(out), C.c_size_t(out.size))
    if rc != MCL_OK:
        raise EngineError(f"mcl_host_skip_field_dir rc={rc}")
    return out


class Engine:
    """One engine == one GPU == one particle shard."""

    def __init__(self, cfg: Config | None = None, **over):
        self.cfg = cfg if cfg is not None else default_config(**over)
        if cfg is not None:
            for k, v in over.items():
                setattr(self.cfg, k, v)
        # (the predecessors of the windowed ray kernel live in the legacy build of the library: load_library)
        self.lib = load_library(legacy=int(self.cfg.ray_kernel) in (RAYS_QUAD, RAYS_CELL))
        h = C.c_void_p()
        rc = self.lib.mcl_create(C.byref(self.cfg), C.byref(h))
        if rc != MCL_OK:
            raise EngineError(f"mcl_create rc={rc}: {self.lib.mcl_last_error(None).decode()}")
        self._h = h
        self.n = 0
        self.n_beams = 0

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.mcl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != MCL_OK:
            raise EngineError(f"{what} rc={rc}: {self.lib.mcl_last_error(self._h).decode()}", rc)

    # -- map / beams
    def set_map(self, grid, resolution, origin_x, origin_y):
        g = _c(grid, np.int8)
        H, W = g.shape
        self._chk(self.lib.mcl_set_map(self._h, _p(g), C.c_uint32(W), C.c_uint32(H), C.c_float(np.float32(resolution)),
                                       C.c_double(origin_x), C.c_double(origin_y)), "mcl_set_map")
        self.map_shape = (H, W)
        self.map_resolution = float(np.float32(resolution))

    def update_map_region(self, cells2d, x0: int, y0: int) -> dict:
        """mcl_update_map_region: the cells [x0, x0 + w) x [y0, y0 + h) of the map replaced by cells2d (h, w), every map-derived
        table brought to what set_map of the edited grid would build.  Returns the statistics of the patch."""
        c = _patch_cells(cells2d)
        st = MapPatchStats()
        self._chk(self.lib.mcl_update_map_region(self._h, _p(c), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(c.shape[1]), C.c_uint32(c.shape[0]),
                                                 C.c_uint32(c.strides[0]), C.byref(st)), "mcl_update_map_region")
        return dict(changed_cells=int(st.changed_cells), changed_stop_cells=int(st.changed_stop_cells), window=tuple(st.window),
                    lf_window=tuple(st.lf_window), free_cells=int(st.free_cells), ms=float(st.ms))

    def map_table(self, name: str) -> np.ndarray:
        """A map-derived table as stored on the device (mcl_get_map_table), flat: one of MAP_TABLES."""
        which, dt = MAP_TABLES[name]
        need = C.c_size_t()
        self._chk(self.lib.mcl_get_map_table(self._h, C.c_int32(which), None, C.c_size_t(0), C.byref(need)), "mcl_get_map_table")
        out = np.empty(need.value // np.dtype(dt).itemsize, dt)
        self._chk(self.lib.mcl_get_map_table(self._h, C.c_int32(which), _p(out), C.c_size_t(need.value), None), "mcl_get_map_table")
        return out

    @property
    def max_range_px(self) -> int:
        v = C.c_int32()
        self._chk(self.lib.mcl_get_max_range_px(self._h, C.byref(v)), "mcl_get_max_range_px")
        return v.value

    def sensor_table(self):
        P = self.max_range_px
        out = np.empty((P + 1) * (P + 1), np.float64)
        self._chk(self.lib.mcl_get_sensor_table(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_sensor_table")
        return out.reshape(P + 1, P + 1)      # [d, r]

    def set_beam_angles(self, angles):
        a = _c(angles, np.float32)
        self._chk(self.lib.mcl_set_beam_angles(self._h, _p(a), C.c_int32(a.size)), "mcl_set_beam_angles")
        self.n_beams = a.size

    # -- particles
    def set_particles(self, xyz_colmajor, weights):
        p = _c(xyz_colmajor, np.float64)
        assert p.ndim == 2 and p.shape[0] == 3
        w = _c(weights, np.float64)
        n = p.shape[1]
        assert w.size == n
        self._chk(self.lib.mcl_set_particles(self._h, _p(p), _p(w), C.c_int64(n)), "mcl_set_particles")
        self.n = self.particle_count()

    def set_particles_shard(self, xyz_colmajor, weights, max_weight_of_the_whole_set):
        """set_particles for one shard of a larger set: weights are quantised against the whole set's maximum weight."""
        p = _c(xyz_colmajor, np.float64)
        w = _c(weights, np.float64)
        n = p.shape[1]
        assert p.ndim == 2 and p.shape[0] == 3 and w.size == n
        self._chk(self.lib.mcl_set_particles_shard(self._h, _p(p), _p(w), C.c_int64(n), C.c_double(max_weight_of_the_whole_set)),
                  "mcl_set_particles_shard")
        self.n = self.particle_count()

    def init_particles_pose(self, pose, n, first_global_index=0, n_total=None):
        p = _c(pose, np.float64)
        self._chk(self.lib.mcl_init_particles_pose(self._h, _p(p), C.c_int64(n), C.c_int64(first_global_index),
                                                   C.c_int64(n_total or n)), "mcl_init_particles_pose")
        self.n = self.particle_count()

    def init_global(self, n, first_global_index=0, n_total=None):
        self._chk(self.lib.mcl_init_global(self._h, C.c_int64(n), C.c_int64(first_global_index), C.c_int64(n_total or n)),
                  "mcl_init_global")
        self.n = self.particle_count()

    def init_particles_gaussian(self, mean, cov, n, first_global_index=0, n_total=None):
        """A Gaussian cloud around `mean` with the 3 x 3 covariance `cov` (an /initialpose, or a cluster of pose_clusters), drawn on
        the device (mcl_init_particles_gaussian)."""
        m, c = _c(mean, np.float64), _c(cov, np.float64)
        assert m.size == 3 and c.size == 9
        self._chk(self.lib.mcl_init_particles_gaussian(self._h, _p(m), _p(c), C.c_int64(n), C.c_int64(first_global_index),
                                                       C.c_int64(n_total or n)), "mcl_init_particles_gaussian")
        self.n = self.particle_count()

    def init_particles_mixture(self, means, covs, counts, n=None, first_global_index=0, n_total=None):
        """One cloud from several Gaussians -- the hits of global_search, or clusters (mcl_init_particles_mixture): means (M, 3),
        covs (M, 3, 3) or one (3, 3) for all, counts (M,) particles per component of the whole set (seed_counts makes them from hit
        scores).  n / first_global_index: this engine's shard of the set (default: all of it)."""
        m, k = _c(means, np.float64).reshape(-1, 3), _c(counts, np.int64).ravel()
        c = _c(covs, np.float64)
        c = _c(np.broadcast_to(c.reshape(-1, 3, 3), (m.shape[0], 3, 3)), np.float64)
        assert k.size == m.shape[0]
        n_total = int(k.sum()) if n_total is None else int(n_total)
        n = n_total - first_global_index if n is None else int(n)
        self._chk(self.lib.mcl_init_particles_mixture(self._h, C.c_int32(m.shape[0]), _p(m), _p(c), _p(k), C.c_int64(n),
                                                      C.c_int64(first_global_index), C.c_int64(n_total)), "mcl_init_particles_mixture")
        self.n = self.particle_count()

    # -- odometry motion models (off by default: the reference's model)
    def set_motion_model(self, model="diff", **fields):
        """Selects the motion model of the updates that follow: "diff" / "omni" with mcl_default_motion_config's values (AMCL's
        alphas) overridden by `fields`, or None / "reference" for the reference's model."""
        if model is None:
            self._chk(self.lib.mcl_set_motion_model(self._h, None), "mcl_set_motion_model")
            return None
        c = default_motion_config(model=model, **fields)
        self._chk(self.lib.mcl_set_motion_model(self._h, C.byref(c)), "mcl_set_motion_model")
        return c

    def motion_model(self) -> MotionConfig:
        c = MotionConfig()
        self._chk(self.lib.mcl_get_motion_model(self._h, C.byref(c)), "mcl_get_motion_model")
        return c

    # -- sensor mount (off by default)
    def set_sensor_mount(self, mount):
        """The sensor's pose (mx, my, mtheta) in the base frame for the sensor stages that follow (mcl_set_sensor_mount); None or
        (0, 0, 0) = no mount.  The particles stay base poses."""
        m = _mount3(mount)
        self._chk(self.lib.mcl_set_sensor_mount(self._h, _p(m)), "mcl_set_sensor_mount")

    def sensor_mount(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_get_sensor_mount(self._h, _p(out)), "mcl_get_sensor_mount")
        return out

    def mount_poses(self, poses):
        """The sensor poses (3, k) of the base poses (3, k), k <= 65536, formed on the device with the current mount
        (mcl_mount_poses): bit for bit what the sensor stages use.  With no mount a copy."""
        p = np.ascontiguousarray(poses, np.float64)
        if p.ndim != 2 or p.shape[0] != 3:
            raise ValueError("poses must be (3, k): the rows x, y, theta")
        out = np.empty_like(p)
        self._chk(self.lib.mcl_mount_poses(self._h, _p(p), C.c_int64(p.shape[1]), _p(out)), "mcl_mount_poses")
        return out

    def sensor_poses(self):
        """The (3, n) sensor poses the last sensor stage read (mcl_get_sensor_poses); MCL_ERR_NOT_READY when none has run with a
        mount or the particles have changed since."""
        out = np.empty((3, self.n), np.float64)
        self._chk(self.lib.mcl_get_sensor_poses(self._h, _p(out), C.c_int64(self.n)), "mcl_get_sensor_poses")
        return out

    def sensor_update_fuse(self, obs):
        """Weighs a further scan into the posterior of the last weighting call (mcl_sensor_update_fuse): the log-weights of `obs`
        under the current beams, mount and sensor model add to the ones in place.  Two lidars:
            e.set_sensor_mount(front); e.set_beam_angles(a_front); e.update(action, scan_front)
            e.set_sensor_mount(rear);  e.set_beam_angles(a_rear);  e.sensor_update_fuse(scan_rear)"""
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_sensor_update_fuse(self._h, _p(o), C.c_int32(o.size)), "mcl_sensor_update_fuse")

    # -- scan de-skew: per-beam sensor offsets (off by default)
    def set_beam_offsets(self, offsets):
        """The (3, n_beams) table of per-beam sensor offsets (rows ox, oy, dtheta: the sensor's pose when beam j was taken, in the
        sensor's frame at the scan's reference time) for the updates that follow (mcl_set_beam_offsets); None = off.  A node:
            e.set_beam_offsets(host_scan_motion_offsets(twist * sweep_time, B, mount=m)); e.update(action, scan)"""
        if offsets is None:
            self._chk(self.lib.mcl_set_beam_offsets(self._h, None, C.c_int32(0)), "mcl_set_beam_offsets")
            return
        o = np.ascontiguousarray(offsets, np.float64)
        if o.ndim != 2 or o.shape[0] != 3:
            raise ValueError("beam offsets are (3, n_beams): the rows ox, oy, dtheta")
        self._chk(self.lib.mcl_set_beam_offsets(self._h, _p(o), C.c_int32(o.shape[1])), "mcl_set_beam_offsets")

    def beam_offsets(self):
        """(the table (3, B) as given -- zeros when off --, rule DS1's float angles (B,) -- the beam angles when off --, whether
        offsets are on) (mcl_get_beam_offsets)."""
        o, a, on = np.empty((3, self.n_beams), np.float64), np.empty(self.n_beams, np.float32), C.c_int32()
        self._chk(self.lib.mcl_get_beam_offsets(self._h, _p(o), _p(a), C.c_int32(self.n_beams), C.byref(on)), "mcl_get_beam_offsets")
        return o, a, bool(on.value)

    def beam_origins(self, poses):
        """(x, y), each (k, B): rule DS2's origin of every beam of the SENSOR poses (3, k), k <= 65536, formed on the device with the
        current table (mcl_beam_origins): bit for bit where the ray stage casts from (a garbage heading -- NaN, |theta| >= 1e6 -- is
        marched literally from here, its walk having no pixel position).  Offsets off: every beam at the pose."""
        p = np.ascontiguousarray(poses, np.float64)
        if p.ndim != 2 or p.shape[0] != 3:
            raise ValueError("poses must be (3, k): the rows x, y, theta")
        out = np.empty((2, p.shape[1], self.n_beams), np.float64)
        self._chk(self.lib.mcl_beam_origins(self._h, _p(p), C.c_int64(p.shape[1]), _p(out)), "mcl_beam_origins")
        return out[0], out[1]

    def _proposal_to_base(self, means, covs):
        """The searches and refinements work in the sensor frame: with a mount set, their means and covariances go to the base frame
        (host_sensor_unmount, host_sensor_mount_cov) before they become a proposal.  No mount: the arrays as they are."""
        m = self.sensor_mount()
        if not m.any():
            return means, covs
        means = np.ascontiguousarray(means, np.float64).reshape(-1, 3)
        covs = np.ascontiguousarray(covs, np.float64).reshape(-1, 3, 3)
        base = host_sensor_unmount(m, means.T).T
        return base, np.stack([host_sensor_mount_cov(m, means[i], covs[i], to_base=True) for i in range(means.shape[0])])

    def update_scan(self, action, ranges, angle_step):
        a, r = _c(action, np.float64), _c(ranges, np.float32)
        self._chk(self.lib.mcl_update_scan(self._h, _p(a), _p(r), C.c_int32(r.size), C.c_int32(angle_step)), "mcl_update_scan")
        self.n = self.particle_count()

    def get_particles(self):
        out = np.empty((3, self.n), np.float64)
        self._chk(self.lib.mcl_get_particles(self._h, _p(out), C.c_int64(self.n)), "mcl_get_particles")
        return out

    def get_weights(self):
        out = np.empty(self.n, np.float64)
        self._chk(self.lib.mcl_get_weights(self._h, _p(out), C.c_int64(self.n)), "mcl_get_weights")
        return out

    def sample_particles(self, k, uniforms=None):
        u = _c(uniforms, np.float64)
        out = np.empty((3, k), np.float64)
        self._chk(self.lib.mcl_sample_particles(self._h, C.c_int32(k), _p(u), _p(out)), "mcl_sample_particles")
        return out

    def particle_mean(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_particle_mean(self._h, _p(out)), "mcl_particle_mean")
        return out

    # -- update
    def update(self, action, obs, normals=None, uniforms=None):
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        nrm, u = _c(normals, np.float64), _c(uniforms, np.float64)
        rows = self.kld_state()[1] if (nrm is not None or u is not None) else self.n    # (KLD on: the size of this update's draw)
        if nrm is not None:
            assert nrm.size == 3 * rows
        if u is not None:
            assert u.size == rows
        self._chk(self.lib.mcl_update(self._h, _p(a), _p(o), C.c_int32(o.size), _p(nrm), _p(u)), "mcl_update")
        self.n = self.particle_count()

    # -- KLD-adaptive particle count (off by default)
    def set_kld(self, on=True, **fields):
        """Switches KLD sampling on with mcl_default_kld_config's values overridden by `fields` (max_particles defaults to the
        smaller of 4194304 and the engine's max_particles), or off (on=False)."""
        if not on:
            self._chk(self.lib.mcl_set_kld(self._h, None), "mcl_set_kld")
            return None
        fields.setdefault("max_particles", min(4194304, int(self.cfg.max_particles)))
        k = default_kld_config(**fields)
        self._chk(self.lib.mcl_set_kld(self._h, C.byref(k)), "mcl_set_kld")
        return k

    def kld_state(self):
        """(bins the last update's draw occupied or -1, children the next update draws)"""
        b, n = C.c_int64(), C.c_int64()
        self._chk(self.lib.mcl_get_kld_state(self._h, C.byref(b), C.byref(n)), "mcl_get_kld_state")
        return b.value, n.value

    # -- recovery by random-particle injection (off by default)
    def set_recovery(self, on=True, **fields):
        """Switches recovery on with mcl_default_recovery_config's values overridden by `fields`, or off (on=False); either way
        the averages start unset."""
        if not on:
            self._chk(self.lib.mcl_set_recovery(self._h, None), "mcl_set_recovery")
            return None
        c = default_recovery_config(**fields)
        self._chk(self.lib.mcl_set_recovery(self._h, C.byref(c)), "mcl_set_recovery")
        return c

    def recovery_state(self):
        """(S, F, p of the next update, children the last update injected); S and F are NaN while unset"""
        st, k = (C.c_double * 3)(), C.c_int64()
        self._chk(self.lib.mcl_get_recovery_state(self._h, st, C.byref(k)), "mcl_get_recovery_state")
        return st[0], st[1], st[2], k.value

    def set_recovery_state(self, S, F):
        """Sets the averages (NaN = unset): restores a saved state, or forces the p of the next update."""
        st = (C.c_double * 2)(S, F)
        self._chk(self.lib.mcl_set_recovery_state(self._h, st), "mcl_set_recovery_state")

    # -- the proposal of an injecting update (sensor resetting)
    def set_recovery_proposal(self, means, covs=None, weights=None):
        """The Gaussian mixture the next injecting update draws its injected children from (mcl_set_recovery_proposal): means
        (M, 3), covs (M, 3, 3), weights (M,) or None for equal ones.  means=None clears it (free cells again).  One shot: the first
        resampling update that injects consumes it."""
        if means is None:
            self._chk(self.lib.mcl_set_recovery_proposal(self._h, C.c_int32(0), None, None, None), "mcl_set_recovery_proposal")
            return
        M, m, c, w = _proposal_arrays(means, covs, weights)
        if M == 0:
            raise ValueError("a proposal needs at least one component (None clears it)")
        self._chk(self.lib.mcl_set_recovery_proposal(self._h, C.c_int32(M), _p(m), _p(c), _p(w) if w is not None else None),
                  "mcl_set_recovery_proposal")

    def recovery_proposal(self):
        """The proposal in place (mcl_get_recovery_proposal): (thresholds, factors) as host_recovery_proposal returns them, or None."""
        n = C.c_int32()
        self._chk(self.lib.mcl_get_recovery_proposal(self._h, C.byref(n), None, None), "mcl_get_recovery_proposal")
        if n.value == 0:
            return None
        thr, fac = np.zeros(n.value, np.uint64), np.zeros((n.value, 9), np.float64)
        self._chk(self.lib.mcl_get_recovery_proposal(self._h, None, _p(thr), _p(fac)), "mcl_get_recovery_proposal")
        return thr, fac

    def propose_from_scan(self, obs, max_hits=16, refine=True, weights="equal", cov=None, refine_fields=None, pruned=False,
                          **search_fields):
        """Sets the proposal from where the scan `obs` fits the map: the search of the sensor model in use (global_search +
        refine_poses with the likelihood field on, else global_search_beam + refine_poses_beam; the model is never switched and an
        error of the search propagates), hits at -inf dropped, one component per hit from the refined mean and covariance.
        refine=False: the hit poses with the covariance `cov` (default: one lattice step, diag((stride_cells res)^2 twice,
        (2 pi / n_headings)^2)).  weights: "equal" (the default: the same update's sensor model ranks the components anyway, and
        with a thousand beams exp(ll - max) gives everything to one hit) or "likelihood" (seed_counts' shares).  No hit left:
        the proposal is cleared.  Returns the hits.  `search_fields` override mcl_default_search_config, `refine_fields`
        mcl_default_refine_config.  pruned=True (likelihood field only): the same hits from global_search_pruned.
            if e.recovery_state()[2] > 0: e.propose_from_scan(scan)
            e.update(action, scan)"""
        if weights not in ("equal", "likelihood"):
            raise ValueError('weights must be "equal" or "likelihood"')
        lf = self.lib.mcl_get_likelihood_table(self._h, None, C.c_size_t(0), None) == MCL_OK
        if pruned and not lf:
            raise EngineError("propose_from_scan: pruned=True needs the likelihood-field model (global_search_pruned)", MCL_ERR_NOT_READY)
        search = self.global_search_pruned if pruned else self.global_search if lf else self.global_search_beam
        hits, _ = search(obs, max_hits=max_hits, **search_fields)
        hits = hits[np.isfinite(hits["log_likelihood"])]
        if hits.size == 0:
            self.set_recovery_proposal(None)
            return hits
        ll = hits["log_likelihood"]
        if refine:
            r, _ = (self.refine_poses if lf else self.refine_poses_beam)(hits["pose"], obs, **(refine_fields or {}))
            means, covs, ll = r["mean"], r["cov"], r["best_log_likelihood"]
        else:
            means = hits["pose"]
            if cov is None:
                sc = default_search_config(**search_fields)
                res = getattr(self, "map_resolution", 0.0)
                cov = np.diag([(sc.stride_cells * res) ** 2, (sc.stride_cells * res) ** 2, (2.0 * np.pi / sc.n_headings) ** 2])
            covs = np.broadcast_to(_c(cov, np.float64).reshape(3, 3), (hits.size, 3, 3))
        w = seed_counts(ll, 1 << 30).astype(np.float64) if weights == "likelihood" else None
        self.set_recovery_proposal(*self._proposal_to_base(means, covs), w)
        return hits

    def propose_from_scans(self, scans, rel, max_hits=16, refine=True, weights="equal", cov=None, refine_fields=None, pruned=True,
                           **search_fields):
        """propose_from_scan over a scan sequence joined by odometry: the hits of global_search_sequence_pruned
        (pruned=False: of global_search_sequence), refined by refine_poses_sequence against the same scans, so that the few
        hypotheses the proposal holds are ranked by every scan and not by the anchor's alone.  Likelihood-field model only
        (MCL_ERR_NOT_READY otherwise; the model is never switched).  propose_from_scan's rules: hits at -inf dropped, one
        component per hit from the refined mean and covariance (refine=False: the hit poses with `cov`, default one lattice
        step), weights "equal" or "likelihood" (seed_counts' shares of the summed scores), the proposal cleared when no hit is
        left.  Returns the hits.
            if e.recovery_state()[2] > 0: e.propose_from_scans(scans, relative_poses(odom))
            e.update(action, scans[-1])"""
        if weights not in ("equal", "likelihood"):
            raise ValueError('weights must be "equal" or "likelihood"')
        if self.lib.mcl_get_likelihood_table(self._h, None, C.c_size_t(0), None) != MCL_OK:
            raise EngineError("propose_from_scans: needs the likelihood-field model (the sequence searches and refine_poses_sequence read its field)",
                              MCL_ERR_NOT_READY)
        search = self.global_search_sequence_pruned if pruned else self.global_search_sequence
        hits, _ = search(scans, rel, max_hits=max_hits, **search_fields)
        hits = hits[np.isfinite(hits["log_likelihood"])]
        if hits.size == 0:
            self.set_recovery_proposal(None)
            return hits
        ll = hits["log_likelihood"]
        if refine:
            r, _ = self.refine_poses_sequence(hits["pose"], scans, rel, **(refine_fields or {}))
            means, covs, ll = r["mean"], r["cov"], r["best_log_likelihood"]
        else:
            means = hits["pose"]
            if cov is None:
                sc = default_search_config(**search_fields)
                res = getattr(self, "map_resolution", 0.0)
                cov = np.diag([(sc.stride_cells * res) ** 2, (sc.stride_cells * res) ** 2, (2.0 * np.pi / sc.n_headings) ** 2])
            covs = np.broadcast_to(_c(cov, np.float64).reshape(3, 3), (hits.size, 3, 3))
        w = seed_counts(ll, 1 << 30).astype(np.float64) if weights == "likelihood" else None
        self.set_recovery_proposal(*self._proposal_to_base(means, covs), w)
        return hits

    # -- likelihood-field sensor model (off by default)
    def set_likelihood_field(self, on=True, **fields):
        """Switches the likelihood-field sensor model on with mcl_default_likelihood_field_config's values (AMCL's) overridden by
        `fields` -- z_hit, z_rand, sigma_hit_m, max_occ_dist_m -- or back to the beam model (on=False)."""
        if not on:
            self._chk(self.lib.mcl_set_likelihood_field(self._h, None), "mcl_set_likelihood_field")
            return None
        c = default_likelihood_field_config(**fields)
        self._chk(self.lib.mcl_set_likelihood_field(self._h, C.byref(c)), "mcl_set_likelihood_field")
        return c

    # -- beam skipping for the likelihood field (off by default)
    def set_beam_skip(self, on=True, **fields):
        """Switches beam skipping on with mcl_default_beam_skip_config's values (AMCL's) overridden by keyword (distance_m,
        threshold, error_threshold), or off.  The likelihood field must be on; switching the field off switches this off too."""
        if not on:
            self._chk(self.lib.mcl_set_beam_skip(self._h, None), "mcl_set_beam_skip")
            return
        c = default_beam_skip_config(**fields)
        self._chk(self.lib.mcl_set_beam_skip(self._h, C.byref(c)), "mcl_set_beam_skip")

    def beam_skip_state(self):
        """What the last update with beam skipping decided (mcl_get_beam_skip_state, rule BS6): the record's fields plus `counts`
        (uint32) and `kept` (uint8: 0 not used, 1 summed, 2 skipped), one entry per beam of the scan."""
        B = int(self.n_beams)
        counts, kept, st = np.zeros(B, np.uint32), np.zeros(B, np.uint8), BeamSkipState()
        self._chk(self.lib.mcl_get_beam_skip_state(self._h, _p(counts), _p(kept), C.c_size_t(B), C.byref(st)), "mcl_get_beam_skip_state")
        out = {name: int(getattr(st, name)) for name, _ in BeamSkipState._fields_}
        out["counts"], out["kept"] = counts, kept
        return out

    def likelihood_field(self):
        """The device's field D of the current map: shape (H, W), uint16."""
        if getattr(self, "map_shape", None) is None:
            raise EngineError("mcl_get_likelihood_field: no map set", MCL_ERR_NOT_READY)
        H, W = self.map_shape
        out = np.empty((H, W), np.uint16)
        self._chk(self.lib.mcl_get_likelihood_field(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_likelihood_field")
        return out

    def likelihood_table(self):
        """The device's table Lf: K + 1 float32 entries."""
        K = C.c_int32()
        self._chk(self.lib.mcl_get_likelihood_table(self._h, None, C.c_size_t(0), C.byref(K)), "mcl_get_likelihood_table")
        out = np.empty(K.value + 1, np.float32)
        self._chk(self.lib.mcl_get_likelihood_table(self._h, _p(out), C.c_size_t(out.size), None), "mcl_get_likelihood_table")
        return out

    # -- the tables under the ray stage, as stored on the device (read-only; tests/test_gpu_ray_tables.py)
    def wedge_fields(self):
        """The wedge fields mcl_set_map built: (WEDGES, Hp, Wps) uint8 in the stored encoding, padding columns included; the
        padded grid is [:, :, :Wp] with Wp = map width + 1."""
        dims = (C.c_int32 * 3)()
        self._chk(self.lib.mcl_get_wedge_fields(self._h, None, C.c_size_t(0), dims), "mcl_get_wedge_fields")
        out = np.empty((WEDGES, dims[0], dims[2]), np.uint8)
        self._chk(self.lib.mcl_get_wedge_fields(self._h, _p(out), C.c_size_t(out.size), None), "mcl_get_wedge_fields")
        return out

    def ring_fields(self):
        """The mirrored, ringed copies of the wedge fields (the global-field and hybrid forms), the whole allocation of
        host_sweep_global_layout as a flat uint8 array; EngineError NOT_READY on an engine that holds none."""
        if getattr(self, "map_shape", None) is None:
            raise EngineError("mcl_get_ring_fields: no map set", MCL_ERR_NOT_READY)
        H, W = self.map_shape
        out = np.empty(max(host_sweep_global_layout(W, H, self.max_range_px)["alloc"], 1), np.uint8)
        self._chk(self.lib.mcl_get_ring_fields(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_ring_fields")
        return out

    def sweep_table(self):
        """((rows, cols) float64, beam_margin): the fp64 table of the last scan as RAYS_SWEEP's ray stage used it."""
        dims = (C.c_int32 * 3)()
        self._chk(self.lib.mcl_get_sweep_table(self._h, None, C.c_size_t(0), dims), "mcl_get_sweep_table")
        out = np.empty((dims[0], dims[1]), np.float64)
        self._chk(self.lib.mcl_get_sweep_table(self._h, _p(out), C.c_size_t(out.size), None), "mcl_get_sweep_table")
        return out, int(dims[2])

    def sort_order(self):
        """The order of the last update's ray stage (radix ordering path): dict(keys, perm, bbox, tilemap, n, fine, fine_sub) -- the
        sorted keys and the particle index per slot, the layout words and tile map the keys were made from (tilemap None for a map
        of more than 8192 tiles), the fine bits of the keys and how many of them per axis are sub-cell bits (None: the rule's).  EngineError NOT_READY when the last ray stage did not order that way."""
        n, fine = C.c_int64(), C.c_int32()
        self._chk(self.lib.mcl_get_sort_order(self._h, None, None, C.c_size_t(0), None, None, C.c_size_t(0), C.byref(n), C.byref(fine)),
                  "mcl_get_sort_order")
        keys, perm, bbox = np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), np.empty(7, np.int32)
        H, W = self.map_shape
        ntx, nty = sort_tile_grid(W, H)
        tm = np.empty(ntx * nty, np.int32) if ntx * nty <= 8192 else None
        self._chk(self.lib.mcl_get_sort_order(self._h, _p(keys), _p(perm), C.c_size_t(n.value), _p(bbox), _p(tm) if tm is not None else None,
                                              C.c_size_t(tm.size if tm is not None else 0), None, None), "mcl_get_sort_order")
        return dict(keys=keys, perm=perm, bbox=bbox, tilemap=tm, n=int(n.value), fine=int(fine.value) & 15,
                    fine_sub=(int(fine.value) >> 4) - 1 if int(fine.value) >> 4 else None)

    def sort_record_form(self) -> str:
        """'heading' when the gather of the last update's radix ordering read (heading, 0, px, py) records the resampling kernel had
        left and took the sincos itself, 'full' when it read (cos, sin, px, py) beside the heading column (mcl_get_sort_record_form)."""
        f = C.c_int32()
        self._chk(self.lib.mcl_get_sort_record_form(self._h, C.byref(f)), "mcl_get_sort_record_form")
        return "heading" if f.value else "full"

    def particle_count(self) -> int:
        n = C.c_int64()
        self._chk(self.lib.mcl_get_particle_count(self._h, C.byref(n)), "mcl_get_particle_count")
        return n.value

    def pose_clusters(self, max_clusters=16, **cfg_fields):
        """The pose hypotheses of the particle set (mcl_pose_clusters): a structured array (CLUSTER_DTYPE) of the
        max_clusters heaviest clusters, heaviest first, and {n_clusters, q_total, q_outside, n_outside}.  `cfg_fields` override
        mcl_default_cluster_config (bin_x_m, bin_y_m, n_theta_bins)."""
        cfg = default_cluster_config(**cfg_fields)
        out = np.zeros(int(max_clusters), CLUSTER_DTYPE)
        n = C.c_int64()
        tot = (C.c_uint64 * 3)()
        self._chk(self.lib.mcl_pose_clusters(self._h, C.byref(cfg), C.c_int32(int(max_clusters)), _p(out) if out.size else None,
                                             C.byref(n), tot), "mcl_pose_clusters")
        return out[:min(n.value, out.size)], dict(n_clusters=n.value, q_total=int(tot[0]), q_outside=int(tot[1]), n_outside=int(tot[2]))

    def cluster_labels(self):
        """Per particle, the rank of its cluster in the last pose_clusters, or -1 (no cluster)."""
        out = np.empty(self.particle_count(), np.int32)
        self._chk(self.lib.mcl_get_cluster_labels(self._h, _p(out), C.c_int64(out.size)), "mcl_get_cluster_labels")
        return out

    @staticmethod
    def _query_poses(poses):
        """(K, 3) poses, or one length-3 pose, as the K x 3 column-major array the ABI takes"""
        p = np.asarray(poses, np.float64)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("poses must be (K, 3) or a single (x, y, theta)")
        return _c(p.T, np.float64)

    def expected_scans(self, poses, want_steps=False):
        """The expected scan of every pose (mcl_query_scans): the ranges in metres of the beams last set, a
        (K, B) float32 array -- what a particle at that pose would see -- and, with want_steps, the step indices (uint16) too.
        `poses`: (K, 3) rows of (x, y, theta), or one pose.  Reads the map and the beams only: the particle set is untouched."""
        p = self._query_poses(poses)
        K = p.shape[1]
        ranges = np.empty((K, self.n_beams), np.float32)
        steps = np.empty((K, self.n_beams), np.uint16) if want_steps else None
        self._chk(self.lib.mcl_query_scans(self._h, _p(p) if K else None, C.c_int32(K), _p(ranges),
                                           _p(steps) if want_steps else None), "mcl_query_scans")
        return (ranges, steps) if want_steps else ranges

    def score_poses(self, poses, obs, tol_steps=2):
        """How well the scan `obs` supports every pose (mcl_score_poses): a structured array (POSE_SCORE_DTYPE) with the
        log-likelihood a particle at that pose would get from sensor_update(obs) under the engine's sensor model, and the beams
        that are valid / agree with the cast ray within tol_steps / hit nothing in range.  weight_mode LOG only."""
        p = self._query_poses(poses)
        K = p.shape[1]
        o = _c(obs, np.float32)
        out = np.zeros(K, POSE_SCORE_DTYPE)
        self._chk(self.lib.mcl_score_poses(self._h, _p(p) if K else None, C.c_int32(K), _p(o), C.c_int32(o.size),
                                           C.c_int32(int(tol_steps)), _p(out)), "mcl_score_poses")
        return out

    def query_counters(self):
        out = np.zeros(2, np.uint64)
        self._chk(self.lib.mcl_get_query_counters(self._h, _p(out)), "mcl_get_query_counters")
        return dict(level3_rays=int(out[0]), device_bytes=int(out[1]))

    # -- global search (the likelihood-field model must be on)
    def global_search(self, obs, max_hits=16, **fields):
        """Scores every pose of a lattice over the map's free cells against the scan `obs` and reports the best-fitting ones
        (mcl_global_search): a structured array (SEARCH_HIT_DTYPE: pose, log_likelihood, index) of at most max_hits hits, best
        first, and {n_hits, n_positions, n_poses, used_beams, device_bytes}.  `fields` override mcl_default_search_config
        (stride_cells, n_headings, beam_stride, nms).  Reads the map, the beams and the likelihood field only."""
        c = default_search_config(**fields)
        o = _c(obs, np.float32)
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(4, np.uint64)
        self._chk(self.lib.mcl_global_search(self._h, C.byref(c), _p(o), C.c_int32(o.size), C.c_int32(int(max_hits)),
                                             _p(hits) if hits.size else None, C.byref(n), _p(st)), "mcl_global_search")
        self._search_poses = int(st[1])
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]))

    def global_search_pruned(self, obs, max_hits=16, block=0, first_pairs=0, prune_reserved=(0, 0, 0, 0, 0, 0), **fields):
        """global_search's hits from the blocks of poses an upper bound cannot rule out (mcl_global_search_pruned):
        the same structured array, bit for bit, without the score volume.  block: lattice positions per block side (2, 4 or 8; 0:
        the default), first_pairs: the (block, heading) pairs the first round scores (0: the default).  n_hits is the number of
        hits written, not the candidates of the volume.  Returns (hits, {n_hits, n_positions, n_poses, used_beams, device_bytes,
        pairs, pairs_scored, rounds, guard_fallbacks})."""
        c, pc = default_search_config(**fields), search_prune_config(block, first_pairs, prune_reserved)
        o = _c(obs, np.float32)
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(8, np.uint64)
        self._chk(self.lib.mcl_global_search_pruned(self._h, C.byref(c), C.byref(pc), _p(o), C.c_int32(o.size), C.c_int32(int(max_hits)),
                                                    _p(hits) if hits.size else None, C.byref(n), _p(st)), "mcl_global_search_pruned")
        self._search_pairs = int(st[4])
        return hits[:n.value], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                    device_bytes=int(st[3]), pairs=int(st[4]), pairs_scored=int(st[5]), rounds=int(st[6]),
                                    guard_fallbacks=int(st[7]))

    def global_search_sequence_pruned(self, scans, rel, max_hits=16, block=0, first_pairs=0, prune_reserved=(0, 0, 0, 0, 0, 0), **fields):
        """global_search_sequence's hits from the blocks of poses an upper bound on the summed score cannot rule out
        (mcl_global_search_sequence_pruned): the same structured array, bit for bit, without the score volume.
        `scans`: (S, B) ranges; `rel`: (S, 3) rows of (dx, dy, dtheta); block and first_pairs as in global_search_pruned.  Returns
        (hits, {global_search_pruned's keys, n_scans}); used_beams counts all scans' beams."""
        o, r = np.asarray(scans, np.float32), np.asarray(rel, np.float64)
        if o.ndim != 2:
            raise ValueError("scans must be (S, B)")
        if r.ndim != 2 or r.shape[1] != 3 or r.shape[0] != o.shape[0]:
            raise ValueError("rel must be (S, 3), one row per scan")
        o, r = _c(o, np.float32), _c(r, np.float64)
        c, pc = default_search_config(**fields), search_prune_config(block, first_pairs, prune_reserved)
        S = o.shape[0]
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(9, np.uint64)
        self._chk(self.lib.mcl_global_search_sequence_pruned(self._h, C.byref(c), C.byref(pc), _p(o) if S else None, _p(r) if S else None,
                                                             C.c_int32(S), C.c_int32(o.shape[1]), C.c_int32(int(max_hits)),
                                                             _p(hits) if hits.size else None, C.byref(n), _p(st)),
                  "mcl_global_search_sequence_pruned")
        self._search_pairs = int(st[4])
        return hits[:n.value], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                    device_bytes=int(st[3]), pairs=int(st[4]), pairs_scored=int(st[5]), rounds=int(st[6]),
                                    guard_fallbacks=int(st[7]), n_scans=int(st[8]))

    def search_bounds(self):
        """The bounds U of the last global_search_pruned or global_search_sequence_pruned (mcl_get_search_bounds): one double per (block, heading) pair, pair =
        k * n_blocks + b in host_search_blocks' order.  Raises before a pruned search and after set_map."""
        out = np.empty(getattr(self, "_search_pairs", 0) or 1, np.float64)
        self._chk(self.lib.mcl_get_search_bounds(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_search_bounds")
        return out

    def global_search_sequence(self, scans, rel, max_hits=16, **fields):
        """global_search over a sequence of scans joined by odometry (mcl_global_search_sequence): every lattice
        pose is the robot's pose at the anchor, and scan s is scored from where that pose puts the robot at scan s.  `scans`:
        (S, B) ranges; `rel`: (S, 3) rows of (dx, dy, dtheta), the pose at scan s in the anchor's frame (relative_poses makes
        them from odometry).  Returns what global_search returns, plus n_scans; used_beams counts all scans' beams.
            rel = relative_poses(odom)
            hits, _ = e.global_search_sequence(scans, rel)
            r, _ = e.refine_poses_sequence(hits["pose"], scans, rel)"""
        c = default_search_config(**fields)
        o = _c(np.atleast_2d(np.asarray(scans, np.float32)), np.float32)
        if o.ndim != 2:
            raise ValueError("scans must be (S, B)")
        r = _rel_rows(rel)
        if r.shape[0] != o.shape[0]:
            raise ValueError("scans and rel must have one row per scan")
        S = o.shape[0]
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(5, np.uint64)
        self._chk(self.lib.mcl_global_search_sequence(self._h, C.byref(c), _p(o) if S else None, _p(r) if S else None, C.c_int32(S),
                                                      C.c_int32(o.shape[1]), C.c_int32(int(max_hits)),
                                                      _p(hits) if hits.size else None, C.byref(n), _p(st)),
                  "mcl_global_search_sequence")
        self._search_poses = int(st[1])
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]), n_scans=int(st[4]))

    def global_search_streamed(self, scans, rel=None, max_hits=16, budget_bytes=0, slab_headings=0, stream_reserved=(0, 0, 0, 0, 0),
                               **fields):
        """global_search (one scan, rel None) or global_search_sequence in slabs of headings (mcl_global_search_streamed, DESIGN.md
        §4.16): the same hits, bit for bit, from at most `budget_bytes` of slab buffers (0: 1 GiB), for lattices of up to 2^40
        poses.  slab_headings = 0 takes the largest slab that fits.  Keeps no volume (search_scores raises afterwards).  Returns
        (hits, {n_hits, n_positions, n_poses, used_beams, device_bytes, slab_headings, n_slabs, headings_scored,
        candidates_compacted})."""
        c = default_search_config(**fields)
        sc = search_stream_config(budget_bytes, slab_headings, stream_reserved)
        o = _c(np.atleast_2d(np.asarray(scans, np.float32)), np.float32)
        if o.ndim != 2:
            raise ValueError("scans must be (B,) or (S, B)")
        S = o.shape[0]
        r = None
        if rel is not None:
            r = _rel_rows(rel)
            if r.shape[0] != S:
                raise ValueError("scans and rel must have one row per scan")
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(8, np.uint64)
        self._chk(self.lib.mcl_global_search_streamed(self._h, C.byref(c), C.byref(sc), _p(o) if o.size else None,
                                                      _p(r) if r is not None and r.size else None, C.c_int32(S), C.c_int32(o.shape[1]),
                                                      C.c_int32(int(max_hits)), _p(hits) if hits.size else None, C.byref(n), _p(st)),
                  "mcl_global_search_streamed")
        self._search_poses = 0
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]), slab_headings=int(st[4]), n_slabs=int(st[5]),
                                                    headings_scored=int(st[6]), candidates_compacted=int(st[7]))

    def global_search_beam(self, obs, max_hits=16, table_budget_bytes=0, **fields):
        """global_search under the beam model (mcl_global_search_beam): the lattice ranked by the table sum over
        cast rays that every update weights particles with, from a per-position ray table shared by all headings.  The scan must
        be evenly spaced and n_headings must divide its angle grid (host_search_beam_grid).  The likelihood field may be on or
        off.  `table_budget_bytes` (0: 256 MiB) bounds the table: the lattice is walked in tiles of positions.  Returns (hits,
        {n_hits, n_positions, n_poses, used_beams, device_bytes, grid_angles, tile_positions, n_tiles, level3_rays})."""
        c = default_search_config(**fields)
        o = _c(obs, np.float32)
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(8, np.uint64)
        self._chk(self.lib.mcl_global_search_beam(self._h, C.byref(c), _p(o), C.c_int32(o.size), C.c_uint64(int(table_budget_bytes)),
                                                  C.c_int32(int(max_hits)), _p(hits) if hits.size else None, C.byref(n), _p(st)),
                  "mcl_global_search_beam")
        self._search_poses, self._search_beam_M = int(st[1]), int(st[4])
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]), grid_angles=int(st[4]), tile_positions=int(st[5]),
                                                    n_tiles=int(st[6]), level3_rays=int(st[7]))

    def search_beam_table(self):
        """The ray table of the last tile of the last global_search_beam (mcl_get_search_beam_table): (first_position, steps) with
        steps of shape (n_positions_of_the_tile, M), uint16 -- E3's step from each position at each grid angle.  M is the
        grid_angles this object's last global_search_beam reported (the C call takes the size and checks it)."""
        first, cnt = C.c_int64(), C.c_int64()
        self._chk(self.lib.mcl_get_search_beam_table(self._h, None, 0, C.byref(first), C.byref(cnt)), "mcl_get_search_beam_table")
        M = getattr(self, "_search_beam_M", 0)
        out = np.empty(cnt.value * M, np.uint16)
        self._chk(self.lib.mcl_get_search_beam_table(self._h, _p(out), C.c_size_t(out.size), None, None), "mcl_get_search_beam_table")
        return int(first.value), out.reshape(cnt.value, M)

    def search_scores(self, n_headings=None):
        """The score volume of the last global_search or global_search_sequence (mcl_get_search_scores): n_headings * n_positions doubles, heading-major;
        with n_headings, reshaped to (n_headings, n_positions)."""
        out = np.empty(getattr(self, "_search_poses", 0) or 1, np.float64)
        self._chk(self.lib.mcl_get_search_scores(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_search_scores")
        return out.reshape(int(n_headings), -1) if n_headings else out

    def search_bytes(self) -> int:
        """Bytes of device memory the search's buffers have asked for so far (0 on an engine that never searched)."""
        v = C.c_uint64()
        self._chk(self.lib.mcl_get_search_bytes(self._h, C.byref(v)), "mcl_get_search_bytes")
        return int(v.value)

    # -- pose refinement (the likelihood-field model must be on)
    def refine_poses(self, poses, obs, **fields):
        """Scores a dense window of poses around every seed pose against the scan `obs` (mcl_refine_poses): a structured array
        (REFINE_DTYPE: best, best_log_likelihood, seed_log_likelihood, best_index, mean, cov, weight_sum), one record per seed, and
        {n_win, n_poses, used_beams, device_bytes}.  `poses`: (M, 3) rows of (x, y, theta), or one pose -- the hits of global_search,
        cluster means, an /initialpose.  `fields` override mcl_default_refine_config (half_xy, half_theta, step_xy_cells,
        step_theta_rad, beam_stride).  Reads the beams and the likelihood field only.  The chain from one scan to a cloud:
            hits, _ = e.global_search(obs)
            r, _ = e.refine_poses(hits["pose"], obs)
            e.init_particles_mixture(r["mean"], r["cov"], seed_counts(r["best_log_likelihood"], n))"""
        c = default_refine_config(**fields)
        p = self._query_poses(poses)
        M = p.shape[1]
        o = _c(obs, np.float32)
        out = np.zeros(M, REFINE_DTYPE)
        st = np.zeros(4, np.uint64)
        self._chk(self.lib.mcl_refine_poses(self._h, C.byref(c), _p(p) if M else None, C.c_int32(M), _p(o), C.c_int32(o.size),
                                            _p(out) if M else None, _p(st)), "mcl_refine_poses")
        self._refine_shape = (M, int(st[0]))
        return out, dict(n_win=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]), device_bytes=int(st[3]))

    def refine_poses_beam(self, poses, obs, **fields):
        """refine_poses under the beam model (mcl_refine_poses_beam): the same window, every pose scored by the
        table sum over cast rays that every update weights particles with -- what score_poses returns with the likelihood field
        off -- in one kernel that stores no ray.  The likelihood field may be on or off.  Returns (records, {n_win, n_poses,
        used_beams, device_bytes, rays, level3_rays}).  The chain from one scan to a cloud, under one model:
            hits, _ = e.global_search_beam(obs, beam_stride=10)
            r, _ = e.refine_poses_beam(hits["pose"], obs)
            e.init_particles_mixture(r["mean"], r["cov"], seed_counts(r["best_log_likelihood"], n))"""
        c = default_refine_config(**fields)
        p = self._query_poses(poses)
        M = p.shape[1]
        o = _c(obs, np.float32)
        out = np.zeros(M, REFINE_DTYPE)
        st = np.zeros(6, np.uint64)
        self._chk(self.lib.mcl_refine_poses_beam(self._h, C.byref(c), _p(p) if M else None, C.c_int32(M), _p(o), C.c_int32(o.size),
                                                 _p(out) if M else None, _p(st)), "mcl_refine_poses_beam")
        self._refine_shape = (M, int(st[0]))
        return out, dict(n_win=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]), device_bytes=int(st[3]), rays=int(st[4]),
                         level3_rays=int(st[5]))

    def refine_poses_sequence(self, poses, scans, rel, **fields):
        """refine_poses against a sequence of scans joined by odometry (mcl_refine_poses_sequence): every seed and
        every window pose is the robot's pose at the anchor, and scan s is scored from where that pose puts the robot at scan s,
        so the records keep the ranking of the sequence search that made the seeds.  `scans`: (S, B) ranges; `rel`: (S, 3) rows
        of (dx, dy, dtheta), the pose at scan s in the anchor's frame (relative_poses makes them from odometry).  Returns
        (records, {refine_poses' keys, n_scans}); used_beams counts all scans' beams, the log-likelihoods are summed scores.
            rel = relative_poses(odom)
            hits, _ = e.global_search_sequence_pruned(scans, rel)
            r, _ = e.refine_poses_sequence(hits["pose"], scans, rel)
            e.init_particles_mixture(r["mean"], r["cov"], seed_counts(r["best_log_likelihood"], n))"""
        c = default_refine_config(**fields)
        p = self._query_poses(poses)
        M = p.shape[1]
        o = _c(np.atleast_2d(np.asarray(scans, np.float32)), np.float32)
        if o.ndim != 2:
            raise ValueError("scans must be (S, B)")
        r = _rel_rows(rel)
        if r.shape[0] != o.shape[0]:
            raise ValueError("scans and rel must have one row per scan")
        S = o.shape[0]
        out = np.zeros(M, REFINE_DTYPE)
        st = np.zeros(5, np.uint64)
        self._chk(self.lib.mcl_refine_poses_sequence(self._h, C.byref(c), _p(p) if M else None, C.c_int32(M), _p(o) if o.size else None,
                                                     _p(r) if S else None, C.c_int32(S), C.c_int32(o.shape[1]),
                                                     _p(out) if M else None, _p(st)), "mcl_refine_poses_sequence")
        self._refine_shape = (M, int(st[0]))
        return out, dict(n_win=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]), device_bytes=int(st[3]), n_scans=int(st[4]))

    def refine_scores(self):
        """The score volume of the last refine_poses, refine_poses_beam or refine_poses_sequence (mcl_get_refine_scores): (M, n_win)
        doubles, window index ix fastest."""
        shape = getattr(self, "_refine_shape", None) or (1, 1)
        out = np.empty(shape, np.float64)
        self._chk(self.lib.mcl_get_refine_scores(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_refine_scores")
        return out

    def refine_bytes(self) -> int:
        """Bytes of device memory the refinement's buffers have asked for so far (0 on an engine that never refined)."""
        v = C.c_uint64()
        self._chk(self.lib.mcl_get_refine_bytes(self._h, C.byref(v)), "mcl_get_refine_bytes")
        return int(v.value)

    def sensor_update(self, obs):
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_sensor_update(self._h, _p(o), C.c_int32(o.size)), "mcl_sensor_update")

    def expected_pose(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_expected_pose(self._h, _p(out)), "mcl_expected_pose")
        return out

    def stage_timings(self):
        out = np.empty(6)
        self._chk(self.lib.mcl_get_stage_timings(self._h, _p(out)), "mcl_get_stage_timings")
        return out

    # -- diagnostics
    def resample_indices(self):
        out = np.empty(self.n, np.int32)
        self._chk(self.lib.mcl_get_resample_indices(self._h, _p(out), C.c_int64(self.n)), "mcl_get_resample_indices")
        return out

    def ray_steps(self):
        """Step index of every ray of the last update (needs keep_ray_steps): uint8 up to 255 px of range, uint16 beyond."""
        if self.max_range_px > 255:
            out = np.empty(self.n * self.n_beams, np.uint16)
            self._chk(self.lib.mcl_get_ray_steps16(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_ray_steps16")
        else:
            out = np.empty(self.n * self.n_beams, np.uint8)
            self._chk(self.lib.mcl_get_ray_steps(self._h, _p(out), C.c_size_t(out.size)), "mcl_get_ray_steps")
        return out.reshape(self.n, self.n_beams)

    def log_weights(self):
        out = np.empty(self.n, np.float64)
        self._chk(self.lib.mcl_get_log_weights(self._h, _p(out), C.c_int64(self.n)), "mcl_get_log_weights")
        return out

    def counters(self):
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.mcl_get_counters(self._h, _p(out)), "mcl_get_counters")
        return dict(exact_fallback_rays=int(out[0]), off_window_particles=int(out[1]), probes=int(out[2]),
                    level2_rays=int(out[3]))

    def compact_list(self):
        """(entries of the compact parent list that describes the current weights or -1, whether the last resampling used one)"""
        n, u = C.c_int64(), C.c_int32()
        self._chk(self.lib.mcl_get_compact_list(self._h, C.byref(n), C.byref(u)), "mcl_get_compact_list")
        return n.value, bool(u.value)

    def compact_guide(self):
        """mcl_get_compact_guide: the guide of the compact parent list as the device holds it, a dict of guide (bmax + 1 uint32
        words), ccdf (the list's uint64 CDF column), s, bmax, n_compact, q_total, m and used (the last update's resampling
        searched through the guide).  EngineError (NOT_READY) without a list or a guide."""
        info = np.zeros(6, np.int64)
        self._chk(self.lib.mcl_get_compact_guide(self._h, None, C.c_size_t(0), None, C.c_size_t(0), _p(info)), "mcl_get_compact_guide")
        if info[1] < 0:
            raise EngineError("mcl_get_compact_guide: no compact list with a guide describes the current particles", MCL_ERR_NOT_READY)
        guide, ccdf = np.empty(int(info[1]) + 1, np.uint32), np.empty(int(info[2]), np.uint64)
        self._chk(self.lib.mcl_get_compact_guide(self._h, _p(guide), C.c_size_t(guide.size), _p(ccdf), C.c_size_t(ccdf.size), _p(info)),
                  "mcl_get_compact_guide")
        return dict(guide=guide, ccdf=ccdf, s=int(info[0]), bmax=int(info[1]), n_compact=int(info[2]), q_total=int(np.uint64(info[3])),
                    m=int(info[4]), used=bool(info[5]))

    def compact_guide_used(self) -> bool:
        """whether the last update's resampling searched the compact list through its guide (mcl_get_compact_guide)"""
        info = np.zeros(6, np.int64)
        self._chk(self.lib.mcl_get_compact_guide(self._h, None, C.c_size_t(0), None, C.c_size_t(0), _p(info)), "mcl_get_compact_guide")
        return bool(info[5])

    def set_debug_count_probes(self, on):
        self._chk(self.lib.mcl_set_debug_count_probes(self._h, C.c_int32(1 if on else 0)), "mcl_set_debug_count_probes")

    def set_debug_force_exact(self, level):
        self._chk(self.lib.mcl_set_debug_force_exact(self._h, C.c_int32(int(level))), "mcl_set_debug_force_exact")

    def ray_kernel_ms(self):
        v = C.c_double()
        self._chk(self.lib.mcl_get_ray_kernel_ms(self._h, C.byref(v)), "mcl_get_ray_kernel_ms")
        return v.value

    def effective_sample_size(self):
        """(N_eff of the current weights, whether the last update resampled)"""
        v, r = C.c_double(), C.c_int32()
        self._chk(self.lib.mcl_get_effective_sample_size(self._h, C.byref(v), C.byref(r)), "mcl_get_effective_sample_size")
        return v.value, bool(r.value)

    def ray_kernel_id(self):
        """The MCL_RAYS_* enumerator of the kernel the last ray stage ran (mcl_get_ray_kernel_id; 0: none yet)."""
        v = C.c_int32()
        self._chk(self.lib.mcl_get_ray_kernel_id(self._h, C.byref(v)), "mcl_get_ray_kernel_id")
        return v.value

    def ray_kernel_name(self):
        return {1: "k_rays_march", 2: "k_rays_skip", 3: "k_rays_quad", 4: "k_rays_cell", 5: "k_rays_sweep", 6: "k_rays_deskew"}.get(self.ray_kernel_id(), "?")

    def ray_kernel_variant(self):
        """Form of k_rays_sweep the last ray stage ran: dict(global_fields, hybrid, turned_directions, pairs)."""
        v = (C.c_int32 * 3)()
        self._chk(self.lib.mcl_get_ray_kernel_variant(self._h, v), "mcl_get_ray_kernel_variant")
        return dict(global_fields=v[0] == 1, hybrid=v[0] == 2, turned_directions=bool(v[1]), pairs=bool(v[2]))

    RAY_KERNEL_NAMES = {0: None, 1: "k_rays_march", 2: "k_rays_skip", 3: "k_rays_quad", 4: "k_rays_cell", 5: "k_rays_sweep", 6: "k_rays_deskew"}

    def planned_ray_kernel(self, n_particles=0):
        """(kernel an update over n_particles WILL run -- None: the configured one cannot run with this map / beam set --, what
        decided): callable before the first update, once the map and the beam angles are set."""
        v, why = C.c_int32(), C.c_char_p()
        self._chk(self.lib.mcl_get_planned_ray_kernel(self._h, C.c_int64(int(n_particles)), C.byref(v), C.byref(why)), "mcl_get_planned_ray_kernel")
        return self.RAY_KERNEL_NAMES.get(v.value, "?"), (why.value or b"").decode()

    # -- multi-GPU staging (raw device pointers as ints)
    def device_ptr(self, which) -> int:
        p = C.c_void_p()
        self._chk(self.lib.mcl_device_ptr(self._h, C.c_int32(which), C.byref(p)), "mcl_device_ptr")
        return int(p.value or 0)

    def export_state(self, d_x=0, d_y=0, d_th=0, d_q=0):
        self._chk(self.lib.mcl_export_state(self._h, C.c_void_p(d_x or None), C.c_void_p(d_y or None),
                                            C.c_void_p(d_th or None), C.c_void_p(d_q or None)), "mcl_export_state")

    def scalars(self):
        out = np.empty(8)
        self._chk(self.lib.mcl_get_scalars(self._h, _p(out)), "mcl_get_scalars")
        return out

    def host_scalars(self):
        """SCALARS as the last stage call read them back (no device access)."""
        out = np.empty(8)
        self._chk(self.lib.mcl_get_host_scalars(self._h, _p(out)), "mcl_get_host_scalars")
        return out

    def stage_propagate(self, d_px, d_py, d_pth, d_cdf, n_parents, q_total, child_first, n_children_total, action, obs):
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_stage_propagate(self._h, C.c_void_p(d_px), C.c_void_p(d_py), C.c_void_p(d_pth),
                                               C.c_void_p(d_cdf), C.c_int64(n_parents), C.c_uint64(q_total),
                                               C.c_int64(child_first), C.c_int64(n_children_total), _p(a), _p(o),
                                               C.c_int32(o.size)), "mcl_stage_propagate")

    def stage_resample(self, d_px, d_py, d_pth, d_cdf, n_parents, q_total, child_first, n_children_total, action):
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_resample(self._h, C.c_void_p(d_px), C.c_void_p(d_py), C.c_void_p(d_pth),
                                              C.c_void_p(d_cdf), C.c_int64(n_parents), C.c_uint64(q_total),
                                              C.c_int64(child_first), C.c_int64(n_children_total), _p(a)), "mcl_stage_resample")

    def export_records(self, d_records):
        self._chk(self.lib.mcl_export_records(self._h, C.c_void_p(d_records)), "mcl_export_records")

    def stage_resample_records(self, d_records, d_cdf, n_parents, q_total, child_first, n_children_total, action):
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_resample_records(self._h, C.c_void_p(d_records), C.c_void_p(d_cdf), C.c_int64(n_parents),
                                                      C.c_uint64(q_total), C.c_int64(child_first), C.c_int64(n_children_total), _p(a)),
                  "mcl_stage_resample_records")

    def stage_resample_indices(self, d_cdf, n_parents, q_total, child_first, n_children_total, d_parent_idx):
        self._chk(self.lib.mcl_stage_resample_indices(self._h, C.c_void_p(d_cdf), C.c_int64(n_parents), C.c_uint64(q_total),
                                                      C.c_int64(child_first), C.c_int64(n_children_total), C.c_void_p(d_parent_idx)),
                  "mcl_stage_resample_indices")

    def stage_distinct_parents(self, d_parent, n_children, n_total, d_distinct, d_slot) -> int:
        """Distinct parents (ascending) of `n_children` global parent indices + every child's position among them; returns
        their number.  All pointers are device memory (int32 in, int64 / int32 out)."""
        cnt = C.c_int64(0)
        self._chk(self.lib.mcl_stage_distinct_parents(self._h, C.c_void_p(d_parent), C.c_int64(n_children), C.c_int64(n_total),
                                                      C.c_void_p(d_distinct), C.c_void_p(d_slot), C.byref(cnt)), "mcl_stage_distinct_parents")
        return int(cnt.value)

    def export_records_at(self, d_index, count, d_out):
        """Packed records of the listed local particles (device int64 indices) -> d_out[count] (device)."""
        self._chk(self.lib.mcl_export_records_at(self._h, C.c_void_p(d_index), C.c_int64(count), C.c_void_p(d_out)), "mcl_export_records_at")

    def stage_motion_records(self, d_records, n_records, d_record_of_child, child_first, n_children_total, action):
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_motion_records(self._h, C.c_void_p(d_records), C.c_int64(n_records), C.c_void_p(d_record_of_child),
                                                    C.c_int64(child_first), C.c_int64(n_children_total), _p(a)), "mcl_stage_motion_records")

    @staticmethod
    def compact_chunk_bytes(chunk_entries) -> int:
        b = C.c_int64()
        rc = load_library().mcl_compact_chunk_bytes(C.c_int64(chunk_entries), C.byref(b))
        if rc != MCL_OK:
            raise EngineError(f"mcl_compact_chunk_bytes rc={rc}")
        return b.value

    def export_compact(self, d_chunk, chunk_entries):
        """This shard's compact parent list -> d_chunk (device memory of compact_chunk_bytes(chunk_entries))."""
        self._chk(self.lib.mcl_export_compact(self._h, C.c_void_p(d_chunk), C.c_int64(chunk_entries)), "mcl_export_compact")

    def stage_resample_compact(self, d_chunks, n_shards, chunk_entries, counts, totals, n_per_shard, self_shard, child_first, n_children_total, action):
        a = _c(action, np.float64)
        c = np.ascontiguousarray(np.asarray(counts, np.int64))
        t = np.ascontiguousarray(np.asarray(totals, np.uint64))
        assert c.size == n_shards and t.size == n_shards
        self._chk(self.lib.mcl_stage_resample_compact(self._h, C.c_void_p(d_chunks), C.c_int32(n_shards), C.c_int64(chunk_entries), _p(c), _p(t),
                                                      C.c_int64(n_per_shard), C.c_int32(self_shard), C.c_int64(child_first),
                                                      C.c_int64(n_children_total), _p(a)), "mcl_stage_resample_compact")

    def stage_rays(self, obs):
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_stage_rays(self._h, _p(o), C.c_int32(o.size)), "mcl_stage_rays")

    def set_reserved_cus(self, n):
        self._chk(self.lib.mcl_set_reserved_cus(self._h, C.c_int32(n)), "mcl_set_reserved_cus")

    def stage_weights(self, global_max):
        self._chk(self.lib.mcl_stage_weights(self._h, C.c_double(global_max)), "mcl_stage_weights")

    def stage_finish(self, sums5):
        s = _c(sums5, np.float64)
        self._chk(self.lib.mcl_stage_finish(self._h, _p(s)), "mcl_stage_finish")

    # ---- the staged flow ordered on the device (include/mcl_hip_engine.h: "ORDERED ON THE DEVICE"): nothing here waits for the
    # stream except stage_complete; `stream` is a raw hipStream_t (torch.cuda.current_stream().cuda_stream)
    def stream_wait_external(self, stream):
        self._chk(self.lib.mcl_stream_wait_external(self._h, C.c_void_p(stream)), "mcl_stream_wait_external")

    def external_wait_stream(self, stream):
        self._chk(self.lib.mcl_external_wait_stream(self._h, C.c_void_p(stream)), "mcl_external_wait_stream")

    def export_compact_async(self, d_chunk, chunk_entries):
        self._chk(self.lib.mcl_export_compact_async(self._h, C.c_void_p(d_chunk), C.c_int64(chunk_entries)), "mcl_export_compact_async")

    def stage_resample_compact_async(self, d_chunks, n_shards, chunk_entries, counts, totals, n_per_shard, self_shard, child_first, n_children_total,
                                     action):
        a = _c(action, np.float64)
        c = np.ascontiguousarray(np.asarray(counts, np.int64))
        t = np.ascontiguousarray(np.asarray(totals, np.uint64))
        assert c.size == n_shards and t.size == n_shards
        self._chk(self.lib.mcl_stage_resample_compact_async(self._h, C.c_void_p(d_chunks), C.c_int32(n_shards), C.c_int64(chunk_entries), _p(c), _p(t),
                                                            C.c_int64(n_per_shard), C.c_int32(self_shard), C.c_int64(child_first),
                                                            C.c_int64(n_children_total), _p(a)), "mcl_stage_resample_compact_async")

    def stage_keep(self, child_first, n_children_total, action):
        """Adaptive resampling kept the set: motion only, every particle its own parent (launch only)."""
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_keep(self._h, C.c_int64(child_first), C.c_int64(n_children_total), _p(a)), "mcl_stage_keep")

    def stage_rays_async(self, obs, d_local_max):
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_stage_rays_async(self._h, _p(o), C.c_int32(o.size), C.c_void_p(d_local_max)), "mcl_stage_rays_async")

    def stage_weights_async(self, d_global_max, d_vec, n_shards, self_shard):
        self._chk(self.lib.mcl_stage_weights_async(self._h, C.c_void_p(d_global_max), C.c_void_p(d_vec), C.c_int32(n_shards), C.c_int32(self_shard)),
                  "mcl_stage_weights_async")

    def stage_complete(self, sums5) -> bool:
        """The one host wait of a device-ordered update.  True: the ray stage's fix-up lists overflowed, run the synchronous
        stages once more (stage_rays .. stage_finish)."""
        s = _c(sums5, np.float64)
        redo = C.c_int32(0)
        self._chk(self.lib.mcl_stage_complete(self._h, _p(s), C.byref(redo)), "mcl_stage_complete")
        return bool(redo.value)

    # ---- the sharded update in native code: an RCCL communicator inside the engine (include/mcl_hip_engine.h: mcl_comm_*)
    @staticmethod
    def comm_available():
        """(True, "") when the library finds an RCCL to use, else (False, why)."""
        why = C.c_char_p()
        rc = load_library().mcl_comm_available(C.byref(why))
        return rc == MCL_OK, (why.value or b"").decode()

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        rc = load_library().mcl_comm_unique_id(buf)
        if rc != MCL_OK:
            raise EngineError(f"mcl_comm_unique_id rc={rc}")
        return bytes(buf)

    def comm_create(self, uid: bytes, n_ranks: int, rank: int):
        """COLLECTIVE: every rank calls it with rank 0's id."""
        assert len(uid) == 128
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        self._chk(self.lib.mcl_comm_create(self._h, buf, C.c_int32(n_ranks), C.c_int32(rank)), "mcl_comm_create")
        self._comm_ranks = n_ranks

    def comm_selftest(self):
        """COLLECTIVE: the three collectives of an update on known data."""
        self._chk(self.lib.mcl_comm_selftest(self._h), "mcl_comm_selftest")

    def comm_destroy(self):
        self._chk(self.lib.mcl_comm_destroy(self._h), "mcl_comm_destroy")

    def comm_set_lists(self, counts, totals):
        c = np.ascontiguousarray(np.asarray(counts, np.int64))
        t = np.ascontiguousarray(np.asarray(totals, np.uint64))
        assert c.size == self._comm_ranks and t.size == self._comm_ranks
        self._chk(self.lib.mcl_comm_set_lists(self._h, _p(c), _p(t)), "mcl_comm_set_lists")

    def comm_update(self, action, obs):
        """One sharded update in one native call (lists, or the dense exchange when there are none); the pose of the whole set.
        Any failure -- this rank's, a peer's, a collective that ran out of time -- raises ShardedUpdateError on EVERY rank from
        the same update (include/mcl_hip_engine.h: the failure protocol of mcl_comm_update); nothing falls back to another exchange."""
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        pose = np.zeros(3)
        rc = self.lib.mcl_comm_update(self._h, _p(a), _p(o), C.c_int32(o.size), _p(pose))
        if rc != MCL_OK:
            raise ShardedUpdateError(f"mcl_comm_update rc={rc}: {self.lib.mcl_last_error(self._h).decode()}", rc,
                                     local=rc not in (MCL_ERR_PEER, MCL_ERR_TIMEOUT))
        return pose

    def comm_vector(self):
        vec = np.zeros(5 + 3 * self._comm_ranks + 2)
        self._chk(self.lib.mcl_comm_get_vector(self._h, _p(vec), C.c_int32(vec.size)), "mcl_comm_get_vector")
        return vec

    def comm_stats(self):
        r, p, w = C.c_uint64(), C.c_uint64(), C.c_int32()
        self._chk(self.lib.mcl_comm_stats(self._h, C.byref(r), C.byref(p), C.byref(w)), "mcl_comm_stats")
        d, wb, rb = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.mcl_comm_last_exchange(self._h, C.byref(d), C.byref(wb), C.byref(rb)), "mcl_comm_last_exchange")
        return dict(list_bytes_received=r.value, list_payload_bytes=p.value, host_waits=w.value, dense=d.value == 1, kept=d.value == 2,
                    weights_received=wb.value, records_received=rb.value)

    def scan_weights(self, d_q, d_cdf, n, offset=0):
        self._chk(self.lib.mcl_scan_weights(self._h, C.c_void_p(d_q), C.c_void_p(d_cdf), C.c_int64(n),
                                            C.c_uint64(offset)), "mcl_scan_weights")


class Group:
    """Several GPUs behind one handle, driven by this one process (mcl_group_*): the particle set is sharded contiguously
    over `devices`; results are bit-identical to one Engine holding all particles."""

    def __init__(self, devices, cfg: Config | None = None, **over):
        self.lib = load_library()
        self.cfg = cfg if cfg is not None else default_config(**over)
        if cfg is not None:
            for k, v in over.items():
                setattr(self.cfg, k, v)
        dev = np.ascontiguousarray(np.asarray(devices, np.int32))
        h = C.c_void_p()
        rc = self.lib.mcl_group_create(C.byref(self.cfg), _p(dev), C.c_int32(dev.size), C.byref(h))
        if rc != MCL_OK:
            raise EngineError(f"mcl_group_create rc={rc}: {self.lib.mcl_group_last_error(None).decode()}")
        self._h = h
        self.size = int(dev.size)
        self.n_total = 0

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mcl_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != MCL_OK:
            raise EngineError(f"{what} rc={rc}: {self.lib.mcl_group_last_error(self._h).decode()}")

    def set_map(self, grid, resolution, origin_x, origin_y):
        g = _c(grid, np.int8)
        H, W = g.shape
        self._chk(self.lib.mcl_group_set_map(self._h, _p(g), C.c_uint32(W), C.c_uint32(H), C.c_float(resolution),
                                             C.c_double(origin_x), C.c_double(origin_y)), "mcl_group_set_map")

    def update_map_region(self, cells2d, x0: int, y0: int):
        """mcl_group_update_map_region: Engine.update_map_region on every engine of the group."""
        c = _patch_cells(cells2d)
        self._chk(self.lib.mcl_group_update_map_region(self._h, _p(c), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(c.shape[1]), C.c_uint32(c.shape[0]),
                                                       C.c_uint32(c.strides[0])), "mcl_group_update_map_region")

    def set_beam_angles(self, angles):
        a = _c(angles, np.float32)
        self._chk(self.lib.mcl_group_set_beam_angles(self._h, _p(a), C.c_int32(a.size)), "mcl_group_set_beam_angles")
        self.n_beams = a.size

    def set_particles(self, p_colmajor, weights):
        p = _c(p_colmajor, np.float64)
        w = _c(weights, np.float64)
        self.n_total = int(p.shape[1])
        self._chk(self.lib.mcl_group_set_particles(self._h, _p(p), _p(w), C.c_int64(self.n_total)), "mcl_group_set_particles")

    def init_particles_pose(self, pose, n_total):
        q = _c(pose, np.float64)
        self.n_total = int(n_total)
        self._chk(self.lib.mcl_group_init_particles_pose(self._h, _p(q), C.c_int64(n_total)), "mcl_group_init_particles_pose")

    def init_global(self, n_total):
        self.n_total = int(n_total)
        self._chk(self.lib.mcl_group_init_global(self._h, C.c_int64(n_total)), "mcl_group_init_global")

    def init_particles_gaussian(self, mean, cov, n_total):
        m, c = _c(mean, np.float64), _c(cov, np.float64)
        assert m.size == 3 and c.size == 9
        self.n_total = int(n_total)
        self._chk(self.lib.mcl_group_init_particles_gaussian(self._h, _p(m), _p(c), C.c_int64(n_total)),
                  "mcl_group_init_particles_gaussian")

    def set_motion_model(self, model="diff", **fields):
        """Engine.set_motion_model on every shard."""
        if model is None:
            self._chk(self.lib.mcl_group_set_motion_model(self._h, None), "mcl_group_set_motion_model")
            return None
        c = default_motion_config(model=model, **fields)
        self._chk(self.lib.mcl_group_set_motion_model(self._h, C.byref(c)), "mcl_group_set_motion_model")
        return c

    def set_sensor_mount(self, mount):
        """Engine.set_sensor_mount on every shard (mcl_group_set_sensor_mount)."""
        m = _mount3(mount)
        self._chk(self.lib.mcl_group_set_sensor_mount(self._h, _p(m)), "mcl_group_set_sensor_mount")

    def update(self, action, obs):
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_group_update(self._h, _p(a), _p(o), C.c_int32(o.size)), "mcl_group_update")

    def expected_pose(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_group_expected_pose(self._h, _p(out)), "mcl_group_expected_pose")
        return out

    def get_particles(self):
        out = np.empty((3, self.n_total))
        self._chk(self.lib.mcl_group_get_particles(self._h, _p(out), C.c_int64(self.n_total)), "mcl_group_get_particles")
        return out

    def get_weights(self):
        out = np.empty(self.n_total)
        self._chk(self.lib.mcl_group_get_weights(self._h, _p(out), C.c_int64(self.n_total)), "mcl_group_get_weights")
        return out

    def resample_indices(self):
        out = np.empty(self.n_total, np.int32)
        self._chk(self.lib.mcl_group_get_resample_indices(self._h, _p(out), C.c_int64(self.n_total)), "mcl_group_get_resample_indices")
        return out

    def stage_timings(self):
        out = np.empty(6)
        self._chk(self.lib.mcl_group_get_stage_timings(self._h, _p(out)), "mcl_group_get_stage_timings")
        return out

    def engine(self, i) -> "Engine":
        """Non-owning view of shard i's engine (diagnostics: sample_particles, counters, ...)."""
        h = C.c_void_p()
        self._chk(self.lib.mcl_group_engine(self._h, C.c_int32(i), C.byref(h)), "mcl_group_engine")
        e = Engine.__new__(Engine)
        e.lib, e.cfg, e._h, e.n, e.n_beams, e._borrowed = self.lib, self.cfg, h, self.n_total // self.size, getattr(self, "n_beams", 0), True
        return e

    def exchange_bytes(self):
        out = np.zeros(2, np.uint64)
        self._chk(self.lib.mcl_group_exchange_bytes(self._h, _p(out)), "mcl_group_exchange_bytes")
        return dict(weights_received_per_device=int(out[0]), parent_records_from_peers=int(out[1]),
                    lists=bool(self.lib.mcl_group_exchanged_lists(self._h)))
