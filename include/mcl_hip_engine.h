/*
 * mcl_hip_engine.h — C ABI of the MI355X particle-filter update engine (libmcl_hip_engine.so).
 *
 * Drop-in boundary for the hot path of AE-HYU/monte_carlo_localization: the bodies of
 *     void ParticleFilter::MCL(const Eigen::Vector3d&, const std::vector<float>&)   src/particle_filter.cpp:652-694
 *     Eigen::Vector3d ParticleFilter::expected_pose()                               src/particle_filter.cpp:696-716
 * plus the state hand-over points that surround them (get_omap cpp:190-224, lidarCB cpp:297-313,
 * initialize_particles_pose cpp:388-398, initialize_global cpp:433-443, visualize cpp:946-958).
 * The reference has no FFI of its own (the functions are private members, hpp:39-43,74-75); the
 * entry points below are what a binding for this path has to offer, one per hand-over point, and
 * INTEGRATION.md shows the ~40-line patch that wires them into the unchanged class.
 *
 * Conventions
 *   - plain C, no C++/Eigen/ROS/torch types; the caller owns every host buffer, the engine owns
 *     all device memory behind the opaque handle and copies in/out synchronously;
 *   - particle matrices use the memory layout of Eigen::MatrixXd(N,3): column-major, i.e. N x's,
 *     then N y's, then N thetas (hpp:102); weights are std::vector<double> (hpp:103);
 *   - every function returns MCL_OK (0) or a negative mcl_status; nothing throws across the ABI.
 *     MCL_ERR_INVALID_ARG / NOT_READY / UNSUPPORTED are detected before anything is touched: the engine state is left as
 *     it was (the host patch then skips the tick exactly like a failed state_lock_.try_lock(), cpp:756).
 *     MCL_ERR_HIP means the HIP runtime failed part-way (out of memory, a lost device): what the call was replacing is
 *     then undefined -- after mcl_set_map / mcl_set_beam_angles the engine reports "not ready" until the call
 *     succeeds, after mcl_update / mcl_stage_* the particle set must be set or initialised again;
 *   - calls on one handle must be serialised by the caller (they are: single-threaded executor
 *     cpp:1022 + state_lock_ cpp:756/387/408).  mcl_update() is synchronous: when it returns the
 *     new particle set, weights and pose are final (its wall time feeds delay compensation,
 *     cpp:792-796).
 */
#ifndef MCL_HIP_ENGINE_H
#define MCL_HIP_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCL_ABI_VERSION 1

typedef struct mcl_engine mcl_engine_t;

typedef enum {
    MCL_OK = 0,
    MCL_ERR_INVALID_ARG = -1,   /* null pointer, size mismatch, bad enum            */
    MCL_ERR_NOT_READY = -2,     /* map / beam angles / particles not set yet        */
    MCL_ERR_HIP = -3,           /* a HIP runtime call failed; see mcl_last_error()  */
    MCL_ERR_NO_DEVICE = -4,     /* no gfx950 device visible                         */
    MCL_ERR_UNSUPPORTED = -5,   /* e.g. ray steps requested but not kept            */
    MCL_ERR_PEER = -6,          /* sharded update: another rank reported a failure; the update is void on every rank */
    MCL_ERR_TIMEOUT = -7        /* sharded update: a collective did not finish in time; the communicator was aborted  */
} mcl_status;

typedef enum {
    MCL_RESAMPLE_MULTINOMIAL = 0, /* what the reference does: std::discrete_distribution, cpp:658-665 */
    MCL_RESAMPLE_SYSTEMATIC = 1   /* one offset per update, u_m = (m + u0)/N                           */
} mcl_resample_mode;

typedef enum {
    MCL_WEIGHT_LOG = 0,           /* sum of log table entries, max-subtracted (default; no underflow)  */
    MCL_WEIGHT_PRODUCT = 1        /* sequential double product + pow, bit-for-bit cpp:566-578 incl.
                                     its underflow at >~200 beams; needs keep_ray_steps                */
} mcl_weight_mode;

typedef enum {
    MCL_RAYS_AUTO = 0,            /* MCL_RAYS_SWEEP from 65536 particles and 2^23 rays when the map and beam set
                                     allow it, else MCL_RAYS_SKIP                                      */
    MCL_RAYS_MARCH = 1,           /* literal fixed-step fp64 march on the int8 grid (cpp:611-650)      */
    MCL_RAYS_SKIP = 2,            /* same sample lattice, empty-space skipping on an LDS-resident
                                     distance-to-obstacle window; exactness guard falls back to MARCH  */
    MCL_RAYS_QUAD = 3,            /* SKIP with the work split by ray direction: one-byte-per-cell quadrant
                                     windows, two workgroups per CU.  LEGACY: only in a library built with
                                     -DMCL_LEGACY_RAY_KERNELS (the tests' libmcl_hip_engine_legacy.so); the product
                                     library answers MCL_ERR_UNSUPPORTED                                */
    MCL_RAYS_CELL = 4,            /* QUAD on particles ordered by grid cell and heading, one particle per
                                     lane: the lanes of a wave trace near-identical rays.  LEGACY, as QUAD */
    MCL_RAYS_SWEEP = 5,           /* cell-sorted particles, one particle per lane, work items planned on the device (runs of
                                     units x direction wedges), 256-cell mirrored LDS windows, 64-bit fixed-point positions,
                                     beam directions turned by the scan's increment (evenly spaced scans); ranges up to 243 px
                                     in LDS windows, beyond that the same walk on mirrored copies of the wedge fields in global
                                     memory (any range whose sixteen fields fit 2^32 bytes).  What AUTO runs from 65 536 particles
                                     and 2^23 rays; below that MCL_RAYS_SKIP. */
    MCL_RAYS_DESKEW = 6           /* reported only (mcl_get_ray_kernel_id, mcl_get_planned_ray_kernel): the kernel of an update with
                                     per-beam sensor offsets on (mcl_set_beam_offsets), one wave per particle, every beam cast from
                                     its own origin.  It cannot be requested through cfg.ray_kernel. */
} mcl_ray_kernel;

/* Upper bound (exclusive) on max_particles and on the particle total of a sharded set: weights are quantised to 2^-36 and
 * their exact sum is kept in 64 bits, so N * 2^36 must stay below 2^64 with one bit to spare. */
#define MCL_MAX_TOTAL_PARTICLES ((int64_t)1 << 27)

/* Numeric subset of the node's parameters (cpp:23-78) + engine knobs. */
typedef struct {
    int64_t max_particles;          /* MAX_PARTICLES, cpp:51                                   */
    int32_t device;                 /* HIP device ordinal                                      */
    uint64_t seed;                  /* Philox key; the reference seeds from random_device cpp:20 */
    double max_range_m;             /* cpp:54                                                  */
    double z_hit, z_short, z_max, z_rand, sigma_hit;   /* cpp:64-68                            */
    double squash_factor;           /* cpp:53 (INV_SQUASH_FACTOR = 1/squash_factor)            */
    double motion_dispersion_x, motion_dispersion_y, motion_dispersion_theta; /* cpp:71-73      */
    int32_t resample_mode;          /* mcl_resample_mode                                       */
    int32_t weight_mode;            /* mcl_weight_mode                                         */
    int32_t ray_kernel;             /* mcl_ray_kernel                                          */
    int32_t keep_ray_steps;         /* !=0: keep the N*B uint8 step indices of the last update */
    int32_t debug_force_exact;      /* 1: every ray takes the literal-march fallback (level 3);
                                       2: every ray takes the fp64 skipping loop (level 2)     */
    int32_t debug_count_probes;     /* !=0: tally examined grid probes (counters[2]); slower   */
    int32_t rays_per_lane;          /* SKIP kernel: independent rays in flight per lane (1..4); 0 = default */
    int32_t resample_neff_permille; /* 0 (default): resample on every update like the reference (cpp:656-665);
                                       r in 1..1000: resample only when the effective sample size
                                       (sum w)^2 / sum w^2 of the previous update is below r/1000 * N, otherwise the
                                       particles keep their identity and their weights multiply */
    int32_t graph_mode;             /* small updates are a chain of dependent launches: 0 (default) and 2 = shorten it once
                                       a first update has run with the same sizes (k_rays_skip path only): up to 8192
                                       particles mcl_update is three launches whose last one writes the result block to
                                       pinned host memory, where the host polls a stamp (MCL_TINY_POLL=0 in the
                                       environment at mcl_create: wait for the stream instead); above that the part after
                                       the resampling kernel is replayed as one hipGraph.  1 = launch by launch.  The
                                       results do not depend on it. */
    int32_t reserved[3];
} mcl_config_t;

/* Fills *cfg with the reference's defaults (config/mcl_config.yaml:6-40, cpp:23-47). */
void mcl_default_config(mcl_config_t *cfg);

int mcl_abi_version(void);

/* ---- lifetime ---------------------------------------------------------------------------- */
/* MCL_ERR_INVALID_ARG, before any device is opened, for a config the engine cannot run: max_particles outside [1, 2^27), a
 * squash_factor or max_range_m that is not finite and > 0, a non-finite or negative z_* or motion_dispersion_*, all four z_* zero,
 * a sigma_hit that is not finite and > 0; mcl_last_error(NULL) says which. */
int mcl_create(const mcl_config_t *cfg, mcl_engine_t **out);
void mcl_destroy(mcl_engine_t *h);
/* Message of the last failing call on this handle ("" if none).  h may be NULL for mcl_create. */
const char *mcl_last_error(const mcl_engine_t *h);

/* ---- map + sensor table: replaces what get_omap() keeps (cpp:190-195) and
 *      precompute_sensor_model() builds (cpp:233-292) ------------------------------------- */
/* data: nav_msgs/OccupancyGrid.data, row-major H x W int8; resolution: MapMetaData.resolution
 * (float32); origin: info.origin.position.{x,y} (map yaw is ignored, cpp:628-629). */
int mcl_set_map(mcl_engine_t *h, const int8_t *data, uint32_t width, uint32_t height,
                float resolution, double origin_x, double origin_y);
/* MAX_RANGE_PX (cpp:195) for the current map. */
int mcl_get_max_range_px(const mcl_engine_t *h, int32_t *out);
/* The engine's sensor_model_table_: (P+1)^2 doubles, Eigen column-major (index d*(P+1)+r). */
int mcl_get_sensor_table(const mcl_engine_t *h, double *out, size_t n);

/* ---- beam geometry: downsampled_angles_ (cpp:306-310, hpp:117) ---------------------------- */
int mcl_set_beam_angles(mcl_engine_t *h, const float *angles, int32_t n_beams);

/* ---- particle state: particles_ / weights_ (hpp:102-103) ---------------------------------- */
/* After initialize_particles_pose / initialize_global rewrote the host copies (cpp:388-398,
 * 433-443).  n must be <= max_particles and becomes the active particle count. */
int mcl_set_particles(mcl_engine_t *h, const double *xyz_colmajor, const double *weights, int64_t n);
/* The same for one shard of a larger set: the fixed-point weights are scaled by the maximum weight of the WHOLE set (every
 * shard must be given the same value), so that the shards' weights are comparable. */
int mcl_set_particles_shard(mcl_engine_t *h, const double *xyz_colmajor, const double *weights, int64_t n, double max_weight_of_the_whole_set);
/* Device-side versions of the two initialisers (Philox draws instead of the host's rng_; same formulas):
 * Gaussian cloud (0.5 m, 0.5 m, 0.4 rad) around `pose` (cpp:388-398) / uniform over free cells with
 * theta ~ U[0,2pi) (cpp:408-443).  n particles become active with weights 1/n_total; first_global_index is
 * this shard's offset in a sharded set (0 and n_total = n on a single GPU).  At 4M-32M particles this
 * replaces a 100-800 MB host->device upload. */
int mcl_init_particles_pose(mcl_engine_t *h, const double pose[3], int64_t n, int64_t first_global_index, int64_t n_total);
int mcl_init_global(mcl_engine_t *h, int64_t n, int64_t first_global_index, int64_t n_total);
int mcl_get_particles(mcl_engine_t *h, double *xyz_colmajor, int64_t n);
int mcl_get_weights(mcl_engine_t *h, double *weights, int64_t n);
/* visualize()'s weighted sample of k rows (cpp:949-956): k draws from the current weights.
 * uniforms: k doubles in [0,1) (e.g. from the host's rng_) or NULL for Philox draws.
 * out: k x 3 column-major.  1 <= k <= 65536, whatever the engine's max_particles (k may exceed it). */
int mcl_sample_particles(mcl_engine_t *h, int32_t k, const double *uniforms, double *out_colmajor);
/* get_current_pose()'s particles_.colwise().mean() (cpp:903-908). */
int mcl_particle_mean(mcl_engine_t *h, double out[3]);

/* ---- the update: body of MCL(action, observation) (cpp:652-694) --------------------------- */
/* action = (forward displacement m, unused, yaw displacement rad) (cpp:761-772);
 * obs = n_beams downsampled ranges in metres (cpp:316-320).
 * Injection hooks for reference-exact parity: normals = N x 3 ROW-major doubles in
 * the reference's draw order (n_x, n_y, n_theta per particle, cpp:496-498), uniforms = N doubles
 * in [0,1) as discrete_distribution would draw them (cpp:663).  Either may be NULL -> Philox. */
int mcl_update(mcl_engine_t *h, const double action[3], const float *obs, int32_t n_beams,
               const double *normals_nx3, const double *uniforms_n);
/* Same update fed with the RAW LaserScan.ranges: the engine keeps every angle_step-th range like
 * lidarCB does (cpp:316-320) — ceil(n_ranges/angle_step) must equal the number of beam angles set. */
int mcl_update_scan(mcl_engine_t *h, const double action[3], const float *ranges, int32_t n_ranges, int32_t angle_step);
/* sensor_model() + normalisation only, on the current particles (cpp:676-686): no resample, no
 * motion.  Used by parity tests of the ray-cast / likelihood stage. */
int mcl_sensor_update(mcl_engine_t *h, const float *obs, int32_t n_beams);

/* ---- expected_pose() (cpp:696-716) --------------------------------------------------------- */
int mcl_expected_pose(mcl_engine_t *h, double out[3]);

/* ---- TimingStats mirror (utils.hpp:51-57): resampling, motion_model, query_prep, ray_casting,
 *      sensor_model (table eval + normalise), total — milliseconds of the LAST update -------- */
int mcl_get_stage_timings(const mcl_engine_t *h, double ms[6]);

/* ---- parity / diagnostics ------------------------------------------------------------------ */
int mcl_get_resample_indices(mcl_engine_t *h, int32_t *idx, int64_t n);      /* parents of last update */
int mcl_get_ray_steps(mcl_engine_t *h, uint8_t *steps, size_t n);            /* N*B, needs keep_ray_steps; MAX_RANGE_PX <= 255 */
int mcl_get_ray_steps16(mcl_engine_t *h, uint16_t *steps, size_t n);         /* the same for any range (cpp:195 has no bound) */
int mcl_get_log_weights(mcl_engine_t *h, double *logw, int64_t n);           /* un-normalised log w   */
/* counters of the last update: [0] rays resolved by the literal-march fallback (level 3),
 * [1] particles that did not fit the LDS window (global-memory path), [2] grid probes examined
 * (only with debug_count_probes), [3] rays re-run by the fp64 loop (level 2) */
int mcl_get_counters(mcl_engine_t *h, uint64_t out[4]);
/* The compact parent list: the scan of an update's fixed-point weights also lists, in index order, the
 * particles whose weight is not zero -- after an update with many beams a few per cent of the set -- and the next
 * resampling searches and gathers from that list instead of the full CDF and record arrays (same draw: a particle with a
 * zero fixed-point weight is never selected).  n_entries: length of the list that describes the current weights, -1 when
 * there is none (more than max_particles / 4 particles carry weight, or a small update); used_by_last_update: whether the
 * last mcl_update / staged resampling drew from a list.  MCL_NO_COMPACT=1 in the environment at mcl_create disables it. */
int mcl_get_compact_list(const mcl_engine_t *h, int64_t *n_entries, int32_t *used_by_last_update);
/* switches cfg.debug_count_probes on an existing engine (the next update tallies counters[2]; bench.py's untimed probe count) */
int mcl_set_debug_count_probes(mcl_engine_t *h, int32_t on);
/* sets cfg.debug_force_exact (0, 1 or 2) on an existing engine, for tests that run a forced and a plain ray stage on one engine */
int mcl_set_debug_force_exact(mcl_engine_t *h, int32_t level);
/* duration (ms) of the dominant kernel (ray cast + likelihood) in the last update, measured
 * with HIP events on the engine's own stream */
int mcl_get_ray_kernel_ms(const mcl_engine_t *h, double *ms);
/* which ray kernel the last update ran: 1 k_rays_march, 2 k_rays_skip, 3 k_rays_quad, 4 k_rays_cell, 5 k_rays_sweep */
int mcl_get_ray_kernel_id(const mcl_engine_t *h, int32_t *kernel);
/* The form of the windowed ray kernel the last ray stage ran (k_rays_sweep, csrc/mcl_rays_sweep.h): out = [1 if it probed the wedge
 * fields in global memory (ranges beyond 243 px), 2 if it walked in LDS windows and went on in those fields where a ray left its
 * window (the hybrid form of such ranges: evenly spaced scans), 1 if it turned the beam direction by the scan's increment instead of fetching it
 * (evenly spaced scans), 1 if it walked two rays per lane].  A performance diagnostic (bench.py prices the instruction stream of the
 * form that ran); results do not depend on it. */
int mcl_get_ray_kernel_variant(const mcl_engine_t *h, int32_t out[3]);
/* Which ray kernel an update over n_particles (<= 0: the active count, or max_particles before any particles are set) WILL run
 * with the current configuration, map and beam set -- the same pure function mcl_update consults, callable before the first
 * update (needs the map and the beam angles).  *kernel as mcl_get_ray_kernel_id, 0 = the configured kernel cannot run with
 * this map / beam set (mcl_update would return MCL_ERR_UNSUPPORTED).  *reason (may be NULL) receives a static string naming
 * what decided, e.g. why AUTO stays off k_rays_sweep: the fast windowed kernels need beam angles that increase over less
 * than a turn and MAX_RANGE_PX <= 243; anything else takes k_rays_skip (same results, several times slower at size). */
int mcl_get_planned_ray_kernel(const mcl_engine_t *h, int64_t n_particles, int32_t *kernel, const char **reason);
/* Effective sample size (sum w)^2 / sum w^2 of the current weights, and whether the last mcl_update resampled
 * (always 1 with resample_neff_permille == 0). */
int mcl_get_effective_sample_size(const mcl_engine_t *h, double *n_eff, int32_t *resampled_last_update);

/* ---- KLD-adaptive particle count (KLD sampling, Fox 2003, as in AMCL) --------------------------------
 * Off by default.  With it on, every mcl_update counts how many pose-space bins the parents it drew occupy, and the NEXT update
 * draws the smallest set that keeps the KL divergence to the posterior within err with confidence z: N_{t+1} is decided from
 * the count of update t, one update of lag -- the batch form of KLD sampling on a GPU (the count is final when the resampling
 * kernel ends, the set it sizes is drawn by the next one).
 *   What is counted: inside update t, the pose of the parent of every one of the N_t children, before the motion model (the
 *     drawn sample, as a KD-tree insertion counts it); in an update that kept its particles (resample_neff_permille) each
 *     particle's own pose.  mcl_sensor_update counts nothing.
 *   Bins: nx = ceil(W * res / bin_x_m), ny = ceil(H * res / bin_y_m) in double (res widened from float); ix = floor((x - ox) *
 *     (1 / bin_x_m)), iy = floor((y - oy) * (1 / bin_y_m)), the reciprocals computed once in double; it = floor((theta + pi) *
 *     (n_theta_bins / (2 pi))) as int64, mod n_theta_bins, non-negative.  A pose whose ix or iy falls outside the grid, any of
 *     whose x, y, theta is not finite, or with |theta| >= 1e9 lands in ONE extra "outside" bin.  Each formula is an add or
 *     subtract followed by a multiply (nothing FMA contraction could fuse): the device, mcl_host_kld_bins and a numpy
 *     restatement agree bit for bit, bin edges included.  A grid of more than 2^31 bits (nx * ny * n_theta_bins + 1) is refused
 *     by mcl_set_kld / mcl_set_map with MCL_ERR_INVALID_ARG.
 *   Target: for k <= 1 occupied bins, max_particles; otherwise a = 2 / (9 (k - 1)), b = 1 - a + sqrt(a) * z,
 *     n = ceil((k - 1) / (2 err) * (b * b * b)), rounded UP to a multiple of round_to, then clamped to [min, max].
 *     n_next = n_current when target <= n_current and target * 1000 >= n_current * shrink_permille (exact integers), otherwise
 *     the target: the hysteresis keeps N steady once tracking, so that the small-update paths (captured graph, three launches)
 *     stay warm.
 *   mcl_set_kld, mcl_set_particles* and mcl_init_* set n_next = clamp(N, min, max) (and bins_last = -1).  An update that kept
 *     its particles and mcl_sensor_update leave n_next alone; with KLD on an update keeps its particles only when n_next == N.
 *   Injected draws: with KLD on, mcl_update's normals / uniforms hold n_next rows (read it with mcl_get_kld_state first).
 *     After the update mcl_get_particle_count is the new N, which mcl_get_particles, _weights, _resample_indices (values below
 *     the previous N), _log_weights, ... take.
 *   Single engine only: mcl_set_kld on an engine with a communicator or in a device group, mcl_comm_create on an engine with
 *     KLD on, and every mcl_stage_* call while KLD is on return MCL_ERR_UNSUPPORTED. */
typedef struct {
    int64_t min_particles, max_particles;   /* 1 <= min <= max <= cfg.max_particles                                          */
    double err;                             /* epsilon of the KLD bound, default 0.01                                         */
    double z;                               /* upper standard-normal quantile (>= 0), default 2.326 (0.99)                    */
    double bin_x_m, bin_y_m;                /* default 0.5, 0.5                                                               */
    int32_t n_theta_bins;                   /* heading bins over one turn, default 36 (10 degrees)                            */
    int32_t round_to;                       /* targets rounded UP to a multiple of this, default 256                          */
    int32_t shrink_permille;                /* keep N while target >= N * permille / 1000 (0..1000, default 800; 1000 = none) */
    int32_t reserved;                       /* must be 0                                                                      */
} mcl_kld_config_t;
/* defaults above; min_particles 256, max_particles 4194304 */
void mcl_default_kld_config(mcl_kld_config_t *k);
int mcl_set_kld(mcl_engine_t *h, const mcl_kld_config_t *k);          /* NULL = off (the default)                           */
int mcl_get_particle_count(const mcl_engine_t *h, int64_t *n);         /* particles held now (the parents of the next update) */
/* bins occupied by the last update's draw (-1: none counted), children the next update draws (N when KLD is off); either
 * pointer may be NULL */
int mcl_get_kld_state(const mcl_engine_t *h, int64_t *bins_last, int64_t *n_next);
/* the two rules above on the host, without a device: occupied bins of n poses (x, y, th: n doubles each) on a width x height
 * map; the next particle count after an update that counted `bins` with n_current particles (k->max_particles is not checked
 * against any engine here) */
int mcl_host_kld_bins(const double *x, const double *y, const double *th, int64_t n, uint32_t width, uint32_t height,
                      float resolution, double origin_x, double origin_y, const mcl_kld_config_t *k, int64_t *bins);
int mcl_host_kld_target(const mcl_kld_config_t *k, int64_t bins, int64_t n_current, int64_t *n_next);

/* ---- pose hypotheses: weighted clusters of the particle set ----------------------------------------------
 * mcl_pose_clusters groups the particles the engine holds now (mcl_get_particle_count) by their fixed-point weights q (those
 * mcl_export_state exports) into connected components of occupied pose-space bins, and reports each with its weight, mean and
 * covariance -- AMCL's cluster statistics.  It runs only when called, on the engine's stream with one host wait, and leaves every
 * engine state as it was: the next update is the one an engine that never clustered would run.
 *   Bins: the KLD bin rule above with this config's bin sizes and heading bins.  A particle with q = 0 or in the "outside" bin
 *     belongs to no cluster (its bin is not occupied).  Two occupied bins touch when |dix| <= 1, |diy| <= 1 and the heading bins
 *     differ by at most 1 modulo n_theta_bins (the heading wraps, x and y do not).  A cluster is a connected component; its name
 *     first_bin is its smallest bin index.
 *   Sums: weight_q = sum q (exact), weight = weight_q / Q with Q = sum q over every particle; mean = (sum q x / W, sum q y / W,
 *     atan2(sum q sin, sum q cos)) with W = weight_q as a double; cov = sum q d d^T / W about the mean, d = (x - mx, y - my,
 *     remainder(theta - mth, 2 pi)), row-major.  The fp64 sums have a fixed order: the same state gives the same bits.
 *   Order: weight_q descending, ties by first_bin ascending.  mcl_get_cluster_labels: the rank of each particle's cluster, or -1.
 *   Q = 0 gives no clusters.  MCL_ERR_INVALID_ARG for a bin size that is not finite and > 0, n_theta_bins < 1, reserved != 0,
 *     max_clusters outside [0, 65536] or a grid of more than 2^31 bits; MCL_ERR_NOT_READY without a map or particles (labels:
 *     before any clustering or after the set changed); MCL_ERR_UNSUPPORTED on an engine with a communicator or in a device group
 *     (a shard cannot cluster the whole set). */
typedef struct {
    double bin_x_m, bin_y_m;                /* default 0.5, 0.5                                                               */
    int32_t n_theta_bins;                   /* default 36                                                                     */
    int32_t reserved;                       /* must be 0                                                                      */
} mcl_cluster_config_t;
typedef struct {
    uint64_t weight_q;                      /* sum of the members' q                                                          */
    double weight;                          /* weight_q / Q                                                                   */
    int64_t n_particles, n_bins, first_bin;
    double mean[3];                         /* x, y, heading                                                                  */
    double cov[9];                          /* row-major, x y heading                                                         */
} mcl_cluster_t;
void mcl_default_cluster_config(mcl_cluster_config_t *c);
/* the max_clusters heaviest into out (out may be NULL when max_clusters == 0); *n_clusters = all of them; totals = {Q, q of the
 * outside bin, particles in the outside bin}.  n_clusters and totals may be NULL. */
int mcl_pose_clusters(mcl_engine_t *h, const mcl_cluster_config_t *c, int32_t max_clusters, mcl_cluster_t *out, int64_t *n_clusters,
                      uint64_t totals[3]);
int mcl_get_cluster_labels(mcl_engine_t *h, int32_t *labels, int64_t n);   /* of the last mcl_pose_clusters; n == N */

/* ---- pose query: expected scans and scan scores of poses that are not particles --------------------------
 * mcl_query_scans casts the beams last set from K given poses -- the "fake scan" of the reference's ancestors, range_libc's
 * calc_range_many -- and mcl_score_poses says how well a scan supports each pose: what a node needs to rank the means of
 * mcl_pose_clusters, to publish the expected scan at its estimate, or to vet an /initialpose before
 * mcl_init_particles_gaussian seeds a cloud there.  Neither touches the particle set.  poses_colmajor is K x 3 column-major
 * (x, y, theta) like every particle array of this header, 1 <= K <= 65536; B is the number of beam angles set.
 *   Q1 step.  steps[k * B + j] is E3's r for a particle at pose k and beam j: bit for bit what mcl_get_ray_steps16 reports for
 *     a particle at that pose, whatever the pose (non-finite, |theta| >= 1e6, off the map, in an occupied cell).  The device
 *     functions are those of the update's ray stage: the fp64 walk on the isotropic skip field with its guard (level 2), the
 *     literal march (level 3) where the guard says so, where the pose is not sane, or with debug_force_exact.
 *   Q2 metres.  ranges_m[k * B + j] is cast_ray's return (cpp:635 / 644 / 649): (float)(r * res) with res the map's float
 *     resolution widened to double for r < MAX_RANGE_PX, and (float)max_range_m of the engine's config for a miss.
 *   Q3 log-likelihood, under the sensor model the engine has now.  Beam model: E4's sum_j (double)L[obs_idx_j][r_kj] with
 *     obs_idx from E2.  Likelihood field on: LF3-LF5, the in-order fp64 sum, by the update's own kernel on the query's buffers.
 *     Either way the value is bit for bit what mcl_get_log_weights gives for a particle at that pose after
 *     mcl_sensor_update(obs).  No fp64 atomics: one wave per pose, lane l adds beams l, l + 64, ... in order, then a fixed
 *     butterfly -- under E4's condition the order is invisible, outside it the value is still reproducible.  weight_mode
 *     PRODUCT refuses mcl_score_poses (MCL_ERR_INVALID_ARG); mcl_query_scans works in that mode.
 *   Q4 agreement, in integers (exact), from cast rays under either sensor model.  Beam j is valid iff its reading is finite and
 *     obs_idx_j < MAX_RANGE_PX; it agrees iff it is valid and |obs_idx_j - r_kj| <= tol_steps, 0 <= tol_steps <= MAX_RANGE_PX.
 *     n_miss counts the rays of the pose with r = MAX_RANGE_PX, valid beam or not.
 *   Q5 read-only.  Both calls use buffers of their own, allocated on the first call and grown with K * B (an engine that never
 *     queries allocates nothing), and none of the update's scratch, tables of the staged observation included.  Captured graphs
 *     and the warm small-update path stay valid: every later update is bit-identical to one of an engine that never queried.
 *     One host wait per call, at its end.
 *   Q6 where it works.  Any engine with a map and beam angles; no particles are needed (MCL_ERR_NOT_READY without a map or
 *     beams).  Shards of a device group and engines with a communicator are accepted: map and beams are replicated and the call
 *     is local.  MCL_ERR_INVALID_ARG for K outside [1, 65536], null poses (null obs / out for the score), n_beams != B,
 *     tol_steps outside [0, MAX_RANGE_PX].
 *   Cost scales with K * B, one lane per ray on the global skip field: made for tens to thousands of poses, not a substitute
 *     for the update at particle-set sizes. */
typedef struct {
    double  log_likelihood;                 /* Q3                                                                             */
    int32_t n_valid;                        /* Q4                                                                             */
    int32_t n_agree;                        /* Q4                                                                             */
    int32_t n_miss;                         /* rays of this pose that ended at step MAX_RANGE_PX (nothing hit in range)       */
    int32_t reserved;
} mcl_pose_score_t;
/* ranges_m, steps: K * B entries each, pose-major; either may be NULL */
int mcl_query_scans(mcl_engine_t *h, const double *poses_colmajor, int32_t K, float *ranges_m, uint16_t *steps);
int mcl_score_poses(mcl_engine_t *h, const double *poses_colmajor, int32_t K, const float *obs, int32_t n_beams,
                    int32_t tol_steps, mcl_pose_score_t *out /* K */);
/* of the pose query: [0] rays of the last call the literal march decided (level 3), [1] bytes of device memory the query's
 * buffers have asked for so far (0 on an engine that never queried) */
int mcl_get_query_counters(const mcl_engine_t *h, uint64_t out[2]);

/* ---- global search: score a pose lattice against a scan, seed from the hits --------------------------------
 * The deterministic alternative to mcl_init_global: every pose of a regular lattice over the map's free cells is scored against
 * one scan under the likelihood-field model, and the best-fitting poses are reported.  mcl_init_particles_mixture (below, with
 * the Gaussian initialisation) turns several hits into one cloud.
 *   S1 positions.  h0 = stride_cells / 2 (integer); lattice columns col = h0 + ix * stride_cells for every ix with col < W, rows
 *     likewise; a lattice cell is a position iff data[row * W + col] == 0 (mcl_init_global's free rule).  Positions are numbered
 *     p = 0 ... in row-major order of (iy, ix).  The pose sits at the cell centre: x = ox + ((double)col + 0.5) * res, res the
 *     map's float resolution widened to double, the multiply and the add each rounded; y likewise.  The host forms the table.
 *   S2 headings.  theta_k = (double)(2 k - n_headings) * (pi / n_headings), pi / n_headings formed once in double on the host.
 *   S3 beams.  Beam j is used iff j % beam_stride == 0 and 0 <= r_j < max_range_m (LF3); the used beams, in beam order.
 *   S4 score.  score[k * n_positions + p] is the likelihood-field log-likelihood (LF4 / LF5) of the pose (x_p, y_p, theta_k): bit
 *     for bit what mcl_score_poses returns for that pose and the same obs (for beam_stride > 1: obs with the readings of the other
 *     beams replaced by NaN).  The in-order fp64 sum, one lane per pose; finite or -inf, never NaN.
 *   S5 hits.  Pose a is better than pose b iff score_a > score_b, or the scores are equal and index_a < index_b.  With nms = 1 a
 *     pose is a candidate iff its score is > -inf and it is better than every lattice neighbour: the positions at (ix + dix,
 *     iy + diy), dix, diy in {-1, 0, 1}, combined with the headings (k + dk) mod n_headings, dk in {-1, 0, 1}, the pose itself
 *     excluded, lattice cells that are no position ignored.  With nms = 0 every pose with a score > -inf is a candidate.
 *     *n_hits = the number of candidates; hits receives the min(max_hits, *n_hits) best, best first.  0 <= max_hits <= 65536;
 *     hits may be NULL when max_hits is 0.  The order is total, so the result is unique.
 *   S6 stats = {n_positions, poses scored, used beams, bytes of device memory the search's buffers have asked for so far}; stats
 *     may be NULL.  mcl_get_search_scores copies the volume of the last search (n == n_headings * n_positions);
 *     MCL_ERR_NOT_READY before any search and after mcl_set_map.
 *   S7 read-only (as Q5).  The search uses buffers of its own, allocated on the first search (mcl_get_search_bytes: 0 on an
 *     engine that never searched), and none of the update's scratch or staged observation; one host wait, at its end (a search
 *     whose lattice differs from the last one's also uploads the new lattice first).  Every later update is bit-identical to
 *     one of an engine that never searched.
 *   S8 where it works.  A map, beam angles and the likelihood-field model ON (the search reads the engine's field D and table
 *     Lf): MCL_ERR_NOT_READY otherwise -- the message says which is missing -- and when the lattice has no position.
 *     MCL_ERR_INVALID_ARG for stride_cells, n_headings or beam_stride < 1, nms outside {0, 1}, reserved != 0, n_beams != B, a
 *     null obs / n_hits (or hits with max_hits > 0), max_hits outside [0, 65536], n_positions * n_headings >=
 *     MCL_MAX_TOTAL_PARTICLES.  Single engine only (the likelihood field is).  A node that tracks with the beam model switches
 *     the field on, searches, seeds, and switches it off: either switch makes the next update plan as after mcl_set_particles. */
typedef struct {
    int32_t stride_cells;                   /* >= 1, default 2: lattice pitch in map cells                                    */
    int32_t n_headings;                     /* >= 1, default 72                                                               */
    int32_t beam_stride;                    /* >= 1, default 1: only beams j with j % beam_stride == 0 are candidates          */
    int32_t nms;                            /* 1 (default): hits are local maxima of the score volume; 0: every pose          */
    int32_t reserved[4];                    /* must be 0                                                                      */
} mcl_search_config_t;
typedef struct {
    double  pose[3];                        /* x, y, theta                                                                    */
    double  log_likelihood;                 /* S4                                                                             */
    int64_t index;                          /* k * n_positions + p                                                            */
} mcl_search_hit_t;
void mcl_default_search_config(mcl_search_config_t *c);
int mcl_global_search(mcl_engine_t *h, const mcl_search_config_t *c /* NULL = the defaults */, const float *obs, int32_t n_beams,
                      int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[4]);
int mcl_get_search_scores(mcl_engine_t *h, double *out, size_t n);
int mcl_get_search_bytes(const mcl_engine_t *h, uint64_t *bytes);
/* S1 / S2 on the host, without a device.  The lattice: *n_positions always; cells (the linear map cell row * W + col of every
 * position) and xy (x, y per position) when given, n must then equal the number of positions (call once with both NULL for it).
 * The headings: n == n_headings.  MCL_ERR_INVALID_ARG for a refused config, a null map or bad dimensions / resolution. */
int mcl_host_search_lattice(const mcl_search_config_t *c, const int8_t *data, uint32_t width, uint32_t height, float resolution,
                            double origin_x, double origin_y, uint32_t *cells, double *xy, size_t n, int64_t *n_positions);
int mcl_host_search_headings(const mcl_search_config_t *c, double *theta, size_t n);

/* ---- global search over a scan sequence joined by odometry -------------------------------------------------
 * One scan from inside a corridor fits many places equally well; the scan taken two metres earlier rarely fits the same places.
 * mcl_global_search_sequence scores every lattice pose against S scans, each from where that pose implies the robot was when
 * the scan arrived.  The lattice pose is the robot's pose at the ANCHOR; rel[s] = (dx, dy, dtheta) is the robot's pose at scan s
 * expressed in the robot's frame at the anchor (mcl_host_relative_poses makes it from odometry).  A caller who wants "where am I
 * now" anchors at the latest scan.  Any finite rel is accepted, zero included; no entry has to be zero.  scans is S x n_beams,
 * scan-major; rel is S x 3, one (dx, dy, dtheta) per scan.  The lattice, the config and the hits are mcl_global_search's.
 *   SQ1 offsets.  With theta_k of S2, ck = cos(theta_k) and sk = sin(theta_k) (the host's cos / sin, in double, once per
 *     heading), the host forms for heading k and scan s
 *       theta_ks = theta_k + dtheta_s                   (one rounded add)
 *       ax_ks = ck * dx_s - sk * dy_s,  ay_ks = sk * dx_s + ck * dy_s     (two rounded multiplies, then one rounded add or subtract;
 *                                                                        no fma: the host unit is compiled with contraction off)
 *     and uploads the table off[(k * S + s) * 3 + {0, 1, 2}] = {ax_ks, ay_ks, theta_ks}.  The device never re-derives it: the
 *     host's and the device's sincos need not agree in the last bit, and a displacement formed on the device could then not be
 *     restated by a test.  mcl_host_search_sequence_offsets is the same code without a device (n == n_headings * S * 3).  A zero
 *     rel gives ax = ay = 0 (of either sign) and theta_ks = theta_k.
 *   SQ2 pose of scan s at lattice pose (p, k): (x_p + ax_ks, y_p + ay_ks, theta_ks), each coordinate one rounded fp64 add on
 *     the device; the device takes sincos(theta_ks) as k_lfield takes it of a particle's heading.  theta_ks is NOT wrapped.
 *   SQ3 beams.  S3 per scan: beam j of scan s is used iff j % beam_stride == 0 and 0 <= r_sj < max_range_m (LF3).  Every scan
 *     gets its own list of used beams, in beam order, by the update's own rule; the lists are concatenated on the device, S + 1
 *     offsets say where each begins.  Scans may have different numbers of used beams, zero included.
 *   SQ4 score.  acc_s is, bit for bit, what mcl_score_poses returns for the pose of SQ2 and scan s (for beam_stride > 1: with the
 *     readings of the other beams replaced by NaN).  score[k * n_positions + p] = ((+0.0 + acc_0) + acc_1) + ... in scan order,
 *     in fp64: finite or -inf, never NaN, never -0.0.  A scan pose off the map scores Lf[K] per used beam, as any pose there.
 *   SQ5 hits.  S5 unchanged, on the summed volume: the same marking, the same sort, the same total order.  A hit's pose is the
 *     lattice pose (the anchor), its log_likelihood the summed score.
 *   SQ6 read-only and placement.  As S7 / S8: the buffers are the search's own (mcl_get_search_bytes counts them), grown for the
 *     S beam lists and the offset table; the volume, the sort keys and the indices do not grow with S.  One host wait, at the
 *     end.  Likelihood-field model ON, single engine only.  mcl_get_search_scores returns the summed volume.  Every later update
 *     is bit-identical to one of an engine that never searched.  stats = S6's four, then [4] = S.
 *   SQ7 identity.  With S = 1 and rel = (0, 0, 0) the volume and the hits are bit for bit those of mcl_global_search with the same
 *     scan: x_p + 0.0 (or + -0.0) is x_p, theta_k + 0.0 is theta_k (theta_k = 0 stays +0.0), and +0.0 + acc_0 is acc_0.
 *   Refused with MCL_ERR_INVALID_ARG, the message naming the cause: n_scans outside [1, MCL_SEARCH_MAX_SCANS]; a null scans or
 *     rel; a rel entry that is not finite; n_beams != B; and everything S8 refuses, MCL_ERR_NOT_READY where S8 says so.
 *   Not here: the beam model, shards.  (Refinement over the same sequence: mcl_refine_poses_sequence.) */
#define MCL_SEARCH_MAX_SCANS 16
int mcl_global_search_sequence(mcl_engine_t *h, const mcl_search_config_t *c /* NULL = the defaults */, const float *scans,
                               const double *rel, int32_t n_scans, int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits,
                               int64_t *n_hits, uint64_t stats[5]);
/* SQ1 on the host, without a device: out receives n == n_headings * n_scans * 3 doubles.  MCL_ERR_INVALID_ARG for a refused
 * config, n_scans outside [1, MCL_SEARCH_MAX_SCANS], a null pointer, a rel entry that is not finite, a wrong n. */
int mcl_host_search_sequence_offsets(const mcl_search_config_t *c, const double *rel, int32_t n_scans, double *out, size_t n);
/* What a node has in hand: n_scans absolute odometry poses (n_scans x 3, one (x, y, theta) per scan, any common frame) to the rel
 * of the call above, rel_s = odom_anchor^-1 o odom_s.  With (ex, ey) = (x_s - x_a, y_s - y_a), ca = cos(theta_a), sa = sin(theta_a):
 * dx = ca * ex + sa * ey, dy = ca * ey - sa * ex, dtheta = theta_s - theta_a wrapped to (-pi, pi]; the anchor's row is exactly
 * +0.0.  All in double on the host.  MCL_ERR_INVALID_ARG for n_scans < 1, anchor outside [0, n_scans), a null pointer, a
 * pose that is not finite.  (n_scans is not held to MCL_SEARCH_MAX_SCANS: a node may keep more poses than it searches with.) */
int mcl_host_relative_poses(const double *odom, int32_t n_scans, int32_t anchor, double *rel);

/* ---- global search in heading slabs: any lattice in a fixed memory budget -----------------------------------
 * mcl_global_search and mcl_global_search_sequence hold the whole score volume and sort all of it, which caps the lattice at
 * 2^27 poses and costs about 32 bytes per pose.  mcl_global_search_streamed reports the same hits from a walk over the volume in
 * slabs of G headings: it keeps a ring of G + 2 score planes, compacts each slab's candidates and merges them into a running
 * list of the best.  Rules S1-S5 and SQ1-SQ5 hold as they stand.  With n = n_headings:
 *   ST1 identity.  The hits (pose, log_likelihood, index) and *n_hits are, bit for bit, those of mcl_global_search when
 *     n_scans == 1 and rel is NULL or zero, and those of mcl_global_search_sequence otherwise -- for the same config and scans,
 *     for every G and every budget, wherever the unstreamed call accepts the lattice.  The total order is S5's: the score, then
 *     the lower index; equal scores on either side of a slab boundary come out in index order.  Nothing depends on the order in
 *     which candidates were collected: a slab's candidates are compacted in index order (a scan over their flags) behind the
 *     running list, whose indices are all lower, and the two are sorted stably by the score's key.
 *   ST2 slabs and the ring.  G above n counts as n.  Slab t marks headings [tG, min((t + 1)G, n)).  Scores live in a ring of
 *     G + 2 heading planes: with more than one slab the linear heading hh in [-1, n] sits in plane (hh + 1) mod (G + 2) and
 *     stands for heading hh mod n, so slab t + 1 reuses the last two planes of slab t, and the wrap neighbours -- heading n - 1
 *     of heading 0, heading 0 of heading n - 1 -- are two headings scored a second time: stats reports n + 2 headings scored.
 *     With G >= n there is one slab, plane = heading, and n headings are scored, none twice.  n = 1 and n = 2 are exactly S5's:
 *     with n = 1 k +- 1 is the pose itself and is excluded, with n = 2 k + 1 and k - 1 are the same neighbour.
 *   ST3 selection.  Per slab the marking flags the candidates (S5, nms 0 or 1) and counts them on the device.  A candidate is
 *     compacted as (key, 64-bit index) unless the running list already holds max_hits entries and the candidate is no better
 *     than the last of them.  The compacted candidates are merged into the running list of the min(max_hits, found) best on the
 *     device: one stable segmented radix sort (rocPRIM) over the list and the slab's compacted candidates, whose length the
 *     device alone knows.  No whole-volume sort, no host wait and no read-back between slabs; one host wait, at the end of the
 *     call (S7).  With max_hits = 0 nothing is compacted or sorted.
 *   ST4 size.  (G + 2) * n_positions < 2^27 per slab; n_positions * n_headings < 2^40 per call; indices are 64-bit wherever they
 *     leave a slab.  mcl_global_search and mcl_global_search_sequence keep their limit of 2^27 poses and its message.
 *   ST5 budget.  mcl_host_search_slabs is the plan, on the host: G, the number of slabs ceil(n / G), and `bytes`, the sum of
 *     every buffer whose size depends on G.  With P = n_positions and L = 65536 + G P:
 *       bytes = 8 (G + 2) P  (the ring)  +  4 G P + 4 G P + 8 G P  (the slab's flags, their scan, the slab's keys)
 *             + 2 * 16 L  (the running list of 65536 and the slab's candidates behind it, twice: the sort goes from one to the other)
 *             + 262144 + floor(G P / 16)  (scratch of the scan and the sort).
 *     mcl_global_search_streamed allocates exactly those, plus what the lattice, the headings and the scans take anyway.
 *     slab_headings = 0: the largest G <= n with bytes <= budget_bytes (0: 1 GiB) that keeps ST4.  When G = 1 does not fit, or
 *     an explicit G does not, the call is refused with MCL_ERR_INVALID_ARG and the message names the bytes needed; nothing is
 *     allocated and no earlier result is disturbed.  Buffers a larger earlier plan left are reused, not shrunk.
 *   ST6 state.  The buffers are the search's own (mcl_get_search_bytes counts them); nothing of the update is touched: every
 *     later update is bit-identical to one of an engine that never searched.  No volume is kept: after a streamed search
 *     mcl_get_search_scores returns MCL_ERR_NOT_READY until an unstreamed search has run.
 *   Readiness and refusals as S8 and SQ (likelihood-field model ON, single engine only; rel may be NULL only with n_scans == 1),
 *     and MCL_ERR_INVALID_ARG for reserved != 0, slab_headings < 0, a G that breaks ST4, n_positions * n_headings >= 2^40.
 *   stats = {n_positions, poses, used beams, bytes of device memory the search's buffers have asked for so far, G, slabs,
 *     headings scored, candidates compacted}; stats may be NULL.
 *   Not here: pruning poses by bounds on partial sums, the beam model, shards.  With nms = 0 and a list that is not yet full,
 *     every pose of a slab is compacted and one workgroup sorts them: correct, and slow on a large slab. */
typedef struct {
    uint64_t budget_bytes;                  /* device bytes the slab buffers may take; 0 = the default, 1 GiB                 */
    int32_t  slab_headings;                 /* G: headings marked per slab; 0 = the largest G that fits the budget            */
    int32_t  reserved[5];                   /* must be 0                                                                      */
} mcl_search_stream_config_t;
void mcl_default_search_stream_config(mcl_search_stream_config_t *c);
int mcl_global_search_streamed(mcl_engine_t *h, const mcl_search_config_t *c /* NULL = the defaults */,
                               const mcl_search_stream_config_t *sc /* NULL = the defaults */, const float *scans,
                               const double *rel /* NULL with n_scans == 1: (0, 0, 0) */, int32_t n_scans, int32_t n_beams,
                               int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[8]);
/* ST5's plan on the host, without a device; any of the three outputs may be NULL.  MCL_ERR_INVALID_ARG for a refused config
 * (either), n_scans outside [1, MCL_SEARCH_MAX_SCANS], n_positions < 1, and what ST4 / ST5 refuse. */
int mcl_host_search_slabs(const mcl_search_config_t *c, const mcl_search_stream_config_t *sc, int64_t n_positions, int32_t n_scans,
                          int32_t *slab_headings, int32_t *n_slabs, uint64_t *bytes);

/* ---- global search under the beam model, from a shared per-position ray table ------------------------------
 * mcl_global_search ranks the lattice by the likelihood field, which ignores free space.  mcl_global_search_beam ranks the same
 * lattice (S1 / S2) by the model every update weights particles with: E4's table sum over cast rays.  All headings of a lattice
 * position share that position's rays when the scan is evenly spaced and the heading step is a multiple of its increment, so a
 * position needs M rays where a pose-by-pose search casts n_headings * B; a pose's score is a sum of table entries.
 *   B1 grid.  a_j = (double)angle_f32[j] of the beams last set.  For B >= 2: inc = (a_{B-1} - a_0) / (B - 1), M = llround(2 pi /
 *     inc); for B = 1: M = n_headings.  delta = 6.283185307179586 / (double)M.  phi_m = phi_0 + (double)m * delta with phi_0 =
 *     a_0 - 3.141592653589793, the product and the sum each rounded once.  s = M / n_headings.  The headings are S2's theta_k,
 *     unchanged, so theta_k + a_0 + j delta is the grid angle of index m(k, j) = (k s + j) mod M.  Refused with
 *     MCL_ERR_INVALID_ARG -- the message says which condition failed -- unless inc > 0, B <= M <= 16384, n_headings divides M,
 *     and max_j |a_j - (a_0 + j delta)| <= 4e-6 rad (the 2e-6 of mcl_set_beam_angles' even-spacing rule and as much again for
 *     the drift between inc and delta; a Hokuyo's 1081 angles give M = 1440 and 2.7e-7).  mcl_host_search_beam_grid is the one
 *     function the engine calls for this; it needs no device.  It writes *max_dev whenever M could be formed, refused or not;
 *     phi (NULL, or n_phi == M entries) receives the grid angles.
 *   B2 ray table.  R[p][m] is E3's step of the ray from the lattice position (x_p, y_p) of S1 at the angle phi_m: bit for bit
 *     what cast_ray returns for that (x, y, angle).  The host forms (cos phi_m, sin phi_m) in double and uploads both.  Level 2
 *     is the update's fp64 walk on the isotropic skip field with its guard, with that direction and the pose query's origin
 *     arithmetic; level 3 -- guard hits and debug_force_exact -- is the literal march with dx = cos phi_m * res taken from the
 *     uploaded table, not from a device cosine, so its additions are cast_ray's additions.  Entries are 8 bits wide when
 *     MAX_RANGE_PX <= 255, else 16.  Lattice positions are cell centres: a grid angle whose sine or cosine is +-0.5 puts every
 *     second sample on a cell edge, and every such ray is level 3 -- far more than the 0.02 % of an update.
 *   B3 score.  row_j is E2's table row of reading j; NaN, +-inf and readings out of range count as E4 counts them.  Beam j is
 *     used iff j % beam_stride == 0.  score[k * n_positions + p] = sum over the used j, ascending, of
 *     (double)L[row_j][R[p][(k s + j) mod M]], from +0.0, in order, in fp64, one lane per pose: finite or -inf, never NaN, never
 *     -0.0.  With beam_stride 1 this is E4's log-weight of a particle at that pose whose beams lie on the grid angles.  It is
 *     NOT bit for bit mcl_score_poses: the float angles sit up to 4e-6 rad off the grid, and a ray that grazes a corner may stop
 *     a step apart (profiles/beam_search.md has the measured share of differing steps).
 *   B4 hits and volume.  S5, S6 (stats[0..3]) and mcl_get_search_scores exactly as for mcl_global_search; n_positions *
 *     n_headings < MCL_MAX_TOTAL_PARTICLES.
 *   B5 tiles.  The table is made and consumed per tile of T positions: T is the largest multiple of 256 with T * M * (1 or 2
 *     bytes) <= table_budget_bytes (0: 256 MiB), no larger than n_positions rounded up to a multiple of 256, and with T * M <=
 *     2^31.  A budget below 256 positions' worth is refused (MCL_ERR_INVALID_ARG).  The volume and the hits do not depend on T.
 *     stats[4..7] = {M, T, tiles, rays of the call the literal march decided}.  mcl_get_search_beam_table copies the LAST tile's
 *     table, position-major (out[t * M + m], n == *n_positions * M) and widened to 16 bits, for tests and debugging; with out
 *     NULL and n 0 it reports the tile's first position and position count alone.  MCL_ERR_NOT_READY before a beam search and
 *     after mcl_set_map.
 *   B6 where it works.  A map and beam angles (MCL_ERR_NOT_READY otherwise); the likelihood field may be on or off, the bits are
 *     the same.  weight_mode LOG only (MCL_ERR_INVALID_ARG in PRODUCT mode).  Single engine only (MCL_ERR_UNSUPPORTED for an
 *     engine with a communicator or in a device group).  Everything S8 refuses of the
 *     config and the arguments is refused here.  Read-only as S7: buffers of the search only (mcl_get_search_bytes counts
 *     them), none of the update's scratch, one host wait; every later update is bit-identical to one of an engine that never
 *     searched.
 *   Not here: a sequence or streamed form, shards.  (Refinement under the beam model: mcl_refine_poses_beam.) */
int mcl_global_search_beam(mcl_engine_t *h, const mcl_search_config_t *c /* NULL = the defaults */, const float *obs, int32_t n_beams,
                           uint64_t table_budget_bytes /* 0 = 256 MiB */, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits,
                           uint64_t stats[8]);
int mcl_host_search_beam_grid(const float *angles, int32_t n_beams, int32_t n_headings, int32_t *M, int32_t *heading_step,
                              double *delta, double *max_dev, double *phi /* M entries, or NULL */, size_t n_phi);
int mcl_get_search_beam_table(mcl_engine_t *h, uint16_t *out, size_t n, int64_t *first_position, int64_t *n_positions);

/* ---- global search with exact pruning: bound blocks of poses, score the survivors ---------------------------
 * mcl_global_search scores every lattice pose with every used beam.  mcl_global_search_pruned reports the same hits -- pose,
 * log_likelihood bits and index, nms included -- from the blocks of poses an upper bound cannot rule out, and keeps no volume.
 * The lattice, the headings, the used beams, the score and the order of the hits are S1 - S5's.  With S = block, n = n_headings:
 *   P1 blocks.  The lattice grid (iy, ix) of S1 is cut into S x S blocks: block (by, bx) holds the lattice cells iy in [by S,
 *     by S + S), ix in [bx S, bx S + S) that the lattice has.  A block is live iff it holds at least one position; the live blocks
 *     are numbered b = 0 ... in row-major order of (by, bx).  A pair is (live block b, heading k), numbered k * n_blocks + b.
 *     mcl_host_search_blocks is the plan without a device: n_blocks, the block grid nbx x nby, w of P2 and, per live block,
 *     (bx, by, positions in it).
 *   P2 pooled field and bound table.  w = (S - 1) * stride_cells + 2.  Dp[y][x], for low corners -(w - 1) <= x <= W - 1 and
 *     -(w - 1) <= y <= H - 1, is the minimum of D' over the w x w window of cells whose low corner is (x, y); D' is the field D
 *     of LF1 inside the map and K outside (a window wholly off the map in either axis is K).  Ub[k] = max over j >= k of Lf[j],
 *     0 <= k <= K, formed on the host from the engine's table: no monotonicity of Lf is assumed.  Dp is built on the device by
 *     two separable passes (rows, then columns) and kept per (map, field, w).  mcl_host_lf_pool (out[(y + w - 1) * (W + w - 1) +
 *     (x + w - 1)], n == (W + w - 1) * (H + w - 1)) and mcl_host_search_bound_table (K + 1 entries) restate both on the host.
 *   P3 the bound of a pair.  (px_lo, py_lo) and (px_hi, py_hi) are LF4's cell coordinates of S1's cell centres of the block's
 *     first and last lattice column and row (the last clipped to the lattice).  For each used beam, in S3's order, the end point's
 *     cell of LF4 -- the two nested fmas and the floors -- is evaluated at both corners: (lx, ly) and (hx, hy).  Both are
 *     monotone in px and py, so the end point's cell of every pose of the block lies in [lx, hx] x [ly, hy].  If hx - lx < w and
 *     hy - ly < w the beam's term is Ub[Dp[ly][lx]] (Ub[K] where (lx, ly) is outside Dp's range); otherwise it is Ub[0] and the
 *     term is counted as a guard fallback (in real arithmetic hi - lo <= (S - 1) stride_cells + 1, so this is not expected).  U
 *     is the in-order fp64 sum of the terms widened to double, from +0.0.  Every term is >= the term of every pose of the block
 *     and rounded addition is monotone, so U >= the score of every pose of the block, compared as doubles, -inf included.
 *     mcl_get_search_bounds copies U in pair order after a call (n == n * n_blocks); MCL_ERR_NOT_READY before one and after
 *     mcl_set_map.
 *   P4 rounds.  The pairs are ranked by U descending, ties by pair number.  Round 1 scores the ranks [0, n_1), n_1 =
 *     min(first_pairs, pairs); first_pairs = 0 stands for max(1024, pairs / 64).  After a round the scored poses are marked by
 *     S5's rule, a neighbour in an unscored pair counting as worse; c is the score of the max_hits-th best of these provisional
 *     candidates (-inf when there are fewer) and t the U of the first unscored pair.  The call stops when nothing is unscored or
 *     c > t: every unscored pose scores <= t, so the max_hits best provisional candidates are candidates of the whole volume and
 *     no unscored pose is better than any of them, ties included.  Otherwise the next round scores up to n_{r+1} = max(j,
 *     min(2 n_r, pairs)): with fewer than max_hits candidates there is no c yet and j = 0 (the doubling alone); else j is the
 *     first rank with U < c, pairs when no rank has one.  The last possible round has scored everything.
 *     mcl_host_search_prune_next is this schedule on the host (n_scored = 0: n_1; first_below_c: j).
 *   P5 result.  hits[0 .. min(max_hits, C)) are exactly the first entries mcl_global_search reports for the same config and
 *     scan, C the candidates of the whole volume; *n_hits is the number WRITTEN: the total candidate count of S5 is not known
 *     without the whole volume.  max_hits = 0 is refused (MCL_ERR_INVALID_ARG): the call would have nothing to do.
 *   P6 where it works.  As S8 (the likelihood-field model ON, single engine only), one scan.  MCL_ERR_INVALID_ARG also for block
 *     outside {2, 4, 8}, first_pairs < 0, reserved != 0, pairs * S * S >= 2^31.  Read-only as S7: buffers of its own
 *     (mcl_get_search_bytes counts them), none of the update's; one host wait per round.  The score volume of an earlier
 *     mcl_global_search stays as it was.  Every later update and search is bit-identical to one of an engine that never called it.
 *   stats = {n_positions, poses of the lattice, used beams, bytes of device memory this call's own buffers have asked for so far
 *     (the pooled field, the block tables, U, the sort buffers over the pairs, the slot map, the store of scores and its sort
 *     buffers), pairs, pairs scored, rounds, guard fallbacks}; stats may be NULL. */
typedef struct {
    int32_t block;                          /* S: 2, 4 or 8, default 8 (S * S <= 64: one wave scores one block)               */
    int32_t first_pairs;                    /* >= 0, default 0 = max(1024, pairs / 64)                                         */
    int32_t reserved[6];                    /* must be 0                                                                      */
} mcl_search_prune_config_t;
void mcl_default_search_prune_config(mcl_search_prune_config_t *c);
int mcl_global_search_pruned(mcl_engine_t *h, const mcl_search_config_t *c /* NULL = the defaults */,
                             const mcl_search_prune_config_t *pc /* NULL = the defaults */, const float *obs, int32_t n_beams,
                             int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[8]);
int mcl_get_search_bounds(mcl_engine_t *h, double *out, size_t n);
/* P1 / P2 / P4 on the host, without a device.  blocks: n x 3 (bx, by, positions) when given, n must then equal *n_blocks. */
int mcl_host_search_blocks(const mcl_search_config_t *c, const mcl_search_prune_config_t *pc, const int8_t *data, uint32_t width,
                           uint32_t height, int32_t *n_blocks, int32_t *w, int32_t *nbx, int32_t *nby, int32_t *blocks, size_t n);
int mcl_host_lf_pool(const uint16_t *D, uint32_t width, uint32_t height, int32_t K, int32_t w, uint16_t *out, size_t n);
int mcl_host_search_bound_table(const float *lf, int32_t K, float *ub /* K + 1 entries */);
int mcl_host_search_prune_next(const mcl_search_prune_config_t *pc, int64_t pairs, int64_t n_scored, int64_t first_below_c,
                               int64_t *n_next);

/* ---- global search over a scan sequence with exact pruning -------------------------------------------------
 * mcl_global_search_sequence scores every lattice pose against every scan and keeps and sorts the whole volume.
 * mcl_global_search_sequence_pruned reports the same hits -- pose, log_likelihood bits and index, nms included -- from the (block,
 * heading) pairs a bound on the SUMMED score cannot rule out, and keeps no volume.  The lattice, the headings, the offsets, the
 * per-scan used beams, the summed score and the order of the hits are S1 - S5's and SQ1 - SQ5's; the blocks, the pooled field, the
 * rounds and the result are P1 - P5's.  scans, rel and n_scans as in mcl_global_search_sequence; c and pc as in
 * mcl_global_search_pruned.  With S = block, n = n_headings, N = n_scans:
 *   PS1 blocks, pooled field, bound table, rounds, result.  P1, P2, P4 and P5 unchanged, w = (S - 1) * stride_cells + 2 included:
 *     a displacement moves a block, it does not stretch it.  hits[0 .. min(max_hits, C)) are exactly the first entries
 *     mcl_global_search_sequence reports for the same config, scans and rel; *n_hits is the number written.
 *   PS2 offsets and beam lists.  SQ1 and SQ3 unchanged: the host forms and uploads the table of (ax_ks, ay_ks, theta_ks), the
 *     device never re-derives it; every scan has its own list of used beams, the lists are concatenated with N + 1 offsets.
 *   PS3 the bound of a pair.  Per scan s: the block's corner centres (x_lo, y_lo) and (x_hi, y_hi) of P3 each get + ax_ks / + ay_ks
 *     by one rounded fp64 add (SQ2's add) and then go through LF4's cell coordinate; with sincos(theta_ks), every used beam of scan s
 *     is evaluated at both corners exactly as in P3 -- the two nested fmas, the floors, the hi - lo < w guard, Ub[Dp[ly][lx]], Ub[K]
 *     off the pooled field, Ub[0] and a guard fallback counted otherwise.  U_s is the in-order fp64 sum of the scan's terms from
 *     +0.0, and U = ((+0.0 + U_0) + U_1) + ... in scan order.  Why it holds: a rounded add is monotone, so x_lo + ax_ks <= x_p +
 *     ax_ks <= x_hi + ax_ks for every position p of the block (y likewise) -- the scan pose of SQ2 lies between the shifted corners
 *     -- and LF4's cell coordinate and the end point's cell are monotone in it, so by P3 every term is >= the pose's term for
 *     that beam.  Rounded addition is monotone in each operand, so U_s >= acc_s of SQ4 and, fold by fold, U >= the summed score of
 *     every pose of the block, compared as doubles, -inf included (a U_s of -inf makes U -inf, and then some acc_s is -inf too).
 *     mcl_get_search_bounds returns U of the last pruned call of either kind.
 *   PS4 score of a scored pair.  Bit for bit SQ4: the scans outside, the beams inside, one accumulator per scan, folded in scan
 *     order; so a scored pose has the bits of mcl_global_search_sequence's volume.
 *   PS5 identity, where it works, buffers.  With N = 1 and rel = (0, 0, 0) the hits, U and stats[0 .. 8) are bit for bit those of
 *     mcl_global_search_pruned with the same scan (SQ7's argument, for the corners as for the positions).  The conditions and the
 *     refusals are P6's and SQ's together: the likelihood-field model ON; single engine only (MCL_ERR_UNSUPPORTED with a
 *     communicator or in a group); MCL_ERR_INVALID_ARG for n_scans outside [1, MCL_SEARCH_MAX_SCANS], a null scans or rel, a rel
 *     entry that is not finite, n_beams != B, max_hits = 0, block outside {2, 4, 8}, first_pairs < 0, reserved != 0, pairs * S * S >=
 *     2^31, and everything S8 refuses, MCL_ERR_NOT_READY where S8 says so.  Read-only: it uses the pooled field, the block tables,
 *     U, the sort buffers and the store of mcl_global_search_pruned and the beam lists, their N + 1 offsets and the offset table of
 *     mcl_global_search_sequence, and nothing else; an engine that never makes this call reports the same mcl_get_search_bytes as
 *     before after every other call.  The score volume of an earlier mcl_global_search / _sequence stays as it was.  One host wait
 *     per round.  Every later update and search is bit-identical to one of an engine that never called it.
 *   stats = the eight of mcl_global_search_pruned (used beams: of all scans, as SQ6), then [8] = N; stats may be NULL.
 *   Not here: a streamed, beam-model or sharded variant.  (Refinement over the same sequence: mcl_refine_poses_sequence.) */
int mcl_global_search_sequence_pruned(mcl_engine_t *h, const mcl_search_config_t *c /* NULL = the defaults */,
                                      const mcl_search_prune_config_t *pc /* NULL = the defaults */, const float *scans,
                                      const double *rel, int32_t n_scans, int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits,
                                      int64_t *n_hits, uint64_t stats[9]);

/* ---- pose refinement: a dense local window around each seed pose, scored against one scan (correlative scan matching on the
 *      likelihood field) ---------------------------------------------------------------------------------
 * A hit of mcl_global_search sits on the search's lattice, a cluster mean or an /initialpose is only roughly right.  For each of
 * M seed poses the refinement scores every pose of a regular window in (x, y, theta) under the likelihood-field model and
 * reports the best window pose and the likelihood-weighted mean and covariance of the window: what mcl_init_particles_mixture /
 * mcl_init_particles_gaussian take.  Read-only, as the pose query and the search are.
 *   R1 window.  nx = ny = 2 half_xy + 1, nt = 2 half_theta + 1, n_win = nx ny nt; the window index of (ix, iy, it) is
 *     w = (it ny + iy) nx + ix (ix fastest).  sx = step_xy_cells * res, res the map's float resolution widened to double, formed
 *     once on the host.  For a seed (x0, y0, t0): x = x0 + (double)(ix - half_xy) * sx, y = y0 + (double)(iy - half_xy) * sx,
 *     theta = t0 + (double)(it - half_theta) * step_theta_rad, the multiply and the add each rounded (no fma) -- on the device
 *     and in mcl_host_refine_window alike.  theta is NOT wrapped (the score takes sincos of any heading; a caller normalises if it
 *     wants to).  The device forms the window poses from the M seeds; no pose table is uploaded.
 *   R2 score.  score[m n_win + w] = LF3-LF5 of window pose w of seed m: bit for bit what mcl_score_poses returns for that pose
 *     and the same obs, with the readings of the beams j, j % beam_stride != 0, replaced by NaN (S3's rule).  The in-order fp64
 *     sum over the used beams; finite or -inf, never NaN.
 *   R3 best.  With q = dix^2 + diy^2 + dit^2 (dix = ix - half_xy, ...: the integer offset from the window centre), pose a is
 *     better than pose b iff score_a > score_b, or the scores are equal and q_a < q_b, or both are equal and w_a < w_b.  (The
 *     field is piecewise constant, so equal scores are common at fine steps: among them the pose nearest the seed wins, not the
 *     lowest index.)  The order is total, so the best pose is unique.  best = its pose by R1, best_index = its w,
 *     best_log_likelihood = its score; seed_log_likelihood = the score of the window centre.
 *   R4 moments, about the best pose b in integer step units: u_i = (ix_i - ix_b, iy_i - iy_b, it_i - it_b), w_i =
 *     exp(s_i - s_b) (0 for s_i = -inf), S = sum w_i, m_a = sum w_i u_ia / S, C_ab = sum w_i u_ia u_ib / S - m_a m_b.  With step =
 *     (sx, sx, step_theta_rad): mean_a = best_a + step_a m_a, cov_ab = (step_a step_b) C_ab + delta_ab step_a^2 / 12 (cov is
 *     row-major and exactly symmetric).  The delta term is the variance of the box a window pose stands for: it keeps cov positive
 *     definite when one pose carries all the weight, so G1 accepts every result.  weight_sum = S (1: one sharp pose; n_win: a
 *     flat window).  All fp64 in a fixed order: window pose i goes to partial sum i % 256 in ascending i, the 256 partial sums
 *     are added by a tree (l += l + 128, 64, ..., 1).  The same state gives the same bits; no atomics.
 *     A void seed (every score of its window -inf): best = the window centre, best_log_likelihood = -inf, weight_sum = 0,
 *     m = 0 and C = 0: mean = the seed, cov = the delta term alone.
 *   R5 stats = {n_win, poses scored (M n_win), used beams, bytes of device memory the refinement's buffers have asked for so
 *     far}; stats may be NULL.  mcl_get_refine_scores copies the volume of the last call (n == M n_win, seed-major);
 *     MCL_ERR_NOT_READY before any call and after mcl_set_map.
 *   R6 read-only (as Q5 / S7).  The refinement uses buffers of its own, allocated on the first call (mcl_get_refine_bytes: 0 on
 *     an engine that never refined), and none of the update's scratch or staged observation; it drops no captured graph and
 *     makes one host wait, at its end, before which only the M result records are copied back.  Every later update is
 *     bit-identical to one of an engine that never refined.
 *   R7 where it works.  A map, beam angles and the likelihood-field model ON: MCL_ERR_NOT_READY otherwise (the message says which
 *     is missing).  MCL_ERR_INVALID_ARG for half_xy or half_theta < 0, a step that is not finite and > 0, beam_stride < 1,
 *     reserved != 0, n_win > 32768, M outside [1, 4096], M n_win >= MCL_MAX_TOTAL_PARTICLES, a null seeds / obs / out,
 *     n_beams != B, a seed with a non-finite component.  Seeds off the map or inside a wall are allowed and score like any pose.
 *     Single engine only (the likelihood field is).  Seeds that refine to the same maximum are not merged, and the window is not
 *     iterated: a caller re-centres and calls again if it wants to.  The same window under the beam model, with the field on or
 *     off: mcl_refine_poses_beam, below. */
typedef struct {
    int32_t half_xy;                        /* >= 0, default 4: window columns / rows = 2 half_xy + 1                          */
    int32_t half_theta;                     /* >= 0, default 10: window headings = 2 half_theta + 1                            */
    double  step_xy_cells;                  /* > 0, finite, default 0.5: position step in map cells                            */
    double  step_theta_rad;                 /* > 0, finite, default pi / 360                                                   */
    int32_t beam_stride;                    /* >= 1, default 1 (S3's rule)                                                     */
    int32_t reserved[3];                    /* must be 0                                                                      */
} mcl_refine_config_t;
typedef struct {
    double  best[3];                        /* R3                                                                             */
    double  best_log_likelihood;
    double  seed_log_likelihood;            /* the score of the window centre                                                 */
    int64_t best_index;                     /* window index of best (R1)                                                      */
    double  mean[3];                        /* R4                                                                             */
    double  cov[9];                         /* R4, row-major                                                                  */
    double  weight_sum;                     /* sum of exp(s_i - s_best): 1 = one sharp pose, 0 = a void seed                  */
} mcl_refine_result_t;
void mcl_default_refine_config(mcl_refine_config_t *c);
/* seeds_colmajor: M x 3 column-major (x of every seed, then y, then theta), as the pose query takes its poses; out: M records */
int mcl_refine_poses(mcl_engine_t *h, const mcl_refine_config_t *c /* NULL = the defaults */, const double *seeds_colmajor,
                     int32_t M, const float *obs, int32_t n_beams, mcl_refine_result_t *out, uint64_t stats[4]);
int mcl_get_refine_scores(mcl_engine_t *h, double *out, size_t n);
int mcl_get_refine_bytes(const mcl_engine_t *h, uint64_t *bytes);
/* R1 and R3 / R4 on the host, without a device.  The window: poses is n_win x 3 row-major, n_win must match the config.  The
 * reduction: what mcl_refine_poses reports for one seed whose window scored `scores` (n_win of them; none may be NaN or +inf).
 * MCL_ERR_INVALID_ARG for a refused config (R7), a null pointer, a resolution that is not finite and > 0, a non-finite seed. */
int mcl_host_refine_window(const mcl_refine_config_t *c, const double seed[3], float resolution, double *poses, size_t n_win);
int mcl_host_refine_reduce(const mcl_refine_config_t *c, const double seed[3], float resolution, const double *scores, size_t n_win,
                           mcl_refine_result_t *out);

/* ---- pose refinement under the beam model: the same window, every pose's beams cast and summed in one kernel --
 * mcl_refine_poses ranks its window by the likelihood field, which ignores free space and which a node that runs the beam model
 * -- the reference's only model, the engine's default -- never otherwise builds.  mcl_refine_poses_beam scores the same window by
 * E4's table sum over cast rays, what every update of such a node weights particles with and what mcl_global_search_beam ranks
 * its lattice by: search, refinement and seeding under one model.  The same config and result structs.
 *   RB1 window.  R1, unchanged: the device forms the window poses from the seeds, multiply and add each rounded; no pose table
 *     is uploaded.
 *   RB2 rays.  For window pose w and beam j the step r(w, j) is Q1's: bit for bit what mcl_query_scans reports for that pose and
 *     beam, and what cast_ray returns for (x, y, theta + (double)angle_f32[j]).  The device functions of the pose query: the
 *     update's fp64 walk on the isotropic skip field with its guard, and the literal march where the guard says so, where the
 *     pose is not sane, or with debug_force_exact.  These are the float beam angles, not B1's grid: no evenly-spaced-scan
 *     condition.  No step is ever stored.
 *   RB3 score.  row_j is E2's table row of reading j; every reading counts as E4 counts it (NaN, +-inf and out-of-range readings
 *     have rows): nothing is masked, unlike R2.  Beam j is used iff j % beam_stride == 0.  The u-th used beam (u ascending with j)
 *     belongs to lane u % 64; each lane adds its (double)L[row_j][r(w, j)] in ascending u from +0.0, and the 64 lane sums are
 *     joined by the butterfly v += shfl_xor(v, off), off = 32, 16, ..., 1 (Q3's order).  With beam_stride 1 the score is bit for
 *     bit mcl_score_poses(...).log_likelihood under the beam model for that pose and the same obs; with stride s, that of an
 *     engine whose beam angles are angles[::s], given obs[::s].  Finite or -inf, never NaN.
 *   RB4 records.  R3 and R4, unchanged; mcl_host_refine_reduce on the volume is the restatement.
 *   RB5 memory and volume.  No step or range volume exists at any time: device memory is the seeds, the records, the M n_win
 *     doubles of the volume, the scan and one table-row offset per beam, and a counter; it does not depend on M n_win B.
 *     stats = {n_win, M n_win, used beams, bytes of device memory the refinement's buffers have asked for so far, rays cast
 *     (= M n_win used beams), rays the literal march decided}; stats may be NULL.  mcl_get_refine_scores returns the volume of
 *     the last refinement of either kind (one buffer, one tag), mcl_get_refine_bytes counts the buffers of both.
 *   RB6 where it works.  A map and beam angles (MCL_ERR_NOT_READY otherwise); the likelihood field may be on or off, the bits are
 *     the same: it reads neither the field nor its table.  weight_mode LOG only (MCL_ERR_INVALID_ARG in PRODUCT mode, as
 *     mcl_score_poses).  Single engine only (MCL_ERR_UNSUPPORTED for an engine with a communicator or in a device group, as B6).
 *     Everything R7 refuses of the config and the arguments is refused here with the same status, and everything R7 allows is
 *     served: up to 2^27 - 1 window poses, a wave each, in launches of 2^22 poses.  Read-only as R6: none of the
 *     update's scratch or staged observation, no captured graph dropped, one host wait at the end; every later update is
 *     bit-identical to one of an engine that never refined.
 *   Not here: a window that is iterated or re-centred, pruning of the window, shards. */
int mcl_refine_poses_beam(mcl_engine_t *h, const mcl_refine_config_t *c /* NULL = the defaults */, const double *seeds_colmajor,
                          int32_t M, const float *obs, int32_t n_beams, mcl_refine_result_t *out, uint64_t stats[6]);

/* ---- pose refinement over a scan sequence joined by odometry -------------------------------------------------
 * The sequence searches rank places one scan cannot tell apart; mcl_refine_poses on the anchor scan then re-ranks their hits by
 * exactly that scan.  mcl_refine_poses_sequence scores every window pose against S scans, each from where that pose implies the
 * robot was when the scan arrived, so the records keep the ranking of the search that made the seeds.  A seed and every window
 * pose is the robot's pose at the ANCHOR.  scans is S x n_beams, scan-major; rel is S x 3 as in mcl_global_search_sequence
 * (rel[s]: the robot's pose at scan s in its frame at the anchor; any finite rel is accepted).  The config, the window (R1), the
 * records and mcl_get_refine_scores / mcl_get_refine_bytes are mcl_refine_poses'.  With nt = 2 half_theta + 1:
 *   RS1 offsets, on the host.  For seed m and window heading index it, theta = R1's heading t0_m + (double)(it - half_theta) *
 *     step_theta_rad (the multiply and the add each rounded: one function on host and device); c = cos(theta), s = sin(theta)
 *     from the host's libm, once per (m, it).  For scan s, in SQ1's arithmetic:
 *       theta_s = theta + dtheta_s                         (one rounded add)
 *       ax = c * dx_s - s * dy_s,  ay = s * dx_s + c * dy_s   (two rounded multiplies, then one rounded add or subtract; no fma:
 *                                                            the host unit is compiled with contraction off)
 *     The table off[((m * nt + it) * S + s) * 3 + {0, 1, 2}] = {ax, ay, theta_s} is uploaded; the device never re-derives it
 *     (SQ1's reason: the host's and the device's sincos need not agree in the last bit).  mcl_host_refine_sequence_offsets is the
 *     same code without a device (n == M * nt * S * 3).  The table has M nt S rows of 24 bytes; a call with more than
 *     MCL_REFINE_SEQ_MAX_ROWS rows is refused before anything is allocated (2^21 rows: 48 MiB pinned and 48 MiB on the device;
 *     4096 seeds x 21 headings x 16 scans = 1 376 256 rows fit).  A zero rel gives ax = ay = 0 (of either sign), theta_s = theta.
 *   RS2 pose of scan s at window pose (m, w): (x_w + ax, y_w + ay, theta_s), x_w and y_w from R1, each coordinate one rounded
 *     fp64 add on the device; theta_s is NOT wrapped; the device takes sincos(theta_s) as k_refine_score takes it of a window
 *     heading.
 *   RS3 beams.  SQ3: every scan gets its own list of used beams (j % beam_stride == 0 and 0 <= r_sj < max_range_m), in beam
 *     order, by the update's own rule; the lists are concatenated on the device, S + 1 offsets say where each begins.  Scans may
 *     have different numbers of used beams, zero included.
 *   RS4 score.  acc_s is, bit for bit, what mcl_score_poses returns for the pose of RS2 and scan s (for beam_stride > 1: with the
 *     readings of the other beams replaced by NaN).  score[m n_win + w] = ((+0.0 + acc_0) + acc_1) + ... in scan order, in
 *     fp64: finite or -inf, never NaN.
 *   RS5 records.  R3 / R4 unchanged, on the summed volume (the same reduction kernel; mcl_host_refine_reduce restates it).  best
 *     and mean are anchor poses, best_log_likelihood and seed_log_likelihood summed scores.
 *   RS6 identity.  With S = 1 and rel = (0, 0, 0) the volume and the M records are bit for bit those of mcl_refine_poses with the
 *     same scan (SQ7's argument), through the sequence's own kernel: the host has no special case for S = 1.
 *   RS7 placement, stats, refusals.  R6 holds: the buffers are the refinement's own -- the table, the S + 1 offsets and a beam
 *     list of S scans beside mcl_refine_poses' (mcl_get_refine_bytes counts them) --, one host wait per call, and every later
 *     update is bit-identical to one of an engine that never refined.  stats = R5's four, with the used beams summed over the
 *     scans, then [4] = S; stats may be NULL.  Everything R7 refuses is refused with the same status; MCL_ERR_INVALID_ARG also
 *     for n_scans outside [1, MCL_SEARCH_MAX_SCANS], a null scans or rel, a rel entry that is not finite, and more than
 *     MCL_REFINE_SEQ_MAX_ROWS rows (the message names the cap and the three factors).
 *   Not here: the beam model (mcl_refine_poses_beam stays single-scan: no beam-model sequence search feeds it), shards, a search
 *     over odometry error, per-scan scores in the record (mcl_score_poses at RS2's poses gives them), a window that is iterated
 *     or re-centred. */
#define MCL_REFINE_SEQ_MAX_ROWS (1 << 21)
int mcl_refine_poses_sequence(mcl_engine_t *h, const mcl_refine_config_t *c /* NULL = the defaults */, const double *seeds_colmajor,
                              int32_t M, const float *scans, const double *rel, int32_t n_scans, int32_t n_beams,
                              mcl_refine_result_t *out, uint64_t stats[5]);
/* RS1 on the host, without a device: out receives n == M * nt * n_scans * 3 doubles.  MCL_ERR_INVALID_ARG for a refused config
 * (NULL = the defaults), M outside [1, 4096], n_scans outside [1, MCL_SEARCH_MAX_SCANS], a null pointer, a seed or a rel entry
 * that is not finite, more than MCL_REFINE_SEQ_MAX_ROWS rows, a wrong n. */
int mcl_host_refine_sequence_offsets(const mcl_refine_config_t *c, const double *seeds_colmajor, int32_t M, const double *rel,
                                     int32_t n_scans, double *out, size_t n);

/* ---- recovery by random-particle injection (augmented MCL, Probabilistic Robotics Table 8.3; AMCL's recovery_alpha_slow /
 *      recovery_alpha_fast) -------------------------------------------------------------------------------
 * Off by default.  With it on, a resampling mcl_update replaces each child, with probability p, by a pose drawn uniformly from
 * the map's free cells, where p follows from two running averages of the update likelihood.
 *   Likelihood of an update (every mcl_update, kept or resampled, and mcl_sensor_update): l = m + log(sum_w) - log(D), with
 *     m = SCALARS[0] (max log-weight), sum_w = SCALARS[1], D = N for a resampled update and mcl_sensor_update, D = the previous
 *     update's sum_w for an update that kept its particles (resample_neff_permille): log sum over the prior normalised weights
 *     of p_i.  m = -inf gives l = -inf.  per_beam = 1 (the default) divides l by the engine's beam count.
 *   Averages: S (slow) and F (fast) are each unset (NaN at the ABI) or a value in [-inf, +inf).  Fold: S <- l if unset, else
 *     logaddexp(S + log1p(-alpha_slow), l + log(alpha_slow)); the same for F with alpha_fast.  logaddexp(a, b) = hi +
 *     log1p(exp(lo - hi)), -inf when both are -inf.  A NaN l leaves both unchanged.  Host double, mcl_host_recovery_step.
 *   Injection: p = 0 when S or F is unset or S = -inf, else clamp(1 - exp(F - S), 0, 1); threshold T = floor(p * 2^53).  A
 *     resampling update with T > 0 unsets S and F before folding in its own l; an update that keeps its particles injects
 *     nothing and resets nothing.
 *   Per child g of update u (Philox as for the other draws): stream 8 gives coin = bits53(v0, v1), injected iff coin < T, and
 *     pick = bits53(v2, v3): cell = free[umulhi(pick << 11, n_free)], x = col * res + ox, y = row * res + oy (mcl_init_global's
 *     rule); stream 9 gives theta = (bits53(v0, v1) * 2^-53 - 0.5) * 2 pi.  An injected child skips the parent search and the
 *     motion model, and its resample index is -1.  Every other child is bit-identical to the child of the same update with
 *     recovery off.  With KLD on the injected pose is the child's counted sample.
 *   mcl_set_particles*, mcl_init_*, mcl_set_map, mcl_set_beam_angles and mcl_set_recovery unset S and F.
 *   MCL_ERR_INVALID_ARG unless 0 < alpha_slow < alpha_fast <= 1 (finite), per_beam is 0 or 1 and reserved is 0.
 *   MCL_ERR_UNSUPPORTED for weight_mode PRODUCT, an engine with a communicator or in a device group, mcl_comm_create while it is
 *     on and every mcl_stage_* call while it is on (single engine only).  MCL_ERR_NOT_READY for an update with T > 0 on a map
 *     without free cells (before anything is launched). */
typedef struct {
    double alpha_slow, alpha_fast;          /* default 0.001, 0.1                                                             */
    int32_t per_beam;                       /* 1 (default): l per beam; 0: AMCL's raw form                                    */
    int32_t reserved;                       /* must be 0                                                                      */
} mcl_recovery_config_t;
void mcl_default_recovery_config(mcl_recovery_config_t *c);
int mcl_set_recovery(mcl_engine_t *h, const mcl_recovery_config_t *c);    /* NULL = off (the default)                       */
/* state = {S, F, p of the next update}; *injected_last = injected children of the last update (0 after one that injected
 * nothing).  Either pointer may be NULL. */
int mcl_get_recovery_state(mcl_engine_t *h, double state[3], int64_t *injected_last);
/* sets S, F (NaN = unset; +inf and recovery off are refused): to restore a saved state, or to force p */
int mcl_set_recovery_state(mcl_engine_t *h, const double state[2]);
/* the rules above on the host, without a device: folds the likelihood of one update into in = {S, F} (reset: unset them
 * first) and gives out = {S, F} and the p of the next update.  MCL_ERR_INVALID_ARG for a refused config, a null pointer,
 * denom that is not > 0 or n_beams < 1. */
int mcl_host_recovery_step(const mcl_recovery_config_t *c, const double in[2], int32_t reset, double max_logw, double sum_w,
                           double denom, int32_t n_beams, double out[2], double *p_next);
/* The proposal of an injecting update (sensor resetting, Lenser & Veloso 2000): a Gaussian mixture -- the hits of
 * mcl_global_search* refined by mcl_refine_poses*, say -- from which the next injecting update draws its injected children instead
 * of from the free cells.  Off by default.
 *   P1 components.  1 <= M <= 4096.  means: M x 3, finite.  covs: M x 9 row-major, each by G1 of mcl_init_particles_gaussian (the
 *     same function: symmetric, positive semi-definite, zero pivots allowed).  weights: M, finite and >= 0, with an in-order double
 *     sum s_M that is finite and > 0; NULL = all 1.  n_components = 0 clears the proposal (the other pointers are not read).
 *     MCL_ERR_INVALID_ARG otherwise, the message naming the component; nothing changes then.
 *   P2 thresholds.  s_k = the in-order double prefix sum of the weights; t_k = (uint64)floor((s_k / s_M) * 2^53) for k < M - 1,
 *     t_{M-1} = 2^53.  The component of an injected child is the first k with pick < t_k, pick = bits53(v2, v3) of stream 8 (the
 *     53 bits the uniform rule turns into a free cell).  A zero-weight component has an empty range and is never drawn.  The
 *     device searches [0, M - 1] whatever the uploaded words hold.
 *   P3 pose.  Child g of update u draws n0, n1 from Philox stream 10 and n2 from stream 11, counter (g, u, stream) as streams 8 / 9,
 *     by G1's Box-Muller (u1 = (bits53(v0, v1) + 1) 2^-53, u2 = bits53(v2, v3) 2^-53; n0 = r cos(2 pi u2), n1 = r sin(2 pi u2) with
 *     r = sqrt(-2 log u1); n2 the cosine branch of stream 11).  With the component's mean (mx, my, mt) and factor L:
 *     x = mx + L00 n0; y = my + (L10 n0 + L11 n1); theta = normalize_angle(mt + (L20 n0 + L21 n1 + L22 n2)).  Stream 9 is not drawn.
 *   P4 what does not change.  Which children are injected (coin < T, the same T), that an injected child skips the parent search
 *     and the motion model, reports parent -1, is the sample KLD counts and is counted in injected_last; how the update plans its
 *     ray stage; every non-injected child, bit for bit.
 *   P5 one shot.  The first resampling update that runs with T > 0 consumes the proposal: the update after it injects from the free
 *     cells again, so a proposal made from an old scan is never drawn from at a later kidnap.  Updates with T = 0, updates that keep
 *     their particles and mcl_sensor_update leave it in place; mcl_set_map clears it; setting or initialising particles, the beams
 *     or the recovery config does not.  Setting it changes neither S nor F and drops no captured graph.
 *   P6 free cells.  An injecting update with a proposal in place needs no free cell (MCL_ERR_NOT_READY is the uniform rule's).
 *   P7 MCL_ERR_UNSUPPORTED for an engine with a communicator or in a device group and for weight_mode PRODUCT, as mcl_set_recovery.
 *     It may be set while recovery is off; it is then never consumed. */
int mcl_set_recovery_proposal(mcl_engine_t *h, int32_t n_components, const double *means /* M x 3 */,
                              const double *covs /* M x 9, row-major */, const double *weights /* M, NULL = all equal */);
/* the proposal in place: *n_components (0: none), its thresholds (M words) and factors (M x 9: mean x, y, theta, L00 L10 L11 L20
 * L21 L22).  Any output may be NULL. */
int mcl_get_recovery_proposal(const mcl_engine_t *h, int32_t *n_components, uint64_t *thresholds, double *factors);
/* P1 / P2 on the host, without a device: the one function the engine itself calls to form what it uploads.  thresholds and
 * factors may be NULL (the arguments are then only checked).  MCL_ERR_INVALID_ARG as P1, and for n_components = 0. */
int mcl_host_recovery_proposal(int32_t n_components, const double *means, const double *covs, const double *weights,
                               uint64_t *thresholds, double *factors);

/* ---- likelihood-field ("endpoint") sensor model (Probabilistic Robotics §6.4; AMCL's laser_model_type likelihood_field;
 *      DESIGN.md §4.10) ---------------------------------------------------------------------------------------------------
 * Off by default (the beam model above).  With it on, the log-weights of mcl_update, mcl_update_scan and mcl_sensor_update come
 * from the end points of the beams looked up in a distance field instead of from ray casts; everything after the log-weights
 * (weights, resampling, adaptive resampling, KLD, recovery, clusters, expected pose) is unchanged.
 *   Field: D[c] = min(d2(c), K), d2 the exact integer squared distance in cells from cell c to the nearest occupied cell (value
 *     > 50; a map without one: D = K everywhere), K = ceil((max_occ_dist_m / res)^2), res the map's float resolution widened to
 *     double.  H x W uint16, row-major; built on the device when the model is switched on with a map set and on every mcl_set_map
 *     while it is on.  K > 65535 is refused (MCL_ERR_INVALID_ARG) by mcl_set_likelihood_field / mcl_set_map.
 *   Table: Lf[k] = (float)(log(z_hit * exp(-(k * res^2) / (2 sigma^2)) + z_rand / max_range_m) * (1 / squash_factor)) for
 *     0 <= k < K, Lf[K] the same with the distance max_occ_dist_m (-(m * m) / (2 sigma^2)); host double, log(0) = -inf.
 *   Beams used: 0 <= r_j < max_range_m (NaN, +-inf, negative and max-range readings contribute nothing).
 *   End point: cell (floor((x + r_j cos(theta + a_j) - ox) / res), floor((y + r_j sin(theta + a_j) - oy) / res)) in fp64;
 *     off the map it reads K.  logw = sum over the used beams, in beam order, of (double)Lf[D[cell]].
 *   MCL_ERR_INVALID_ARG for sigma_hit_m or max_occ_dist_m not finite and > 0, a z_* negative or not finite, z_hit = z_rand = 0,
 *     reserved != 0.  MCL_ERR_UNSUPPORTED for weight_mode PRODUCT, an engine with a communicator or in a device group,
 *     mcl_comm_create while it is on, every mcl_stage_* call while it is on, and the ray read-backs (mcl_get_ray_steps*,
 *     mcl_get_ray_kernel_id, mcl_get_ray_kernel_variant) after a likelihood-field update.  Switching the model (either way)
 *     drops what the beam model's updates cache between updates: the next update plans as after mcl_set_particles. */
typedef struct {
    double z_hit, z_rand;                   /* default 0.5, 0.5                                                               */
    double sigma_hit_m;                     /* default 0.2                                                                    */
    double max_occ_dist_m;                  /* default 2.0 (AMCL's laser_likelihood_max_dist)                                 */
    int32_t reserved[2];                    /* must be 0                                                                      */
} mcl_likelihood_field_config_t;
void mcl_default_likelihood_field_config(mcl_likelihood_field_config_t *c);
int mcl_set_likelihood_field(mcl_engine_t *h, const mcl_likelihood_field_config_t *c);   /* NULL = beam model (the default) */
/* the device field (H x W uint16) and table (K + 1 floats); MCL_ERR_NOT_READY while the model is off or no map is set.  The
 * table: out may be NULL (n is then ignored), *K (may be NULL) receives K. */
int mcl_get_likelihood_field(mcl_engine_t *h, uint16_t *out, size_t n);
int mcl_get_likelihood_table(mcl_engine_t *h, float *out, size_t n, int32_t *K);
/* the same on the host, without a device (the restatements the device is tested against); cfg supplies max_range_m and
 * squash_factor */
int mcl_host_likelihood_field(const int8_t *data, uint32_t width, uint32_t height, float resolution,
                              const mcl_likelihood_field_config_t *c, uint16_t *out, size_t n);
int mcl_host_likelihood_table(const mcl_config_t *cfg, const mcl_likelihood_field_config_t *c, float resolution, float *out,
                              size_t n, int32_t *K);

/* ---- beam skipping for the likelihood field (AMCL's likelihood_field_prob with do_beamskip, beam_skip_distance,
 *      beam_skip_threshold, beam_skip_error_threshold) ---------------------------------------------------------
 * Off by default; it can only be on while the likelihood field is.  A beam whose measured end point lies near a mapped obstacle
 * for only a small share of the particle set -- an obstacle that is not in the map -- is left out of every particle's weight.
 * It applies to mcl_update, mcl_update_scan and mcl_sensor_update and only changes how the log-weights are produced; everything
 * after them (weights, resampling, adaptive resampling, KLD, recovery, clusters, expected pose) is unchanged.  The side calls
 * (mcl_score_poses, every mcl_global_search*, every mcl_refine_poses*, and with them propose_from_scan of the Python binding)
 * score poses, not a set: they ignore it.
 *   BS1 agreement.  Ka = ceil((distance_m / res)^2), the expression K is formed with (res the float resolution widened), held
 *     at 65536.  A used beam (LF3) of a particle agrees iff its end cell (LF4, the same rotation-form arithmetic) is on the map
 *     and D[cell] < Ka -- for an integer squared distance d^2 exactly d * res < distance_m.  Off the map a beam never agrees
 *     (AMCL's !MAP_VALID).  With Ka > K every end point on the map agrees, as with AMCL's clamped occ_dist.
 *   BS2 counts.  cnt[j] = the number of the update's n particles (the set this update weights: after resampling and motion)
 *     whose beam j agrees.  Integers added in any order: exact, and the same for every schedule.
 *   BS3 keep.  AMCL keeps a beam iff cnt / (double)n > threshold.  The host forms, once per update, min_count = the least integer
 *     c in [1, n + 1] with (double)c / (double)n > threshold (searched up and down from floor(threshold * n): exact whatever the
 *     rounding); the device compares integers: kept iff cnt[j] >= min_count.
 *   BS4 too many skipped.  n_skipped = the number of used beams not kept; min_skipped = the least integer s >= 0 with
 *     (double)s >= error_threshold * (double)n_used, held at n_used + 1.  If n_skipped >= min_skipped, integrate_all = 1 and every
 *     used beam is kept (AMCL: the filter may have converged to a wrong pose).  AMCL's loop also counts out-of-range beams as
 *     skipped; here only used beams enter either side of the comparison.  error_threshold = 0 always integrates all, a value
 *     above 1 never does (a scan without a used beam has nothing to keep either way: 0 >= 0 sets integrate_all).
 *   BS5 log-weight.  logw_i = sum over the kept used beams, in beam order, of (double)Lf[D[cell_ij]]: LF5 over the kept beams, the
 *     in-order fp64 sum.  So an update with beam skipping equals, bit for bit, the same update without it on the scan whose
 *     skipped beams read NaN: log-weights, weights, resample indices, the next particles, the pose, the KLD state and the
 *     recovery averages (recovery keeps dividing by B, as it does for unused beams).
 *   BS6 state.  After such an update mcl_get_beam_skip_state reads, per scan beam j in [0, B): counts[j] (0 for an unused beam)
 *     and kept[j] (0 not used, 1 summed, 2 skipped), and the record below.  counts, kept and st may each be NULL; n must be B.
 *     MCL_ERR_NOT_READY before the first such update and while the feature is off.
 *   MCL_ERR_INVALID_ARG for distance_m not finite and > 0, threshold outside [0, 1], error_threshold not finite and >= 0,
 *     reserved != 0.  mcl_set_beam_skip returns MCL_ERR_NOT_READY while the likelihood field is off;
 *     mcl_set_likelihood_field(NULL) switches beam skipping off too, re-setting the field's config while it is on keeps it.  The
 *     likelihood field's refusals (communicator, device group, mcl_stage_*, weight_mode PRODUCT) cover this feature: it cannot be
 *     on without the field.  Agreement is counted over the set being weighted, with no memory across updates; there is no pz^3
 *     term and no gaussian_norm. */
typedef struct {
    double distance_m;                      /* default 0.5 (AMCL's beam_skip_distance)                                        */
    double threshold;                       /* default 0.3 (beam_skip_threshold)                                              */
    double error_threshold;                 /* default 0.9 (beam_skip_error_threshold)                                        */
    int32_t reserved[2];                    /* must be 0                                                                      */
} mcl_beam_skip_config_t;
typedef struct {
    int64_t n_particles, min_count;         /* BS2's n, BS3                                                                   */
    int32_t n_used, n_kept, n_skipped, min_skipped, integrate_all, ka;     /* n_kept = n_used when integrate_all              */
} mcl_beam_skip_state_t;
void mcl_default_beam_skip_config(mcl_beam_skip_config_t *c);
int mcl_set_beam_skip(mcl_engine_t *h, const mcl_beam_skip_config_t *c);                 /* NULL = off (the default) */
int mcl_get_beam_skip_state(mcl_engine_t *h, uint32_t *counts, uint8_t *kept, size_t n, mcl_beam_skip_state_t *st);
/* BS1 / BS3 / BS4 and the mask on the host, without a device: the functions the engine itself forms its thresholds with.  Any
 * output may be NULL.  n_particles in [1, 2^31), n_used >= 0; counts_used / kept_used hold the used beams only, kept_used in
 * BS6's coding (1 summed, 2 skipped); counts_used may be NULL only with n_used = 0. */
int mcl_host_beam_skip_thresholds(const mcl_beam_skip_config_t *c, float resolution, int64_t n_particles, int32_t n_used,
                                  int32_t *ka, int64_t *min_count, int32_t *min_skipped);
int mcl_host_beam_skip_plan(const mcl_beam_skip_config_t *c, const uint32_t *counts_used, int32_t n_used, int64_t n_particles,
                            uint8_t *kept_used, int32_t *n_skipped, int32_t *integrate_all);

/* ---- sensor mount: a lidar that is not at the robot's origin, and a further scan fused into the same posterior
 *      (AMCL's static base -> laser transform) -------------------------------------------------------------------
 * Off by default.  The particles stay base poses; only the sensor stages see the mount.
 *   SM1 the mount.  m = (mx, my, mtheta): the sensor's pose in the base frame, metres and radians, every component finite,
 *     |mtheta| <= 2 pi (else MCL_ERR_INVALID_ARG, nothing touched).  (0, 0, 0), with either sign of zero, means no mount: the state
 *     after mcl_create.
 *   SM2 the sensor pose of a base pose (x, y, theta), fp64, in this order, no contraction: s, c = sincos(theta);
 *     xs = x + (c mx - s my); ys = y + (s mx + c my); thetas = theta + mtheta (one rounded add, not wrapped).  A non-finite input
 *     gives what these operations give; the sensor stage treats (xs, ys, thetas) exactly as it treats a particle there.
 *   SM3 what sees it.  mcl_update, mcl_update_scan, mcl_sensor_update, mcl_sensor_update_fuse, the staged calls (mcl_stage_rays*)
 *     and the device group, with every ray kernel and every tail, the likelihood field with and without beam skipping, and
 *     mcl_query_scans / mcl_score_poses, whose input poses are base poses.  The kernels are handed the sensor poses; the sort keys,
 *     the bounding box and the tile layout are theirs.
 *   SM4 what does not.  Resampling, motion, KLD bins, clusters, recovery injection, the initialisers, the weights and the expected
 *     pose, mcl_get_particles, mcl_sample_particles and mcl_particle_mean work on the base poses.  Every mcl_global_search* and
 *     mcl_refine_poses* is defined in the SENSOR frame and ignores the mount: its poses are sensor poses, and
 *     mcl_host_sensor_unmount / mcl_host_sensor_mount_cov bring a hit, a mean and a covariance to the base frame.
 *   SM5 off is off.  With no mount nothing new is allocated or launched and every result keeps its bits.  With a mount the
 *     resampling kernel prepares nothing for the ray stage, which makes its own constants, keys and layout from the sensor poses.
 *   SM6 setting it voids the captured graphs and the ordering layout, like mcl_set_beam_angles; particles, weights, beams, the map
 *     and every option stay.  The scratch of the sensor poses (three columns of max_particles doubles) is reserved by the first
 *     sensor stage that runs with a mount.
 * mcl_mount_poses runs SM2 on the device with the current mount on k <= 65536 arbitrary poses (column-major in and out, buffers of
 * its own): bit for bit what the stages use; with no mount it copies.  mcl_get_sensor_poses reads the poses the last sensor stage
 * actually read: MCL_ERR_NOT_READY when none has run with a mount or the particles have changed since, MCL_ERR_INVALID_ARG when n
 * is not that stage's count.
 * mcl_sensor_update_fuse weighs a FURTHER scan into the same posterior: the work of mcl_sensor_update with the current beams, mount
 * and sensor model (beam skipping applies to this scan alone), then logw_i <- prev_i + new_i -- one rounded fp64 add, prev exactly
 * what mcl_get_log_weights returned before the call, -inf stays -inf -- and the unchanged weight stage on the sum (E5 included;
 * with adaptive resampling the carry is that of the sum).  MCL_ERR_NOT_READY unless the last weighting call (mcl_update*,
 * mcl_sensor_update, this call) was on the current particle set: mcl_set_particles*, the initialisers, the staged calls (every
 * staged resample, every staged ray stage) and mcl_set_map void that; the beams, the mount, the likelihood field and beam skipping may change in between.  weight_mode LOG,
 * single engine only (MCL_ERR_UNSUPPORTED otherwise).  It counts no KLD bins and folds nothing into the recovery averages. */
int mcl_set_sensor_mount(mcl_engine_t *h, const double mount[3]);
int mcl_get_sensor_mount(const mcl_engine_t *h, double out[3]);
int mcl_mount_poses(mcl_engine_t *h, const double *poses_colmajor, int64_t k, double *out_colmajor);
int mcl_get_sensor_poses(mcl_engine_t *h, double *out_colmajor, int64_t n);
int mcl_sensor_update_fuse(mcl_engine_t *h, const float *obs, int32_t n_beams);
/* On the host, no device: SM2 with the host's libm over n >= 1 column-major poses; its inverse b = s (-) m: theta = thetas - mtheta,
 * then x = xs - (c mx - s my), y = ys - (s mx + c my) with s, c = sincos(theta); and J cov J^T (row-major 3 x 3) with the
 * Jacobian of SM2 at the base pose `pose` (to_base = 0) or of the inverse at the sensor pose `pose` (to_base = 1).
 * MCL_ERR_INVALID_ARG for a mount SM1 refuses, a null pointer, n < 1, a non-finite pose or covariance entry (mount_cov). */
int mcl_host_sensor_mount(const double mount[3], const double *poses_colmajor, int64_t n, double *out_colmajor);
int mcl_host_sensor_unmount(const double mount[3], const double *poses_colmajor, int64_t n, double *out_colmajor);
int mcl_host_sensor_mount_cov(const double mount[3], const double pose[3], const double cov9[9], int to_base, double out9[9]);

/* ---- scan de-skew: per-beam sensor offsets, for a scan taken while the robot moves ------------------------------
 * Off by default.  A table of B triples o_j = (ox_j, oy_j, dtheta_j): the sensor's pose when beam j was taken, expressed in the
 * sensor's frame at the scan's reference time -- the time at which the particles are the robot's pose.  S_i = (xs, ys, thetas) is
 * particle i's sensor pose: SM2's output with a mount, the particle itself without one.
 *   DS1 effective angle.  a'_j = (float)((double)a_j + dtheta_j); its direction pair (cos, sin) is formed of that float exactly as
 *     mcl_set_beam_angles forms a beam's.  In directions, an engine with offsets is an engine whose beam angles are a'.  The table
 *     is formed on the host once per mcl_set_beam_offsets (B sincos) and lives in buffers of its own: the engine's own beam
 *     directions and angles, and everything the side calls read, stay untouched.
 *   DS2 origin.  With (s, c) = sincos(thetas), taken once per particle as the ray stage takes it: x_ij = xs + (c ox_j - s oy_j),
 *     y_ij = ys + (s ox_j + c oy_j) -- SM2's arithmetic and order, fp64, no contraction.  Its pixel position is
 *     ((x_ij - origin_x) / res, (y_ij - origin_y) / res); a garbage heading (NaN, |thetas| >= 1e6) gives NaN, as for a particle.
 *   DS3 step.  r_ij is E3's step of cast_ray from (x_ij, y_ij) at angle thetas + (double)a'_j: bit for bit what mcl_query_scans
 *     returns for beam j of the pose (x_ij, y_ij, thetas) on an engine whose angles are a'.  debug_force_exact 1 and 2 are honoured.
 *   DS4 weight.  The rows are E2 of the scan, unchanged; logw_i = sum_j (double)L[row_j][r_ij] (E4), added in Q3's fixed order (lane
 *     strides, then the butterfly): the same state gives the same bits, also for tables outside E4's exactness condition.
 *   DS5 likelihood field.  The used beam's pair becomes ((ox_j + r_j c'_j) inv_res, (oy_j + r_j s'_j) inv_res) with DS1's pair
 *     (c'_j, s'_j); LF3-LF5 and BS1-BS5 are unchanged.  Only the update path forms its pairs so: mcl_query_scans / mcl_score_poses,
 *     every mcl_global_search* and every mcl_refine_poses* ignore the offsets, as they ignore beam skipping.
 *   DS6 off and zero.  NULL is off: nothing is launched, allocated or changed, every result keeps its bits.  A table of zeros is on
 *     and takes the new path; under both models its log-weights equal the plain update's bit for bit.  mcl_set_beam_angles turns
 *     the offsets off: the table belonged to the old beams.
 * Honoured by mcl_update, mcl_update_scan, mcl_sensor_update and mcl_sensor_update_fuse, under the beam model (one kernel,
 * MCL_RAYS_DESKEW, one launch; ray steps are kept where cfg.keep_ray_steps asks) and under the likelihood field with and without beam
 * skipping, with and without a mount.  With offsets on an update runs launch by launch (no one-workgroup tail, no captured graph),
 * and the resampling kernel prepares nothing for the ray stage.  Turning them on or off voids the captured graphs once; a new table
 * while they are on is one asynchronous upload on the engine's stream, with no host wait and no reset.
 * mcl_set_beam_offsets: MCL_ERR_NOT_READY before the beam angles exist; MCL_ERR_INVALID_ARG for n_beams != B or a non-finite
 * component; MCL_ERR_UNSUPPORTED with a communicator or in a device group (the mcl_stage_* calls are refused while offsets are on),
 * with weight_mode PRODUCT, and with cfg.ray_kernel other than MCL_RAYS_AUTO.  mcl_get_beam_offsets: the table as given (zeros when
 * off), DS1's float angles (the beam angles when off), whether they are on; any output may be NULL.
 * mcl_beam_origins runs DS2 on the device for k <= 65536 given SENSOR poses (column-major 3 x k) and the current table (zeros when
 * off): x[k * B] then y[k * B], pose-major -- bit for bit the origins the ray stage casts from for a sane heading; for a garbage
 * heading (NaN, |thetas| >= 1e6) the stage gives the ray a NaN pixel position and marches it literally from this origin (DS2), and
 * this call returns what DS2's additions give, finite or not.
 * On the host, no device.  mcl_host_scan_motion_offsets is the constant-twist rule a node needs.  motion = (u, v, w): the base's
 * body-frame twist integrated over the scan's unit of t (the odometry twist times the sweep duration); t: one stamp per beam
 * (NULL: j / (B - 1), 0 for B = 1); t_ref: the reference time in the same unit; mount: SM1's (NULL: the sensor at the base).
 *   DM1 with tau = t_j - t_ref and theta = tau w: Delta = (tau (A u - Bc v), tau (Bc u + A v), theta), A = sin theta / theta,
 *     Bc = (1 - cos theta) / theta; for |theta| < 1e-8 the series A = 1 - theta^2 / 6, Bc = theta / 2.
 *   DM2 o_j = m^-1 o Delta o m: the sensor's pose under Delta (SM2's lines), then R(-mtheta) (that position - (mx, my)); its heading
 *     component is theta whatever the mount.  A zero twist gives a table of zeros.
 * MCL_ERR_INVALID_ARG for a non-finite input, a mount SM1 refuses, a null pointer, n_beams < 1.
 * mcl_host_beam_offset_table is DS1 as the setter runs it (effective_angles: B floats; dirs: cos[B] then sin[B]; either may be
 * NULL), mcl_host_beam_offset_pairs DS5's pair of every beam (pairs: x[B] then y[B], in cells) from such a table's dirs. */
int mcl_set_beam_offsets(mcl_engine_t *h, const double *offsets_colmajor /* 3 x n_beams: ox, oy, dtheta; NULL = off */, int32_t n_beams);
int mcl_get_beam_offsets(const mcl_engine_t *h, double *offsets_colmajor, float *effective_angles, int32_t n_beams, int32_t *on);
int mcl_beam_origins(mcl_engine_t *h, const double *sensor_poses_colmajor, int64_t k, double *xy /* x[k*B] then y[k*B], pose-major */);
int mcl_host_scan_motion_offsets(const double motion[3], const double mount[3] /* NULL: sensor at the base */,
                                 const double *t /* n_beams stamps; NULL: j/(B-1), 0 for B = 1 */, double t_ref,
                                 int32_t n_beams, double *offsets_colmajor);
int mcl_host_beam_offset_table(const float *angles, const double *offsets_colmajor, int32_t n_beams, float *effective_angles, double *dirs);
int mcl_host_beam_offset_pairs(const float *ranges, const double *offsets_colmajor, const double *dirs, int32_t n_beams, double resolution,
                               double *pairs);

/* ---- odometry motion models and covariance-based pose initialisation (Probabilistic Robotics Table 5.6,
 *      sample_motion_model_odometry; AMCL's robot_model_type differential / omnidirectional with alpha1..alpha5;
 *      DESIGN.md §4.11) ---------------------------------------------------------------------------------------------------
 * Off by default (MCL_MOTION_REFERENCE: the reference's arc plus map-frame noise of fixed size, motion_dispersion_*).
 *   M1 action.  With DIFF or OMNI, action = (dx, dy, dtheta): the robot's displacement since the previous update, expressed in
 *     the robot's frame at the previous update (the odometry delta turned by minus the old odometry heading).  (forward, 0, yaw)
 *     is a valid DIFF action.  With REFERENCE nothing changes (action[1] stays unused).
 *   M2 angles.  norm(z) = atan2(sin z, cos z); adiff(a, b): a = norm(a); b = norm(b); d1 = a - b; d2 = 2 pi - |d1|; if d1 > 0:
 *     d2 = -d2; return |d1| < |d2| ? d1 : d2.  Used on the host only.
 *   M3 per-update scalars, host double, mcl_host_motion_scalars (the one function the engine itself calls for them):
 *     trans = sqrt(dx^2 + dy^2); ft = floor_trans_m, fr = floor_rot_rad.
 *     DIFF: rot1 = trans < 0.01 ? 0 : atan2(dy, dx); rot2 = adiff(dtheta, rot1); r1n = min(|adiff(rot1, 0)|, |adiff(rot1, pi)|),
 *       r2n likewise from rot2 (a robot may reverse without a half turn of noise);
 *       s1 = sqrt(a1 r1n^2 + a2 trans^2 + fr^2), st = sqrt(a3 trans^2 + a4 r1n^2 + a4 r2n^2 + ft^2),
 *       s2 = sqrt(a1 r2n^2 + a2 trans^2 + fr^2).  out = {rot1, trans, rot2, s1, st, s2, 0, 0}.
 *     OMNI: rot = dtheta, bearing = atan2(dy, dx); st = sqrt(a3 trans^2 + a1 rot^2 + ft^2), sr = sqrt(a4 rot^2 + a2 trans^2 + fr^2),
 *       ss = sqrt(a1 rot^2 + a5 trans^2 + ft^2).  out = {bearing, trans, rot, st, sr, ss, 0, 0}.
 *   M4 floors.  With every sigma 0 each child equals its parent, so the set of a standing robot collapses onto duplicates (AMCL
 *     only updates after the robot moved; an engine updated on every tick does not).  The two floors are a standard deviation
 *     added in quadrature; 0 (the default) is AMCL exactly.
 *   M5 per child (normals n0, n1, n2 exactly the three the reference model draws: Philox streams 0 and 1, or row m of the injected
 *     normals), fp64:
 *     DIFF: r1 = rot1 - s1 n0; t = trans - st n1; r2 = rot2 - s2 n2; x' = x + t cos(theta + r1); y' = y + t sin(theta + r1);
 *       theta' = normalize_angle(theta + (r1 + r2)).
 *     OMNI: t = trans + st n0; r = rot + sr n1; s = ss n2; b = bearing + theta; x' = x + (t cos b + s sin b);
 *       y' = y + (t sin b - s cos b); theta' = normalize_angle(theta + r).
 *     normalize_angle: subtract / add 2 pi while outside [-pi, pi].  motion_dispersion_* are not used by DIFF / OMNI.
 *   M6 what does not change: the draw of the parent, the Philox streams and counters, what KLD counts (the parent's pose before the
 *     motion), recovery (an injected child skips the motion model whatever the model), kept updates of adaptive resampling (every
 *     particle moves by M5), mcl_sensor_update (no motion), the per-particle constants and sort keys made from the moved pose.
 *     The staged and sharded updates (mcl_stage_*, mcl_comm_update, mcl_group_update) honour the engine's model; every rank must
 *     set the same config (not checked).  Children are bit-identical for any number of shards.
 *   G1 Gaussian init.  cov row-major, symmetric to 1e-12 max|cov| and positive semi-definite.  The host forms the lower Cholesky
 *     factor L in double; a pivot p with |p| <= 1e-12 max diag counts as 0 and zeroes its column (a covariance without heading
 *     uncertainty is allowed), a pivot below that is MCL_ERR_INVALID_ARG, as are non-finite entries.  Particle g draws n0, n1, n2
 *     as mcl_init_particles_pose does (streams 5 / 6, the init counter) and gets x = mx + L00 n0; y = my + (L10 n0 + L11 n1);
 *     theta = normalize_angle(mt + (L20 n0 + L21 n1 + L22 n2)); weights 1 / n_total; everything else as mcl_init_particles_pose.
 *   MCL_ERR_INVALID_ARG: unknown model, reserved != 0, a negative or non-finite alpha or floor, a null output.  The two
 *     mcl_host_motion_* functions restate DIFF and OMNI only (MCL_ERR_INVALID_ARG for REFERENCE); a non-finite action is passed
 *     through (NaN children).  Setting the model touches no particle state, drops no captured graph and resets no recovery average. */
typedef enum { MCL_MOTION_REFERENCE = 0, MCL_MOTION_DIFF = 1, MCL_MOTION_OMNI = 2 } mcl_motion_model;
typedef struct {
    int32_t model;                          /* mcl_motion_model                                                               */
    int32_t reserved;                       /* must be 0                                                                      */
    double alpha1, alpha2, alpha3, alpha4, alpha5;   /* AMCL's, default 0.2 each; finite, >= 0                                */
    double floor_trans_m, floor_rot_rad;    /* default 0, 0; finite, >= 0 (M4)                                                */
} mcl_motion_config_t;
void mcl_default_motion_config(mcl_motion_config_t *c);                  /* model = MCL_MOTION_DIFF, AMCL's defaults          */
int mcl_set_motion_model(mcl_engine_t *h, const mcl_motion_config_t *c);  /* NULL or model REFERENCE = the reference's model  */
int mcl_get_motion_model(const mcl_engine_t *h, mcl_motion_config_t *out);
int mcl_host_motion_scalars(const mcl_motion_config_t *c, const double action[3], double out[8]);
/* M5 on the host, without a device: n poses (column-major 3 x n) and normals (n x 3 row-major) -> children (column-major) */
int mcl_host_motion_sample(const mcl_motion_config_t *c, const double action[3], const double *xyz_colmajor,
                           const double *normals_nx3, int64_t n, double *out_colmajor);
int mcl_init_particles_gaussian(mcl_engine_t *h, const double mean[3], const double cov[9], int64_t n,
                                int64_t first_global_index, int64_t n_total);
/* G1's factor on the host, without a device: L = {L00, L10, L11, L20, L21, L22}; MCL_ERR_INVALID_ARG as mcl_init_particles_gaussian */
int mcl_host_gaussian_factor(const double cov[9], double L[6]);
/* A mixture of n_components Gaussians (several hits of mcl_global_search, or several clusters, as ONE cloud).  means: M x 3, covs:
 * M x 9 (row-major each), counts: M particles per component, >= 0, describing the WHOLE set: their sum must equal n_total; 1 <= M
 * <= 4096.  The particle with global index g belongs to the component whose prefix range [sum counts[0..c), sum counts[0..c]) holds
 * g; it draws n0, n1, n2 exactly as G1 does (same streams and counter, indexed by g) and applies that component's mean and factor
 * by G1's rules.  So rows [a, b) of a mixture equal rows [a, b) of mcl_init_particles_gaussian(mean_c, cov_c) with the same n_total
 * wherever [a, b) lies inside component c, and M = 1 is mcl_init_particles_gaussian bit for bit.  Everything else (weights
 * 1 / n_total, what the call resets) as G1.  MCL_ERR_INVALID_ARG as G1 per component (the message names it); nothing changes then. */
int mcl_init_particles_mixture(mcl_engine_t *h, int32_t n_components, const double *means, const double *covs, const int64_t *counts,
                               int64_t n, int64_t first_global_index, int64_t n_total);

/* ---- host-side precomputation, callable without a device (what mcl_set_map uploads) --------- */
/* (P+1)^2 doubles, Eigen column-major (index d*(P+1)+r): the restatement of precompute_sensor_model
 * (cpp:233-292) the engine uses.  MCL_ERR_INVALID_ARG for the sensor fields mcl_create refuses (a non-finite or negative
 * z_*, all four z_* zero, a non-finite sigma_hit or sigma_hit <= 0). */
int mcl_host_sensor_table(const mcl_config_t *cfg, int32_t max_range_px, double *out, size_t n);
/* Skip-distance field of DESIGN.md §4.2 on the padded grid: (height+1) x (width+1) bytes, row-major,
 * 0 = stop cell, otherwise how many samples the fixed-step march may advance from a sample in that cell. */
int mcl_host_skip_field(const int8_t *data, uint32_t width, uint32_t height, uint8_t *out, size_t n);
/* Same for rays whose direction lies in `quadrant` (0:+x+y 1:-x+y 2:-x-y 3:+x-y): only stop cells a ray of that
 * quadrant can still reach bound the jump. */
int mcl_host_skip_field_dir(const int8_t *data, uint32_t width, uint32_t height, int32_t quadrant, uint8_t *out, size_t n);
/* Same for rays whose direction angle lies in wedge `wedge` of MCL_WEDGES equal sectors of the turn (sector k spans
 * [2*pi*k/MCL_WEDGES, 2*pi*(k+1)/MCL_WEDGES]); the fields MCL_RAYS_CELL stages in LDS. */
#define MCL_WEDGES 16
int mcl_host_skip_field_wedge(const int8_t *data, uint32_t width, uint32_t height, int32_t wedge, uint8_t *out, size_t n);
/* The wedge field under the tight rule, which is what mcl_set_map builds for the ray kernels: a stop cell bounds the jump by the
 * distance from the origin to the part of its offset square that lies INSIDE the (closed) wedge, not by the distance between the
 * two cell squares (csrc/mcl_wedge.h has the argument and the margins).  Never smaller than mcl_host_skip_field_wedge, 0 in the
 * same cells.  MCL_WEDGE_METRIC=0 in the environment of mcl_set_map keeps the Euclidean rule on the device (an A/B switch). */
int mcl_host_skip_field_wedge_tight(const int8_t *data, uint32_t width, uint32_t height, int32_t wedge, uint8_t *out, size_t n);
/* What the tight rule allows per stop-cell offset: for (ox, oy) in [-255, 255]^2, row-major in oy then ox (n = 511 * 511),
 * values[] = the uncapped skip a stop at that offset permits and reachable[] = 1 where the field search counts the offset as
 * reachable in this wedge.  Host only; for tests and tools. */
int mcl_host_wedge_tight_table(int32_t wedge, int32_t *values, uint8_t *reachable, size_t n);
/* Layout of the copies of the wedge fields that the global-field form of the ray kernel (ranges beyond 243 px) probes in place:
 * out = [usable (0 / 1), row pitch, rows per field (ringed grid + tail of stop rows), bytes per field, bytes of the allocation,
 * the largest byte offset a walk can form].  The kernel addresses the allocation from its start with offsets >= 0; a walk
 * starts inside the ringed grid of its field and advances by at most max_range_px samples of at most one cell per axis, so
 * out[5] < out[4] < 2^32 is the whole memory-safety argument (tests/test_sweep_addressing.py enumerates it).  Host only. */
int mcl_host_sweep_global_layout(uint32_t width, uint32_t height, int32_t max_range_px, int64_t out[6]);
/* ---- the tables under the ray stage, read back from the device as stored (for tests: tests/test_gpu_ray_tables.py holds them to
 *      the host functions above byte for byte).  Each call only copies: it launches nothing and changes no state.
 *   Wedge fields: what mcl_set_map built (the tight rule, or the Euclidean one under MCL_WEDGE_METRIC=0).  MCL_WEDGES fields of Hp
 *     rows x Wps bytes (Hp = height + 1, Wp = width + 1, Wps = Wp rounded up to a multiple of 8), n = MCL_WEDGES * Hp * Wps, in the
 *     stored encoding: a stop cell is 255, a skip above 127 is 127, the padding columns [Wp, Wps) are 0.  dims (may be NULL)
 *     receives {Hp, Wp, Wps}; out may be NULL (n is then ignored).  MCL_ERR_NOT_READY without a map or without wedge fields.
 *   Ring fields: the mirrored, ringed copies the global-field and hybrid forms probe, the whole allocation: n = out[4] of
 *     mcl_host_sweep_global_layout.  Field k (quadrant q = k / (MCL_WEDGES / 4)) starts at k * out[3]: (Hp + 4) rows of out[1] bytes
 *     with the stored wedge field at offset (2, 2), mirrored in x for q = 1, 2 and in y for q = 2, 3; every other byte, the tail
 *     rows up to out[3] included, is 255.  MCL_ERR_NOT_READY when the engine holds none (the LDS form).
 *   Sweep table: the fp64 table of the last scan as MCL_RAYS_SWEEP's ray stage used it, rows x cols doubles, row-major.  Row r
 *     stands for r - 127 samples left: entry (r, j + margin) = (double)L[obs_idx[j]][P - max(r - 127, 0)] for beam j and
 *     r <= P + 127, L the float log table and obs_idx the scan's table rows; the last row (r = P + 128), the columns before
 *     `margin` and those from margin + n_beams on are 0.  dims (may be NULL) receives {rows = P + 129, cols, margin}; out may be
 *     NULL.  MCL_ERR_NOT_READY when no sweep ray stage has built the table for the current scan (mcl_set_map and
 *     mcl_set_beam_angles drop it).
 *   A wrong n is MCL_ERR_INVALID_ARG. */
int mcl_get_wedge_fields(mcl_engine_t *h, uint8_t *out, size_t n, int32_t dims[3]);
int mcl_get_ring_fields(mcl_engine_t *h, uint8_t *out, size_t n);
int mcl_get_sweep_table(mcl_engine_t *h, double *out, size_t n, int32_t dims[3]);
/* ---- the order the ray stage worked in (for tests and tools: tests/test_gpu_sort_fine.py, tools/order_trip_sim.py).
 * The key the particles are ordered by, computed on the host by the code the device runs (csrc/mcl_sort_key.h):
 *   coarse (22 bits: tile, cell, half cell, heading bin -- what units, cuts and windows are made from) << fine | fine bits,
 *   fine in 0 .. 10: fs = max(fine - 2, 0) / 4 further sub-cell bits per axis (y above x), then ft = fine - 2 fs further heading
 *   bits; all zero for a particle whose cell lies outside the box, whose position or heading is not finite, or whose heading
 *   is 2^32 rad or more.  keys[i] >> fine is the key of fine = 0 for every fine.  Another split of the same bits is asked for
 *   as fine | (fs + 1) << 4 (fs sub-cell bits per axis, 2 fs <= fine; wherever a `fine` is passed or returned below).
 * bbox: the seven layout words (min / max sort cell in x and y as {x0, y0, x1, y1}, occupied tiles, 1 when the tiles are numbered
 * compactly, window play); tilemap: compact id per 32 x 32-cell tile of the padded map, row-major, ntx_abs tiles per row (used
 * when bbox[5] != 0, may be NULL otherwise); px, py: pixel coordinates (x - origin_x) / resolution, NaN for a particle whose
 * heading is not finite or beyond 1e6 rad, as the engine forms them; theta: headings; n: particles to key; n_layout: particles of
 * the set the layout is made for (its density decides the split of the bits: the engine passes the size of the set).  Host only. */
int mcl_host_sort_key(const int32_t bbox[7], const int32_t *tilemap, int32_t ntx_abs, uint32_t width, uint32_t height,
                      const double *px, const double *py, const double *theta, int64_t n, int64_t n_layout, int32_t fine, uint32_t *keys);
/* The order of the last update's ray stage when it went through the radix sort (MCL_SORT=radix, or 3 000 000 particles and more):
 * keys[s] = sorted key of slot s, perm[s] = index of the particle in slot s (n entries each, either may be NULL), bbox (may be
 * NULL) = the layout words the keys were made from, tilemap (may be NULL; n_tiles = tiles of the padded map, (width / 32 + 1) x
 * (height / 32 + 1), at most 8192) = the tile numbering that goes with them (meaningful when bbox[5] != 0),
 * *n_out / *fine (may be NULL) = particles ordered and fine bits of the keys
 * (MCL_SORT_FINE=<0..10> in the environment of mcl_create sets them, MCL_SORT_FINE_SUB=<fs> their split; 0 is the coarse key alone).  Copies only.
 * MCL_ERR_NOT_READY when the last ray stage did not order that way, MCL_ERR_INVALID_ARG for a wrong n. */
int mcl_get_sort_order(mcl_engine_t *h, uint32_t *keys, uint32_t *perm, size_t n, int32_t bbox[7], int32_t *tilemap, size_t n_tiles,
                       int64_t *n_out, int32_t *fine);
/* The form of the per-particle constants that ordering's gather read: *heading_form = 1 when the resampling kernel had left
 * (heading, 0, pixel x, pixel y) and the gather took the sincos (one scattered fetch per particle), 0 for the full
 * (cos, sin, pixel x, pixel y) beside the heading column (the first update of a set, whose keys k_sort_keys makes).
 * MCL_ERR_NOT_READY as above. */
int mcl_get_sort_record_form(mcl_engine_t *h, int32_t *heading_form);
/* ---- the guide of the compact parent list (csrc/mcl_compact_guide.h; for tests and tools: tests/test_compact_guide_host.py,
 * tests/test_gpu_compact_guide.py).  The scan that writes the list (mcl_get_compact_list) also writes, for 2^m evenly spaced
 * thresholds, where the list's search starts:
 *   s = max(0, bit_width(q_total) - m), the bucket of a threshold is thr >> s, bmax = q_total >> s;
 *   guide[b], b = 0 .. bmax: the first list position p with ccdf[p] >= (b << s); a reader takes guide[b + 1] as n_compact when
 *   b + 1 > bmax.  For thr in bucket b the first entry with ccdf > thr lies in [guide[b], guide[b + 1]].
 * mcl_host_compact_guide fills guide (n_guide = bmax + 1 words; NULL: only *s / *bmax are computed) from a list's strictly increasing
 * CDF column whose last entry is q_total, by the rule the scan kernel follows -- entry p writes the words of the boundaries in
 * (ccdf[p - 1], ccdf[p]], entry 0 also word 0 -- and reports in *n_written (may be NULL) how many words it stored: bmax + 1, each once.
 * mcl_host_compact_search returns for each of n thresholds the position the resampling kernel selects: the first entry with
 * ccdf > thr, found between the two guide words, clamped to n_compact - 1.  It reads word b + 1 of every bucket it looks up without
 * using the one behind bmax, so n_guide >= bmax + 2 (the engine's table has that word too).  m in 8 .. 20.  Host only. */
int mcl_host_compact_guide(const uint64_t *ccdf, int64_t n_compact, uint64_t q_total, int32_t m, uint32_t *guide, size_t n_guide,
                           int32_t *s, uint32_t *bmax, int64_t *n_written);
int mcl_host_compact_search(const uint64_t *ccdf, int64_t n_compact, const uint32_t *guide, size_t n_guide, int32_t s, uint32_t bmax,
                            const uint64_t *thr, int64_t n, int64_t *pos);
/* The guide of the list that describes the current particles, as the device holds it: info = {s, bmax, n_compact, q_total (the
 * grand total the scan left on the device), m, 1 when the last update's resampling searched through the guide}; guide (may be
 * NULL) receives n_guide = bmax + 1 words, ccdf (may be NULL) the list's n_ccdf = n_compact CDF values.  Copies only.
 * Without a list, with an empty one or without a guide (MCL_RESAMPLE_GUIDE=0 in the environment of mcl_create) a call that asks
 * for guide or ccdf is MCL_ERR_NOT_READY, and one that asks for neither reports {-1, -1, the list's length or -1, 0, m or 0, the
 * last draw's path}; MCL_ERR_INVALID_ARG for a wrong size.  The guide serves the multinomial draw of a single engine without KLD sizing; systematic
 * resampling, KLD sampling, sharded lists, a dense CDF and injected indices keep the search through ctop, and an engine configured
 * for systematic resampling, with KLD sampling on, with a communicator or in a device group does not have its scans write a guide
 * (the call is then MCL_ERR_NOT_READY as above).  MCL_RESAMPLE_GUIDE_M=<8..20> sets m (default 17). */
int mcl_get_compact_guide(mcl_engine_t *h, uint32_t *guide, size_t n_guide, uint64_t *ccdf, size_t n_ccdf, int64_t info[6]);

/* ---- multi-GPU staging (one engine per rank; collectives are the host's) -- */
/* Device pointers of engine-owned buffers so the host can hand them to RCCL without copies. */
typedef enum {
    MCL_BUF_X = 0, MCL_BUF_Y = 1, MCL_BUF_THETA = 2,  /* current particle columns, double[N]      */
    MCL_BUF_QWEIGHT = 3,                               /* uint64[N] fixed-point weights (2^-36)    */
    MCL_BUF_LOGW = 4,                                  /* double[N]                                */
    MCL_BUF_SCALARS = 5                                /* double[8]: max logw, sum w, sum q (as
                                                          u64 bits), sum wx, wy, wsin, wcos, -    */
} mcl_buffer_id;
int mcl_device_ptr(mcl_engine_t *h, int32_t which, void **dev_ptr);
/* Copies the current particle columns and fixed-point weights into caller-owned DEVICE buffers
 * (n entries each; any of them may be NULL), synchronously. */
int mcl_export_state(mcl_engine_t *h, double *d_x, double *d_y, double *d_theta, uint64_t *d_q);
/* Host copy of SCALARS (see mcl_buffer_id), valid after stage_propagate / stage_weights / update. */
int mcl_get_scalars(mcl_engine_t *h, double out[8]);
/* The host copy of SCALARS the last stage call already read back (valid right after mcl_stage_rays: [0] = local
 * max log-weight; after mcl_stage_weights: the local sums): no device access, no synchronisation. */
int mcl_get_host_scalars(const mcl_engine_t *h, double out[8]);
/* Stage 1: resample this rank's n children [child_first, child_first+n) out of the GLOBAL parent
 * set (device pointers, n_parents entries each: columns + inclusive global CDF of q with total
 * q_total), apply motion, cast rays, leave log-weights and the local max in SCALARS[0]. */
int mcl_stage_propagate(mcl_engine_t *h, const double *d_px, const double *d_py, const double *d_pth,
                        const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total,
                        int64_t child_first, int64_t n_children_total,
                        const double action[3], const float *obs, int32_t n_beams);
/* Stage 1 in two halves, so that the host can start gathering the children for the NEXT update while the
 * ray kernel of this one runs: mcl_stage_resample returns when the children (resampled + moved) are final,
 * mcl_stage_rays casts their rays and leaves the local max log-weight in SCALARS[0]. */
int mcl_stage_resample(mcl_engine_t *h, const double *d_px, const double *d_py, const double *d_pth,
                       const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total,
                       int64_t child_first, int64_t n_children_total, const double action[3]);
/* The same with the parents as packed records {x, y, theta, unused} (4 doubles each): one all-gather instead of
 * three and one fetch per gathered parent.  mcl_export_records copies this engine's current particles in that
 * form to d_records (N x 32 bytes, device memory). */
int mcl_export_records(mcl_engine_t *h, void *d_records);
int mcl_stage_resample_records(mcl_engine_t *h, const void *d_records, const uint64_t *d_cdf, int64_t n_parents,
                               uint64_t q_total, int64_t child_first, int64_t n_children_total, const double action[3]);
/* The exchange without wholesale gathers: only the fixed-point weights (8 B per particle) are gathered; each rank then
 * asks which parents its children selected (mcl_stage_resample_indices: global parent index per local child, written to
 * a caller-owned DEVICE buffer of N int32, engine state untouched), fetches the distinct ones from their owners with
 * whatever transport the host has (torch.distributed all-to-all in dist.py), and hands the compact record table plus the
 * per-child position in it to mcl_stage_motion_records, which gathers, applies the motion model and makes the children
 * current.  Same random streams as the fused call: bit-identical children. */
/* Helpers of that exchange, so that the host needs no pass over n_total elements of its own:
 *   mcl_stage_distinct_parents: d_parent[n_children] (global indices < n_total, DEVICE) -> the distinct ones in ascending
 *     order (= grouped by owning shard) in d_distinct (DEVICE, room for n_children int64), the position of every child's
 *     parent among them in d_slot (DEVICE, n_children int32) and their number in *count (host).  A bitmap over the
 *     global indices and its popcount prefix: every pass but the marking runs over n_total / 32 words.
 *   mcl_export_records_at: the packed records {x, y, theta, unused} of the listed local particles (indices into this
 *     engine's current set, DEVICE int64) -> d_out[count] (DEVICE): what a shard answers a request with. */
int mcl_stage_distinct_parents(mcl_engine_t *h, const int32_t *d_parent, int64_t n_children, int64_t n_total,
                               int64_t *d_distinct, int32_t *d_slot, int64_t *count);
int mcl_export_records_at(mcl_engine_t *h, const int64_t *d_index, int64_t count, void *d_out);
int mcl_stage_resample_indices(mcl_engine_t *h, const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total, int64_t child_first,
                               int64_t n_children_total, int32_t *d_parent_idx);
int mcl_stage_motion_records(mcl_engine_t *h, const void *d_records, int64_t n_records, const int32_t *d_record_of_child,
                             int64_t child_first, int64_t n_children_total, const double action[3]);
/* The exchange of a sharded set when every shard has a compact parent list (mcl_get_compact_list; the usual case after an
 * update with many beams): the shards gather their LISTS -- 44 B per particle that carries weight, a few per cent of the set --
 * instead of every weight, and nothing else has to travel: the merged lists are the whole parent population.
 *   mcl_compact_chunk_bytes: size of a chunk of chunk_entries list entries (a multiple of 64, the same on every shard and at
 *     least the longest list); mcl_export_compact copies this engine's list into d_chunk (DEVICE memory of that size); the
 *     host gathers the chunks in shard order (all-gather) into d_chunks;
 *   mcl_stage_resample_compact: counts[r] = length of shard r's list, totals[r] = its fixed-point weight total (SCALARS[2] of
 *     shard r as uint64); merges the chunks into one CDF, draws this shard's children from it (same thresholds as every other
 *     path: bit-identical children), applies the motion model and makes the children current.  Global parent index =
 *     shard * n_per_shard + local index. */
int mcl_compact_chunk_bytes(int64_t chunk_entries, int64_t *bytes);
int mcl_export_compact(mcl_engine_t *h, void *d_chunk, int64_t chunk_entries);
int mcl_stage_resample_compact(mcl_engine_t *h, const void *d_chunks, int32_t n_shards, int64_t chunk_entries, const int64_t *counts,
                               const uint64_t *totals, int64_t n_per_shard, int32_t self_shard, int64_t child_first, int64_t n_children_total,
                               const double action[3]);
int mcl_stage_rays(mcl_engine_t *h, const float *obs, int32_t n_beams);
/* Leave n_cus compute units out of k_rays_quad's persistent grid (it otherwise occupies every CU for the
 * whole kernel, which would serialise a collective launched beside it). */
int mcl_set_reserved_cus(mcl_engine_t *h, int32_t n_cus);
/* Stage 2: given the GLOBAL max log-weight, compute w, q and the local partial sums (SCALARS). */
int mcl_stage_weights(mcl_engine_t *h, double global_max_logw);
/* Stage 3: install the GLOBAL sums (sum w, wx, wy, wsin, wcos) so that get_weights /
 * expected_pose report globally normalised values. */
int mcl_stage_finish(mcl_engine_t *h, const double global_sums[5]);
/* ---- the same stages ORDERED ON THE DEVICE: one host wait per update ----------------------------------------------------
 * The calls above return when their stage has finished (the host reads a value between them).  The *_async forms only enqueue
 * on the engine's stream; the values the stages exchange stay in device memory the caller owns (its collective library's
 * buffers), and the caller's stream and the engine's are ordered by events:
 *   mcl_external_wait_stream(h, s): work enqueued on s after the call waits for everything enqueued on the engine so far;
 *   mcl_stream_wait_external(h, s): the engine's later work waits for everything enqueued on s so far (s: a hipStream_t).
 * One update of a sharded set, lists known from the previous update's sums:
 *   mcl_export_compact_async -> [s waits] all-gather of the chunks on s -> [engine waits] mcl_stage_resample_compact_async ->
 *   mcl_stage_rays_async (local max log-weight -> *d_local_max) -> [s waits] all-reduce MAX on s -> [engine waits]
 *   mcl_stage_weights_async (reads *d_global_max; writes this shard's part of the SUM vector, 5 + 3 * n_shards + 2 doubles:
 *   [sum w, sum w x, sum w y, sum w sin, sum w cos | per shard: list length + 1 (0: no list), low / high 32 bits of its
 *   fixed-point weight total | 1.0 if this shard's ray stage overflowed its fix-up lists | sum w^2], the other shards' slots zeroed)
 *   -> [s waits] all-reduce SUM on s, copy to the host, THE host wait -> mcl_stage_complete(global sums, &redo): waits for the
 *   engine's stream (already drained), takes over the read-backs the synchronous calls do one by one.  *redo = 1 (the last
 *   but one element of the summed vector is non-zero on every rank then): this shard's log-weights are incomplete -- run
 *   mcl_stage_rays, the MAX exchange, mcl_stage_weights, the SUM exchange and mcl_stage_finish once more (all ranks).
 * Results are those of the synchronous calls bit for bit (same kernels, same order). */
/* Adaptive resampling (cfg.resample_neff_permille = r > 0) in a sharded set.  The decision is the host's, from the sums of the
 * PREVIOUS update over the whole set (the same numbers on every shard): keep when (sum w)^2 >= r / 1000 * N_total * sum w^2.
 * mcl_stage_keep then replaces the exchange and the resampling call of this update: every particle is its own parent (reported
 * as child_first + its index), the motion model runs with the same random streams, and the ray stage adds the previous
 * update's log-weights minus their global maximum, as mcl_update does.  Launch only.  MCL_ERR_NOT_READY before the first staged
 * update of a particle set.  (mcl_comm_update and mcl_group_update take the decision themselves.) */
int mcl_stage_keep(mcl_engine_t *h, int64_t child_first, int64_t n_children_total, const double action[3]);
int mcl_stream_wait_external(mcl_engine_t *h, void *stream);
int mcl_external_wait_stream(mcl_engine_t *h, void *stream);
int mcl_export_compact_async(mcl_engine_t *h, void *d_chunk, int64_t chunk_entries);
int mcl_stage_resample_compact_async(mcl_engine_t *h, const void *d_chunks, int32_t n_shards, int64_t chunk_entries, const int64_t *counts,
                                     const uint64_t *totals, int64_t n_per_shard, int32_t self_shard, int64_t child_first,
                                     int64_t n_children_total, const double action[3]);
int mcl_stage_rays_async(mcl_engine_t *h, const float *obs, int32_t n_beams, double *d_local_max);
int mcl_stage_weights_async(mcl_engine_t *h, const double *d_global_max, double *d_vec, int32_t n_shards, int32_t self_shard);
int mcl_stage_complete(mcl_engine_t *h, const double global_sums[5], int32_t *redo);
/* ---- one process per GPU, the exchange in native code (RCCL on the engine's own stream) -----------------------------------
 * The engine holds an RCCL communicator; mcl_comm_update is ONE sharded update: all-gather of the compact parent lists,
 * resampling + motion from the merged lists, ray stage, all-reduce MAX of the max log-weight, weights + scan + list,
 * all-reduce SUM of the sums -- the three collectives enqueued on the engine's stream between its kernels (no second stream,
 * no event between streams, no host code between the stages), ONE host wait at the end.  Bit-identical to mcl_update of a
 * single engine holding all shards (same kernels as the staged calls above).
 *   mcl_comm_available: MCL_OK when an RCCL library can be used (the one already loaded in the process, e.g. a torch
 *     process's, else librccl.so.1 of the ROCm installation; taken with dlopen -- the engine does not link RCCL);
 *   mcl_comm_unique_id: on ONE rank; the host passes the 128 bytes to every rank (any channel: MPI, torch.distributed, a file);
 *   mcl_comm_create: COLLECTIVE (every rank calls it, ncclCommInitRank inside); one rank per device;
 *   mcl_comm_update: == ParticleFilter::MCL(action, observation) + expected_pose() (cpp:652-716) for the whole sharded set.  The
 *     shards' list lengths and weight totals come from the PREVIOUS update's summed vector (mcl_stage_weights_async documents
 *     it), which the communicator keeps.  When they are not known (the first update after the particles were set or
 *     initialised on every rank) or some shard has no list, the update takes the DENSE exchange instead, also on the engine's
 *     stream: all-gather of every shard's fixed-point weights and packed records (8 + 32 B per particle), one global CDF, the
 *     same draw (one more host wait, for the weight total).  Every rank decides from the same numbers, so every rank issues the
 *     same collectives.  The global sums are installed as mcl_stage_finish does; mcl_comm_get_vector returns the summed vector
 *     (5 + 3 * n_ranks + 2 doubles) of the last update.  mcl_comm_set_lists hands over list lengths (-1: none) and weight totals
 *     found by other means (a host that ran an update through the stage calls);
 *   mcl_comm_stats: bytes the last LIST exchange delivered to this rank (padded chunks) / carried (entries), host waits of the
 *     last update; mcl_comm_last_exchange: *dense = 0 the last update exchanged lists, 1 it took the dense exchange (with the bytes
 *     received), 2 it exchanged nothing (adaptive resampling kept the set). */
int mcl_comm_available(const char **why);
int mcl_comm_unique_id(unsigned char id[128]);
int mcl_comm_create(mcl_engine_t *h, const unsigned char id[128], int32_t n_ranks, int32_t rank);
int mcl_comm_selftest(mcl_engine_t *h);   /* COLLECTIVE: the three collectives of an update on known data; MCL_OK or what failed */
int mcl_comm_destroy(mcl_engine_t *h);
int mcl_comm_set_lists(mcl_engine_t *h, const int64_t *counts, const uint64_t *totals);
int mcl_comm_update(mcl_engine_t *h, const double action[3], const float *obs, int32_t n_beams, double pose_out[3]);
int mcl_comm_get_vector(const mcl_engine_t *h, double *vec_out, int32_t n);
int mcl_comm_stats(const mcl_engine_t *h, uint64_t *list_bytes_received, uint64_t *list_payload_bytes, int32_t *host_waits);
int mcl_comm_last_exchange(const mcl_engine_t *h, int32_t *dense, uint64_t *weights_bytes, uint64_t *records_bytes);

/* Inclusive scan of q (uint64) on the engine's stream: cdf[i] = offset + q[0] + ... + q[i]. */
int mcl_scan_weights(mcl_engine_t *h, const uint64_t *d_q, uint64_t *d_cdf, int64_t n, uint64_t offset);

/* ---- several GPUs behind one handle (SURVEY.md §8(b).1 "device list", §8(e)) -------------------------------------
 * The reference is ONE process (main, cpp:1019-1025; MCL called from timer_update, cpp:777): a group owns one engine per
 * listed device, shards the particle set contiguously (n_total / n_devices each; cfg->max_particles is PER DEVICE,
 * cfg->device is ignored) and mirrors the single-engine entry points the host patch uses.  Per update a device receives
 * the other shards' compact parent lists (44 B per particle that carries weight; mcl_get_compact_list) and draws its own
 * children from the merged lists -- or, when some shard has no list (first update, flat weights), the other shards'
 * fixed-point weights (8 B per particle), scans the same exact global CDF and reads each selected parent where it lives (peer
 * pointer over xGMI); the maximum is taken on the devices (each reads its peers' maxima), the sums are combined on the host (one
 * wait per update); the phases are ordered by events between the devices' streams.  Results are bit-identical to a single engine
 * holding all particles.  The devices must have peer access to each other; weight_mode LOG only; resample_neff_permille works
 * on the sums of the whole set. */
typedef struct mcl_group mcl_group_t;
int mcl_group_create(const mcl_config_t *cfg, const int32_t *devices, int32_t n_devices, mcl_group_t **out);
void mcl_group_destroy(mcl_group_t *g);
const char *mcl_group_last_error(const mcl_group_t *g);
int32_t mcl_group_size(const mcl_group_t *g);
int mcl_group_engine(mcl_group_t *g, int32_t i, mcl_engine_t **out);           /* the i-th shard's engine (diagnostics) */
int mcl_group_set_map(mcl_group_t *g, const int8_t *data, uint32_t width, uint32_t height, float resolution, double origin_x,
                      double origin_y);
int mcl_group_set_beam_angles(mcl_group_t *g, const float *angles, int32_t n_beams);
/* xyz: n_total x 3 column-major, weights: n_total (any non-negative weights with a positive maximum: every shard is scaled
 * by the maximum of the whole set); n_total a multiple of the device count */
int mcl_group_set_particles(mcl_group_t *g, const double *xyz, const double *weights, int64_t n_total);
int mcl_group_init_particles_pose(mcl_group_t *g, const double pose[3], int64_t n_total);
int mcl_group_init_global(mcl_group_t *g, int64_t n_total);
/* mcl_init_particles_gaussian / mcl_set_motion_model on every shard (the same particles as one engine holding them all) */
int mcl_group_init_particles_gaussian(mcl_group_t *g, const double mean[3], const double cov[9], int64_t n_total);
int mcl_group_set_motion_model(mcl_group_t *g, const mcl_motion_config_t *c);
int mcl_group_set_sensor_mount(mcl_group_t *g, const double mount[3]);    /* the same mount on every engine of the group (§4.25) */
int mcl_group_update(mcl_group_t *g, const double action[3], const float *obs, int32_t n_beams);
int mcl_group_expected_pose(mcl_group_t *g, double out[3]);
int mcl_group_get_particles(mcl_group_t *g, double *xyz, int64_t n_total);
int mcl_group_get_weights(mcl_group_t *g, double *weights, int64_t n_total);
int mcl_group_get_resample_indices(mcl_group_t *g, int32_t *idx, int64_t n_total);   /* global parent indices */
int mcl_group_get_stage_timings(const mcl_group_t *g, double ms[6]);           /* per stage: the slowest device */
/* bytes the last update moved between devices: [0] received by the device that received MOST for the parent population -- the
 * other shards' compact lists (44 B per particle that carries weight, copied entry-exact) or, when some shard had no list, their
 * fixed-point weights (8 B per particle);
 * [1] parent records read from peers by ALL devices (weights exchange only; children with a remote parent x 32 B: an upper
 * bound, a shared parent is cached after its first fetch).  mcl_group_exchanged_lists: 1 when the last update exchanged lists. */
int mcl_group_exchange_bytes(const mcl_group_t *g, uint64_t out[2]);
int32_t mcl_group_exchanged_lists(const mcl_group_t *g);

/* ---- map patches: a changed rectangle of the grid without a full mcl_set_map --------------------------------
 * mcl_update_map_region replaces the cells [x0, x0 + width) x [y0, y0 + height) of the map held by `cells` (row-major, row_stride
 * cells per row, >= width); dimensions, resolution and origin stay.  Afterwards the engine is, byte for byte, an engine on which
 * mcl_set_map was called with the edited grid: the grid, the isotropic skip field and its nibble copy, the four quadrant fields,
 * the sixteen wedge fields under the rule the last mcl_set_map used (MCL_WEDGE_METRIC is not read again), their ringed copies where
 * held, the free-cell list and the likelihood field when the model is on; and it voids what mcl_set_map voids (the captured
 * graphs and the ordering layout, the recovery averages, the recovery proposal, the fuse call's log-weights, the searches'
 * lattice, volumes and tables through the map epoch).  The particles, the beams and what depends on the range or the resolution
 * alone stay.  Every later result equals, bit for bit, that of the engine given the full mcl_set_map instead.
 *   The device work follows the changed cells, not the map: each table is rebuilt inside the window around the cells whose stop bit
 * (value > 50) changed that mcl_host_map_patch_plan forms.  A patch that changes no value returns MCL_OK with changed_cells = 0,
 * launches nothing and voids nothing; one that changes values but no stop bit rewrites the grid and the free list only.
 * Synchronous, like mcl_set_map.  MCL_ERR_NOT_READY without a map; MCL_ERR_INVALID_ARG for a null pointer, an empty rectangle,
 * one that leaves the map, or row_stride < width (nothing changes then).  MCL_ERR_HIP part-way leaves "map not set".
 *   Sharded ranks (mcl_comm_*) must all be given the same patch; that is not checked. */
typedef struct {
    int32_t changed_cells, changed_stop_cells;   /* cells whose value / whose (value > 50) differs from the map held */
    int32_t window[4];                            /* x0, y0, x1, y1 (inclusive, padded-grid cells) of the skip-field window rebuilt; x1 < x0: none */
    int32_t lf_window[4];                         /* the same for the likelihood field, grid cells; none when the model is off */
    int64_t free_cells;                           /* n_free after the patch */
    double  ms;                                   /* wall time of the call */
} mcl_map_patch_stats_t;
int mcl_update_map_region(mcl_engine_t *h, const int8_t *cells, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                          uint32_t row_stride /* cells per row of `cells`, >= width */, mcl_map_patch_stats_t *st /* may be NULL */);
/* The windows of a patch whose stop-bit changes lie in the box stop_bbox = {x0, y0, x1, y1} (grid cells, inclusive) of a
 * map_w x map_h map: window = the padded-grid cells of the skip fields a change in the box can alter (the box's padded cells
 * widened by 254, the reach of a skip value capped at 255; the quadrant and wedge fields change inside it, on the side their rays
 * come from), lf_window = the grid cells of a likelihood field of reach lf_reach (the box widened by it; {0, 0, -1, -1} for
 * lf_reach <= 0).  Both clipped to the map, as is the box.  MCL_ERR_INVALID_ARG for a null pointer, an inverted box or one with
 * no cell inside the map.  Host only; the device path forms its windows here. */
int mcl_host_map_patch_plan(uint32_t map_w, uint32_t map_h, const int32_t stop_bbox[4] /* grid cells, inclusive */,
                            int32_t lf_reach /* <= 0: model off */, int32_t window[4], int32_t lf_window[4]);
/* A map-derived table as stored on the device (copies only, like mcl_get_wedge_fields): the grid (int8, H x W), the isotropic skip
 * field (Hp x Wps bytes), its nibble copy (Hp x Wps / 2), quadrant field 0 .. 3 (Hp x Wps; MCL_ERR_NOT_READY on a map that has
 * none) or the free-cell list (n_free uint32).  *needed (may be NULL) receives the byte count; out may be NULL (n_bytes is then
 * ignored), else n_bytes must equal it. */
enum { MCL_MAP_TABLE_GRID = 0, MCL_MAP_TABLE_SKIP = 1, MCL_MAP_TABLE_SKIP_NIBBLES = 2, MCL_MAP_TABLE_QUADRANT0 = 3 /* .. 6 */,
       MCL_MAP_TABLE_FREE_CELLS = 7 };
int mcl_get_map_table(mcl_engine_t *h, int32_t which, void *out, size_t n_bytes, size_t *needed);
/* mcl_update_map_region on every engine of the group (no statistics); the first failure is the group's error, as mcl_group_set_map's. */
int mcl_group_update_map_region(mcl_group_t *g, const int8_t *cells, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
                                uint32_t row_stride);

#ifdef __cplusplus
}
#endif
#endif /* MCL_HIP_ENGINE_H */
