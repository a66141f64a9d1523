// mcl_engine_internal.h -- what the translation units of libmcl_hip_engine.so share: the engine object, the status helpers, and
// the handful of engine-side functions the sharded hosts are built on.  Not part of the ABI (include/mcl_hip_engine.h is).
//   mcl_engine.hip   the engine: map / beams / particles, the update and its stages, every kernel
//   mcl_engine_access.hip  the engine's entry points that launch nothing: read-backs, reports of host state, option setters
//   mcl_host_math.hip  the host arithmetic (tables, fields, per-update scalars) and the ABI's mcl_host_*: no HIP, no mcl_engine
//   mcl_comm.hip     mcl_comm_*: one process per GPU, the collectives of an update over RCCL on the engine's stream
//   mcl_group.hip    mcl_group_*: several GPUs behind one handle, driven by one process (peer copies)
//   mcl_cluster.hip  mcl_pose_clusters: the pose hypotheses of the particle set (its own kernels, called outside the update)
//   mcl_query.hip    mcl_query_scans / mcl_score_poses: expected scans and scan scores of poses that are not particles (its own
//                    kernels and buffers, called outside the update)
//   mcl_search.hip   mcl_global_search: the likelihood-field score of every pose of a lattice over the map, and its hits (its own
//                    kernels and buffers, called outside the update)
//   mcl_refine.hip   mcl_refine_poses: the score of a dense window around each seed pose, its best pose, mean and covariance (its
//                    own kernels and buffers, called outside the update)
//   mcl_map_patch.hip  mcl_update_map_region: a changed rectangle of the map into every map-derived table (the kernels are
//                    mcl_map_patch.h's, reached through the launch_patch_* functions below), mcl_get_map_table
//   mcl_buffers.h    Buf / DevBuf / HostBuf: every device and pinned buffer of the files above owns its memory through these
// Only mcl_engine.hip includes the kernels (mcl_kernels.h: the ordered list of the per-stage headers); mcl_engine_access.hip
// launches none, mcl_comm.hip and mcl_group.hip reach the few kernels they launch through the launch_* functions below.  Every
// function declared here is defined once, under this name.
#pragma once
#include "../../include/mcl_hip_engine.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "mcl_types.h"
#include "mcl_wedge.h"
#include "mcl_host_math.h"
#include "mcl_buffers.h"

enum { EV_START = 0, EV_RESAMPLE, EV_QUERY, EV_RAYS, EV_SENSOR, EV_K0, EV_K1, EV_COUNT };   // K0..K1 bracket the dominant kernel


constexpr unsigned long long kExactCap = 1ull << 16;   // level-3 rays per launch handled by k_rays_exact (more: inline)
// d_result / h_result: [0..7] scalars, [8..11] counters, [12] work-list overflow flag, [13] work counter, [14] level-3 list
// length, [15] far-list length (and the staging word of a global maximum), [16] length of the compact parent list, [17] pose-space
// bins the update's draw occupied (KLD sampling, mcl_set_kld)
constexpr int kResultWords = 18;
constexpr int kResultGuideTotal = 18;        // d_result word (device only, behind the copied ones): the grand total of the scan that wrote the compact list's guide
constexpr int kResultAlloc = 32;             // words d_result is allocated with
static_assert(kResultGuideTotal >= kResultWords && kResultGuideTotal < kResultAlloc, "the guide's total lies behind the copied words, inside the block");
constexpr int kResultStage = 40;             // h_result word that stages a host value on its way to the device
constexpr int kResultStamp = 32;             // h_result word a small update's last kernel stamps (the host polls it)

struct mcl_comm;
void comm_free(struct mcl_comm *c);        // mcl_comm.hip
void comm_forget(struct mcl_comm *c);      // mcl_comm.hip: the particle set changed, what the exchange knew is void
struct mcl_cluster;
void cluster_free(struct mcl_cluster *c);  // mcl_cluster.hip
struct mcl_query;
void query_free(struct mcl_query *q);      // mcl_query.hip
struct mcl_search;
void search_free(struct mcl_search *s);    // mcl_search.hip
struct mcl_refine;
void refine_free(struct mcl_refine *r);    // mcl_refine.hip

// ---- the three records that travel between the pieces of an update, and the environment's knobs
// What the resampling launch prepared for the ray stage of the same update.  resample_ray_extras is the only writer of the
// resampling part, tail_launches of obs_wait; plan_rays copies it into the RayPlan, launch_rays consumes it, ray_handoff_void voids it.
struct RayHandoff {
    bool constants = false;             // d_pc holds the constants of the current particles (ordering modes: and the per-particle scratch is zeroed)
    bool stale_layout = false;          // this update orders by the previous update's layout: d_bbox / d_tilemap are not remade
    bool keys = false;                  // ... and the resampling kernel wrote the (key, index) pairs of the library sort
    bool heading = false;               // ... and, for k_rays_sweep, d_pc in the heading form (heading, 0, pixel x, pixel y): k_sort_gather finishes the constants;
                                        //   a launch that does not come to that gather has k_particle_prep make the full form (plan_rays)
    bool folded = false; mcl::PrepClear passed{};   // the resampling kernel also cleared the few words that are not per particle: exactly these
    bool obs_wait = false;              // the scan's tables are built on stream2: the stream waits for ev_obs where the ray stage first reads them
};
// Stage events BOUND TO DISPATCHES: the stop event of hipExtLaunchKernelGGL costs nothing, a hipEventRecord between two kernels of
// a stream ~3 us of pipeline (tools/ubench/event_cost.hip; elapsed times across different launches are valid).  A launch that binds
// one says so (launch_resample and scan_weights to their callers, the ray stage here); the code that would record it then does not.
struct StageEvents {
    bool rays_bound = false;            // EV_RAYS is k_combine_logw's stop event (ray_combine); cleared by the callers of launch_rays
    bool query_skipped = false;         // EV_QUERY was not recorded: the tables were built beside the ordering (tail_launches' timings)
};
// The ordering layout (bounding box, occupied tiles) of an update's children is made on the second stream right after the
// resampling kernel and used by the NEXT update, whose resampling kernel then writes the sort keys itself: d_bbox / d_tilemap are
// the layout in use, d_*_nx the one being made; swapped at the end of an update.  wanted (layout_mark: ev_children is recorded
// behind the resampling kernel) -> pending (next_layout_launch: the kernels are on stream2, ev_layout behind them) -> valid, n
// (layout_adopt: d_bbox describes the previous update's n children; cleared by graph_reset: map, beams, particles set from outside).
struct NextLayout {
    bool wanted = false, pending = false, valid = false; int64_t n = 0;
    hipEvent_t ev_children = nullptr, ev_layout = nullptr;
    DevBuf<int> d_bbox_nx, d_tilemap_nx, d_tilemark_nx;
};
// Read once at mcl_create (read_knobs), never on the update path; 0 / negative = default where a number is wanted.
// (MCL_WEDGE_METRIC, MCL_NO_BEAM_PAD and MCL_SWEEP_NO_REC are read where the map / the beams are set.)
struct EnvKnobs {
    int64_t cell_min = 0, cell_slice = 0;            // MCL_CELL_MIN, MCL_CELL_SLICE
    int qslices_per_cu = 0, qside = 0, sweep_g = 0;  // MCL_QSLICES_PER_CU, MCL_QSIDE, MCL_SWEEP_G
    int tiny_poll = 1, no_compact = 0;  // MCL_TINY_POLL=0: a tiny update waits for the stream, not the stamp; MCL_NO_COMPACT=1: the scan writes no compact list
    int sort_radix = -1;                // MCL_SORT=radix / hist forces one ordering path; default: by size
    int sort_fine = -1;                 // MCL_SORT_FINE=<0..10>: fine key bits of the radix path (0: the coarse key alone); default: mcl::kSortFineDefault
    int sort_fine_sub = -1;             // MCL_SORT_FINE_SUB=<fs>: how many of them per axis are sub-cell bits; default: the rule of SortLayout for a
                                        //   given MCL_SORT_FINE, mcl::kSortFineSubDefault with the default bits
    int fix_wg = 0;                     // MCL_FIX_WG=<n>: workgroups of k_rays_fix per CU in the flat deal (default mcl::kFixWgPerCu)
    bool fix_deal_seg = false;          // MCL_FIX_DEAL=seg: k_rays_fix deals per segment (what it does anyway beyond mcl::kFixSegMax segments)
    int resample_guide = 1;             // MCL_RESAMPLE_GUIDE=0: no guide of the compact list, the resampling search goes through ctop (the search of earlier rounds)
    int guide_m = 0;                    // MCL_RESAMPLE_GUIDE_M=<8..20>: log2 of the guide's buckets (default mcl::kGuideLog2Default)
    std::string debug_wg;               // MCL_DEBUG_WG=<file>: four words per persistent workgroup (ray_debug_dump)
    bool no_bucket_cuts = false;        // MCL_NO_BUCKET_CUTS: units on the plain grid of 1024 slots, sparse sets ordered by whole tiles (rounds 2-3 before the cuts)
    bool sweep_global = false;          // MCL_SWEEP_GLOBAL=1: k_rays_sweep on the wedge fields in global memory whatever the range
    int sweep_hybrid = 1;               // MCL_SWEEP_HYBRID=0: ranges beyond the window take the global-field form alone; 2: the hybrid also for a fresh / spread set
    int sw_guide = 0;                   // MCL_SW_GUIDE=<n>: the guide of k_sweep_plan's run lengths (default 2; 3 for the forms of ranges beyond the LDS window)
    int sw_split16 = -1;                // MCL_SW_SPLIT16=0/1 forces RayArgs::split16 (default: by size)
    int sweep_pairs = -1;               // MCL_SWEEP_PAIRS: -1 the engine decides, 0 / 1 forced (A/B measurements)
    bool no_obs_overlap = false;        // MCL_NO_OBS_OVERLAP: the observation tables are built on the main stream, after the resampling kernel
    bool no_prep_fold = false;          // MCL_NO_PREP_FOLD: k_prep_small stays a launch of its own
    bool no_stale_layout = false;       // MCL_NO_STALE_LAYOUT: every update makes its own layout first (rounds 1-3)
    bool comm_no_pregather = false;     // MCL_COMM_NO_PREGATHER: mcl_comm_update gathers the lists when it starts, not when the previous one ends
    bool comm_no_lists = false;         // MCL_COMM_NO_LISTS: mcl_comm_update takes the dense exchange on every update
};

// What the last radix ordering worked from, for mcl_get_sort_order: the layout buffers its keys were made from (d_bbox / d_tilemap at the time:
// layout_adopt swaps them out at the end of the update, and nothing writes them before the next update), n and the fine bits.
// heading: its gather read the heading form of d_pc (RayHandoff::heading).
struct OrderLast { const int *bbox = nullptr, *tilemap = nullptr; int64_t n = 0; int fine = 0; bool heading = false; };

struct mcl_engine {
    mcl_config_t cfg{};
    int num_cu = 256;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;      // the per-update observation tables and the next layout are built here, beside the main stream's kernels
    std::string err;
    // ---- map
    bool have_map = false;
    int W = 0, H = 0, P = 0, Wp = 0, Hp = 0, Wps = 0, tw_cells = 0;
    double res = 0, ox = 0, oy = 0;
    std::vector<double> table;          // (P+1)^2 column-major (d*(P+1)+r)
    DevBuf<int8_t> d_grid;
    DevBuf<uint8_t> d_dist;
    DevBuf<uint8_t> d_dist4;            // nibble-packed copy of d_dist (k_rays_skip's LDS window is a straight copy of it)
    DevBuf<uint8_t> d_distq[4];         // directional skip fields, one per quadrant (k_rays_quad / k_rays_far)
    DevBuf<uint8_t> d_distw;            // kWedges wedge fields (k_rays_cell, k_rays_sweep's LDS windows), each Hp x Wps bytes
    DevBuf<float> d_L;                  // [r_obs][d]
    DevBuf<double> d_table;             // double table (product mode)
    DevBuf<uint32_t> d_free;            // linear indices of free cells (data == 0), row-major, cpp:199-213
    uint64_t n_free = 0; uint32_t init_idx = 0;
    std::vector<uint64_t> free_row;     // H + 1: entries of d_free before row y (a map patch splices the rows it touches, mcl_map_patch.hip)
    bool wedge_tight = true;            // the rule of the wedge fields held (MCL_WEDGE_METRIC as mcl_set_map read it)
    // ---- beams, and the tables of one scan
    int B = 0, bpad = 0;
    std::vector<float> angles;
    std::vector<double2> beam_cs_host;  // (cos, sin) of every beam angle (set_beam_angles)
    DevBuf<float> d_angle;
    DevBuf<double2> d_beam_cs;
    DevBuf<double2> d_beam_csx;         // k_rays_sweep's copy with virtual beams either side (set_beam_angles)
    DevBuf<double2> d_beam_csxg;        // the same for the global-field form: a virtual beam repeats the first / last REAL beam
    // k_rays_sweep<.., REC> (an evenly spaced scan): directions of the grid angles a0 + j inc, every beam's offset from its grid angle
    // (one entry per table column), cos / sin of the increment; rec_ok: the scan qualifies
    DevBuf<double2> d_beam_csi;
    DevBuf<double> d_beam_err;
    double rec_c = 1.0, rec_s = 0.0; bool rec_ok = false;
    bool quad_ok = false;               // beam angles monotone over less than a full turn
    int beam_pad = 0, beam_margin = 0;
    int wedge_beams_max = 0;            // the most beams a direction wedge of 2 pi / 16 holds (mcl_set_beam_angles)
    DevBuf<int32_t> d_obs_idx;
    DevBuf<float> d_obs;
    HostBuf<float> h_obs;               // pinned staging for the per-update scan
    hipEvent_t ev_obs = nullptr;        // the tables below were built on stream2 (handoff.obs_wait: the ray stage has yet to wait for it)
    DevBuf<float> d_Lt;                 // [Lt | Lt with the rows reversed (k_rays_cell)]
    DevBuf<double> d_Ltd;               // k_rays_sweep's fp64 table (mcl_rays_sweep.h), built per update when that kernel runs
    int ltd_cols = 0;
    bool ltd_ready = false;             // d_Ltd holds the table of the observation in d_obs_idx (cleared when a new scan is staged)
    // ---- particle set
    int64_t cap = 0, N = 0;
    bool have_particles = false;
    DevBuf<double> d_x[2], d_y[2], d_th[2];
    int cur = 0;
    DevBuf<double4> d_pack[2];          // (x, y, theta, -) records of buffer 0/1, written by k_resample_motion
    bool pack_valid[2] = {false, false};
    DevBuf<int32_t> d_idx;
    DevBuf<double> d_inject;            // cap*4 (normals + uniforms)
    DevBuf<double> d_tmp;               // cap*3 doubles; 4 k after an mcl_sample_particles of more than 3/4 cap rows
    bool resampled_last = true;
    bool far_fresh = true;              // no ray stage has seen the current particle set yet (set / initialised since the last one)
    uint32_t update_idx = 0;
    // ---- weights, CDF, compact list
    DevBuf<double> d_w, d_logw;
    DevBuf<double> d_logw_acc;          // the kernels with work lists accumulate here with atomics; k_combine_logw (legacy kernels: k_gather_logw) -> d_logw
    DevBuf<double> d_carry[2];          // logw - max of the last update (adaptive resampling: what a kept particle carries)
    int carry_idx = 0;                  // d_carry[carry_idx] is current; k_weights writes the other one
    bool carry_valid = false, carry_pending = false;
    DevBuf<uint64_t> d_q, d_cdf;
    DevBuf<uint64_t> d_blocktot;        // the scan's spine (reserve_scan_spine)
    const uint64_t *blocktot_for = nullptr;   // which CDF array d_blocktot currently describes
    int64_t blocktot_n = 0;
    DevBuf<uint64_t> d_leaders;         // last CDF entry of every 16-entry group of the array d_blocktot describes
    DevBuf<double> d_part;              // kRedBlocks * 8: per-workgroup partial sums (k_weights)
    DevBuf<double> d_maxpart;           // kRedBlocks: per-workgroup maxima of d_logw (k_combine_logw / k_reduce_max)
    bool max_partials_ready = false;    // k_combine_logw left the per-workgroup maxima of d_logw in d_maxpart
    bool sums_pending = false;          // k_weights left partial sums that the next scan's spine turns into scalars[1..7]
    DevBuf<uint32_t> d_bm;              // mcl_stage_distinct_parents: bitmap over the global particle indices, its popcounts and their prefix
    DevBuf<uint64_t> d_bm_pop, d_bm_pref;
    // compact list of the particles with a non-zero fixed-point weight, written by the scan of d_q (mcl::CompactOut)
    DevBuf<uint32_t> d_blockcnt;        // per scan tile of the engine's own set (sized at mcl_create)
    DevBuf<uint64_t> d_ccdf, d_ctop;
    DevBuf<uint32_t> d_cidx;
    DevBuf<double4> d_crec;
    // the list's guide (mcl_compact_guide.h): written by the scan that writes the list while the engine can use it (guide_wanted:
    // a single engine without KLD sizing), read by the multinomial draw; null with MCL_RESAMPLE_GUIDE=0 or systematic resampling.
    // guide_pending / guide_valid follow compact_pending / compact_n: one writer (scan_weights), voided wherever the list is.
    DevBuf<uint32_t> d_cguide;
    int guide_m = 0;                    // log2 of its buckets
    bool guide_pending = false;         // the last scan of the engine's own weights wrote the guide beside the list
    bool guide_valid = false;           // ... and the list it belongs to is the valid one (compact_n > 0)
    bool graph_guide[2] = {false, false};   // the captured tail of particle buffer 0 / 1 writes the guide
    bool guide_used = false;            // the last resampling searched through it
    int64_t compact_cap = 0;            // room in the list (cap / 4, at least 4096)
    int64_t compact_n = -1;             // entries of the list that describes d_cdf / the current particles; -1: none
    bool compact_pending = false;       // the last scan wrote a list; its length arrives with the next result read-back
    bool compact_used = false;          // the last resampling drew from a compact list
    unsigned long long list_epoch = 0;  // counts the rewrites of the compact list (a gathered copy of an older one is stale)
    DevBuf<uint64_t> d_gcdf, d_gtop;    // merged CDF of the shards' gathered lists (mcl_stage_resample_compact)
    // ---- ordering (k_rays_cell, k_rays_sweep: the particles by tile, cell and heading)
    DevBuf<double4> d_pcs;              // cap: pc in sorted order
    DevBuf<double> d_ths;               // cap: heading in sorted order
    DevBuf<uint32_t> d_perm, d_skey, d_srank;   // cap each
    DevBuf<uint32_t> d_skey2, d_sval2;  // MCL_SORT=radix: sorted keys / indices
    DevBuf<uint8_t> d_sort_tmp;         // rocPRIM's scratch, in bytes
    DevBuf<uint32_t> d_tile_used;       // one mark per kHistTile buckets of the sort histogram: touched by this update's sort
    DevBuf<uint32_t> d_hist, d_histpart;                   // kSortBuckets, kSortBuckets / kHistTile
    DevBuf<int> d_bbox;                 // 7: bounding box, occupied tiles, numbering in use, window play
    OrderLast order_last;               // (ray_order; voided where the layout is: graph_reset)
    DevBuf<uint32_t> d_cut_start, d_cut_end;   // kSwMaxCuts each: where the buckets of a sparse set start / end in the radix-sorted order (zero between sorts)
    DevBuf<int> d_tilemap, d_tilemark;  // kSortMaxTiles each: tile of the map -> compact id; marks of the occupied tiles (zero between sorts)
    DevBuf<double2> d_slice_mean;       // one per slice of the sorted order
    DevBuf<double4> d_unit_sums;        // per unit of the sorted order: (sum px, sum py, count, -), bounding box
    DevBuf<uint32_t> d_unit_begin;      // first slot of every unit + one (k_unit_table)
    DevBuf<int> d_nunits;               // number of units of this update's sorted order
    // ---- ray-stage work lists
    DevBuf<double4> d_pc;               // cap: per-particle constants of every ray kernel but the literal march (k_particle_prep, or the resampling kernel)
    DevBuf<short4> d_qr;                // cap: per-particle quadrant ranges (k_rays_quad)
    DevBuf<uint8_t> d_steps;
    DevBuf<unsigned long long> d_fix_list, d_fix_count;      // d_fix_count: 8 words (64 bytes) per segment
    unsigned long long *d_fix_over = nullptr;
    DevBuf<unsigned long long> d_exact_list;     // level-3 rays for k_rays_exact; its counter is word 14 of d_result
    unsigned long long fix_cap = 0; int fix_segments = 0;
    DevBuf<uint8_t> d_far;              // cap * 4 flags
    DevBuf<uint32_t> d_far_list;        // k_rays_sweep: slots with a flagged quadrant (cap entries, allocated on first use)
    DevBuf<uint32_t> d_far_sorted, d_far_cnt;   // the same in ascending order (k_far_*), per-2048-slot counts
    DevBuf<int4> d_items;               // k_rays_sweep's work items (guided schedule), planned on the device every update
    DevBuf<int4> d_centres;             // per run of units: window centre, first unit, units (k_sweep_plan)
    DevBuf<int> d_nitems;               // number of work items (written by k_sweep_plan)
    int64_t plan_n = 0;
    int reserved_cus = 0;               // CUs the persistent grids leave free (for RCCL kernels running beside them)
    // ---- which ray kernel, which form of k_rays_sweep, and its fields in global memory
    bool sweep_layout_ok = false;       // k_rays_sweep's static LDS ends where its raw window offset (kQLdsBase) assumes
    bool sweep_hyb_layout_ok = false;   // ... and of its hybrid form
    bool sweep_rec_layout_ok = false;   // the same for the <.., REC> instantiations (LDS form: window + offset table; global form: the table)
    bool quad_layout_ok = false, cell_layout_ok = false;   // the same for k_rays_quad / k_rays_cell
    bool skip_layout_ok = false;        // k_rays_skip has no static LDS (its window is addressed from LDS offset 0)
    int qside = 0;                      // k_rays_quad window side (0: not usable for this map)
    // k_rays_sweep on the wedge fields in GLOBAL memory (ranges a 256-cell LDS window cannot hold; MCL_SWEEP_GLOBAL=1 forces it)
    DevBuf<uint8_t> d_distg;            // kWedges mirrored fields with a two-cell stop ring and a tail of stop rows each (k_ring_field)
    int distg_pitch = 0;                // row pitch
    size_t distg_stride = 0;            // bytes per field, tail included
    const char *distg_why_not = nullptr;     // why the global-field form of k_rays_sweep is not available for this map, if it is not
    bool sweep_global = false;          // this map takes the global-field variant (decided at mcl_set_map)
    int hyb_backoff = 0, hyb_skip = 0;  // updates in the global-field form after a hybrid update that flagged many particles (sweep_hybrid_decide)
    int last_sweep_global = 0, last_sweep_rec = 0, last_sweep_pairs = 0;    // the form of k_rays_sweep the last ray stage ran
    bool last_work_lists = false;       // the last ray stage ran a kernel with fix-up lists (quad, cell, sweep): fix_lists_overflowed
    int last_mode = 0;                  // the MCL_RAYS_* enumerator of the kernel the last ray stage ran (0: none yet)
    // ---- hand-offs between the pieces of an update, and what outlives one
    RayHandoff handoff;
    // the few words the ray stage wants cleared (k_prep_small's job): what the last windowed launch passed, so that the NEXT
    // update's resampling kernel can do it (handoff.folded).  A cache across updates, not a hand-off: dropped by graph_reset alone.
    mcl::PrepClear prep_cache{};
    bool prep_cache_valid = false; int64_t prep_cache_n = 0;
    hipEvent_t ev[EV_COUNT]{};
    StageEvents stage_ev;
    NextLayout layout;
    // hipGraph of the update's tail (observation upload ... result read-back) for the k_rays_skip path, one per particle buffer
    hipGraphExec_t graph_exec[2] = {nullptr, nullptr};
    bool graph_warm = false;            // a regular update has run since the sizes / map / beams last changed
    bool capturing = false;
    hipEvent_t ev_ext_in = nullptr, ev_ext_out = nullptr;   // ordering against a caller's stream (mcl_stream_wait_external / mcl_external_wait_stream)
    bool stage_async_rays = false, stage_async_weights = false;
    bool stage_kept = false;            // the staged flow's last children are the previous particles themselves (mcl_stage_keep)
    // ---- results and timings
    DevBuf<unsigned long long> d_result;      // the words of the constant block above (kResultWords): one D2H copy
    HostBuf<unsigned long long> h_result;     // pinned mirror of d_result
    double *d_scalars = nullptr;        // 8 (a view into d_result, like the next one and d_fix_over)
    unsigned long long *d_counters = nullptr;  // 4
    unsigned long long result_seq = 0;  // stamps the result block a small update writes to pinned memory (h_result[kResultStamp])
    double h_scalars[8]{}; uint64_t q_total = 0;
    double global_sums[5]{};            // sum w, wx, wy, wsin, wcos actually used for outputs
    bool have_idx = false, have_steps = false, have_logw = false;
    double timings[6]{}, ray_ms = 0;
    bool ray_ms_is_graph_tail = false;  // ray_ms is the whole captured tail of a small update, not one kernel
    unsigned long long h_counters[4]{}, h_fix_count = 0;
    // ---- options
    // KLD-adaptive particle count (mcl_set_kld): the resampling kernel marks the bin of every drawn parent in
    // d_kld_bm and lists the words of new bins in d_kld_list; the counter of update t is d_kld_cnt[kld_parity], the clearing
    // kernel of that update zeroes the other one
    bool kld_on = false;
    bool in_group = false;              // one of a device group's engines (mcl_group_create): KLD is refused
    mcl_kld_config_t kld{};
    int64_t kld_nx = 0, kld_ny = 0;     // bin grid of the current map
    uint64_t kld_bits = 0;              // kld_nx * kld_ny * n_theta_bins + 1 (the outside bin)
    int64_t kld_n_next = 0;             // children the next mcl_update draws
    int64_t kld_bins_last = -1;         // bins the last update's draw occupied (-1: none counted)
    DevBuf<uint32_t> d_kld_bm, d_kld_list;
    DevBuf<unsigned int> d_kld_cnt;     // 2 counters
    int kld_parity = 0;
    // recovery by injection (mcl_set_recovery): the averages S, F (NaN: unset) on the host; an injecting update
    // counts its injected children in d_recov_cnt[recov_parity] and zeroes the other counter.  recov_cnt_slot: the counter of the
    // last update (-1: it injected nothing); recov_injected: the count once read (-1: not read yet)
    bool recov_on = false;
    mcl_recovery_config_t recov{};
    double recov_S = __builtin_nan(""), recov_F = __builtin_nan("");
    DevBuf<unsigned int> d_recov_cnt;        // 2 counters
    int recov_parity = 0, recov_cnt_slot = -1;
    int64_t recov_injected = 0;
    // the proposal the next injecting update draws its injected children from (mcl_set_recovery_proposal): mix_n
    // components (0: none -- the free cells), as uploaded (thresholds, 9 doubles per component) and the host's copy of both for
    // the getter.  Allocated by the first call that sets one.
    int32_t mix_n = 0;
    std::vector<uint64_t> mix_thr; std::vector<double> mix_fac;
    DevBuf<uint64_t> d_mix_thr; DevBuf<double> d_mix_fac;
    // likelihood-field sensor model (mcl_set_likelihood_field): the field and table of the current map (lf_K < 0:
    // not built), the used beams of an update's scan staged in pinned memory; last_lf: the last log-weights came from k_lfield
    bool lf_on = false, last_lf = false;
    mcl_likelihood_field_config_t lf{};
    int lf_K = -1;
    unsigned long long lf_epoch = 0;    // counts the fields built (what the pruned search pools belongs to one of them)
    DevBuf<uint16_t> d_lf_D;
    DevBuf<float> d_lf_tab;
    std::vector<float> lf_tab;
    DevBuf<double2> d_lf_beams;
    HostBuf<double2> h_lf_beams;
    // beam skipping (mcl_set_beam_skip; only while lf_on): the per-beam counters, the mask, the compacted beam
    // list and the state record of the last such update, all reserved by the first update that runs with it on.  bs_have: that
    // state is readable; bs_idx: the scan beam of every used beam of that update (lf_used_beams), bs_B its scan's beam count
    bool bs_on = false, bs_have = false;
    mcl_beam_skip_config_t bs{};
    int bs_B = 0;
    std::vector<int32_t> bs_idx;
    DevBuf<unsigned int> d_bs_cnt;
    DevBuf<uint8_t> d_bs_kept;
    DevBuf<double2> d_bs_beams;
    DevBuf<mcl_beam_skip_state_t> d_bs_state;
    // motion model (mcl_set_motion_model): REFERENCE, or an odometry model whose per-update scalars go to the
    // k_resample_odo* kernels as plain arguments
    mcl_motion_config_t motion{};
    // sensor mount (mcl_set_sensor_mount): the sensor's pose in the base frame (mounted: not all zero); the sensor
    // poses of the particles, written by k_mount_poses in front of a sensor stage and reserved by the first stage that runs with a
    // mount.  last_mounted: the last sensor stage read them (d_pc then holds the sensors' headings, not the particles');
    // sp_valid / sp_n: they are those of the current particles (mcl_get_sensor_poses)
    double mount[3] = {0.0, 0.0, 0.0};
    bool mounted = false, last_mounted = false, sp_valid = false;
    int64_t sp_n = 0;
    DevBuf<double> d_sx, d_sy, d_sth;
    // per-beam sensor offsets (mcl_set_beam_offsets): on or off; the table as given (3 x B column-major), DS1's float
    // angles a' and direction pairs on the host (the getter; DS5's pair formation), and ONE device block [pairs | table | angles] (mcl_host::deskew_block_words) with
    // its pinned staging twin, so that a new table is one asynchronous copy.  Buffers of their own: beam_cs / angles stay untouched.
    bool ds_on = false;
    int ds_B = 0;
    std::vector<double> ds_off;
    std::vector<float> ds_angle;
    std::vector<double2> ds_cs_host;
    DevBuf<double> d_ds;
    HostBuf<double> h_ds;
    const double2 *d_ds_cs() const { return reinterpret_cast<const double2 *>(d_ds.p); }
    const double *d_ds_off() const { return d_ds.p + 2 * (size_t)ds_B; }
    const float *d_ds_angle() const { return reinterpret_cast<const float *>(d_ds.p + 5 * (size_t)ds_B); }
    // mcl_sensor_update_fuse: the log-weights of the previous weighting call while the new ones are formed (reserved by the first
    // such call); weighted: the last weighting call (mcl_update*, mcl_sensor_update, the fuse call) was on the current particles
    DevBuf<double> d_logw_prev;
    bool weighted = false;
    // ---- side-call owners (released by mcl_destroy before the engine's own buffers, the streams idle)
    struct mcl_comm *comm = nullptr;    // RCCL communicator of a sharded set (mcl_comm_create), or null
    // pose clustering (mcl_pose_clusters): its own buffers, allocated on the first call; set_epoch counts the
    // changes of the particle set or its weights (the labels of a clustering are valid while it is unchanged)
    struct mcl_cluster *clu = nullptr;
    unsigned long long set_epoch = 0;
    // pose query (mcl_query_scans / mcl_score_poses): its own buffers, allocated on the first call
    struct mcl_query *qry = nullptr;
    // global search (mcl_global_search): its own buffers, allocated on the first call.  Its lattice is formed on
    // the host from the map's cells (grid_host, kept by mcl_set_map); map_epoch counts the maps set (a lattice and a score volume
    // belong to one of them)
    struct mcl_search *srch = nullptr;
    std::vector<int8_t> grid_host;
    unsigned long long map_epoch = 0;
    // pose refinement (mcl_refine_poses): its own buffers, allocated on the first call
    struct mcl_refine *rfn = nullptr;
    // ---- knobs
    EnvKnobs env;
};

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                        \
            return MCL_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

#define MCL_HIDDEN __attribute__((visibility("hidden")))    // on what the split of the engine unit made shared: the dynamic symbols stay the ones the library had
#define MCL_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// Did the fix-up lists of the last ray stage overflow?  (h_fix_count: the flag as fetched with the result block.)  Its log-weights
// are incomplete then, and the caller runs the stage again with the self-contained k_rays_skip (force_skip).
inline bool fix_lists_overflowed(const mcl_engine *h) { return h->last_work_lists && h->h_fix_count != 0; }

// One read-back step: the engine's device selected, the copies enqueued on its stream in the order given (an entry without a
// destination is skipped), one wait for the stream.
struct ReadBack { void *dst; const void *src; size_t bytes; };
MCL_HIDDEN inline int read_back(mcl_engine *h, std::initializer_list<ReadBack> copies)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (const ReadBack &c : copies)
        if (c.dst) HIPCHK(h, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

// Where the parents of a staged resample come from.
struct ParentSource {
    const double *px = nullptr, *py = nullptr, *pth = nullptr;     // gathered columns, n_parents entries each
    const void *records = nullptr;                                  // gathered (or compacted) packed records
    const double4 *rank_records[mcl::kMaxShards] = {};              // one record array per shard (peer pointers, same process)
    int64_t n_per_rank = 0;
    int self_rank = 0;
    unsigned long long *remote_count = nullptr;
    const unsigned char *cchunks = nullptr;                         // the shards' compact lists, gathered as chunks
    int64_t cchunk_entries = 0;
    const uint64_t *gcdf = nullptr, *gtop = nullptr;                // their merged CDF (k_compact_merge)
    const int32_t *idx_in = nullptr;                                // parents decided by an earlier index-only pass (into `records`)
    int32_t *idx_only_out = nullptr;                                // index-only pass: parents go here, nothing else happens
    bool keep = false;                                              // adaptive resampling kept the set: every particle is its own parent (motion only)
};

// ---- engine-side functions the sharded hosts and the clustering use (defined in mcl_engine.hip)
namespace mcl_host {
int fail(mcl_engine *h, int code, const char *msg);
int fail(mcl_engine *h, int code, const std::string &msg);
// what the option setters of both engine units refuse on a sharded engine, and what they reset
MCL_HIDDEN inline int refuse_shared(mcl_engine *h, const char *what)
{
    return !h->comm && !h->in_group ? MCL_OK : fail(h, MCL_ERR_UNSUPPORTED, std::string(what) + " is single-engine only: this engine has a communicator or belongs to a device group");
}
inline void recov_unset(mcl_engine *h) { h->recov_S = h->recov_F = NAN; }
// a new particle set (set / initialised): the next update draws clamp(N, min, max)
inline void kld_reset(mcl_engine *h)
{
    h->kld_bins_last = -1;
    h->kld_n_next = h->kld_on ? std::min(std::max(h->N, h->kld.min_particles), h->kld.max_particles) : h->N;
}
MCL_HIDDEN int kld_alloc(mcl_engine *h);
// The ordering's tiles over the padded map: occupied tiles are numbered compactly when the map has at most kSortMaxTiles of them
struct SortTiles { int ntx_abs, nty_abs; bool ok; };
MCL_HIDDEN SortTiles sort_tiles(const mcl_engine *h);
std::string &create_error();                 // what mcl_*_last_error(NULL) reports (thread-local)
bool ready(mcl_engine *h, bool need_particles);
float elapsed(hipEvent_t a, hipEvent_t b);
void graph_reset(mcl_engine *h);
// room in d_blocktot for the scan of n entries (scan_weights); a spine that moves drops the captured graphs and the layout
int reserve_scan_spine(mcl_engine *h, int64_t n);
// bind_sensor: this is the last kernel of its stage; set where EV_SENSOR became the stop event of the scan's last kernel (the engine's own weights, no capture)
int scan_weights(mcl_engine *h, const uint64_t *d_q, uint64_t *d_cdf, int64_t n, uint64_t offset, uint64_t *d_total, bool *bind_sensor = nullptr);
void unpack_result(mcl_engine *h);
int layout_adopt(mcl_engine *h, int64_t n);
int set_particles_impl(mcl_engine_t *h, const double *xyz, const double *weights, int64_t n, const double *weight_scale);
int stage_resample_launch(mcl_engine_t *h, const ParentSource &src, const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total,
                          int64_t child_first, int64_t n_children_total, const double action[3]);
int export_compact_launch(mcl_engine_t *h, void *d_chunk, int64_t chunk_entries, int dst_device, hipStream_t stream);
int stage_resample_compact_launch(mcl_engine_t *h, const void *d_chunks, int32_t n_shards, int64_t chunk_entries, const int64_t *counts,
                                  const uint64_t *totals, int64_t n_per_shard, int32_t self_shard, int64_t child_first,
                                  int64_t n_children_total, const double action[3], unsigned long long *remote_count);
int stage_rays_launch(mcl_engine_t *h, const float *obs, int32_t n_beams, bool force_skip, double *d_max_out = nullptr);
void stage_rays_note(mcl_engine_t *h);
int stage_rays_finish(mcl_engine_t *h, const float *obs, int32_t n_beams);
int stage_weights_launch(mcl_engine_t *h, double global_max_logw, const double *d_global_max = nullptr);
int stage_weights_finish(mcl_engine_t *h);
void stage_commit_carry(mcl_engine_t *h);
// the few kernels mcl_comm.hip / mcl_group.hip launch themselves (on `stream`)
void launch_copy_double(hipStream_t stream, const double *src, double *dst);
void launch_set_double(hipStream_t stream, double *dst, double v);
void launch_spin_ms(hipStream_t stream, double ms);
void launch_stage_pack(hipStream_t stream, const unsigned long long *d_result, double *d_vec, int n_shards, int self, int listed, unsigned long long list_cap);
void launch_pack_records(hipStream_t stream, const double *x, const double *y, const double *th, int64_t n, double4 *out);
void launch_group_max(hipStream_t stream, const mcl::GroupMaxArgs &a);
// the kernels of a map patch (mcl_map_patch.h), table by table, enqueued on the engine's stream; windows inclusive {x0, y0, x1, y1},
// the temporaries the caller's (launch_patch_* reserve them by the window and they live until the caller has waited for the stream)
struct MapPatchTmp { DevBuf<uint8_t> mask, g, hq[4]; DevBuf<int32_t> nxt, prv; DevBuf<mcl::WedgeRow> rows; DevBuf<uint16_t> lf_g; };
int launch_patch_skip_field(mcl_engine *h, const int32_t win[4], MapPatchTmp &t);                      // d_dist, d_dist4
int launch_patch_quadrant(mcl_engine *h, int q, const int32_t win[4], MapPatchTmp &t);                 // d_distq[q]
int launch_patch_wedges(mcl_engine *h, const int32_t win[4], const int32_t quad[4][4], MapPatchTmp &t);  // d_distw (after d_dist), d_distg
int launch_patch_lfield(mcl_engine *h, const int32_t win[4], int reach, int K, MapPatchTmp &t);        // d_lf_D
// the likelihood field's K and reach on the current map (lf_build's), the model on
inline void lf_reach_of(const mcl_engine *h, int &K, int &reach)
{
    K = lf_cap(&h->lf, (float)h->res);
    reach = (int)std::ceil(std::sqrt((double)K));                        // the least reach with reach^2 >= K
    while (reach * reach < K) ++reach;
    while (reach > 0 && (reach - 1) * (reach - 1) >= K) --reach;
}
// the likelihood field outside the update (mcl_query.hip): the used beams of a scan in beam order (LF3) into `out` (B entries of
// room), their number returned, with `idx` given also the scan beam of each; k_lfield over n poses and nb such beams on the engine's
// stream, the caller's buffers throughout
int lf_used_beams(const mcl_engine *h, const float *obs, int stride, double2 *out, int32_t *idx = nullptr, bool deskew = false);   // deskew: DS5's pairs (the update path alone)
int launch_lfield_on(mcl_engine *h, const double *x, const double *y, const double *th, int64_t n, const double2 *d_beams, int nb,
                     double *logw);
}  // namespace mcl_host
