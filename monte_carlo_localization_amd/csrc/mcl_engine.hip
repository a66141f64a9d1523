// mcl_engine.hip — C-ABI shim (include/mcl_hip_engine.h) over the HIP kernels in mcl_kernels.h: the engine object, its buffers and
// streams, the update and its stages (kernel launches on the engine's own stream + HIP-event stage timings, utils.hpp:51-57).
// The host arithmetic (sensor table, distance fields, motion scalars, ...) is in mcl_host_math.hip, the launch-free entry points in mcl_engine_access.hip.
// There is NO CPU fallback: without a gfx950 device mcl_create fails with MCL_ERR_NO_DEVICE.
#include "../../include/mcl_hip_engine.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mcl_engine_internal.h"
#include "mcl_kernels.h"
#include "mcl_lfield.h"
#include "mcl_mount.h"

static_assert(MCL_WEDGES == mcl::kWedges || MCL_KWEDGES != 16, "include/mcl_hip_engine.h and csrc/mcl_wedge.h disagree");

using namespace mcl_host;

namespace {

thread_local std::string g_create_error;

int ensure_lt(mcl_engine *h)
{
    MCL_TRY(h->d_Lt.reserve(h, 2 * (size_t)(h->P + 1) * h->bpad));     // [Lt | Lt with the rows reversed (k_rays_cell)]
    h->ltd_cols = (h->B + 2 * h->beam_margin + 64) & ~63;              // beam j in column j + beam_margin; at least one all-zero column after the last beam
    const size_t need_d = (size_t)mcl::sweep_table_rows(h->P) * h->ltd_cols;
    if (need_d > h->d_Ltd.cap) {
        MCL_TRY(h->d_Ltd.reserve(h, need_d));
        h->ltd_ready = false;
    }
    return MCL_OK;
}

void build_ltd(mcl_engine *h);
struct RayPlan;
void ray_kernel_deskew(mcl_engine *h, const RayPlan &p, mcl::RayArgs &a);
int sensor_poses(mcl_engine *h, const double *&x, const double *&y, const double *&th, int64_t n);

// weights/q/sums from either log-weights (from_log) or raw weights already in d_w.  defer_sums: the caller scans d_q next
// (scan_weights), whose one-workgroup spine then also reduces the partial sums -- one launch less.
int weight_stats(mcl_engine *h, bool from_log, const double *d_max_override, bool defer_sums = false)
{
    const int64_t n = h->N;
    const double *src = from_log ? h->d_logw : h->d_w;
    const double *max_parts = nullptr;
    if (!d_max_override) {
        if (!(from_log && h->max_partials_ready))        // k_combine_logw already left the per-workgroup maxima in d_maxpart
            hipLaunchKernelGGL(mcl::k_reduce_max, dim3(mcl::kRedBlocks), dim3(mcl::kRedThreads), 0, h->stream, src, n, h->d_maxpart);
        max_parts = h->d_maxpart;                        // every workgroup of k_weights reduces them itself (no k_final_max in between)
    }
    h->max_partials_ready = false;
    hipLaunchKernelGGL(mcl::k_weights, dim3(mcl::kRedBlocks), dim3(mcl::kRedThreads), 0, h->stream, src, from_log ? 1 : 0,
                       d_max_override ? d_max_override : h->d_scalars, h->d_x[h->cur], h->d_y[h->cur], h->d_th[h->cur], n, h->d_w, h->d_q, h->d_part,
                       (from_log && h->cfg.resample_neff_permille > 0) ? h->d_carry[h->carry_idx ^ 1] : (double *)nullptr,
                       max_parts, mcl::kRedBlocks);
    h->carry_pending = from_log && h->cfg.resample_neff_permille > 0;     // the caller commits it (commit_carry)
    if (!from_log) h->carry_valid = false;
    if (defer_sums) h->sums_pending = true;
    else hipLaunchKernelGGL(mcl::k_final_sums, dim3(1), dim3(mcl::kRedThreads), 0, h->stream, h->d_part, mcl::kRedBlocks, h->d_scalars);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

int fetch_scalars(mcl_engine *h)
{
    // scalars, counters and the work-list overflow flag in one copy into pinned memory
    HIPCHK(h, hipMemcpyAsync(h->h_result, h->d_result, kResultWords * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_result(h);
    return MCL_OK;
}

// ---- ray modes: choose_ray_mode's answers are the public MCL_RAYS_* enumerators (0: the configured kernel cannot run); what the
// host code asks of one
bool mode_work_lists(int mode) { return mode == MCL_RAYS_QUAD || mode == MCL_RAYS_CELL || mode == MCL_RAYS_SWEEP; }   // quadrant / wedge windows + fix-up lists
bool mode_orders(int mode) { return mode == MCL_RAYS_CELL || mode == MCL_RAYS_SWEEP; }       // cell-sorted particles, one particle per lane
bool mode_sweep(int mode) { return mode == MCL_RAYS_SWEEP; }
bool mode_fills_pc(int mode) { return mode != 0 && mode != MCL_RAYS_MARCH && mode != MCL_RAYS_DESKEW; }   // every kernel but the literal march and k_rays_deskew works from d_pc

// The hybrid form of k_rays_sweep (ranges beyond the LDS window: the walk leaves the window into the global wedge fields where a
// ray is that long): for evenly spaced scans (the turned-direction walk), when both sets of fields exist.  MCL_SWEEP_HYBRID=0:
// the global-field form alone, as in round 4.
bool sweep_hybrid(const mcl_engine *h)
{
    return h->sweep_global && h->env.sweep_hybrid != 0 && h->rec_ok && h->sweep_hyb_layout_ok && h->d_beam_err != nullptr &&
           h->d_distw != nullptr && h->d_distg != nullptr && (size_t)mcl::kSwWinBytes + (size_t)h->ltd_cols * 8 <= 80 * 1024 - 64;
}

// (... of THIS update: a set that was just initialised, or whose last update left many particles to the far pass -- the spread
//  cloud of a re-localisation --, takes the global-field form: every lane has its own origin there, where the hybrid's windows
//  would hand a good part of such a cloud to the far pass.  fine025 stand-in, 4M uniform: first update 39 ms against 64.)
bool sweep_far_expected(const mcl_engine *h) { return h->far_fresh || h->h_result[15] >= mcl::kFarWindowedMin / 2; }
// Decided ONCE per update (launch_rays).  A hybrid update that left many particles to the far pass -- a cloud that has not converged
// yet -- is followed by 1, 2, 4 .. 32 updates in the global-field form before the hybrid is tried again (a global-field update
// flags nothing, so its count says nothing about the cloud: without the back-off the two forms would alternate).
// MCL_SWEEP_HYBRID=2: always the hybrid (the tests' setting).
bool sweep_hybrid_decide(mcl_engine *h)
{
    if (!sweep_hybrid(h)) return false;
    if (h->env.sweep_hybrid == 2) return true;
    if (h->far_fresh) { h->hyb_backoff = 0; h->hyb_skip = 0; return false; }
    if (h->last_sweep_global == 2) {
        if (h->h_result[15] >= mcl::kFarWindowedMin / 2) { h->hyb_backoff = h->hyb_backoff ? std::min(32, 2 * h->hyb_backoff) : 1; h->hyb_skip = h->hyb_backoff; }
        else h->hyb_backoff = 0;
    }
    if (h->hyb_skip > 0) { --h->hyb_skip; return false; }
    return true;
}

// cells the particles of one k_rays_sweep work item may spread over (per axis): what the 256-cell LDS window leaves beside a
// ray's reach, or -- on the global wedge fields -- the span of the cell field minus the reach on both sides
int sweep_play(const mcl_engine *h, bool hybrid)
{
    if (hybrid) return mcl::kSwSide - (mcl::kSwHybReach + 2) - 3;
    if (h->sweep_global) return 1 << 20;             // every lane has its own origin there: no window a run could outgrow
    return mcl::kSwSide - (h->P + 2) - 3;
}

// the window play the units of a layout are cut for and k_sweep_plan works with (0: no windowed kernel; -1: no cuts at all, MCL_NO_BUCKET_CUTS)
int unit_play(const mcl_engine *h, int mode, bool hybrid)
{
    return h->env.no_bucket_cuts ? -1 : (mode_sweep(mode) ? sweep_play(h, hybrid) : 0);
}

// upper bound on the units of n sorted particles: the plain grid plus one cut per bucket of a sparse set (mcl::k_unit_table)
int64_t max_sweep_units(int64_t n) { return (n + mcl::kSwUnit - 1) / mcl::kSwUnit + mcl::kSwMaxCuts + 2; }

// Work items of k_rays_sweep: made on the device from this update's unit statistics (k_sweep_plan, mcl_rays_sweep.h);
// the host only sizes the list (every unit on its own, once per wedge group, is the longest it can get).
int launch_sweep_plan(mcl_engine *h, int64_t n, int nwg, int g, bool hybrid)
{
    const int ngroups = mcl::kWedges / g;
    MCL_TRY(h->d_items.reserve(h, (size_t)max_sweep_units(n) * ngroups));
    MCL_TRY(h->d_centres.reserve(h, (size_t)max_sweep_units(n)));
    MCL_TRY(h->d_nitems.reserve(h, 1));
    const int play = sweep_play(h, hybrid);                             // cells a window leaves for the particles of an item
    // (EV_K0 = the stop event of the kernel before the ray kernel, EV_K1 = the ray kernel's own: its duration, dispatch included, at no cost)
    hipExtLaunchKernelGGL(mcl::k_sweep_plan, dim3(1), dim3(1024), mcl::kPlanLds, h->stream, nullptr, h->ev[EV_K0], 0, h->d_unit_sums.p, h->d_nunits.p, ngroups, nwg,
                          (double)(play / 2 - 1), h->env.sw_guide > 0 ? h->env.sw_guide : (h->sweep_global ? 3 : 2), h->d_items.p, h->d_centres.p, h->d_nitems.p);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

// Which ray kernel a launch over n particles takes, as its MCL_RAYS_* enumerator (MARCH .. SWEEP); 0 = the configured kernel
// cannot run with this map / beam set.  A pure function of the configuration, the map, the beam set and n, so that
// callers (graph eligibility, table building, mcl_get_planned_ray_kernel) can ask before anything is launched.  *why, when
// given, receives a static sentence saying what decided (the kernels that address their LDS window from a raw offset are
// only chosen when the host-side layout check of mcl_create passed: no configuration can make the device abort).
int choose_ray_mode(const mcl_engine *h, int64_t n, bool force_skip, const char **why = nullptr)
{
    const char *dummy;
    const char *&w = why ? *why : dummy;
    const int rk = h->cfg.ray_kernel;
    // per-beam sensor offsets (mcl_set_beam_offsets): every beam has its own origin, which one kernel handles; the
    // setter refuses a configured kernel, so nothing below is overruled
    if (rk == MCL_RAYS_DESKEW) { w = "MCL_RAYS_DESKEW cannot be configured: it is the kernel of an update with per-beam offsets on (mcl_set_beam_offsets); set ray_kernel to MCL_RAYS_AUTO"; return 0; }
    if (h->ds_on) { w = "per-beam sensor offsets are on (mcl_set_beam_offsets): k_rays_deskew casts every beam from its own origin, in one launch (under the likelihood field no ray kernel runs: k_lfield takes the offsets in its beams' pairs)"; return MCL_RAYS_DESKEW; }
    if (rk == MCL_RAYS_MARCH) { w = "configured: MCL_RAYS_MARCH"; return MCL_RAYS_MARCH; }
    // k_rays_skip without its LDS layout (never seen): the literal march, same results
    if (rk == MCL_RAYS_SKIP || force_skip) {
        if (!h->skip_layout_ok) { w = "k_rays_skip's LDS layout check failed at mcl_create: literal march"; return MCL_RAYS_MARCH; }
        w = force_skip ? "fix-up list overflow: the stage is re-run with k_rays_skip" : "configured: MCL_RAYS_SKIP";
        return MCL_RAYS_SKIP;
    }
    const char *no_windows = nullptr;                        // why the windowed kernels (quad / cell / sweep) are out, if they are
    if (!h->quad_ok) no_windows = "beam angles are not monotone over less than a turn (or more than 16383 beams): the windowed kernels need contiguous beam ranges per direction wedge";
    else if (h->qside <= 0) no_windows = "MAX_RANGE_PX leaves less than 32 cells of play in a 280-cell byte window: the windowed kernels cannot hold a ray";
    [[maybe_unused]] const bool windows_ok = no_windows == nullptr;           // monotone beams over less than a turn, room for a byte window
#ifdef MCL_LEGACY_RAY_KERNELS
    if (rk == MCL_RAYS_QUAD) { w = windows_ok && h->quad_layout_ok ? "configured: MCL_RAYS_QUAD" : (no_windows ? no_windows : "k_rays_quad's LDS layout check failed"); return windows_ok && h->quad_layout_ok ? MCL_RAYS_QUAD : 0; }
    if (rk == MCL_RAYS_CELL) { w = windows_ok && h->cell_layout_ok ? "configured: MCL_RAYS_CELL" : (no_windows ? no_windows : "k_rays_cell's LDS layout check failed"); return windows_ok && h->cell_layout_ok ? MCL_RAYS_CELL : 0; }
#else
    // k_rays_quad / k_rays_cell, the predecessors of k_rays_sweep, are not part of this library (csrc/mcl_rays_legacy.h, a build
    // flag; the tests load libmcl_hip_engine_legacy.so for them)
    if (rk == MCL_RAYS_QUAD || rk == MCL_RAYS_CELL) { w = "MCL_RAYS_QUAD / MCL_RAYS_CELL are not built into this library (build flag MCL_LEGACY_RAY_KERNELS)"; return 0; }
#endif
    // its windows are 256 cells wide (mcl_rays_sweep.h) and addressed from a raw LDS offset checked at mcl_create
    // ... or, for ranges beyond that, probes the same wedge fields in global memory
    const char *no_sweep = h->quad_ok ? nullptr : no_windows;
    if (!no_sweep) {
        if (h->sweep_global) { if (!h->d_distg) no_sweep = h->distg_why_not ? h->distg_why_not : "k_rays_sweep's global-field form: fields not built"; }
        else if (!mcl::sweep_window_fits(h->P)) no_sweep = "MAX_RANGE_PX > 243: a 256-cell window of k_rays_sweep cannot hold a ray plus 8 cells of play";
        else if (!h->sweep_layout_ok) no_sweep = "k_rays_sweep's LDS layout check failed at mcl_create";
    }
    const bool sweep_ok = no_sweep == nullptr;
    if (rk == MCL_RAYS_SWEEP) { w = sweep_ok ? "configured: MCL_RAYS_SWEEP" : no_sweep; return sweep_ok ? MCL_RAYS_SWEEP : 0; }
    // AUTO: one particle per lane on cell-sorted particles pays once there are enough particles to fill the machine
    // with 64-particle groups and enough rays to amortise the sort (measured, wall ms skip / quad / cell:
    // 4096 x 1081 0.16/0.28/0.40, 65536 x 1081 0.55/0.56/0.44, 65536 x 61 0.21/0.33/0.25, 262144 x 61 0.47/0.76/0.40);
    // below that the self-contained k_rays_skip (one launch, no work lists) is the quickest
    const int64_t cell_min = h->env.cell_min > 0 ? h->env.cell_min : 65536;
    const bool big = n >= cell_min && n * (int64_t)h->B >= (8 << 20);
    if (big && sweep_ok) {
        w = sweep_hybrid(h) ? "AUTO: at least 65536 particles and 2^23 rays, evenly spaced beams; MAX_RANGE_PX > 243 (or MCL_SWEEP_GLOBAL): k_rays_sweep walks in LDS windows and goes on in the wedge fields in global memory where a ray leaves its window"
          : h->sweep_global ? "AUTO: at least 65536 particles and 2^23 rays, monotone beams; MAX_RANGE_PX > 243 (or MCL_SWEEP_GLOBAL): k_rays_sweep probes the wedge fields in global memory"
                            : "AUTO: at least 65536 particles and 2^23 rays, monotone beams, MAX_RANGE_PX <= 243";
        return MCL_RAYS_SWEEP;
    }
#ifdef MCL_LEGACY_RAY_KERNELS
    if (big && windows_ok && h->cell_layout_ok) { w = no_sweep; return MCL_RAYS_CELL; }
#endif
    if (!h->skip_layout_ok) { w = "k_rays_skip's LDS layout check failed at mcl_create: literal march"; return MCL_RAYS_MARCH; }
    w = !big ? "AUTO: fewer than 65536 particles or 2^23 rays: the self-contained k_rays_skip is the quickest" : no_sweep;
    return MCL_RAYS_SKIP;
}

// Two ways to the same kind of order (which lanes share a wave; never results).  Counting sort with per-XCD
// histograms: one returning L2 atomic per particle (~1 per clock and XCD) + a scatter.  From 3M particles a radix
// sort of (key, index) pairs is quicker -- keys only, rocPRIM's device sort (a plain library sort), then a gather:
// 4M x 1081 6.57 -> 6.47 ms per update; below, its fixed cost of a dozen launches loses (2M +0.03, 262 144 +0.05 ms).
bool sort_radix(const mcl_engine *h, int64_t n) { return h->env.sort_radix >= 0 ? h->env.sort_radix != 0 : n >= 3000000; }
// The fine key bits of the radix path (SortLayout::fine), the one place they come from: ray_order's keys, sort width and gather, and the
// keys the resampling kernel writes.  The counting sort has none (its histogram is the coarse key space).
// (one word, mcl::sort_fine_code: the bits and, where MCL_SORT_FINE_SUB or the default names it, how many of them per axis are sub-cell bits)
int sort_fine(const mcl_engine *h)
{
    const int f = h->env.sort_fine >= 0 ? std::min(h->env.sort_fine, mcl::kSortMaxFine) : mcl::kSortFineDefault;
    const int fs = h->env.sort_fine_sub >= 0 ? h->env.sort_fine_sub : (h->env.sort_fine >= 0 ? -1 : mcl::kSortFineSubDefault);
    return mcl::sort_fine_code(f, std::min(fs, 5));
}

// The layout the ordering works from, on `stream`: the bounding box of the particles in d_pc (every 16th of a large set), and
// the occupied tiles of the map numbered compactly when the map has at most kSortMaxTiles of them (bbox[5] says so)
void launch_layout(mcl_engine *h, hipStream_t stream, int64_t n, int *bbox, int *tilemark, int *tilemap)
{
    const auto [ntx_abs, nty_abs, tiles_ok] = sort_tiles(h);
    const int bstride = n >= (1 << 20) ? 16 : 1;
    hipLaunchKernelGGL(mcl::k_cell_bbox, dim3((unsigned)std::min<int64_t>((n / bstride + 255) / 256, 128)), dim3(256), 0, stream, h->d_pc, n,
                       bstride, h->Wp, h->Hp, bbox, tiles_ok ? tilemark : (int *)nullptr, ntx_abs);
    if (tiles_ok) hipLaunchKernelGGL(mcl::k_tile_compact, dim3(1), dim3(1024), 0, stream, bbox, tilemark, tilemap, ntx_abs * nty_abs);
}

// The windowed pass over what k_rays_sweep's windows did not fit (k_rays_skip<.., FAR>): ordered list of the flagged slots,
// then persistent workgroups with the 568-cell nibble window.  Every kernel stands down on the device when the launch flagged
// fewer than kFarWindowedMin slots (the tracking regime: none), and k_rays_far stands down when this pass runs.
int launch_far_windowed(mcl_engine *h, const mcl::RayArgs &a, int64_t n, bool count)
{
    const unsigned nb = (unsigned)((n + mcl::kFarTile - 1) / mcl::kFarTile);
    const uint32_t *flags32 = reinterpret_cast<const uint32_t *>(h->d_far.p);
    hipLaunchKernelGGL(mcl::k_far_count, dim3(nb), dim3(256), 0, h->stream, flags32, n, a.far_count, h->d_far_cnt);
    hipLaunchKernelGGL(mcl::k_far_spine, dim3(1), dim3(1024), 0, h->stream, h->d_far_cnt, (int)nb, a.far_count);
    hipLaunchKernelGGL(mcl::k_far_scatter, dim3(nb), dim3(256), 0, h->stream, flags32, n, a.far_count, h->d_far_cnt, h->d_far_sorted);
    const size_t lds = (size_t)h->tw_cells * h->tw_cells / 2;
    if (count) hipLaunchKernelGGL((mcl::k_rays_skip<1, true, true>), dim3(h->num_cu), dim3(mcl::kRayThreads), lds, h->stream, a);
    // (one ray per lane: two / four in flight measured 52 / 67 ms against 46 on the uniform levine cloud)
    else hipLaunchKernelGGL((mcl::k_rays_skip<1, false, true>), dim3(h->num_cu), dim3(mcl::kRayThreads), lds, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

// ---- the ray stage: plan_rays decides, launch_rays launches in phases that read the plan
// Everything a launch decides before or between its kernels.  Filled by plan_rays with arithmetic on the engine's state: no
// runtime call, nothing reserved.
struct RayPlan {
    int mode = 0;                                           // choose_ray_mode's answer (0: cannot run)
    bool lists = false, ordered = false, sweep = false;     // mode_work_lists / mode_orders / mode_sweep of it
    bool count = false;                                     // debug_count_probes: the COUNT instantiations
    bool timed = false;                                     // without work lists: EV_K0 / EV_K1 recorded around the kernel
    int R = 1;                                              // k_rays_skip: rays per lane
    int grid = 1;                                           // k_rays_march / k_rays_skip: workgroups
    size_t lds = 0;                                         // ... and the nibble window of k_rays_skip
    int nsl = 1, items_per_slice = 4, sweep_g = 1;          // slices (units for k_rays_sweep), work items per slice, wedges per item
    int nseg = 1, fix_split = 1;                            // persistent workgroups = fix-up list segments; k_rays_fix workgroups per segment
    bool fix_flat = false; int fix_grid = 1;                // k_rays_fix: the flat deal (else per segment) and its grid
    unsigned long long segcap = 0;                          // entries per segment
    unsigned gfar = 1;                                      // k_rays_far's grid
    bool hyb = false, glob = false, rec = false, pairs = false;   // the form of k_rays_sweep
    size_t qlds = 0;                                        // LDS of the kernel with work lists
    bool far_windowed = false, radix = false;
    // what the resampling launch left for this stage (RayHandoff): constants in d_pc | ordering by the previous layout | (key, index)
    // pairs written | the few words cleared, given clear_passed | the wait for ev_obs is this launch's to issue
    bool constants_ready = false, stale_layout = false, keys_written = false, clear_folded = false, obs_wait = false;
    bool heading_form = false;                              // d_pc holds the heading form and the radix gather of this launch reads it
    mcl::PrepClear clear_passed{};
};

// Slices, list segments and grids of the kernels with work lists (quad, cell, sweep)
void plan_work_lists(const mcl_engine *h, int64_t n, RayPlan &p)
{
    // item granularity: 32 slices per CU (measured best at 4M: 4/8/16/32/64 -> 22.1/20.2/19.7/19.6/20.2 ms), but at
    // least 256 particles per slice so that the 78 KB window load stays amortised
    const int spc = h->env.qslices_per_cu > 0 ? h->env.qslices_per_cu : 32;
    p.nsl = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)spc * h->num_cu, (n + 255) / 256));
    if (p.ordered) {
        // k_rays_cell: a slice is a run of the sorted order; 2048 particles = two 64-particle groups per wave.  Longer
        // slices amortise the window load better, shorter ones balance the persistent workgroups better
        // (measured at 4M: 1024/2048/4096/8192/16384 -> 8.59/8.04/7.86/7.96/8.64 ms; at 256k: 2048/4096 -> 0.68/0.79 ms)
        int64_t slice_len = h->env.cell_slice > 0 ? std::max<int64_t>(64, h->env.cell_slice) : (n >= (1 << 21) ? 4096 : 2048);
        p.nsl = (int)std::max<int64_t>(1, (n + slice_len - 1) / slice_len);
    }
    if (p.sweep) {
        // k_rays_sweep: a work item is (run of 1024-particle units, G wedges); the G wedges of a group share one
        // partial-sum array.  G = 2 (measured at 4M x 1081, ray kernel / update ms, same device: G = 1 6.50 / 7.87,
        // 2 6.54 / 7.86, 4 6.69 / 7.97, 8 6.99 / 8.27, 16 7.62 / 8.90: a longer item is a longer tail); G = 1 up to 2M
        // particles, where the finer items balance better than the sixteen partial-sum arrays cost (262 144 x 1081:
        // 0.58 / 0.80 -> 0.53 / 0.77, 1M: 1.72 / 2.13 -> 1.63 / 2.07; at 4M G = 1 and 2 are level).
        // Round 3: with the per-wedge sums added atomically (no partial-sum array per group) G = 1 wins at every size
        // (4M x 1081, ms per update G = 1 / 2 / 4: 6.80 / 6.91 / 7.08; levine stand-in 7.89 / 8.00 / 8.24)
        p.sweep_g = h->env.sweep_g > 0 ? h->env.sweep_g : 1;
        if (p.sweep_g > mcl::kWedges || (mcl::kWedges % p.sweep_g) != 0) p.sweep_g = 1;
        p.nsl = (int)((n + mcl::kSwUnit - 1) / mcl::kSwUnit);
    }
    p.items_per_slice = p.sweep ? mcl::kWedges / p.sweep_g : (p.ordered ? mcl::kWedges : 4);
    const int max_wg = 2 * (h->num_cu - h->reserved_cus);             // persistent: 2 workgroups per CU
    p.nseg = (int)std::min<int64_t>(max_wg, p.items_per_slice * (int64_t)p.nsl);   // one segment per persistent workgroup
    // work list for undecided rays (~0.06 % of the rays in practice): one segment per persistent workgroup of
    // k_rays_quad with room for 1/256 of that workgroup's share of the rays (at least 2048 entries)
    // (both forms of k_rays_sweep work with 32 fractional bits: a walk of ~70 rays is handed over once in several thousand)
    const unsigned long long rays_per_seg = (unsigned long long)n * h->B / p.nseg + 64, seg_div = 256;
    p.segcap = std::max<unsigned long long>(2048, (rays_per_seg / seg_div + 7) & ~7ull);
    // small launch: room for every ray.  A segment may serve a single (units, wedge) item there, and twice the even share covers a
    // scan of a quarter turn and more (a Hokuyo puts 91 of its 1081 beams into one wedge: 1.35 sixteenths); a 45-degree scan puts
    // half its beams into one wedge, so k_rays_sweep's share follows the scan (wedge_beams_max), within the 64 MB the factor 2
    // takes at 4M rays
    unsigned long long share = 2;
    if (p.sweep && h->B > 0) {
        const unsigned long long rays = std::max<unsigned long long>(1, (unsigned long long)n * h->B);
        const unsigned long long by_scan = ((unsigned long long)h->wedge_beams_max * p.items_per_slice + h->B - 1) / h->B;
        share = std::max<unsigned long long>(2, std::min<unsigned long long>(by_scan, (8ull << 20) / rays));
    }
    if ((unsigned long long)n * h->B <= (4ull << 20)) p.segcap = (share * rays_per_seg + 7) & ~7ull;
    // k_rays_far is bound by global-memory latency: 4 workgroups per CU worth of blocks (2 resident at a time)
    p.gfar = (unsigned)std::max<int64_t>(1, std::min<int64_t>(4 * (int64_t)h->num_cu, (n + 15) / 16));
    p.fix_split = std::max(1, std::min(16, (mcl::kFixWgPerCu * h->num_cu) / std::max(p.nseg, 1)));   // ~8 workgroups of k_rays_fix per CU (2 .. 16 per segment: no difference, round 4)
    // k_rays_fix deals the listed rays of ALL segments evenly over its grid when a workgroup's LDS holds the prefix of their counts (32-bit
    // sums); otherwise fix_split workgroups share a segment.  MCL_FIX_DEAL=seg takes the latter on any launch, MCL_FIX_WG=<per CU> sizes the
    // flat grid (profiles/fix_pass.md): A/B switches on one build, the same results.
    p.fix_flat = !h->env.fix_deal_seg && p.nseg <= mcl::kFixSegMax && (unsigned long long)p.nseg * p.segcap < (1ull << 32);
    p.fix_grid = p.fix_flat ? std::max(1, (h->env.fix_wg > 0 ? std::min(h->env.fix_wg, 16) : mcl::kFixWgPerCu) * h->num_cu) : p.nseg * p.fix_split;
}

// Which form of k_rays_sweep THIS update takes, and whether the windowed far pass goes with it
void plan_sweep_form(mcl_engine *h, RayPlan &p)
{
    p.hyb = sweep_hybrid_decide(h);                    // LDS windows as far as they reach, the global fields beyond
    p.glob = h->sweep_global && !p.hyb;                // probes in global memory: no window in LDS
    // REC: the walk turns the beam direction by the scan's increment instead of fetching it (evenly spaced scans; the beams'
    // offsets from the grid sit in LDS behind the window: 8 bytes per table column)
    // (... as long as two workgroups still fit a CU's 160 KB: up to ~1800 table columns; more beams than that fetch their directions)
    p.rec = h->rec_ok && h->sweep_rec_layout_ok && h->d_beam_err != nullptr && (size_t)mcl::kSwWinBytes + (size_t)h->ltd_cols * 8 <= 80 * 1024 - 64;
    // the windowed far pass (four launches that stand down on the device when little is flagged) is only launched when
    // there is reason to expect work for it: the previous ray stage flagged a fair number of slots, or the particle set
    // is fresh (set / initialised since).  A misjudgement costs time, never results: without it k_rays_far takes all.
    p.far_windowed = sweep_far_expected(h);
    // PAIRS (two rays per lane) where the walk waits for memory: always in the global-field form; in LDS windows for a set
    // that was set / initialised since the last update (the spread cloud of a re-localisation: -11 % on its first update, where
    // the tracking cloud gains nothing and the levine stand-in loses 2 %); MCL_SWEEP_PAIRS=0 / 1 overrides
    p.pairs = p.rec && !p.hyb && (h->env.sweep_pairs >= 0 ? h->env.sweep_pairs != 0 : (p.glob || p.far_windowed));
    p.qlds = (p.glob ? 0 : (size_t)mcl::kSwWinBytes) + (p.rec ? (size_t)h->ltd_cols * 8 : 0);
}

// The one piece of state written here is the hybrid's back-off (sweep_hybrid_decide, once per launch that takes k_rays_sweep);
// the other two a decision leaves behind, far_fresh and last_sweep_*, are written by launch_rays where its reservations are through.
RayPlan plan_rays(mcl_engine *h, int64_t n, bool force_skip, bool direct_table)
{
    RayPlan p;
    p.mode = choose_ray_mode(h, n, force_skip);
    p.lists = mode_work_lists(p.mode); p.ordered = mode_orders(p.mode); p.sweep = mode_sweep(p.mode);
    p.count = h->cfg.debug_count_probes != 0;
    p.R = h->cfg.rays_per_lane > 0 ? h->cfg.rays_per_lane : 1;   // measured on MI355X: the kernel is VALU-issue-bound, extra chains per lane only add idle slots
    p.grid = (int)std::max<int64_t>(1, std::min<int64_t>(h->num_cu, (n + 15) / 16));
    p.lds = (size_t)h->tw_cells * h->tw_cells / 2;
    p.timed = !p.lists && !h->capturing && !direct_table;
    if (p.mode == MCL_RAYS_DESKEW) p.grid = (int)((n + mcl::kDeskewWaves - 1) / mcl::kDeskewWaves);      // a wave per particle: no lists, not ordered, no sweep
    const RayHandoff &ho = h->handoff;
    p.constants_ready = ho.constants;
    // the heading form of d_pc has one reader that finishes it, the gather of the radix path in front of k_rays_sweep, whose kernels
    // (fix-up, far, exact) read the gathered pcs by slot; a launch that takes another road (the counting sort, k_rays_cell whose
    // fix-up and far kernels read d_pc by particle index, a kernel that reads d_pc itself) makes the full form with k_particle_prep,
    // as if nothing had been prepared
    p.heading_form = ho.heading && ho.keys && ho.stale_layout && mode_sweep(p.mode) && sort_radix(h, n);
    if (ho.heading && !p.heading_form) p.constants_ready = false;
    if (!p.lists) return p;
    plan_work_lists(h, n, p);
    if (p.sweep) plan_sweep_form(h, p);
    else p.qlds = (size_t)h->qside * h->qside;
    p.stale_layout = p.ordered && ho.stale_layout;           // d_bbox / d_tilemap hold the layout to order by: not remade
    p.keys_written = ho.keys; p.clear_folded = ho.folded; p.clear_passed = ho.passed; p.obs_wait = ho.obs_wait;
    p.radix = p.ordered && sort_radix(h, n);
    return p;
}

// Phase 1: what a ray kernel is given whatever its kind (the work lists and the ordering add theirs once they are reserved)
mcl::RayArgs ray_args(const mcl_engine *h, const double *x, const double *y, const double *th, int64_t n, bool direct_table)
{
    mcl::RayArgs a{};
    a.x = x; a.y = y; a.th = th; a.n = n;
    a.pc = h->d_pc;
    a.B = h->B; a.bpad = h->bpad; a.P = h->P;
    a.beam_cs = h->d_beam_cs; a.beam_angle = h->d_angle; a.Lt = h->d_Lt;
    a.Ltr = h->d_Lt + (size_t)(h->P + 1) * h->bpad;
    a.beam_a0 = h->B > 0 ? (double)h->angles[0] : 0.0;
    a.beam_alast = h->B > 0 ? (double)h->angles[h->B - 1] : 0.0;
    const double span = h->B > 1 ? (double)h->angles[h->B - 1] - (double)h->angles[0] : 0.0;
    a.beam_inv_inc = span > 0.0 ? (double)(h->B - 1) / span : 0.0;
    a.logw = h->d_logw;
    a.grid = h->d_grid; a.W = h->W; a.H = h->H;
    a.res = h->res; a.ox = h->ox; a.oy = h->oy;
    if (direct_table) { a.Ldirect = h->d_L; a.obs_idx = h->d_obs_idx; }       // small updates: no per-update table (do_update)
    a.dist = h->d_dist; a.dist4 = h->d_dist4; a.Wp = h->Wp; a.Hp = h->Hp; a.Wps = h->Wps;
    for (int q = 0; q < 4; ++q) a.distq[q] = h->d_distq[q];
    a.tw_cells = h->tw_cells;
    a.counters = h->d_counters;
    a.force_exact = h->cfg.debug_force_exact;
    return a;
}

// Phase 2 (keep_ray_steps): one byte per step index up to 255 px of range, two beyond (allocated here: both the map and the beam set size it)
int ray_step_buffer(mcl_engine *h, mcl::RayArgs &a)
{
    if (!h->cfg.keep_ray_steps) return MCL_OK;
    const size_t need = (size_t)h->cap * h->B * (h->P > 255 ? 2 : 1);
    if (need > h->d_steps.cap) {
        if (h->capturing) return fail(h, MCL_ERR_HIP, "step buffer missing during capture (internal)");
        graph_reset(h);
        MCL_TRY(h->d_steps.reserve(h, need));
    }
    if (h->P > 255) a.steps16 = reinterpret_cast<uint16_t *>(h->d_steps.p);
    else a.steps = h->d_steps;
    return MCL_OK;
}

// Phase 3a (work lists): the fix-up lists, one segment per persistent workgroup, and what the kernels are told of them
int ray_fix_lists(mcl_engine *h, const RayPlan &p, mcl::RayArgs &a)
{
    MCL_TRY(h->d_fix_list.reserve(h, (size_t)p.nseg * p.segcap));
    MCL_TRY(h->d_fix_count.reserve(h, (size_t)p.nseg * 8));
    h->fix_cap = p.segcap;
    h->fix_segments = p.nseg;
    a.qr = p.ordered ? nullptr : h->d_qr;
    a.qside = p.sweep ? mcl::kSwSide : h->qside;
    a.nslices = p.nsl;
    a.fix_list = h->d_fix_list; a.fix_count = h->d_fix_count; a.fix_cap = h->fix_cap; a.fix_segments = p.nseg;
    a.exact_list = h->d_exact_list; a.exact_count = h->d_result + 14; a.exact_cap = kExactCap;
    a.far_flags = h->d_far;
    a.work_counter = h->d_fix_over + 1;                // second word of the 16-byte scratch block
    a.logw = h->d_logw_acc;
    return MCL_OK;
}

// Phase 3: per-particle constants.  With work lists the same pass zeroes the stage's scratch (partial sums are added atomically);
// k_rays_skip only wants the constants, and an update's resampling kernel has usually left them in d_pc already.
void ray_prep(mcl_engine *h, const RayPlan &p, const mcl::RayArgs &a)
{
    const dim3 grid((unsigned)((a.n + 255) / 256));
    if (!p.lists) {
        if (p.mode == MCL_RAYS_SKIP && !p.constants_ready)
            hipLaunchKernelGGL(mcl::k_particle_prep, grid, dim3(256), 0, h->stream, a.x, a.y, a.th, a.n, h->ox, h->oy, h->res, h->d_pc, h->d_angle, h->B,
                               (short4 *)nullptr, mcl::PrepClear{});
        return;
    }
    mcl::PrepClear clr{};
    clr.logw_acc = h->d_logw_acc; clr.far_flags = reinterpret_cast<uint32_t *>(h->d_far.p);
    clr.fix_count = h->d_fix_count; clr.fix_words = p.nseg * 8; clr.fix_over = h->d_fix_over; clr.exact_count = h->d_result + 14;
    if (p.sweep) clr.far_count = h->d_result + 15;
    if (p.ordered && !p.stale_layout) clr.bbox = h->d_bbox;          // (the histogram is left all-zero by k_hist_clear of the previous sort)
    clr.bbox_play = unit_play(h, p.mode, p.hyb);
    if (p.ordered && p.constants_ready) {          // the resampling kernel left the constants and zeroed the per-particle scratch
        clr.logw_acc = nullptr; clr.far_flags = nullptr;
        // ... and, from the second update of a configuration on, the few words that are not per particle as well
        const mcl::PrepClear &pc0 = p.clear_passed;
        const bool done = p.clear_folded && clr.fix_count == pc0.fix_count && clr.fix_words == pc0.fix_words &&
                          clr.fix_over == pc0.fix_over && clr.exact_count == pc0.exact_count && clr.far_count == pc0.far_count &&
                          clr.bbox == pc0.bbox && clr.bbox_play == pc0.bbox_play && !clr.hist && !pc0.hist;
        if (!done) hipLaunchKernelGGL(mcl::k_prep_small, dim3(1), dim3(256), 0, h->stream, clr);
        if (!h->capturing) { h->prep_cache = clr; h->prep_cache_valid = true; h->prep_cache_n = a.n; }
    } else {
        hipLaunchKernelGGL(mcl::k_particle_prep, grid, dim3(256), 0, h->stream, a.x, a.y, a.th, a.n, h->ox, h->oy, h->res, h->d_pc, h->d_angle, h->B,
                           p.ordered ? (short4 *)nullptr : h->d_qr, clr);
    }
}

// Phase 7 for MCL_RAYS_MARCH.  (Up here, and k_rays_skip's launch in ray_kernel below: the compiler lays a unit's kernels out in the
// order their instantiations are first named, and the names of this file keep the order they always had -- march, the library
// sort, the kernels with work lists, skip -- so that a change of the host code leaves the code object byte for byte as it was.)
void ray_kernel_march(mcl_engine *h, const RayPlan &p, const mcl::RayArgs &a)
{
    if (p.count) hipLaunchKernelGGL((mcl::k_rays_march<true>), dim3(p.grid), dim3(mcl::kRayThreads), 0, h->stream, a);
    else hipLaunchKernelGGL((mcl::k_rays_march<false>), dim3(p.grid), dim3(mcl::kRayThreads), 0, h->stream, a);
}

// Phase 4 (cell, sweep): order the particles by (tile, cell, heading): bounding box -> bucket histogram (the atomic's return
// value is the rank inside the bucket) -> exclusive scan -> scatter of pc / qr / index; or (sort_radix) a library sort of
// (key, index) pairs and a gather
int ray_order(mcl_engine *h, const RayPlan &p, const mcl::RayArgs &a)
{
    const int64_t n = a.n;
    const unsigned nb256 = (unsigned)((n + 255) / 256);
    const int nparts = (int)(mcl::kSortKeySpace / mcl::kHistTile);
    const int ntx_abs = sort_tiles(h).ntx_abs;
    if (!p.stale_layout) launch_layout(h, h->stream, n, h->d_bbox, h->d_tilemark, h->d_tilemap);
    if (!p.radix) {
        hipLaunchKernelGGL(mcl::k_sort_hist, dim3(nb256), dim3(256), 0, h->stream, h->d_pc, a.th, n, h->Wp, h->Hp, h->d_bbox, h->d_hist,
                           h->d_skey, h->d_srank, h->d_tile_used, h->d_tilemap, ntx_abs);
        hipLaunchKernelGGL(mcl::k_hist_partials, dim3(nparts), dim3(256), 0, h->stream, h->d_hist, h->d_histpart, h->d_tile_used);
        hipLaunchKernelGGL(mcl::k_hist_final, dim3(nparts), dim3(256), 0, h->stream, h->d_hist, h->d_histpart, h->d_tile_used);
        hipLaunchKernelGGL(mcl::k_sort_scatter, dim3(nb256), dim3(256), 0, h->stream, h->d_pc, a.th, n, h->d_skey, h->d_srank,
                           h->d_hist, h->d_pcs, h->d_ths, h->d_perm);
        return MCL_OK;
    }
    MCL_TRY(h->d_skey2.reserve(h, (size_t)h->cap));
    MCL_TRY(h->d_sval2.reserve(h, (size_t)h->cap));
    // (the keys carry sort_fine(h) bits below the coarse 22: they only order the particles inside a bucket, and every reader drops them)
    const int fine = sort_fine(h), key_bits = mcl::kSortKeyLog2 + mcl::sort_fine_bits(fine);
    size_t tb = 0;
    HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, h->d_skey.p, h->d_skey2.p, h->d_srank.p, h->d_sval2.p, (size_t)n, 0, key_bits, h->stream));
    MCL_TRY(h->d_sort_tmp.reserve(h, tb));
    if (!(p.stale_layout && p.keys_written))    // (else the resampling kernel wrote the pairs)
        hipLaunchKernelGGL(mcl::k_sort_keys, dim3(nb256), dim3(256), 0, h->stream, h->d_pc, a.th, n, h->Wp, h->Hp, h->d_bbox, h->d_skey, h->d_srank,
                           h->d_tilemap, ntx_abs, fine);
    tb = h->d_sort_tmp.cap;
    HIPCHK(h, rocprim::radix_sort_pairs(h->d_sort_tmp.p, tb, h->d_skey.p, h->d_skey2.p, h->d_srank.p, h->d_sval2.p, (size_t)n, 0, key_bits, h->stream));
    hipLaunchKernelGGL(mcl::k_sort_gather, dim3(nb256), dim3(256), 0, h->stream, h->d_pc, a.th, n, h->d_sval2, h->d_pcs, h->d_ths, h->d_perm,
                       p.sweep ? h->d_skey2 : (const uint32_t *)nullptr, h->d_bbox, h->d_cut_start, h->d_cut_end, fine, p.heading_form ? 1 : 0);
    h->order_last = {h->d_bbox.p, h->d_tilemap.p, n, fine, p.heading_form};   // (mcl_get_sort_order, mcl_get_sort_record_form)
    return MCL_OK;
}

// Phase 5 (cell, sweep): what the kernel works from in the sorted order -- k_rays_sweep the unit table and the units' sums,
// k_rays_cell the means of its slices
int ray_units(mcl_engine *h, const RayPlan &p, mcl::RayArgs &a)
{
    const int64_t n = a.n;
    const int nparts = (int)(mcl::kSortKeySpace / mcl::kHistTile);
    if (p.sweep) {
        // units of the sorted order (cut at tile borders when the set is ordered by whole tiles), from the bucket
        // offsets the scatter has just used -- before they are cleared
        const size_t mu = (size_t)max_sweep_units(n);
        MCL_TRY(h->d_unit_sums.reserve(h, mu * 2));
        MCL_TRY(h->d_unit_begin.reserve(h, mu + 1));
        MCL_TRY(h->d_nunits.reserve(h, 1));
        hipLaunchKernelGGL(mcl::k_unit_table, dim3(1), dim3(1024), 0, h->stream, h->d_bbox, n, h->d_hist, h->d_histpart, h->d_tile_used,
                           p.radix ? h->d_cut_start : (uint32_t *)nullptr, h->d_cut_end, h->d_unit_begin, h->d_nunits, (int)mu);
        // (... and, after a counting sort, the histogram's used tiles back to zero: k_hist_clear's work)
        hipLaunchKernelGGL(mcl::k_unit_sums, dim3((unsigned)std::min<int64_t>(max_sweep_units(n), (n + mcl::kSwUnit - 1) / mcl::kSwUnit + 256)), dim3(256), 0, h->stream, h->d_pcs, h->d_unit_begin, h->d_nunits,
                           h->d_unit_sums, p.radix ? (uint32_t *)nullptr : h->d_hist, h->d_tile_used, nparts);
    } else {
        if (!p.radix) hipLaunchKernelGGL(mcl::k_hist_clear, dim3(nparts), dim3(256), 0, h->stream, h->d_hist, h->d_tile_used);
        MCL_TRY(h->d_slice_mean.reserve(h, (size_t)p.nsl));
        hipLaunchKernelGGL(mcl::k_slice_means, dim3((unsigned)p.nsl), dim3(256), 0, h->stream, h->d_pcs, n, (n + p.nsl - 1) / p.nsl, h->d_slice_mean);
    }
    a.pcs = h->d_pcs; a.ths = h->d_ths; a.perm = h->d_perm; a.slice_mean = h->d_slice_mean;
    a.distw = h->d_distw; a.distw_stride = (size_t)h->Hp * h->Wps;
    return MCL_OK;
}

// Phase 6 (sweep): the table of this scan, the work items (k_sweep_plan) and the lists of the far pass
int ray_sweep_items(mcl_engine *h, const RayPlan &p, mcl::RayArgs &a)
{
    if (!h->d_Ltd) return fail(h, MCL_ERR_HIP, "k_rays_sweep: table not allocated (internal)");
    if (!h->ltd_ready) build_ltd(h);          // a caller whose table decision was made for another particle count
    MCL_TRY(launch_sweep_plan(h, a.n, p.nseg, p.sweep_g, p.hyb));
    a.sweep_g = p.sweep_g; a.Ltd = h->d_Ltd; a.ltd_cols = h->ltd_cols;
    a.split16 = h->env.sw_split16 >= 0 ? h->env.sw_split16 : 0;
    a.beam_csx = h->sweep_global ? h->d_beam_csxg : h->d_beam_csx; a.beam_pad = h->beam_pad; a.beam_margin = h->beam_margin;
    a.beam_csi = h->d_beam_csi; a.beam_err = h->d_beam_err; a.rec_k = 2.0 * h->rec_c;
    a.distg = h->d_distg; a.distg_stride = h->distg_stride; a.distg_pitch = h->distg_pitch;
    a.items = h->d_items; a.centres = h->d_centres; a.nitems = 0; a.nitems_ptr = h->d_nitems; a.unit_sums = h->d_unit_sums; a.unit_begin = h->d_unit_begin; a.slot_space = 1;
    MCL_TRY(h->d_far_list.reserve(h, (size_t)h->cap));
    MCL_TRY(h->d_far_sorted.reserve(h, (size_t)h->cap));
    MCL_TRY(h->d_far_cnt.reserve(h, (size_t)h->cap / mcl::kFarTile + 2));
    a.far_sorted = h->d_far_sorted;
    a.far_windowed = p.far_windowed ? 1 : 0;
    a.far_list = h->d_far_list; a.far_count = h->d_result + 15;      // word 15 of the result block, zeroed by phase 3
    return MCL_OK;
}

// Phases 7 and 8 with work lists: the ray kernel, then what it left undecided -- the particles its windows did not fit (windowed far
// pass, k_rays_far), the listed rays (k_rays_fix), the exact march (k_rays_exact).  Every form is named here once; COUNT
// (debug_count_probes) is the caller's template argument.  k_rays_sweep's stop event is EV_K1 (its duration, dispatch included, at no
// cost; EV_K0 is k_sweep_plan's); the legacy kernels are bracketed by records.
template <bool COUNT>
int ray_kernel_lists(mcl_engine *h, const RayPlan &p, const mcl::RayArgs &a)
{
    const dim3 qg((unsigned)p.nseg), b(mcl::kRayThreads);   // persistent: 2 workgroups per CU
    if (!p.sweep) HIPCHK(h, hipEventRecord(h->ev[EV_K0], h->stream));
    if (p.hyb) hipExtLaunchKernelGGL((mcl::k_rays_sweep<COUNT, false, true, false, true>), qg, b, p.qlds, h->stream, nullptr, h->ev[EV_K1], 0, a);
    else if (p.glob && p.rec) hipExtLaunchKernelGGL((mcl::k_rays_sweep<COUNT, true, true, true>), qg, b, p.qlds, h->stream, nullptr, h->ev[EV_K1], 0, a);
    else if (p.glob) hipExtLaunchKernelGGL((mcl::k_rays_sweep<COUNT, true>), qg, b, p.qlds, h->stream, nullptr, h->ev[EV_K1], 0, a);
    else if (p.sweep && p.rec && p.pairs) hipExtLaunchKernelGGL((mcl::k_rays_sweep<COUNT, false, true, true>), qg, b, p.qlds, h->stream, nullptr, h->ev[EV_K1], 0, a);
    else if (p.sweep && p.rec) hipExtLaunchKernelGGL((mcl::k_rays_sweep<COUNT, false, true>), qg, b, p.qlds, h->stream, nullptr, h->ev[EV_K1], 0, a);
    else if (p.sweep) hipExtLaunchKernelGGL((mcl::k_rays_sweep<COUNT>), qg, b, p.qlds, h->stream, nullptr, h->ev[EV_K1], 0, a);
#ifdef MCL_LEGACY_RAY_KERNELS
    else if (p.ordered) hipLaunchKernelGGL((mcl::k_rays_cell<COUNT>), qg, b, p.qlds, h->stream, a);
    else hipLaunchKernelGGL((mcl::k_rays_quad<COUNT>), qg, b, p.qlds, h->stream, a);
#endif
    if (!p.sweep) HIPCHK(h, hipEventRecord(h->ev[EV_K1], h->stream));
    if (p.sweep && p.far_windowed) MCL_TRY(launch_far_windowed(h, a, a.n, COUNT));
    hipLaunchKernelGGL((mcl::k_rays_far<COUNT>), dim3(p.gfar), b, 0, h->stream, a);
    hipLaunchKernelGGL((mcl::k_rays_fix<COUNT>), dim3((unsigned)p.fix_grid), dim3(256), 0, h->stream, a, p.fix_flat ? 1 : 0);
    hipLaunchKernelGGL((mcl::k_rays_exact<COUNT>), dim3(2 * h->num_cu), dim3(256), 0, h->stream, a);
    return MCL_OK;
}
// (instantiated here, not at the end of the unit: mcl_create's layout checks name the forms of k_rays_sweep too, and the first naming places a kernel)
template int ray_kernel_lists<true>(mcl_engine *, const RayPlan &, const mcl::RayArgs &);
template int ray_kernel_lists<false>(mcl_engine *, const RayPlan &, const mcl::RayArgs &);

// Phase 7 (and 8): the ray kernel of the plan's mode; without work lists one launch, timed by records unless it is part of a captured tail
int ray_kernel(mcl_engine *h, const RayPlan &p, const mcl::RayArgs &a)
{
    if (p.lists) return p.count ? ray_kernel_lists<true>(h, p, a) : ray_kernel_lists<false>(h, p, a);
    const dim3 g(p.grid), b(mcl::kRayThreads);
    if (p.timed) HIPCHK(h, hipEventRecord(h->ev[EV_K0], h->stream));
    if (p.mode == MCL_RAYS_MARCH) ray_kernel_march(h, p, a);
    else if (p.mode == MCL_RAYS_DESKEW) { mcl::RayArgs d = a; ray_kernel_deskew(h, p, d); }
    else if (p.count) hipLaunchKernelGGL((mcl::k_rays_skip<1, true>), g, b, p.lds, h->stream, a);
    else {
        switch (p.R) {
        case 1: hipLaunchKernelGGL((mcl::k_rays_skip<1, false>), g, b, p.lds, h->stream, a); break;
        case 2: hipLaunchKernelGGL((mcl::k_rays_skip<2, false>), g, b, p.lds, h->stream, a); break;
        case 3: hipLaunchKernelGGL((mcl::k_rays_skip<3, false>), g, b, p.lds, h->stream, a); break;
        default: hipLaunchKernelGGL((mcl::k_rays_skip<4, false>), g, b, p.lds, h->stream, a); break;
        }
    }
    if (p.timed) HIPCHK(h, hipEventRecord(h->ev[EV_K1], h->stream));
    return MCL_OK;
}

// Phase 9 (work lists): the accumulators -> d_logw in particle order, and the overflow flag of the fix-up lists
void ray_combine(mcl_engine *h, const RayPlan &p, int64_t n)
{
    if (p.sweep) {
        // the slot accumulators (k_rays_sweep's per-wedge sums + what the far / fix / exact kernels added) -> d_logw in particle
        // order, the per-workgroup maxima, and the overflow flag of the fix-up lists (k_fix_overflow's job for the other kernels)
        hipExtLaunchKernelGGL(mcl::k_combine_logw, dim3(mcl::kRedBlocks), dim3(256), 0, h->stream, nullptr, h->ev[EV_RAYS], 0, n, h->d_perm.p, h->d_logw_acc.p,
                              h->d_logw.p, h->d_maxpart.p, h->d_fix_count.p, p.nseg, p.segcap, h->d_fix_over);
        h->stage_ev.rays_bound = true;         // (the stage's last kernel: EV_RAYS is its stop event)
        h->max_partials_ready = true;
    } else {
        hipLaunchKernelGGL(mcl::k_fix_overflow, dim3(1), dim3(256), 0, h->stream, h->d_fix_count, p.nseg, p.segcap, h->d_fix_over);
        hipLaunchKernelGGL(mcl::k_gather_logw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_logw_acc, n, h->d_logw);
    }
}

// Phase 10 (MCL_DEBUG_WG): four words per persistent workgroup, cleared before the ray kernel and written to the named file after the stage
int ray_debug_begin(mcl_engine *h, const RayPlan &p, mcl::RayArgs &a, DevBuf<unsigned long long> &d_dbg)
{
    if (h->env.debug_wg.empty()) return MCL_OK;
    MCL_TRY(d_dbg.reserve(h, (size_t)p.nseg * 4));
    HIPCHK(h, hipMemset(d_dbg, 0, (size_t)p.nseg * 32));
    a.dbg = d_dbg;
    return MCL_OK;
}

int ray_debug_dump(mcl_engine *h, const RayPlan &p, DevBuf<unsigned long long> &d_dbg)
{
    if (!d_dbg) return MCL_OK;
    std::vector<unsigned long long> hd((size_t)p.nseg * 4);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(hd.data(), d_dbg, hd.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *f = fopen(h->env.debug_wg.c_str(), "wb")) { fwrite(hd.data(), 8, hd.size(), f); fclose(f); }
    return MCL_OK;
}

// Nothing is prepared for a ray stage any more: the one way the hand-off is voided (graph_reset, the top of an update and of a staged
// resample, a staged ray stage with no resample before it) and consumed (launch_rays; tail_graph for the launches its graph replays).
// A wait owed on ev_obs stays owed until it is issued: it orders the streams, and graph_reset can run inside launch_rays before it.
void ray_handoff_void(mcl_engine *h)
{
    const bool owed = h->handoff.obs_wait;
    h->handoff = {};
    h->handoff.obs_wait = owed;
}

// The ray stage of n particles: log-weights into d_logw.  force_skip: the redo after a fix-up list overflow (fix_lists_overflowed).
// Consumes the hand-off of the resampling launch where it ends well (an early error return leaves it standing, as it leaves the stage
// unrun); recorded into a graph it consumes nothing: every replay finds the constants in d_pc, and tail_graph consumes them.
int launch_rays(mcl_engine *h, const double *x, const double *y, const double *th, int64_t n, bool force_skip = false, bool direct_table = false)
{
    MCL_TRY(sensor_poses(h, x, y, th, n));      // (a mount: k_mount_poses in front of the stage's first kernel, and the stage reads its output)
    mcl::RayArgs a = ray_args(h, x, y, th, n, direct_table);
    MCL_TRY(ray_step_buffer(h, a));
    h->last_work_lists = false;
    h->last_lf = false;
    h->max_partials_ready = false;
    const RayPlan p = plan_rays(h, n, force_skip, direct_table);
    if (p.mode == 0) {
        // (the sentence mcl_get_planned_ray_kernel gives for the same configuration: an error that says what to change)
        const char *why = "";
        choose_ray_mode(h, n, force_skip, &why);
        return fail(h, MCL_ERR_UNSUPPORTED, std::string("MCL_RAYS_QUAD / MCL_RAYS_CELL / MCL_RAYS_SWEEP not usable with this map / beam set: ") + why);
    }
    DevBuf<unsigned long long> d_dbg;
    if (p.lists) MCL_TRY(ray_fix_lists(h, p, a));
    ray_prep(h, p, a);
    h->order_last = {};                     // (ray_order's radix path sets it)
    if (p.ordered) { MCL_TRY(ray_order(h, p, a)); MCL_TRY(ray_units(h, p, a)); }
    // the tables of this update's scan were built on the second stream beside the resampling and the ordering: from here on they are read
    if (p.obs_wait) { h->handoff.obs_wait = false; HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_obs, 0)); }
    if (p.sweep) MCL_TRY(ray_sweep_items(h, p, a));
    // What a decision leaves behind is written once per launch: the hybrid's back-off by plan_rays, before anything is launched;
    // far_fresh and last_sweep_* here, behind every reservation that can still fail and before the debug buffer's (as they always were).
    if (p.sweep) h->far_fresh = false;
    if (p.lists) { h->last_sweep_global = p.glob ? 1 : (p.hyb ? 2 : 0); h->last_sweep_rec = p.rec ? 1 : 0; h->last_sweep_pairs = (p.rec && (p.glob || p.pairs)) ? 1 : 0; }
    if (p.lists) MCL_TRY(ray_debug_begin(h, p, a, d_dbg));
    MCL_TRY(ray_kernel(h, p, a));
    if (p.lists) {
        ray_combine(h, p, n);
        MCL_TRY(ray_debug_dump(h, p, d_dbg));
        h->last_work_lists = true;
    }
    h->last_mode = p.mode;
    if (!h->capturing) ray_handoff_void(h);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

// obs -> obs_idx upload + per-update transposed log table
void stage_observation(mcl_engine *h, const float *obs, int stride)
{
    h->ltd_ready = false;
    for (int j = 0; j < h->B; ++j) h->h_obs[j] = obs[(size_t)j * stride];   // cpp:316-320 when stride = ANGLE_STEP
}

// k_rays_sweep's fp64 table of the observation whose table rows are in d_obs_idx
void build_ltd(mcl_engine *h)
{
    dim3 gd((h->ltd_cols + 255) / 256, mcl::sweep_table_rows(h->P));
    hipLaunchKernelGGL(mcl::k_build_ltd, gd, dim3(256), 0, h->stream, h->d_L, h->d_obs_idx, h->B, h->ltd_cols, h->P, h->beam_margin, h->d_Ltd);
    h->ltd_ready = true;
}

// the pinned staging buffer -> obs_idx + per-update transposed log table
int upload_observation(mcl_engine *h)
{
    HIPCHK(h, hipMemcpyAsync(h->d_obs, h->h_obs, (size_t)h->B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (!h->capturing) MCL_TRY(ensure_lt(h));               // no allocation while a graph is being captured (sizes are warm)
    dim3 g((h->bpad + 255) / 256, h->P + 1);
    hipLaunchKernelGGL(mcl::k_obs_build_lt, g, dim3(256), 0, h->stream, h->d_obs, h->res, h->P, h->d_L, h->B, h->bpad, h->d_obs_idx, h->d_Lt,
                       h->d_Lt + (size_t)(h->P + 1) * h->bpad);
    if (mode_sweep(choose_ray_mode(h, h->N, false))) build_ltd(h);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

int prepare_observation(mcl_engine *h, const float *obs, int stride)
{
    stage_observation(h, obs, stride);
    return upload_observation(h);
}

int sensor_and_weights(mcl_engine *h, const double *d_global_max, bool defer_sums = false)
{
    // d_logw holds the log-weights of the current particle set
    if (h->cfg.weight_mode == MCL_WEIGHT_PRODUCT) {
        if (!h->cfg.keep_ray_steps) return fail(h, MCL_ERR_UNSUPPORTED, "weight_mode PRODUCT needs keep_ray_steps");
        int64_t n = h->N;
        hipLaunchKernelGGL(mcl::k_product_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->P > 255 ? (const uint8_t *)nullptr : h->d_steps,
                           h->P > 255 ? reinterpret_cast<const uint16_t *>(h->d_steps.p) : (const uint16_t *)nullptr, h->d_obs_idx, n, h->B, h->d_table, h->P + 1, 1.0 / h->cfg.squash_factor, h->d_w);
        HIPCHK(h, hipGetLastError());
        return weight_stats(h, false, nullptr, defer_sums);
    }
    return weight_stats(h, true, d_global_max, defer_sums);
}

// weights, sums and the CDF of the current log-weights (the tail of an update).  Small updates take one launch.
// kld (a small update with KLD on, result_to_host): the tail also clears the words the resampling kernel marked
int weights_and_cdf(mcl_engine *h, bool result_to_host = false, const mcl::KldArgs *kld = nullptr, bool *bind_sensor = nullptr)
{
    const int64_t n = h->N;
    if (h->cfg.weight_mode == MCL_WEIGHT_LOG && h->cfg.resample_neff_permille == 0 && n <= mcl::kTinyTailMax) {
        // d_pc holds (cos, sin) of the current headings whenever a ray kernel other than the literal march ran on them
        const double4 *pc = mode_fills_pc(h->last_mode) && !h->last_lf && !h->last_mounted ? h->d_pc : nullptr;   // (a mounted stage leaves the SENSORS' headings there)
        if (kld && result_to_host)
            hipLaunchKernelGGL(mcl::k_tiny_tail<true>, dim3(1), dim3(1024), (size_t)n * sizeof(uint64_t), h->stream, h->d_logw, h->d_x[h->cur],
                               h->d_y[h->cur], h->d_th[h->cur], pc, n, h->d_w, h->d_q, h->d_cdf, h->d_scalars, h->h_result, ++h->result_seq, *kld);
        else
            hipLaunchKernelGGL(mcl::k_tiny_tail<false>, dim3(1), dim3(1024), (size_t)n * sizeof(uint64_t), h->stream, h->d_logw, h->d_x[h->cur],
                               h->d_y[h->cur], h->d_th[h->cur], pc, n, h->d_w, h->d_q, h->d_cdf, h->d_scalars,
                               result_to_host ? h->h_result : (unsigned long long *)nullptr, ++h->result_seq, mcl::KldArgs{});
        HIPCHK(h, hipGetLastError());
        h->max_partials_ready = false;
        h->carry_pending = false;
        h->blocktot_for = nullptr;             // no spine / leaders for this CDF: the resampling search bisects it directly
        h->compact_n = -1; h->compact_pending = false; h->guide_valid = h->guide_pending = false; h->list_epoch++;
        return MCL_OK;
    }
    MCL_TRY(sensor_and_weights(h, nullptr, true));             // (the sums are finished by the scan's spine)
    return scan_weights(h, h->d_q, h->d_cdf, n, 0, nullptr, bind_sensor);   // CDF for the next resample / visualize
}

// The scan of the engine's own weights as the last kernel of its stage -- behind the weights of an update's tail (all: weights_and_cdf),
// or alone behind the staged flow's -- with EV_SENSOR closed by its stop event where it can be bound, else by a record behind it.
int close_sensor_stage(mcl_engine *h, bool all)
{
    bool bound = false;
    MCL_TRY(all ? weights_and_cdf(h, false, nullptr, &bound) : scan_weights(h, h->d_q, h->d_cdf, h->N, 0, nullptr, &bound));
    if (!bound) HIPCHK(h, hipEventRecord(h->ev[EV_SENSOR], h->stream));
    return MCL_OK;
}

// Every mcl_stage_* entry point starts here: the staged (sharded) flow is refused while a single-engine feature is on (MCL_OK: none is)
int refuse_stage(mcl_engine *h)
{
    const char *on = !h ? nullptr : h->kld_on ? "KLD sampling (mcl_set_kld)" : h->recov_on ? "recovery (mcl_set_recovery)"
                   : h->lf_on ? "the likelihood field (mcl_set_likelihood_field)"
                   : h->ds_on ? "per-beam sensor offsets (mcl_set_beam_offsets; pass NULL to switch them off)" : nullptr;
    if (!on) return MCL_OK;
    return fail(h, MCL_ERR_UNSUPPORTED, std::string(on) + " is single-engine only: the mcl_stage_* calls are refused while it is on");
}

// the field and the table of the current map on the device (model on, map set, K checked by the caller)
int lf_build(mcl_engine *h)
{
    int K, reach;
    lf_reach_of(h, K, reach);
    lf_table(h->cfg, h->lf, h->res, K, h->lf_tab);
    h->lf_K = -1;                                                         // until both buffers hold this map's
    h->lf_epoch++;
    h->d_lf_D.drop(); h->d_lf_tab.drop();
    const size_t cells = (size_t)h->W * h->H;
    MCL_TRY(h->d_lf_D.reserve(h, cells));
    MCL_TRY(h->d_lf_tab.reserve(h, h->lf_tab.size()));
    DevBuf<uint16_t> d_g;
    MCL_TRY(d_g.reserve(h, cells));
    const dim3 grid((unsigned)((cells + 255) / 256));
    hipLaunchKernelGGL(mcl::k_lf_cols, grid, dim3(256), 0, h->stream, h->d_grid, h->W, h->H, reach, d_g.p);
    hipLaunchKernelGGL(mcl::k_lf_rows, grid, dim3(256), 0, h->stream, d_g.p, h->W, h->H, reach, K, h->d_lf_D);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->d_lf_tab, h->lf_tab.data(), h->lf_tab.size() * sizeof(float), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(h, MCL_ERR_HIP, std::string("building the likelihood field: ") + hipGetErrorString(e));
    h->lf_K = K;
    return MCL_OK;
}

// The sensor stage with beam skipping on, in k_lfield's place between the same events: the counting pass (BS1,
// BS2; it also leaves the full sums in d_logw), the plan (BS3, BS4, the state record) and the summing pass over the kept beams
// (BS5), with no host wait between them -- n and nb are known here, so min_count and min_skipped are.  d_bs_cnt is zeroed by the
// caller, in-stream.
int launch_lfield_skip(mcl_engine *h, const double *x, const double *y, const double *th, int64_t n, int nb)
{
    mcl::LfArgs a{};
    a.x = x; a.y = y; a.th = th; a.n = n;
    a.beams = h->d_lf_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.logw = h->d_logw;
    const int ka = mcl_host::bs_ka(&h->bs, (float)h->res);
    const int64_t min_count = mcl_host::bs_min_count(h->bs.threshold, n);
    const int min_skipped = mcl_host::bs_min_skipped(h->bs.error_threshold, nb);
    const bool lds_table = h->lf_K < mcl::kLfLdsEntries;
    const int tab_words = lds_table ? (h->lf_K + 1 + 3) & ~3 : 0;
    const bool lds_cnt = nb <= mcl::kBsLdsBeams && tab_words + nb <= mcl::kLfLdsEntries;
    mcl::BsCountArgs b{};
    b.cnt = h->d_bs_cnt; b.tiles = (n + 255) / 256; b.ka = (uint32_t)ka; b.cnt_off = tab_words;
    const size_t lds = (size_t)(tab_words + (lds_cnt ? nb : 0)) * sizeof(float);
    const dim3 grid1((unsigned)std::min<int64_t>(b.tiles, (int64_t)h->num_cu * mcl::kBsWorkgroupsPerCu)), grid((unsigned)b.tiles);
    if (lds_table && lds_cnt)
        hipLaunchKernelGGL((mcl::k_lfield_agree<true, true>), grid1, dim3(256), lds, h->stream, a, b);
    else if (lds_table)
        hipLaunchKernelGGL((mcl::k_lfield_agree<true, false>), grid1, dim3(256), lds, h->stream, a, b);
    else if (lds_cnt)
        hipLaunchKernelGGL((mcl::k_lfield_agree<false, true>), grid1, dim3(256), lds, h->stream, a, b);
    else
        hipLaunchKernelGGL((mcl::k_lfield_agree<false, false>), grid1, dim3(256), lds, h->stream, a, b);
    mcl::BsPlanArgs p{};
    p.cnt = h->d_bs_cnt; p.beams = h->d_lf_beams; p.nb = nb; p.n = n; p.min_count = min_count; p.min_skipped = min_skipped; p.ka = ka;
    p.kept = h->d_bs_kept; p.beams_kept = h->d_bs_beams; p.st = h->d_bs_state;
    hipLaunchKernelGGL(mcl::k_lf_skip_plan, dim3(1), dim3(256), 0, h->stream, p);
    a.beams = h->d_bs_beams;
    if (lds_table)
        hipLaunchKernelGGL(mcl::k_lfield_kept<true>, grid, dim3(256), (size_t)(h->lf_K + 1) * sizeof(float), h->stream, a, h->d_bs_state.p);
    else
        hipLaunchKernelGGL(mcl::k_lfield_kept<false>, grid, dim3(256), 0, h->stream, a, h->d_bs_state.p);
    HIPCHK(h, hipGetLastError());
    h->bs_B = h->B;
    h->bs_idx.resize((size_t)nb);
    h->bs_have = true;
    return MCL_OK;
}

// The sensor stage of a likelihood-field update: the used beams of the scan in beam order (LF3), one copy, k_lfield (LF4, LF5) --
// or, with beam skipping on, the zeroed counters and launch_lfield_skip's three kernels in its place.
// EV_QUERY / EV_K0 .. EV_K1 bracket the kernels (stage 3 and mcl_get_ray_kernel_ms).
int launch_lfield(mcl_engine *h, const float *obs, int stride, int64_t n)
{
    MCL_TRY(h->h_lf_beams.reserve(h, (size_t)h->B));
    MCL_TRY(h->d_lf_beams.reserve(h, (size_t)h->B));
    if (h->bs_on) { h->bs_have = false; h->bs_idx.resize((size_t)h->B); }
    const int nb = mcl_host::lf_used_beams(h, obs, stride, h->h_lf_beams, h->bs_on ? h->bs_idx.data() : nullptr, h->ds_on);   // (DS5: the update path alone)
    if (nb > 0)
        HIPCHK(h, hipMemcpyAsync(h->d_lf_beams, h->h_lf_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    if (h->bs_on) {
        MCL_TRY(h->d_bs_cnt.reserve(h, (size_t)h->B));
        MCL_TRY(h->d_bs_kept.reserve(h, (size_t)h->B));
        MCL_TRY(h->d_bs_beams.reserve(h, (size_t)h->B));
        MCL_TRY(h->d_bs_state.reserve(h, 1));
        if (nb > 0) HIPCHK(h, hipMemsetAsync(h->d_bs_cnt, 0, (size_t)nb * sizeof(unsigned int), h->stream));
    }
    HIPCHK(h, hipEventRecord(h->ev[EV_QUERY], h->stream));
    const double *x = h->d_x[h->cur], *y = h->d_y[h->cur], *th = h->d_th[h->cur];
    MCL_TRY(sensor_poses(h, x, y, th, n));      // (a mount: the field is read at the sensors' poses)
    HIPCHK(h, hipEventRecord(h->ev[EV_K0], h->stream));
    const int rc = h->bs_on ? launch_lfield_skip(h, x, y, th, n, nb) : mcl_host::launch_lfield_on(h, x, y, th, n, h->d_lf_beams, nb, h->d_logw);
    if (rc != MCL_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[EV_K1], h->stream));
    h->max_partials_ready = false;
    h->last_work_lists = false;
    h->last_lf = true;
    return MCL_OK;
}

}  // namespace

// ---- engine functions the other units use too (mcl_engine_internal.h); the stage_* ones are further down, beside their entry points
int mcl_host::fail(mcl_engine *h, int code, const char *msg) { if (h) h->err = msg; return code; }
int mcl_host::fail(mcl_engine *h, int code, const std::string &msg) { return fail(h, code, msg.c_str()); }

std::string &mcl_host::create_error() { return g_create_error; }      // what mcl_*_last_error(NULL) reports

// ---- KLD-adaptive particle count (mcl_set_kld)
// the bitmap, the list and the two counters for the current map (allocated on the first need, grown, zeroed)
int mcl_host::kld_alloc(mcl_engine *h)
{
    if (!h->kld_on || !h->have_map) return MCL_OK;
    const size_t words = (size_t)((h->kld_bits + 31) / 32);
    const size_t list = (size_t)std::min<uint64_t>((uint64_t)h->cap, h->kld_bits);
    MCL_TRY(h->d_kld_bm.reserve(h, words));
    MCL_TRY(h->d_kld_list.reserve(h, list));
    MCL_TRY(h->d_kld_cnt.reserve(h, 2));
    HIPCHK(h, hipMemsetAsync(h->d_kld_bm, 0, words * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_kld_cnt, 0, 2 * sizeof(unsigned int), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->kld_parity = 0;
    return MCL_OK;
}

SortTiles mcl_host::sort_tiles(const mcl_engine *h)
{
    const int ntx_abs = ((h->Wp * mcl::kSortSub - 1) >> 5) + 1, nty_abs = ((h->Hp * mcl::kSortSub - 1) >> 5) + 1;
    return {ntx_abs, nty_abs, (int64_t)ntx_abs * nty_abs <= mcl::kSortMaxTiles};
}

bool mcl_host::ready(mcl_engine *h, bool need_particles)
{
    return h && h->have_map && h->B > 0 && (!need_particles || h->have_particles);
}

float mcl_host::elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms;
}

void mcl_host::graph_reset(mcl_engine *h)
{
    for (int k = 0; k < 2; ++k)
        if (h->graph_exec[k]) { (void)hipGraphExecDestroy(h->graph_exec[k]); h->graph_exec[k] = nullptr; }
    h->graph_warm = false;
    h->prep_cache_valid = false;
    h->layout.valid = false;
    h->order_last = {};
    ray_handoff_void(h);                    // whatever changed (map, beams, particles, a buffer): the ray stage makes its own constants
}

// mcl_update is not refused on an engine with a communicator or in a group, so such an engine can hold a captured graph too: a spine
// that moves drops the graphs for every caller.  The stream is idle before its memory goes.
int mcl_host::reserve_scan_spine(mcl_engine *h, int64_t n)
{
    const size_t need = (size_t)n / mcl::kScanTile + 2;
    if (need <= h->d_blocktot.cap) return MCL_OK;
    graph_reset(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return h->d_blocktot.reserve(h, need);
}

int mcl_host::scan_weights(mcl_engine *h, const uint64_t *d_q, uint64_t *d_cdf, int64_t n, uint64_t offset, uint64_t *d_total, bool *bind_sensor)
{
    int nb = (int)((n + mcl::kScanTile - 1) / mcl::kScanTile);
    // the scan of the engine's own weights also leaves the compact list of the particles that carry weight
    mcl::CompactOut co{};
    const bool own = d_q == h->d_q && d_cdf == h->d_cdf && offset == 0 && !h->env.no_compact && h->d_ccdf;
    if (own) {
        co.block_cnt = h->d_blockcnt; co.ccdf = h->d_ccdf; co.cidx = h->d_cidx; co.crec = h->d_crec; co.ctop = h->d_ctop;
        co.x = h->d_x[h->cur]; co.y = h->d_y[h->cur]; co.th = h->d_th[h->cur];
        co.cap = (uint32_t)h->compact_cap; co.total = h->d_result + 16;
        // the guide, while this engine can draw through it: a single engine (a sharded set searches the merged lists) without KLD sizing.
        // The spine leaves the grand total in its own word of the result block (besides the caller's d_total, if any): k_scan_final,
        // the resampling kernel and mcl_get_compact_guide all take the shift from that one word.
        if (h->d_cguide && !h->kld_on && !h->comm && !h->in_group) {
            co.guide = h->d_cguide; co.q_total = reinterpret_cast<const uint64_t *>(h->d_result.p + kResultGuideTotal); co.guide_m = h->guide_m;
        }
    }
    hipLaunchKernelGGL(mcl::k_scan_partials, dim3(nb), dim3(mcl::kScanThreads), 0, h->stream, d_q, n, h->d_blocktot, co.block_cnt);
    // (the spine is one workgroup that runs right after k_weights: it also finishes that kernel's partial sums, when asked)
    const bool fold = h->sums_pending && d_q == h->d_q;
    hipLaunchKernelGGL(mcl::k_scan_spine, dim3(1), dim3(1024), 0, h->stream, h->d_blocktot, nb, offset, d_total, co.block_cnt, co.total,
                       fold ? h->d_part : (const double *)nullptr, mcl::kRedBlocks, h->d_scalars, const_cast<uint64_t *>(co.q_total));
    if (fold) h->sums_pending = false;
    const size_t nlead = (size_t)((n + 15) >> mcl::kLeaderShift) + 1;
    if (nlead > h->d_leaders.cap) {
        graph_reset(h);                    // a captured update graph holds the old pointer
        MCL_TRY(h->d_leaders.reserve(h, nlead));
    }
    if (bind_sensor && own && !h->capturing) {          // the stage's last kernel: EV_SENSOR is its stop event, and the caller is told
        hipExtLaunchKernelGGL(mcl::k_scan_final, dim3(nb), dim3(mcl::kScanThreads), 0, h->stream, nullptr, h->ev[EV_SENSOR], 0, d_q, n, h->d_blocktot.p, d_cdf,
                              h->d_leaders.p, co);
        *bind_sensor = true;
    } else {
        hipLaunchKernelGGL(mcl::k_scan_final, dim3(nb), dim3(mcl::kScanThreads), 0, h->stream, d_q, n, h->d_blocktot, d_cdf, h->d_leaders, co);
    }
    HIPCHK(h, hipGetLastError());
    h->blocktot_for = d_cdf; h->blocktot_n = n;
    if (d_cdf == h->d_cdf) { h->compact_n = -1; h->compact_pending = own; h->guide_valid = false; h->guide_pending = co.guide != nullptr; h->list_epoch++; }
    return MCL_OK;
}

void mcl_host::unpack_result(mcl_engine *h)
{
    std::memcpy(h->h_scalars, h->h_result, 8 * sizeof(double));
    std::memcpy(h->h_counters, h->h_result + 8, 4 * sizeof(unsigned long long));
    h->h_fix_count = h->h_result[12];
    uint64_t qt;
    std::memcpy(&qt, &h->h_scalars[2], 8);
    h->q_total = qt;
    h->global_sums[0] = h->h_scalars[1];
    h->global_sums[1] = h->h_scalars[3];
    h->global_sums[2] = h->h_scalars[4];
    h->global_sums[3] = h->h_scalars[5];
    h->global_sums[4] = h->h_scalars[6];
    // length of the compact list the scan of this update's weights wrote (word 16); unusable when it outgrew its arrays
    if (h->compact_pending) {
        const unsigned long long na = h->h_result[16];
        h->compact_n = na <= (unsigned long long)h->compact_cap ? (int64_t)na : -1;       // 0: a valid, empty list (no weight here)
        h->compact_pending = false;
        h->guide_valid = h->guide_pending && h->compact_n > 0;
        h->guide_pending = false;
    }
}

int mcl_abi_version(void) { return MCL_ABI_VERSION; }

const char *mcl_last_error(const mcl_engine_t *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// The tuning knobs of the environment, read once per engine (never on the update path)
static EnvKnobs read_knobs()
{
    EnvKnobs k;
    if (const char *e = getenv("MCL_CELL_MIN")) k.cell_min = atoll(e);
    if (const char *e = getenv("MCL_CELL_SLICE")) k.cell_slice = atoll(e);
    if (const char *e = getenv("MCL_QSLICES_PER_CU")) k.qslices_per_cu = atoi(e);
    if (const char *e = getenv("MCL_QSIDE")) k.qside = atoi(e);
    if (const char *e = getenv("MCL_SWEEP_G")) k.sweep_g = atoi(e);
    if (const char *e = getenv("MCL_TINY_POLL")) k.tiny_poll = atoi(e);
    if (const char *e = getenv("MCL_NO_COMPACT")) k.no_compact = atoi(e);
    if (const char *e = getenv("MCL_SORT")) k.sort_radix = std::strcmp(e, "radix") == 0 ? 1 : (std::strcmp(e, "hist") == 0 ? 0 : -1);
    if (const char *e = getenv("MCL_SORT_FINE")) k.sort_fine = atoi(e);
    if (const char *e = getenv("MCL_SORT_FINE_SUB")) k.sort_fine_sub = atoi(e);
    if (const char *e = getenv("MCL_FIX_WG")) k.fix_wg = atoi(e);
    if (const char *e = getenv("MCL_FIX_DEAL")) k.fix_deal_seg = std::strcmp(e, "seg") == 0;
    if (const char *e = getenv("MCL_RESAMPLE_GUIDE")) k.resample_guide = atoi(e);
    if (const char *e = getenv("MCL_RESAMPLE_GUIDE_M")) k.guide_m = atoi(e);
    if (const char *e = getenv("MCL_DEBUG_WG")) k.debug_wg = e;
    k.no_bucket_cuts = getenv("MCL_NO_BUCKET_CUTS") != nullptr;
    if (const char *e = getenv("MCL_SWEEP_GLOBAL")) k.sweep_global = atoi(e) != 0;
    if (const char *e = getenv("MCL_SWEEP_HYBRID")) k.sweep_hybrid = atoi(e);
    if (const char *e = getenv("MCL_SW_GUIDE")) k.sw_guide = atoi(e);
    if (const char *e = getenv("MCL_SW_SPLIT16")) k.sw_split16 = atoi(e) != 0;
    if (const char *e = getenv("MCL_SWEEP_PAIRS")) k.sweep_pairs = atoi(e) != 0 ? 1 : 0;
    k.no_obs_overlap = getenv("MCL_NO_OBS_OVERLAP") != nullptr;
    k.no_prep_fold = getenv("MCL_NO_PREP_FOLD") != nullptr;
    k.no_stale_layout = getenv("MCL_NO_STALE_LAYOUT") != nullptr;
    k.comm_no_pregather = getenv("MCL_COMM_NO_PREGATHER") != nullptr;
    k.comm_no_lists = getenv("MCL_COMM_NO_LISTS") != nullptr;
    return k;
}

int mcl_create(const mcl_config_t *cfg, mcl_engine_t **out)
{
    if (cfg && (cfg->resample_neff_permille < 0 || cfg->resample_neff_permille > 1000)) return MCL_ERR_INVALID_ARG;
    g_create_error.clear();
    if (!cfg || !out) { g_create_error = "null argument"; return MCL_ERR_INVALID_ARG; }
    *out = nullptr;
    // weights are quantised to 2^-36 and summed in uint64 (E5/E6): N * 2^36 must stay below 2^64 with a bit to spare
    if (cfg->max_particles <= 0 || cfg->max_particles >= MCL_MAX_TOTAL_PARTICLES || cfg->squash_factor <= 0 || cfg->max_range_m <= 0) {
        g_create_error = "bad config (max_particles must be in [1, 2^27) / squash_factor / max_range_m)";
        return MCL_ERR_INVALID_ARG;
    }
    if (!std::isfinite(cfg->squash_factor) || !std::isfinite(cfg->max_range_m)) {
        g_create_error = "bad config (squash_factor and max_range_m must be finite)";
        return MCL_ERR_INVALID_ARG;
    }
    if (const char *why = bad_sensor_fields(*cfg)) { g_create_error = why; return MCL_ERR_INVALID_ARG; }
    {
        const double disp[3] = {cfg->motion_dispersion_x, cfg->motion_dispersion_y, cfg->motion_dispersion_theta};
        for (double v : disp)
            if (!std::isfinite(v) || v < 0.0) {
                g_create_error = "bad config (motion_dispersion_x/y/theta must be finite and >= 0)";
                return MCL_ERR_INVALID_ARG;
            }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        g_create_error = "no HIP device (this engine has no CPU path)";
        return MCL_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipSetDevice(cfg->device) != hipSuccess || hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) {
        g_create_error = "hipSetDevice/hipGetDeviceProperties failed";
        return MCL_ERR_NO_DEVICE;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName + ", engine is built for gfx950 only";
        return MCL_ERR_NO_DEVICE;
    }
    mcl_engine *h = new mcl_engine();
    h->cfg = *cfg;
    h->env = read_knobs();
    h->num_cu = prop.multiProcessorCount;
    h->cap = cfg->max_particles;
    auto bail = [&](const char *what) {
        g_create_error = std::string(what) + ": " + h->err;
        mcl_destroy(h);
        return MCL_ERR_HIP;
    };
#define CRT(call)                                                         \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) { h->err = hipGetErrorString(e_); return bail(#call); } \
    } while (0)
    CRT(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CRT(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    CRT(hipEventCreateWithFlags(&h->ev_obs, hipEventDisableTiming));
    for (int i = 0; i < EV_COUNT; ++i) CRT(hipEventCreate(&h->ev[i]));
#define CRB(buf, n) do { if ((buf).reserve(h, (n))) return bail(#buf); } while (0)
    const size_t cap = (size_t)h->cap;
    for (int b = 0; b < 2; ++b) {
        CRB(h->d_x[b], cap); CRB(h->d_y[b], cap); CRB(h->d_th[b], cap);
        CRB(h->d_pack[b], cap);
    }
    CRB(h->d_w, cap); CRB(h->d_logw, cap); CRB(h->d_tmp, cap * 3);
    CRB(h->d_logw_acc, cap);
    CRB(h->d_carry[0], cap); CRB(h->d_carry[1], cap);
    CRB(h->d_q, cap); CRB(h->d_cdf, cap);
    CRB(h->d_blocktot, cap / mcl::kScanTile + 2);
    CRB(h->d_blockcnt, cap / mcl::kScanTile + 2);
    h->compact_cap = std::max<int64_t>(4096, ((h->cap / 4 + 63) / 64) * 64);
    CRB(h->d_ccdf, (size_t)h->compact_cap);
    CRB(h->d_ctop, (size_t)h->compact_cap / 64 + 1);
    CRB(h->d_cidx, (size_t)h->compact_cap);
    CRB(h->d_crec, (size_t)h->compact_cap);
    if (h->env.resample_guide && h->cfg.resample_mode == MCL_RESAMPLE_MULTINOMIAL) {     // (the systematic comb never reads one)
        h->guide_m = h->env.guide_m > 0 ? std::min(std::max(h->env.guide_m, mcl::kGuideLog2Min), mcl::kGuideLog2Max) : mcl::kGuideLog2Default;
        CRB(h->d_cguide, mcl::guide_words(h->guide_m));
        CRT(hipMemset(h->d_cguide, 0, mcl::guide_words(h->guide_m) * sizeof(uint32_t)));  // (the word behind the last boundary is fetched, never written, never used)
    }
    CRB(h->d_idx, cap);
    CRB(h->d_part, (size_t)mcl::kRedBlocks * 8);
    CRB(h->d_maxpart, (size_t)mcl::kRedBlocks);
    CRB(h->d_result, kResultAlloc);
    CRT(hipMemset(h->d_result, 0, kResultAlloc * 8));
    CRB(h->h_result, 48);
    std::memset(h->h_result, 0, 48 * 8);
    h->d_scalars = reinterpret_cast<double *>(h->d_result.p);
    h->d_counters = h->d_result + 8;
    h->d_fix_over = h->d_result + 12;
    CRB(h->d_exact_list, (size_t)kExactCap);
    CRB(h->d_inject, cap * 4);
    CRB(h->d_pc, cap);
    CRB(h->d_qr, cap);
    CRB(h->d_far, cap * 4);
    CRB(h->d_pcs, cap);
    CRB(h->d_ths, cap);
    CRB(h->d_perm, cap);
    CRB(h->d_skey, cap);
    CRB(h->d_srank, cap);
    CRB(h->d_hist, (size_t)mcl::kSortBuckets);
    CRB(h->d_histpart, (size_t)(mcl::kSortKeySpace / mcl::kHistTile));
    CRB(h->d_tile_used, (size_t)(mcl::kSortKeySpace / mcl::kHistTile));
    CRT(hipMemset(h->d_hist, 0, (size_t)mcl::kSortBuckets * 4));          // kept all-zero between sorts (k_hist_clear)
    CRT(hipMemset(h->d_tile_used, 0, (size_t)(mcl::kSortKeySpace / mcl::kHistTile) * 4));
    CRB(h->d_bbox, 8);
    CRB(h->layout.d_bbox_nx, 8);
    CRB(h->layout.d_tilemap_nx, (size_t)mcl::kSortMaxTiles);
    CRB(h->layout.d_tilemark_nx, (size_t)mcl::kSortMaxTiles);
    CRT(hipMemset(h->layout.d_tilemark_nx, 0, (size_t)mcl::kSortMaxTiles * sizeof(int)));
    CRT(hipEventCreateWithFlags(&h->layout.ev_children, hipEventDisableTiming));
    CRT(hipEventCreateWithFlags(&h->layout.ev_layout, hipEventDisableTiming));
    CRT(hipEventCreateWithFlags(&h->ev_ext_in, hipEventDisableTiming));
    CRT(hipEventCreateWithFlags(&h->ev_ext_out, hipEventDisableTiming));
    CRB(h->d_cut_start, (size_t)mcl::kSwMaxCuts);
    CRB(h->d_cut_end, (size_t)mcl::kSwMaxCuts);
    CRT(hipMemset(h->d_cut_start, 0, (size_t)mcl::kSwMaxCuts * sizeof(uint32_t)));
    CRT(hipMemset(h->d_cut_end, 0, (size_t)mcl::kSwMaxCuts * sizeof(uint32_t)));
    CRB(h->d_tilemap, (size_t)mcl::kSortMaxTiles);
    CRB(h->d_tilemark, (size_t)mcl::kSortMaxTiles);
    CRT(hipMemset(h->d_tilemark, 0, (size_t)mcl::kSortMaxTiles * sizeof(int)));
    CRT(hipMemset(h->d_fix_over, 0, 16));
    CRT(hipMemset(h->d_scalars, 0, 8 * sizeof(double)));
    CRT(hipMemset(h->d_counters, 0, 4 * sizeof(unsigned long long)));
    CRT(hipDeviceSynchronize());        // the memsets above ran on the null stream; everything later uses h->stream
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<3, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_skip<4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
#ifdef MCL_LEGACY_RAY_KERNELS
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_quad<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_quad<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_cell<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_cell<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
#endif
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_tiny_tail<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_tiny_tail<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_sweep_plan), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024 - 64));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024 - 64));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024 - 64));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, false, true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024 - 64));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, false, true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024 - 64));
    CRT(hipFuncSetAttribute(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024 - 64));
    {   // The hand-written probe loops address their LDS window from a raw offset: k_rays_sweep / k_rays_cell / k_rays_quad
        // from kQLdsBase (their static LDS must end exactly there), k_rays_skip from 0 (it must have no static LDS).  A
        // toolchain that lays a kernel out differently takes that kernel out of choose_ray_mode's choices -- the engine then
        // runs the next one down, same results -- so that no configuration can reach a malformed launch.
        auto static_lds_is = [](const void *fn, size_t want) {
            hipFuncAttributes fa{};
            return hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.sharedSizeBytes == want;
        };
        const size_t qb = (size_t)mcl::kQLdsBase;
        h->sweep_layout_ok = static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false>), qb) && static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true>), qb);
        {
            // (the global form has one static word less: its dynamic LDS -- 16-byte aligned -- still starts at kQLdsBase)
            auto static_lds_fits = [](const void *fn, size_t lo, size_t hi) {
                hipFuncAttributes fa{};
                return hipFuncGetAttributes(&fa, fn) == hipSuccess && fa.sharedSizeBytes > lo && fa.sharedSizeBytes <= hi;
            };
            h->sweep_hyb_layout_ok = static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, false, true, false, true>), qb) &&
                                     static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, false, true, false, true>), qb);
            h->sweep_rec_layout_ok = static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, false, true>), qb) &&
                                     static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, false, true>), qb) &&
                                     static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, false, true, true>), qb) &&
                                     static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, false, true, true>), qb) &&
                                     static_lds_fits(reinterpret_cast<const void *>(&mcl::k_rays_sweep<false, true, true, true>), 0, qb) &&
                                     static_lds_fits(reinterpret_cast<const void *>(&mcl::k_rays_sweep<true, true, true, true>), 0, qb);
        }
#ifdef MCL_LEGACY_RAY_KERNELS
        h->cell_layout_ok = static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_cell<false>), qb) && static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_cell<true>), qb);
        h->quad_layout_ok = static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_quad<false>), qb) && static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_quad<true>), qb);
#endif
        h->skip_layout_ok = static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, false>), 0) && static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, true>), 0) &&
                            static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, false, true>), 0) && static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<1, true, true>), 0) &&
                            static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<2, false>), 0) && static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<3, false>), 0) &&
                            static_lds_is(reinterpret_cast<const void *>(&mcl::k_rays_skip<4, false>), 0);
        (void)hipGetLastError();
    }
#undef CRB
#undef CRT
    *out = h;
    return MCL_OK;
}

void mcl_destroy(mcl_engine_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);           // both, before anything is released
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    if (h->comm) { comm_free(h->comm); h->comm = nullptr; }
    if (h->clu) { cluster_free(h->clu); h->clu = nullptr; }
    if (h->qry) { query_free(h->qry); h->qry = nullptr; }
    if (h->srch) { search_free(h->srch); h->srch = nullptr; }
    if (h->rfn) { refine_free(h->rfn); h->rfn = nullptr; }
    graph_reset(h);
    for (int i = 0; i < EV_COUNT; ++i)
        if (h->ev[i]) (void)hipEventDestroy(h->ev[i]);
    if (h->ev_obs) (void)hipEventDestroy(h->ev_obs);
    if (h->layout.ev_children) (void)hipEventDestroy(h->layout.ev_children);
    if (h->layout.ev_layout) (void)hipEventDestroy(h->layout.ev_layout);
    if (h->ev_ext_in) (void)hipEventDestroy(h->ev_ext_in);
    if (h->ev_ext_out) (void)hipEventDestroy(h->ev_ext_out);
    if (h->stream2) (void)hipStreamDestroy(h->stream2);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;                            // (every buffer goes with it)
}

int mcl_set_map(mcl_engine_t *h, const int8_t *data, uint32_t width, uint32_t height, float resolution, double origin_x,
                double origin_y)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!data || width == 0 || height == 0 || width > 200000 || height > 200000) return fail(h, MCL_ERR_INVALID_ARG, "bad map dimensions");
    int64_t kld_nx = 0, kld_ny = 0;
    uint64_t kld_bits = 0;
    if (h->kld_on && resolution > 0.0f && !kld_grid(&h->kld, width, height, resolution, kld_nx, kld_ny, kld_bits))
        return fail(h, MCL_ERR_INVALID_ARG, "KLD: the bin grid over this map exceeds 2^31 bits");
    if (h->lf_on && resolution > 0.0f && lf_cap(&h->lf, resolution) < 0)
        return fail(h, MCL_ERR_INVALID_ARG, "likelihood field: K = ceil((max_occ_dist_m / resolution)^2) exceeds 65535 on this map");
    graph_reset(h);
    if (!(resolution > 0.0f)) return fail(h, MCL_ERR_INVALID_ARG, "invalid map resolution");   // cpp:236-240
    recov_unset(h);
    h->weighted = false;                    // (mcl_sensor_update_fuse: log-weights formed against the old map are not added to)
    h->mix_n = 0;                           // a proposal belongs to the map its scan was matched against
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const double res = (double)resolution;                    // cpp:191
    const int P = (int)(h->cfg.max_range_m / res);            // cpp:195
    // cpp:195 has no bound; the engine's tables are (P + 1)^2 doubles and its step indices 16 bits.  Up to 243 px the windowed
    // kernels apply, up to 281 px k_rays_skip's LDS window, beyond that k_rays_skip's global-field path (same results)
    if (P < 1 || P > 2047) return fail(h, MCL_ERR_UNSUPPORTED, "MAX_RANGE_PX must be in [1, 2047]");
    h->W = (int)width; h->H = (int)height; h->P = P;
    h->res = res; h->ox = origin_x; h->oy = origin_y;
    h->grid_host.assign(data, data + (size_t)width * height);      // (the global search forms its lattice from it)
    h->map_epoch++;
    h->Wp = h->W + 1; h->Hp = h->H + 1; h->Wps = (h->Wp + 7) & ~7;
    // LDS window: as large as 160 KiB allows (nibbles), multiple of 8 cells
    h->tw_cells = 568;
    // k_rays_quad: byte window of side S in half the LDS (S*S <= 80 KiB, S % 8 == 0); usable when the extent
    // budget S - (P+2) - 3 is at least 48 cells, otherwise k_rays_skip's full-LDS nibble window is used
    { const int S = h->env.qside > 0 ? h->env.qside : 280; h->qside = (S - (P + 2) - 3 >= 32) ? S : 0; }
    // k_rays_sweep: the 256-cell LDS windows hold ranges up to 243 px; beyond that (or with MCL_SWEEP_GLOBAL=1) the same walk
    // probes mirrored copies of the wedge fields in global memory, a position's cell dwords being absolute offsets there (no
    // bound on the range from the position format)
    h->sweep_global = h->env.sweep_global || !mcl::sweep_window_fits(P);
    h->distg_why_not = nullptr;
    const bool want_wedges = h->qside > 0 || h->sweep_global;     // wedge + quadrant fields (k_rays_far reads the latter)
    build_sensor_table(h->cfg, P, h->table);
    const int tw = P + 1;
    std::vector<float> L((size_t)tw * tw);
    const double inv_squash = 1.0 / h->cfg.squash_factor;     // cpp:53
    for (int r = 0; r < tw; ++r)
        for (int d = 0; d < tw; ++d) L[(size_t)r * tw + d] = (float)(std::log(h->table[(size_t)d * tw + r]) * inv_squash);
    std::vector<uint8_t> dist;
    build_distance_field(data, h->W, h->H, h->Wp, h->Hp, h->Wps, dist);
    h->have_map = false;                 // until every buffer below exists again: a failure leaves "map not set", never dangling pointers
    h->d_grid.drop(); h->d_dist.drop(); h->d_dist4.drop(); h->d_L.drop(); h->d_table.drop();     // drop + reserve: the exact size
    for (int q = 0; q < 4; ++q) h->d_distq[q].drop();
    MCL_TRY(h->d_grid.reserve(h, (size_t)h->W * h->H));
    MCL_TRY(h->d_dist.reserve(h, dist.size()));
    MCL_TRY(h->d_L.reserve(h, L.size()));
    MCL_TRY(h->d_table.reserve(h, h->table.size()));
    HIPCHK(h, hipMemcpy(h->d_grid, data, (size_t)h->W * h->H, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_dist, dist.data(), dist.size(), hipMemcpyHostToDevice));
    {
        std::vector<uint8_t> d4(dist.size() / 2);          // Wps is a multiple of 8
        for (size_t k = 0; k < d4.size(); ++k)
            d4[k] = (uint8_t)(std::min<int>(dist[2 * k], 15) | (std::min<int>(dist[2 * k + 1], 15) << 4));
        MCL_TRY(h->d_dist4.reserve(h, d4.size()));
        HIPCHK(h, hipMemcpy(h->d_dist4, d4.data(), d4.size(), hipMemcpyHostToDevice));
    }
    if (want_wedges) {
        static const int qsx[4] = {1, -1, -1, 1}, qsy[4] = {1, 1, -1, -1};
        std::vector<uint8_t> dq;
        for (int q = 0; q < 4; ++q) {
            build_directional_field(data, h->W, h->H, h->Wp, h->Hp, h->Wps, qsx[q], qsy[q], dq);
            MCL_TRY(h->d_distq[q].reserve(h, dq.size()));
            HIPCHK(h, hipMemcpy(h->d_distq[q], dq.data(), dq.size(), hipMemcpyHostToDevice));
        }
    }
    h->d_distw.drop(); h->d_distg.drop();
    if (want_wedges) {
        // wedge fields for k_rays_cell (mcl_wedge.h), built on the device from the isotropic field's stop cells
        const size_t fsz = (size_t)h->Hp * h->Wps, ncell = (size_t)h->Hp * h->Wp;
        DevBuf<int32_t> d_nxt, d_prv;
        DevBuf<mcl::WedgeRow> d_rows;
        std::vector<mcl::WedgeRow> rows(2 * mcl::kWedgeR + 1);
        MCL_TRY(h->d_distw.reserve(h, fsz * mcl::kWedges));
        HIPCHK(h, hipMemsetAsync(h->d_distw, 0, fsz * mcl::kWedges, h->stream));   // same stream as the kernels that fill it
        MCL_TRY(d_nxt.reserve(h, ncell));
        MCL_TRY(d_prv.reserve(h, ncell));
        MCL_TRY(d_rows.reserve(h, rows.size()));
        hipLaunchKernelGGL(mcl::k_row_tables, dim3((h->Hp + 63) / 64), dim3(64), 0, h->stream, h->d_dist, h->Wp, h->Hp, h->Wps, d_nxt, d_prv);
        // the tight rule of mcl_wedge.h (jumps bounded by the distance travelled inside the wedge); MCL_WEDGE_METRIC=0 keeps the
        // Euclidean rule: the same binary with either field, for A/B measurements (read here, so a process can build both)
        const char *metric = getenv("MCL_WEDGE_METRIC");
        const bool tight = !(metric && atoi(metric) == 0);
        h->wedge_tight = tight;
        int rc_w = MCL_OK;
        for (int k = 0; k < mcl::kWedges && rc_w == MCL_OK; ++k) {
            mcl::wedge_rows(k, rows.data());
            if (hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(mcl::WedgeRow), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
                hipStreamSynchronize(h->stream) != hipSuccess) { rc_w = MCL_ERR_HIP; break; }
            if (tight)
                hipLaunchKernelGGL(mcl::k_wedge_field_tight, dim3((h->Wp + 255) / 256, h->Hp), dim3(256), 0, h->stream, d_nxt, d_prv, h->Wp, h->Hp, h->Wps,
                                   d_rows, mcl::wedge_cone(k), h->d_distw + (size_t)k * fsz);
            else
                hipLaunchKernelGGL(mcl::k_wedge_field, dim3((h->Wp + 255) / 256, h->Hp), dim3(256), 0, h->stream, d_nxt, d_prv, h->Wp, h->Hp, h->Wps,
                               d_rows, h->d_distw + (size_t)k * fsz);
            if (hipStreamSynchronize(h->stream) != hipSuccess) rc_w = MCL_ERR_HIP;   // rows[] is reused by the next wedge
        }
        if (rc_w != MCL_OK) return fail(h, rc_w, "building the wedge fields failed");
        if (h->sweep_global) {
            // the copies k_rays_sweep<.., GLOBAL> probes: every field mirrored for its quadrant, with a two-cell ring of stop bytes
            // and a TAIL of stop rows (k_ring_field; the allocation is stop-filled first).  Memory safety does not rest on the rays
            // being valid: a walk starts in a cell of the ringed grid, runs towards +x, +y only and advances by at most P samples
            // in total whatever bytes it reads (mcl::sweep_global_layout: the largest offset it can form lies inside its own
            // field's tail; tests/test_sweep_addressing.py enumerates the corners).
            const mcl::SweepGlobalLayout gl = mcl::sweep_global_layout(h->Wp, h->Hp, P);
            if (!gl.ok) {
                h->distg_why_not = "k_rays_sweep's global-field form needs the sixteen ringed fields (with their tails) in less than 2^32 bytes and rows / pitch below 2^24: this map is too large for it";
            } else {
                h->distg_pitch = gl.pitch;
                h->distg_stride = gl.stride;
                MCL_TRY(h->d_distg.reserve(h, gl.alloc));
                HIPCHK(h, hipMemsetAsync(h->d_distg, 0xFF, gl.alloc, h->stream));
                for (int k = 0; k < mcl::kWedges; ++k) {
                    const int q = k >> mcl::kWedgeShift;
                    hipLaunchKernelGGL(mcl::k_ring_field, dim3((h->distg_pitch + 255) / 256, h->Hp + 4), dim3(256), 0, h->stream, h->d_distw + (size_t)k * fsz,
                                       h->Wp, h->Hp, h->Wps, h->distg_pitch, (q == 0 || q == 3) ? 1 : 0, (q == 0 || q == 1) ? 1 : 0,
                                       h->d_distg + (size_t)k * h->distg_stride);
                }
                HIPCHK(h, hipGetLastError());
                HIPCHK(h, hipStreamSynchronize(h->stream));
            }
        }
    }
    HIPCHK(h, hipMemcpy(h->d_L, L.data(), L.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_table, h->table.data(), h->table.size() * sizeof(double), hipMemcpyHostToDevice));
    h->d_Lt.drop(); h->d_Ltd.drop(); h->ltd_ready = false;
    {   // free-space list for initialize_global (cpp:199-213, 411-421): row-major order of data == 0
        std::vector<uint32_t> fr;
        for (size_t i = 0; i < (size_t)h->W * h->H; ++i)
            if (data[i] == 0) fr.push_back((uint32_t)i);
        h->d_free.drop();
        h->n_free = fr.size();
        h->free_row.assign((size_t)h->H + 1, 0);             // (a map patch splices whole rows of the list)
        for (size_t y = 0, i = 0; y <= (size_t)h->H; ++y) {
            while (i < fr.size() && fr[i] < y * (size_t)h->W) ++i;
            h->free_row[y] = i;
        }
        if (h->n_free) {
            MCL_TRY(h->d_free.reserve(h, fr.size()));
            HIPCHK(h, hipMemcpy(h->d_free, fr.data(), fr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        }
    }
    h->have_map = true;
    if (h->kld_on) {
        h->kld_nx = kld_nx; h->kld_ny = kld_ny; h->kld_bits = kld_bits;
        const int rc = kld_alloc(h);
        if (rc) { h->have_map = false; return rc; }
    }
    h->lf_K = -1;                        // (the model off: built when it is switched on)
    if (h->lf_on) {
        const int rc = lf_build(h);
        if (rc) { h->have_map = false; return rc; }
    }
    return MCL_OK;
}

// ---- the kernels of a map patch (mcl_map_patch.h; the flow is mcl_map_patch.hip's), one function per table.  Every launch covers
// a window inside the table it writes; what it reads lies inside the extended region formed here, clipped to the grid.
namespace {
inline mcl::PatchWin patch_win(const int32_t w[4]) { return mcl::PatchWin{w[0], w[1], w[2] - w[0] + 1, w[3] - w[1] + 1}; }
inline dim3 patch_grid(int w, int rows) { return dim3((unsigned)((w + 255) / 256), (unsigned)rows); }
int patch_launched(mcl_engine *h, const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MCL_OK : fail(h, MCL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

int mcl_host::launch_patch_skip_field(mcl_engine *h, const int32_t win[4], MapPatchTmp &t)
{
    const mcl::PatchWin w = patch_win(win);
    const int R = mcl::kPatchReach;
    // the dilated stop set around the window, out to the one-cell stop border of the work grid at most
    const int ex0 = std::max(win[0] - R, -1), ey0 = std::max(win[1] - R, -1), ex1 = std::min(win[2] + R, h->Wp), ey1 = std::min(win[3] + R, h->Hp);
    const mcl::PatchWin e{ex0, ey0, ex1 - ex0 + 1, ey1 - ey0 + 1};
    MCL_TRY(t.mask.reserve(h, (size_t)e.w * e.h));
    MCL_TRY(t.g.reserve(h, (size_t)e.w * w.h));
    hipLaunchKernelGGL(mcl::k_patch_stop_mask, patch_grid(e.w, e.h), dim3(256), 0, h->stream, h->d_grid.p, h->W, h->Wp, h->Hp, e, t.mask.p);
    hipLaunchKernelGGL(mcl::k_patch_iso_cols, patch_grid(e.w, w.h), dim3(256), 0, h->stream, t.mask.p, e, w.y0, w.h, t.g.p);
    hipLaunchKernelGGL(mcl::k_patch_iso_rows, patch_grid(w.w, w.h), dim3(256), 0, h->stream, t.g.p, e, h->d_grid.p, h->W, h->Wp, h->Hp, w, h->Wps, h->d_dist.p);
    const int b0 = win[0] / 2, bw = win[2] / 2 - b0 + 1;            // whole bytes of the nibble copy (win[2] / 2 < Wps / 2)
    hipLaunchKernelGGL(mcl::k_patch_nibbles, patch_grid(bw, w.h), dim3(256), 0, h->stream, h->d_dist.p, h->Wps, b0, w.y0, bw, h->d_dist4.p);
    return patch_launched(h, "map patch, isotropic field");
}

int mcl_host::launch_patch_quadrant(mcl_engine *h, int q, const int32_t win[4], MapPatchTmp &t)
{
    static const int qsx[4] = {1, -1, -1, 1}, qsy[4] = {1, 1, -1, -1};
    const mcl::PatchWin w = patch_win(win);
    const int R = mcl::kPatchReach + 1;
    // the rows ahead of the window, the row beyond the grid included
    const int ey0 = qsy[q] > 0 ? win[1] : std::max(win[1] - R, -1), ey1 = qsy[q] > 0 ? std::min(win[3] + R, h->Hp) : win[3], eh = ey1 - ey0 + 1;
    MCL_TRY(t.hq[q].reserve(h, (size_t)w.w * eh));
    hipLaunchKernelGGL(mcl::k_patch_quad_rows, patch_grid(w.w, eh), dim3(256), 0, h->stream, h->d_grid.p, h->W, h->Wp, h->Hp, qsx[q], w, ey0, eh, t.hq[q].p);
    hipLaunchKernelGGL(mcl::k_patch_quad_cols, patch_grid(w.w, w.h), dim3(256), 0, h->stream, t.hq[q].p, h->d_grid.p, h->W, h->Wp, h->Hp, qsy[q], w, ey0, eh,
                       h->Wps, h->d_distq[q].p);
    return patch_launched(h, "map patch, quadrant field");
}

int mcl_host::launch_patch_wedges(mcl_engine *h, const int32_t win[4], const int32_t quad[4][4], MapPatchTmp &t)
{
    constexpr int nrow = 2 * mcl::kWedgeR + 1;
    static const std::vector<mcl::WedgeRow> all_rows = [] {          // (constants of the wedges; they outlive every copy enqueued from them)
        std::vector<mcl::WedgeRow> r((size_t)mcl::kWedges * nrow);
        for (int k = 0; k < mcl::kWedges; ++k) mcl::wedge_rows(k, r.data() + (size_t)k * nrow);
        return r;
    }();
    // the row tables of the window widened by the offsets a cell searches, in that region's own coordinates
    const int ex0 = std::max(win[0] - mcl::kWedgeR, 0), ey0 = std::max(win[1] - mcl::kWedgeR, 0);
    const int ex1 = std::min(win[2] + mcl::kWedgeR, h->Wp - 1), ey1 = std::min(win[3] + mcl::kWedgeR, h->Hp - 1);
    const mcl::PatchWin e{ex0, ey0, ex1 - ex0 + 1, ey1 - ey0 + 1};
    MCL_TRY(t.nxt.reserve(h, (size_t)e.w * e.h));
    MCL_TRY(t.prv.reserve(h, (size_t)e.w * e.h));
    MCL_TRY(t.rows.reserve(h, all_rows.size()));
    HIPCHK(h, hipMemcpyAsync(t.rows.p, all_rows.data(), all_rows.size() * sizeof(mcl::WedgeRow), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(mcl::k_patch_row_tables, dim3((e.h + 63) / 64), dim3(64), 0, h->stream, h->d_dist.p, h->Wps, e, t.nxt.p, t.prv.p);
    const size_t fsz = (size_t)h->Hp * h->Wps;
    for (int k = 0; k < mcl::kWedges; ++k) {
        const int q = k >> mcl::kWedgeShift;
        const mcl::PatchWin w = patch_win(quad[q]);
        uint8_t *field = h->d_distw.p + (size_t)k * fsz;
        if (h->wedge_tight)
            hipLaunchKernelGGL(mcl::k_patch_wedge_field<true>, patch_grid(w.w, w.h), dim3(256), 0, h->stream, t.nxt.p, t.prv.p, e, w, h->Wps,
                               t.rows.p + (size_t)k * nrow, mcl::wedge_cone(k), field);
        else
            hipLaunchKernelGGL(mcl::k_patch_wedge_field<false>, patch_grid(w.w, w.h), dim3(256), 0, h->stream, t.nxt.p, t.prv.p, e, w, h->Wps,
                               t.rows.p + (size_t)k * nrow, mcl::WedgeCone{}, field);
        if (h->d_distg)
            hipLaunchKernelGGL(mcl::k_patch_ring_field, patch_grid(w.w, w.h), dim3(256), 0, h->stream, field, h->Wp, h->Hp, h->Wps, h->distg_pitch,
                               (q == 0 || q == 3) ? 1 : 0, (q == 0 || q == 1) ? 1 : 0, w, h->d_distg.p + (size_t)k * h->distg_stride);
    }
    return patch_launched(h, "map patch, wedge fields");
}

int mcl_host::launch_patch_lfield(mcl_engine *h, const int32_t win[4], int reach, int K, MapPatchTmp &t)
{
    const mcl::PatchWin w = patch_win(win);
    const int ex0 = std::max(win[0] - reach, 0), ew = std::min(win[2] + reach, h->W - 1) - ex0 + 1;
    MCL_TRY(t.lf_g.reserve(h, (size_t)ew * w.h));
    hipLaunchKernelGGL(mcl::k_patch_lf_cols, patch_grid(ew, w.h), dim3(256), 0, h->stream, h->d_grid.p, h->W, h->H, reach, ex0, ew, w.y0, w.h, t.lf_g.p);
    hipLaunchKernelGGL(mcl::k_patch_lf_rows, patch_grid(w.w, w.h), dim3(256), 0, h->stream, t.lf_g.p, ex0, ew, h->W, reach, K, w, h->d_lf_D.p);
    return patch_launched(h, "map patch, likelihood field");
}

int mcl_set_beam_angles(mcl_engine_t *h, const float *angles, int32_t n_beams)
{
    if (h) graph_reset(h);
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!angles || n_beams <= 0 || n_beams > 65536) return fail(h, MCL_ERR_INVALID_ARG, "bad beam angles");
    recov_unset(h);
    h->ds_on = false;                    // DS6: a table of offsets belonged to the old beams (graph_reset above has voided what held it)
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->B = 0;                            // until every buffer below exists again (ready() tests B > 0)
    h->bpad = (n_beams + 63) & ~63;
    h->quad_ok = n_beams < 16384;
    for (int j = 1; j < n_beams && h->quad_ok; ++j)
        if (!(angles[j] > angles[j - 1])) h->quad_ok = false;
    if (h->quad_ok && !((double)angles[n_beams - 1] - (double)angles[0] < 2.0 * M_PI - 1e-3)) h->quad_ok = false;
    h->angles.assign(angles, angles + n_beams);
    // padded so that k_rays_skip never clamps its beam index, with at least one entry after the last beam: k_rays_sweep's
    // beam walk requests the NEXT beam's direction on every trip, the last one included.  A multiple of 768 = lcm(256, 192):
    // k_rays_skip<R> reads whole groups of 64 R entries, and with three rays per lane a group is 192 of them (2701 beams: 2880
    // entries read, where a multiple of 256 gave 2816)
    const int ncs = (n_beams + 1 + 767) / 768 * 768;
    std::vector<double2> cs(ncs);
    for (int j = 0; j < ncs; ++j) {
        double a = (double)angles[j < n_beams ? j : n_beams - 1];   // cpp:533 widens the float angle
        cs[j] = make_double2(std::cos(a), std::sin(a));
    }
    h->beam_cs_host.assign(cs.begin(), cs.begin() + n_beams);
    // k_rays_sweep pads the lanes whose scan begins or ends inside a wedge with virtual beams -- the angular grid of the scan
    // continued beyond its ends -- up to the beams of a full wedge.  Only for an evenly spaced scan (every angle within a quarter
    // of the spacing of the grid through the first and the last) that leaves a wedge of the turn uncovered (no second range).
    h->beam_pad = 0; h->beam_margin = 0;
    const double span = n_beams > 1 ? (double)angles[n_beams - 1] - (double)angles[0] : 0.0;
    const double inc = n_beams > 1 ? span / (double)(n_beams - 1) : 0.0;
    const double wedge = 2.0 * M_PI / (double)mcl::kWedges;
    // the most beams one direction wedge holds, wherever a heading puts it: a closed interval of 2 pi / 16 of beam angle, around
    // the turn (what one work item of k_rays_sweep can hand to its fix-up list segment per particle: plan_work_lists)
    h->wedge_beams_max = n_beams;
    if (h->quad_ok) {
        const auto turned = [&](int k) { return (double)angles[k % n_beams] + (k >= n_beams ? 2.0 * M_PI : 0.0); };
        int most = 1;
        for (int i = 0, j = 0; j < 2 * n_beams; ++j) {
            while (turned(j) - turned(i) > wedge + 1e-9) ++i;
            most = std::max(most, std::min(j - i + 1, (int)n_beams));
        }
        h->wedge_beams_max = most;
    }
    if (h->quad_ok && inc > 0.0 && span + wedge < 2.0 * M_PI - 1e-3 && !getenv("MCL_NO_BEAM_PAD")) {
        bool regular = true;
        for (int j = 0; j < n_beams && regular; ++j)
            regular = std::fabs((double)angles[j] - ((double)angles[0] + (double)j * inc)) < 0.25 * inc;
        const double per_wedge = wedge / inc;
        if (regular && per_wedge >= 2.0 && per_wedge <= 120.0) {
            h->beam_pad = (int)std::ceil(per_wedge - 1e-9);          // (beam_pad - 1) spacings are less than a wedge
            h->beam_margin = (h->beam_pad + 2 + 7) & ~7;
        }
    }
    const int ncsx = n_beams + 2 * h->beam_margin + 8;
    // The LDS form continues the scan's angular grid beyond its ends (a virtual ray then looks like its neighbours' real ones).
    // Such a ray may leave the lane's wedge by a beam or so, where the wedge's skip field does not hold for it: harmless in an
    // LDS window (it can only read the window), NOT in the global-field form, where a ray that jumps a wall near the map border
    // would leave the field -- there a virtual beam repeats the first / last real beam (inside the wedge by construction).
    std::vector<double2> csx(ncsx), csxg(ncsx);
    for (int i = 0; i < ncsx; ++i) {
        const int j = i - h->beam_margin;
        const double ac = (double)angles[j < 0 ? 0 : (j < n_beams ? j : n_beams - 1)];
        double a;
        if (j >= 0 && j < n_beams) a = (double)angles[j];
        else if (h->beam_margin > 0) a = (double)angles[0] + (double)j * inc;
        else a = ac;
        csx[i] = make_double2(std::cos(a), std::sin(a));
        csxg[i] = make_double2(std::cos(ac), std::sin(ac));
    }
    h->d_angle.drop(); h->d_beam_cs.drop(); h->d_beam_csx.drop(); h->d_beam_csxg.drop(); h->d_obs_idx.drop(); h->d_obs.drop();
    h->d_beam_csi.drop(); h->d_beam_err.drop();
    h->rec_ok = false;
    if (h->beam_margin > 0 && !getenv("MCL_SWEEP_NO_REC")) {
        // REC: the walk turns the direction by the grid increment instead of fetching it (mcl_rays_sweep.h).  Every beam must lie
        // within 2e-6 rad of the grid through the first and the last (the second-order term of its offset, e^2 / 2 * 2^32 units,
        // then stays below 1e-2 unit of the guard's budget): the float rounding of a0 + j inc, which is what a lidar driver
        // publishes, is a few 1e-8.
        const int ecols = (n_beams + 2 * h->beam_margin + 64) & ~63;          // = ltd_cols (ensure_lt)
        std::vector<double2> csi(ncsx);
        std::vector<double> err((size_t)ecols, 0.0);
        double worst = 0.0;
        for (int i = 0; i < ncsx; ++i) {
            const int j = i - h->beam_margin;
            const double ag = (double)angles[0] + (double)j * inc;
            csi[i] = make_double2(std::cos(ag), std::sin(ag));
            if (j >= 0 && j < n_beams && i < ecols) { err[i] = (double)angles[j] - ag; worst = std::max(worst, std::fabs(err[i])); }
        }
        if (worst <= 2e-6 && ncsx <= ecols + 8) {
            MCL_TRY(h->d_beam_csi.reserve(h, (size_t)ncsx));
            HIPCHK(h, hipMemcpy(h->d_beam_csi, csi.data(), (size_t)ncsx * sizeof(double2), hipMemcpyHostToDevice));
            MCL_TRY(h->d_beam_err.reserve(h, (size_t)ecols));
            HIPCHK(h, hipMemcpy(h->d_beam_err, err.data(), (size_t)ecols * sizeof(double), hipMemcpyHostToDevice));
            h->rec_c = std::cos(inc); h->rec_s = std::sin(inc);
            h->rec_ok = true;
        }
    }
    h->h_obs.drop();
    MCL_TRY(h->d_obs.reserve(h, (size_t)n_beams));
    MCL_TRY(h->h_obs.reserve(h, (size_t)n_beams));
    MCL_TRY(h->d_angle.reserve(h, (size_t)n_beams));
    MCL_TRY(h->d_beam_cs.reserve(h, (size_t)ncs));
    MCL_TRY(h->d_obs_idx.reserve(h, (size_t)n_beams));
    HIPCHK(h, hipMemcpy(h->d_angle, angles, (size_t)n_beams * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_beam_cs, cs.data(), (size_t)ncs * sizeof(double2), hipMemcpyHostToDevice));
    MCL_TRY(h->d_beam_csx.reserve(h, (size_t)ncsx));
    HIPCHK(h, hipMemcpy(h->d_beam_csx, csx.data(), (size_t)ncsx * sizeof(double2), hipMemcpyHostToDevice));
    MCL_TRY(h->d_beam_csxg.reserve(h, (size_t)ncsx));
    HIPCHK(h, hipMemcpy(h->d_beam_csxg, csxg.data(), (size_t)ncsx * sizeof(double2), hipMemcpyHostToDevice));
    h->d_Lt.drop(); h->d_Ltd.drop(); h->ltd_ready = false;
    h->B = n_beams;
    return MCL_OK;
}

// The particles in the current buffer and the weights in d_w are a new set of n (set from outside or initialised): its fixed-point
// weights, sums and CDF (d_max_override: the weight to scale by, on the device), and everything kept about the old set is dropped.
static int adopt_particle_set(mcl_engine *h, int64_t n, const double *d_max_override)
{
    MCL_TRY(weight_stats(h, false, d_max_override, true));
    MCL_TRY(scan_weights(h, h->d_q, h->d_cdf, n, 0, nullptr));
    MCL_TRY(fetch_scalars(h));
    h->have_particles = true;
    h->far_fresh = true;
    h->pack_valid[0] = h->pack_valid[1] = false;
    h->have_idx = h->have_steps = h->have_logw = false;
    h->sp_valid = h->weighted = false;
    comm_forget(h->comm);                   // a sharded set: the other shards' lists are unknown again
    h->stage_kept = false;
    kld_reset(h);
    recov_unset(h);
    return MCL_OK;
}

// weight_scale: the weight the fixed-point values are scaled by (null: this call's own maximum).  A shard of a larger set
// must use the maximum over the WHOLE set, or the shards' fixed-point weights are not comparable.
int mcl_host::set_particles_impl(mcl_engine_t *h, const double *xyz, const double *weights, int64_t n, const double *weight_scale)
{
    if (h) graph_reset(h);
    if (!h) return MCL_ERR_INVALID_ARG;
    h->set_epoch++;
    if (!xyz || !weights || n <= 0 || n > h->cap) return fail(h, MCL_ERR_INVALID_ARG, "bad particle arrays / count");
    if (weight_scale && !(*weight_scale > 0.0)) return fail(h, MCL_ERR_INVALID_ARG, "weight scale must be positive");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t nb = (size_t)n * sizeof(double);
    const int c = h->cur;
    HIPCHK(h, hipMemcpyAsync(h->d_x[c], xyz, nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_y[c], xyz + n, nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_th[c], xyz + 2 * n, nb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_w, weights, nb, hipMemcpyHostToDevice, h->stream));
    h->N = n;
    if (weight_scale) {
        std::memcpy(&h->h_result[kResultStage], weight_scale, sizeof(double));        // pinned: stays valid until the copy has run
        HIPCHK(h, hipMemcpyAsync(h->d_scalars, &h->h_result[kResultStage], sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    return adopt_particle_set(h, n, weight_scale ? h->d_scalars : nullptr);
}

int mcl_set_particles(mcl_engine_t *h, const double *xyz, const double *weights, int64_t n)
{
    return set_particles_impl(h, xyz, weights, n, nullptr);
}

int mcl_set_particles_shard(mcl_engine_t *h, const double *xyz, const double *weights, int64_t n, double max_weight_of_the_whole_set)
{
    return set_particles_impl(h, xyz, weights, n, &max_weight_of_the_whole_set);
}

static int finish_init(mcl_engine *h, int64_t n, int64_t n_total)
{
    graph_reset(h);
    h->set_epoch++;
    h->N = n;
    hipLaunchKernelGGL(mcl::k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_w, n, 1.0 / (double)n_total);
    HIPCHK(h, hipGetLastError());
    const int rc = adopt_particle_set(h, n, nullptr);
    if (rc == MCL_OK) h->init_idx++;
    return rc;
}

// what the four initialisers ask of their arguments alike (given: the call's own pointers are)
static int check_init(mcl_engine *h, bool given, int64_t n, int64_t first_global_index, int64_t n_total)
{
    if (given && n > 0 && n <= h->cap && first_global_index >= 0 && n_total >= n && n_total < MCL_MAX_TOTAL_PARTICLES) return MCL_OK;
    return fail(h, MCL_ERR_INVALID_ARG, "bad init arguments (the sharded total must stay below 2^27)");
}

int mcl_init_particles_pose(mcl_engine_t *h, const double pose[3], int64_t n, int64_t first_global_index, int64_t n_total)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    MCL_TRY(check_init(h, pose != nullptr, n, first_global_index, n_total));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int c = h->cur;
    hipLaunchKernelGGL(mcl::k_init_pose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, pose[0], pose[1], pose[2], n,
                       first_global_index, (uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32), h->init_idx, h->d_x[c], h->d_y[c], h->d_th[c]);
    HIPCHK(h, hipGetLastError());
    return finish_init(h, n, n_total);
}

int mcl_init_global(mcl_engine_t *h, int64_t n, int64_t first_global_index, int64_t n_total)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "map not set");                 // cpp:403
    if (h->n_free == 0) return fail(h, MCL_ERR_NOT_READY, "No free space found in map!");   // cpp:423-427
    MCL_TRY(check_init(h, true, n, first_global_index, n_total));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int c = h->cur;
    hipLaunchKernelGGL(mcl::k_init_global, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_free, h->n_free, h->W, h->res,
                       h->ox, h->oy, n, first_global_index, (uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32), h->init_idx, h->d_x[c],
                       h->d_y[c], h->d_th[c]);
    HIPCHK(h, hipGetLastError());
    return finish_init(h, n, n_total);
}

int mcl_get_weights(mcl_engine_t *h, double *weights, int64_t n)
{
    if (!h || !weights) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    if (n != h->N) return fail(h, MCL_ERR_INVALID_ARG, "n != active particle count");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(mcl::k_normalized, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_w, n, h->global_sums[0], h->d_tmp);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(weights, h->d_tmp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_sample_particles(mcl_engine_t *h, int32_t k, const double *uniforms, double *out)
{
    if (!h || !out || k <= 0 || k > 65536) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    double *d_u = nullptr;
    // the rows and the uniforms share d_tmp (3 cap doubles from mcl_create): a draw of more than three quarters of the engine's
    // capacity -- any draw at all from an engine of one particle -- grows it (no graph holds this pointer; the stream is idle first)
    if ((size_t)k * 4 > h->d_tmp.cap) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        MCL_TRY(h->d_tmp.reserve(h, (size_t)k * 4));
    }
    double *d_out = h->d_tmp;
    if (uniforms) {
        d_u = h->d_tmp + (size_t)3 * k;
        HIPCHK(h, hipMemcpyAsync(d_u, uniforms, (size_t)k * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    const int c = h->cur;
    hipLaunchKernelGGL(mcl::k_sample, dim3((k + 63) / 64), dim3(64), 0, h->stream, h->d_x[c], h->d_y[c], h->d_th[c], h->d_cdf, h->N,
                       h->q_total, d_u, (uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32), h->update_idx, k, d_out);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)3 * k * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_particle_mean(mcl_engine_t *h, double out[3])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int c = h->cur;
    const int nb = 256;
    hipLaunchKernelGGL(mcl::k_colsum, dim3(nb), dim3(mcl::kRedThreads), 0, h->stream, h->d_x[c], h->d_y[c], h->d_th[c], h->N, h->d_part);
    HIPCHK(h, hipGetLastError());
    std::vector<double> part((size_t)nb * 4);
    HIPCHK(h, hipMemcpyAsync(part.data(), h->d_part, part.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double s[3] = {0, 0, 0};
    for (int b = 0; b < nb; ++b) { s[0] += part[b * 4]; s[1] += part[b * 4 + 1]; s[2] += part[b * 4 + 2]; }
    for (int k = 0; k < 3; ++k) out[k] = s[k] / (double)h->N;
    return MCL_OK;
}

// The fields of ResampleArgs that mcl_update and the staged resample fill alike: the CDF and the spine of the scan that produced it,
// mode, seed, the systematic offset of this update, the reference model's dispersions, the children's columns in the other buffer.
static void resample_common_args(const mcl_engine *h, mcl::ResampleArgs &a, const uint64_t *d_cdf, int64_t n_parents)
{
    a.cdf = d_cdf; a.n_parents = n_parents;
    a.tile_excl = (d_cdf && h->blocktot_for == d_cdf && h->blocktot_n == n_parents) ? h->d_blocktot : nullptr;   // spine of the scan that produced d_cdf
    a.leaders = a.tile_excl ? h->d_leaders : nullptr;
    a.mode = h->cfg.resample_mode;
    a.seed_lo = (uint32_t)h->cfg.seed; a.seed_hi = (uint32_t)(h->cfg.seed >> 32);
    a.update_idx = h->update_idx;
    a.k0 = a.mode == MCL_RESAMPLE_SYSTEMATIC ? systematic_offset(a.seed_lo, a.seed_hi, h->update_idx) : 0;
    a.disp_x = h->cfg.motion_dispersion_x; a.disp_y = h->cfg.motion_dispersion_y; a.disp_th = h->cfg.motion_dispersion_theta;
    const int nx = h->cur ^ 1;
    a.cx = h->d_x[nx]; a.cy = h->d_y[nx]; a.cth = h->d_th[nx];
    a.do_motion = 1;
}

// What the resampling kernel does for the ray stage that follows it in the same update (mcl_update and the staged flow alike):
// the per-particle constants come out of it (k_rays_skip: one launch less per small update; k_rays_cell / k_rays_sweep: also the
// per-particle scratch their stage wants zeroed, a pass over the children less), and from the second update of a configuration on
// the (key, index) pairs of the ordering and the few words launch_rays would clear.
static void resample_ray_extras(mcl_engine *h, int64_t n, mcl::ResampleArgs &a, bool fresh_children = false)
{
    if (h->mounted) return;                 // SM5: the ray stage works on the sensors' poses, which this kernel does not form
    const int rmode = choose_ray_mode(h, n, false);
    if (!(rmode == MCL_RAYS_SKIP || mode_orders(rmode))) return;
    a.pc_out = h->d_pc; a.ox = h->ox; a.oy = h->oy; a.res = h->res;
    if (mode_orders(rmode)) { a.clr_logw_acc = h->d_logw_acc; a.clr_far_flags = reinterpret_cast<uint32_t *>(h->d_far.p); }
    RayHandoff &ho = h->handoff;
    ho.constants = true;
    // The ordering of the ray stage works from the layout (bounding box, occupied tiles) of the PREVIOUS update's children
    // when there is one: the set moves by a cell or so per update and the order only decides which rays share a wave.
    // Radix ordering: this kernel then writes the (key, index) pairs too and the sort starts right after it.
    const auto [ntx_abs, nty_abs, tiles_ok] = sort_tiles(h);
    // (not for children injected anywhere on the map: fresh_children, an update of recovery injection -- DESIGN.md §4.9)
    if (mode_orders(rmode) && h->layout.valid && h->layout.n == n && !h->env.no_stale_layout && !fresh_children) {
        ho.stale_layout = true;
        if (sort_radix(h, n) && h->d_skey2) {
            a.key_out = h->d_skey; a.val_out = h->d_srank; a.key_bbox = h->d_bbox; a.key_tilemap = tiles_ok ? h->d_tilemap : nullptr;
            a.key_ntx = ntx_abs; a.key_Wp = h->Wp; a.key_Hp = h->Hp; a.key_fine = sort_fine(h);
            ho.keys = true;
            // ... and, in front of k_rays_sweep, leaves the sincos of the constants to the gather behind that sort (k_rays_cell's
            // fix-up and far kernels read (cos, sin) from d_pc by particle index; so does the one-workgroup tail of a small set)
            if (mode_sweep(rmode) && n > mcl::kTinyTailMax) { a.pc_heading = 1; ho.heading = true; }
        }
    }
    if (mode_orders(rmode) && h->prep_cache_valid && h->prep_cache_n == n && !h->env.no_prep_fold) {
        a.prep = h->prep_cache; a.prep_on = 1;      // launch_rays checks that this is what it would have cleared
        if (ho.stale_layout) a.prep.bbox = nullptr;          // the layout in d_bbox is in use: not reset
        ho.passed = a.prep;
        ho.folded = true;
    }
}

// After the resampling kernel: the layout of THESE children, for the next update, on the second stream beside the sort and the ray stage.
// (in two steps: the event right behind the resampling kernel, the launches once the ray stage has been submitted -- the
//  ordering kernels of the main stream are on the critical path of a small update, these are not)
static int layout_mark(mcl_engine *h, int64_t n)
{
    h->layout.wanted = false;
    if (!mode_orders(choose_ray_mode(h, n, false)) || h->env.no_stale_layout) return MCL_OK;
    HIPCHK(h, hipEventRecord(h->layout.ev_children, h->stream));
    h->layout.wanted = true;
    // (launched right here the layout kernels share the device with the sort: measured 0.04-0.06 ms per update slower at 1M and
    //  4M particles than behind the ray stage, where they run in the shadow of the persistent kernel's tail)
    return MCL_OK;
}

static int next_layout_launch(mcl_engine *h, int64_t n)
{
    if (!h->layout.wanted) return MCL_OK;
    h->layout.wanted = false;
    // (the layout of the NEXT update, made beside this one's ray stage: whether that update takes the hybrid form is not known
    //  yet -- its units are cut for the hybrid's windows, which costs the global-field form nothing but shorter runs)
    const int play = unit_play(h, choose_ray_mode(h, n, false), sweep_hybrid(h));
    HIPCHK(h, hipStreamWaitEvent(h->stream2, h->layout.ev_children, 0));
    hipLaunchKernelGGL(mcl::k_bbox_init, dim3(1), dim3(64), 0, h->stream2, h->layout.d_bbox_nx, play);
    launch_layout(h, h->stream2, n, h->layout.d_bbox_nx, h->layout.d_tilemark_nx, h->layout.d_tilemap_nx);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->layout.ev_layout, h->stream2));
    h->layout.pending = true;
    return MCL_OK;
}

// End of an update: the layout made beside its ray stage becomes the one the next update orders by.
int mcl_host::layout_adopt(mcl_engine *h, int64_t n)
{
    if (!h->layout.pending) return MCL_OK;
    HIPCHK(h, hipEventSynchronize(h->layout.ev_layout));
    std::swap(h->d_bbox, h->layout.d_bbox_nx); std::swap(h->d_tilemap, h->layout.d_tilemap_nx);
    h->layout.valid = true; h->layout.n = n; h->layout.pending = false;
    return MCL_OK;
}

// after an update with KLD on: the count came back in word 17 of the result block; a resampling update decides the next size
static void kld_decide(mcl_engine *h, bool kept)
{
    h->kld_bins_last = (int64_t)h->h_result[17];
    if (!kept) h->kld_n_next = kld_target(&h->kld, h->kld_bins_last, h->N);
}

// after an update that formed weights, with recovery on: the averages take in its likelihood (an injecting update unsets them first)
static void recov_after(mcl_engine *h, bool injected, bool kept, double prev_sum_w, int64_t n)
{
    if (!h->recov_on) return;
    if (injected) recov_unset(h);
    const double l = recov_likelihood(h->recov, h->h_scalars[0], h->h_scalars[1], kept ? prev_sum_w : (double)n, h->B);
    recov_fold(h->recov, h->recov_S, h->recov_F, l);
}

// the odometry arguments of an update's resampling kernel; false: the reference model (the kernels and arguments of always)
static bool odo_args_of(const mcl_engine *h, const double action[3], mcl::OdoArgs &o)
{
    if (h->motion.model == MCL_MOTION_REFERENCE || !action) return false;
    double s[8];
    if (mcl_host_motion_scalars(&h->motion, action, s) != MCL_OK) return false;
    o.model = h->motion.model; o.pad = 0;
    for (int i = 0; i < 6; ++i) o.s[i] = s[i];
    return true;
}

// The resampling kernel of an update: one of twelve entry points, [odometry model][KLD][injection: none | uniform | mixture]; the
// arguments follow ResampleArgs in that order of the ones that are present (kld, rec or mix -- never both --, odo: null = absent).
// timed: EV_RESAMPLE is the kernel's stop event, and the answer says so.
static bool launch_resample(mcl_engine *h, dim3 grid, size_t lds, bool timed, mcl::ResampleArgs &a, mcl::KldArgs *kld, mcl::RecArgs *rec,
                            mcl::MixArgs *mix, mcl::OdoArgs *odo)
{
    static const void *const entry[2][2][3] = {
        {{(const void *)mcl::k_resample_motion, (const void *)mcl::k_resample_motion_rec, (const void *)mcl::k_resample_motion_mix},
         {(const void *)mcl::k_resample_motion_kld, (const void *)mcl::k_resample_motion_kld_rec, (const void *)mcl::k_resample_motion_kld_mix}},
        {{(const void *)mcl::k_resample_odo, (const void *)mcl::k_resample_odo_rec, (const void *)mcl::k_resample_odo_mix},
         {(const void *)mcl::k_resample_odo_kld, (const void *)mcl::k_resample_odo_kld_rec, (const void *)mcl::k_resample_odo_kld_mix}}};
    void *args[4];
    int na = 0;
    args[na++] = &a;
    if (kld) args[na++] = kld;
    if (rec) args[na++] = rec;
    if (mix) args[na++] = mix;
    if (odo) args[na++] = odo;
    const void *fn = entry[odo ? 1 : 0][kld ? 1 : 0][mix ? 2 : (rec ? 1 : 0)];
    if (timed) (void)hipExtLaunchKernel(fn, grid, dim3(256), args, lds, h->stream, nullptr, h->ev[EV_RESAMPLE], 0);
    else (void)hipLaunchKernel(fn, grid, dim3(256), args, lds, h->stream);
    return timed;
}

// One mcl_update / mcl_sensor_update, on do_update's stack: the call, what plan_update decided about it, what the resampling launch left
struct Update {
    const double *action; const float *obs; int obs_stride; const double *uniforms; bool resample_and_move;
    std::chrono::steady_clock::time_point t0;
    int64_t n_par, n;                   // parents; children: every stage after the resampling kernel runs on them
    bool kld, keep, rec, mix;           // KLD sizes this draw | adaptive resampling keeps the set | the injecting kernel runs | ... from the proposal
    uint64_t rec_thr; double prev_sum_w;
    bool tiny, graph_ok;                // the tail: one workgroup | the captured graph | (neither) launch by launch
    // (resampling launch) the bins the tiny tail clears | the scan's tables are built on the second stream | EV_RESAMPLE is the kernel's stop event
    mcl::KldArgs kld_cur; bool obs_early, resample_bound;
    bool fuse;                          // mcl_sensor_update_fuse: the previous log-weights (d_logw_prev) are added to this stage's
};

// Phase 1: what this update is -- sizes, keep, recovery, and which of the three tails it takes.  Nothing is submitted here.
static int plan_update(mcl_engine *h, Update &u)
{
    // parents and children: the same number unless KLD sampling (mcl_set_kld) decided another size for this update's draw
    u.n_par = h->N;
    u.kld = u.resample_and_move && h->kld_on;
    u.n = u.kld ? h->kld_n_next : u.n_par;
    if (u.kld && (u.n < 1 || u.n > h->cap)) return fail(h, MCL_ERR_INVALID_ARG, "KLD: particle count out of range");
    // adaptive resampling (off by default): keep the particles when the previous update left an effective sample
    // size (sum w)^2 / sum w^2 of at least r * N; their weights then multiply, i.e. the log-weights add
    // (with KLD on only while the next size is the current one: a kept set cannot change its size)
    if (u.resample_and_move && h->cfg.resample_neff_permille > 0 && h->carry_valid && !u.uniforms && u.n == u.n_par) {
        const double sw = h->h_scalars[1], sww = h->h_scalars[7];
        u.keep = sww > 0.0 && sw * sw >= ((double)h->cfg.resample_neff_permille / 1000.0) * (double)u.n * sww;
    }
    if (h->cfg.resample_neff_permille > 0 && h->cfg.weight_mode == MCL_WEIGHT_PRODUCT)
        return fail(h, MCL_ERR_UNSUPPORTED, "resample_neff_permille needs weight_mode LOG");
    // recovery (mcl_set_recovery, off by default): a resampling update whose threshold is > 0 runs the injecting kernel
    u.prev_sum_w = h->h_scalars[1];
    u.rec_thr = (h->recov_on && u.resample_and_move && !u.keep) ? recov_threshold(recov_p(h->recov_S, h->recov_F)) : 0;
    u.rec = u.rec_thr > 0;
    u.mix = u.rec && h->mix_n > 0;          // a proposal in place (mcl_set_recovery_proposal): the injected children come from it
    if (u.rec && !u.mix && h->n_free == 0) return fail(h, MCL_ERR_NOT_READY, "recovery: the map has no free cell to inject particles into");
    // Small updates are launch-bound (about twenty launches for ~0.06 ms of kernels): once a regular update has run with these sizes
    // (graph_warm: every buffer exists) on the k_rays_skip path, one of two short tails takes its place.  Eligibility is a pure function
    // of the configuration and the sizes (choose_ray_mode), never of what the previous update happened to run: k_rays_skip chosen
    // outright has no work lists, no allocation and no fallback.  (Neither a likelihood-field update -- DESIGN.md §4.10 -- nor one that
    // changes the size of the set, which do_update treats as a set from outside, takes them.)
    const bool small = u.resample_and_move && !h->lf_on && h->cfg.graph_mode != 1 && h->graph_warm && u.n == u.n_par && !u.keep &&
                       h->cfg.weight_mode == MCL_WEIGHT_LOG && h->cfg.resample_neff_permille == 0 && choose_ray_mode(h, u.n, false) == MCL_RAYS_SKIP;
    // tiny: three launches and no copy: resampling + motion + per-particle constants + table rows of the scan | rays against the static
    // table | weights, sums, CDF and the result block written straight to pinned host memory, all in one workgroup
    u.tiny = small && u.n <= mcl::kTinyTailMax;
    // graph: everything after the resampling kernel is one hipGraph per particle buffer (observation upload ... result read-back)
    u.graph_ok = small && !u.tiny && !h->cfg.debug_count_probes;
    return MCL_OK;
}

// Phase 2: the resampling kernel (+ motion) of an update, and what is submitted right behind it.
static int launch_update_resample(mcl_engine *h, Update &u, const double *d_norm, const double *d_uni)
{
    const int64_t n = u.n, n_par = u.n_par;
    const int c = h->cur, nx = c ^ 1;
    mcl::ResampleArgs a{};
    a.px = h->d_x[c]; a.py = h->d_y[c]; a.pth = h->d_th[c]; a.q_total = h->q_total;
    resample_common_args(h, a, h->d_cdf, n_par);
    // parents: the compact list the last scan left (the particles that carry weight: a few per cent after an update
    // with many beams) when it exists, else the full CDF and the packed records
    const bool compact = !u.keep && h->compact_n > 0;
    if (compact) {
        a.ccdf = h->d_ccdf; a.ctop = h->d_ctop; a.n_compact = h->compact_n; a.cidx = h->d_cidx; a.crec = h->d_crec;
        a.cpack = nullptr;               // the next update most likely draws from a compact list again: no record per child
        // the list's guide, for the multinomial draw (the systematic comb compares 128-bit products; a KLD-sized draw keeps the ctop search)
        if (h->guide_valid && a.mode == MCL_RESAMPLE_MULTINOMIAL && !u.kld) {
            a.cguide = h->d_cguide; a.cguide_q = reinterpret_cast<const uint64_t *>(h->d_result.p + kResultGuideTotal); a.cguide_m = h->guide_m;
        }
    } else {
        if (!h->pack_valid[c] && n_par > 65536 && !u.keep) {   // records first: one fetch per gathered parent instead of three
            hipLaunchKernelGGL(mcl::k_pack_records, dim3((unsigned)((n_par + 255) / 256)), dim3(256), 0, h->stream, h->d_x[c], h->d_y[c], h->d_th[c], n_par, h->d_pack[c]);
            h->pack_valid[c] = true;
        }
        a.ppack = h->pack_valid[c] ? h->d_pack[c] : nullptr;
        a.cpack = h->d_pack[nx];
    }
    a.idx_out = h->d_idx;
    a.n_children = n; a.child_first = 0; a.n_children_total = n;
    a.uniforms = d_uni; a.normals = d_norm;
    if (a.mode == MCL_RESAMPLE_SYSTEMATIC && u.uniforms)
        a.k0 = (uint32_t)(std::min(std::max(u.uniforms[0], 0.0), 0.99999999976716936) * 4294967296.0);
    motion_scalars(u.action, a.dt, a.v, a.w);
    a.do_resample = u.keep ? 0 : 1;
    a.clear_counters = h->d_counters;
    if (u.tiny) {
        // the scan goes from the pinned staging buffer to table rows inside this kernel (no copy node, no table build)
        stage_observation(h, u.obs, u.obs_stride);
        a.obs_src = h->h_obs; a.obs_idx_out = h->d_obs_idx; a.obs_B = h->B; a.obs_P = h->P; a.res = h->res;
    }
    if (!h->lf_on) resample_ray_extras(h, n, a, u.rec);
    size_t cdf_lds = 0;
    if (!a.tile_excl && a.do_resample && n_par <= mcl::kTinyTailMax) { a.cdf_lds_entries = (int)n_par; cdf_lds = (size_t)n_par * sizeof(uint64_t); }
    const dim3 grid((unsigned)((n + 255) / 256));
    mcl::RecArgs rec_args{};
    mcl::MixArgs mix_args{};
    if (u.rec) {
        rec_args.thr = u.rec_thr; rec_args.free_cells = h->d_free; rec_args.n_free = h->n_free; rec_args.W = h->W;
        rec_args.res = h->res; rec_args.ox = h->ox; rec_args.oy = h->oy;
        rec_args.count = h->d_recov_cnt + h->recov_parity; rec_args.count_next = h->d_recov_cnt + (h->recov_parity ^ 1);
        if (u.mix) {
            mix_args.thr = u.rec_thr; mix_args.thresholds = h->d_mix_thr; mix_args.factors = h->d_mix_fac; mix_args.n_comp = h->mix_n;
            mix_args.count = rec_args.count; mix_args.count_next = rec_args.count_next;
            h->mix_n = 0;                   // one shot (P5): the next injecting update draws from free space again
        }
        h->recov_cnt_slot = h->recov_parity; h->recov_injected = -1;
        h->recov_parity ^= 1;
    }
    if (u.kld) {
        // the bins of the drawn parents are marked by the resampling kernel; the words it set are cleared and the count
        // lands in word 17 of the result block -- by the one-workgroup tail of a small update, else by one launch right here
        u.kld_cur = kld_args_of(&h->kld, h->kld_nx, h->kld_ny, h->ox, h->oy);
        u.kld_cur.bm = h->d_kld_bm; u.kld_cur.list = h->d_kld_list;
        u.kld_cur.count = h->d_kld_cnt + h->kld_parity; u.kld_cur.count_next = h->d_kld_cnt + (h->kld_parity ^ 1);
        u.kld_cur.result = h->d_result + 17;
        h->kld_parity ^= 1;
    }
    // (the motion model's scalars are plain arguments of this launch, which is outside the captured graph and the tail)
    mcl::OdoArgs odo_cur{};
    const bool odo = odo_args_of(h, u.action, odo_cur);
    u.resample_bound = launch_resample(h, grid, cdf_lds, !u.tiny && !h->capturing, a, u.kld ? &u.kld_cur : nullptr, u.rec && !u.mix ? &rec_args : nullptr,
                                       u.mix ? &mix_args : nullptr, odo ? &odo_cur : nullptr);
    if (u.kld && !u.tiny) {
        const int64_t most = std::min<int64_t>(n, (int64_t)h->kld_bits);
        hipLaunchKernelGGL(mcl::k_kld_clear, dim3((unsigned)std::min<int64_t>((most + 255) / 256, 1024)), dim3(256), 0, h->stream, u.kld_cur);
    }
    HIPCHK(h, hipGetLastError());
    h->N = n;                          // the children: the ray stage and everything after it run on them
    if (a.pc_out) MCL_TRY(layout_mark(h, n));
    // The tables of this update's scan (table rows of the observed ranges, Lt, Ltd) depend on nothing the resampling and ordering
    // kernels produce: with a windowed ray kernel they are built on a second stream beside those, and the ray stage waits for
    // them (a copy and two or three small launches off the critical path of an update: ~15 us).  Enqueued AFTER the resampling
    // kernel: that one is on the critical path, and a small update is bound by the order the host submits in.
    if (!u.tiny && !h->lf_on && !h->env.no_obs_overlap && mode_work_lists(choose_ray_mode(h, n, false))) {
        std::swap(h->stream, h->stream2);
        const int rc_obs = prepare_observation(h, u.obs, u.obs_stride);
        hipError_t ee = rc_obs ? hipSuccess : hipEventRecord(h->ev_obs, h->stream);
        std::swap(h->stream, h->stream2);
        if (rc_obs) return rc_obs;
        HIPCHK(h, ee);
        u.obs_early = true;
    }
    h->cur = nx;                       // cpp:689 as a pointer swap
    h->sp_valid = false;               // (the sensor poses of the parents)
    h->resampled_last = !u.keep;
    h->pack_valid[nx] = a.cpack != nullptr;
    h->compact_used = compact;
    h->guide_used = a.cguide != nullptr;
    h->have_idx = true;
    return MCL_OK;
}

// Phase 3, the one-workgroup tail of a small update: rays against the static table, then weights, sums, CDF and result in one launch.
static int tail_tiny(mcl_engine *h, const Update &u)
{
    MCL_TRY(launch_rays(h, h->d_x[h->cur], h->d_y[h->cur], h->d_th[h->cur], u.n, false, true));
    MCL_TRY(weights_and_cdf(h, true, u.kld ? &u.kld_cur : nullptr));
    // The result block lands in pinned memory stamped with this update's sequence number: spin on the stamp instead of
    // the stream's completion signal (the signal's path through the runtime costs several microseconds at this size).
    // Everything later on this engine is ordered behind the kernels by the stream; a stamp that never comes (a faulted
    // kernel) ends in the ordinary synchronisation, which reports the error.
    bool seen = false;
    if (h->env.tiny_poll) {
        const volatile unsigned long long *stamp = h->h_result + kResultStamp;
        const auto give_up = u.t0 + std::chrono::milliseconds(20);
        for (unsigned spin = 0; !seen; ++spin) {
            seen = __atomic_load_n(stamp, __ATOMIC_ACQUIRE) == h->result_seq;
            if (!seen && (spin & 1023u) == 1023u && std::chrono::steady_clock::now() > give_up) break;
        }
    }
    if (!seen) HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_result(h);
    // one unit, reported as the ray-cast stage (resampling, query prep and the tail are inside it), so that the six
    // stages still add up to the total the host uses for delay compensation: finish_update fills in [3] = [5]
    h->timings[0] = 0.0; h->timings[1] = 0.0; h->timings[2] = 0.0; h->timings[4] = 0.0;
    h->ray_ms_is_graph_tail = true;
    return MCL_OK;
}

// The captured tail of this particle buffer exists (captured here on its first use); the scan is staged for it.  false: this
// update -- and, after a failed capture, every later one of this engine -- runs launch by launch.
static bool graph_ready(mcl_engine *h, const Update &u)
{
    stage_observation(h, u.obs, u.obs_stride);
    const int gi = h->cur;
    if (h->graph_exec[gi]) return true;
    // nothing executes during capture, so a failure here simply falls back to the launch-by-launch path
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
    h->capturing = true;
    int rc = upload_observation(h);
    if (!rc) rc = launch_rays(h, h->d_x[gi], h->d_y[gi], h->d_th[gi], u.n);
    if (!rc) rc = weights_and_cdf(h);
    h->graph_guide[gi] = h->guide_pending;          // (what the captured scan writes, at every replay)
    hipError_t ce = hipSuccess;
    if (!rc) ce = hipMemcpyAsync(h->h_result, h->d_result, kResultWords * 8, hipMemcpyDeviceToHost, h->stream);
    h->capturing = false;
    const hipError_t ee = hipStreamEndCapture(h->stream, &graph);
    hipError_t ie = hipErrorUnknown;
    if (!rc && ce == hipSuccess && ee == hipSuccess && graph && h->last_mode == MCL_RAYS_SKIP)
        ie = hipGraphInstantiate(&h->graph_exec[gi], graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (ie == hipSuccess) return true;
    h->graph_exec[gi] = nullptr;
    graph_reset(h);
    (void)hipGetLastError();
    h->cfg.graph_mode = 1;          // do not try again on this engine
    return false;
}

// Phase 3, the captured tail: one graph launch and one wait.
static int tail_graph(mcl_engine *h, const Update &u)
{
    HIPCHK(h, hipGraphLaunch(h->graph_exec[h->cur], h->stream));
    ray_handoff_void(h);                   // (the replayed ray stage took the constants)
    if (h->mounted) { h->sp_valid = true; h->sp_n = u.n; }      // (... and the replayed k_mount_poses wrote these children's sensor poses)
    HIPCHK(h, hipEventRecord(h->ev[EV_SENSOR], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->compact_pending = h->d_ccdf != nullptr && !h->env.no_compact && u.n > mcl::kTinyTailMax;   // the captured scan wrote a list
    h->guide_valid = false; h->guide_pending = h->compact_pending && h->graph_guide[h->cur];       // ... and, if it did at capture, the guide
    unpack_result(h);
    h->carry_pending = false;
    // the captured tail is one unit: its time is reported as the ray-cast stage (query prep and table evaluation
    // are inside it), so that the six stages still add up to the total the host uses for delay compensation
    h->timings[0] = elapsed(h->ev[EV_START], h->ev[EV_RESAMPLE]);
    h->timings[1] = 0.0; h->timings[2] = 0.0; h->timings[4] = 0.0;
    h->timings[3] = elapsed(h->ev[EV_RESAMPLE], h->ev[EV_SENSOR]);      // the graph as a whole
    h->ray_ms_is_graph_tail = true;
    return MCL_OK;
}

// adaptive resampling kept the set: the previous update's log-weights (minus their maximum) add to this one's
static void add_carry(mcl_engine *h, int64_t n)
{
    hipLaunchKernelGGL(mcl::k_add_carry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_logw, h->d_carry[h->carry_idx], n);
    h->max_partials_ready = false;
}

// mcl_sensor_update_fuse: the log-weights the previous weighting call left for these particles add to this scan's
static void add_prev_logw(mcl_engine *h, int64_t n);

// Phase 3, launch by launch: every regular update, and the first of a configuration (which leaves graph_warm).
static int tail_launches(mcl_engine *h, const Update &u)
{
    h->ray_ms_is_graph_tail = false;
    h->stage_ev = {};
    if (h->lf_on) {
        // the likelihood field: no observation tables, no ordering, no ray stage; k_lfield writes d_logw
        MCL_TRY(launch_lfield(h, u.obs, u.obs_stride, u.n));
    } else {
        // (tables made beside the ordering: the ordering kernels of the ray stage do not read them either, so the stream waits for them
        //  where the ray kernel is launched -- launch_rays --, not here: 13 us of a 262 144-particle update; and there is no
        //  query-preparation stage on this stream, nothing to time)
        h->handoff.obs_wait = h->stage_ev.query_skipped = u.obs_early;
        if (!u.obs_early) {
            MCL_TRY(prepare_observation(h, u.obs, u.obs_stride));
            HIPCHK(h, hipEventRecord(h->ev[EV_QUERY], h->stream));
        }
        const int rc = launch_rays(h, h->d_x[h->cur], h->d_y[h->cur], h->d_th[h->cur], u.n);
        if (h->handoff.obs_wait) { h->handoff.obs_wait = false; HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_obs, 0)); }      // (a path that launched no windowed kernel)
        MCL_TRY(rc);
        MCL_TRY(next_layout_launch(h, u.n));      // (second stream; behind the ray stage in submission order, beside it on the device)
    }
    if (u.keep) add_carry(h, u.n);
    if (u.fuse) add_prev_logw(h, u.n);
    if (u.keep || u.fuse || !h->stage_ev.rays_bound) HIPCHK(h, hipEventRecord(h->ev[EV_RAYS], h->stream));
    MCL_TRY(close_sensor_stage(h, true));
    MCL_TRY(fetch_scalars(h));             // one D2H copy (scalars, counters, overflow flag); synchronises the stream
    if (fix_lists_overflowed(h)) {
        // more undecided rays than the work list holds (only with debug_force_exact at large sizes or a
        // pathological map): redo the ray stage with the self-contained k_rays_skip
        HIPCHK(h, hipMemsetAsync(h->d_counters, 0, 4 * sizeof(unsigned long long), h->stream));
        MCL_TRY(launch_rays(h, h->d_x[h->cur], h->d_y[h->cur], h->d_th[h->cur], u.n, true));
        if (u.keep) add_carry(h, u.n);
        if (u.fuse) add_prev_logw(h, u.n);
        MCL_TRY(weights_and_cdf(h));
        MCL_TRY(fetch_scalars(h));
    }
    if (h->carry_pending) { h->carry_idx ^= 1; h->carry_valid = true; h->carry_pending = false; }   // this update's logw - max
    MCL_TRY(layout_adopt(h, u.n));
    h->graph_warm = true;                  // every buffer this configuration needs exists now
    h->timings[0] = elapsed(h->ev[EV_START], h->ev[EV_RESAMPLE]);
    h->timings[1] = 0.0;                   // motion is fused into the resample/gather kernel
    h->timings[2] = h->stage_ev.query_skipped ? 0.0 : elapsed(h->ev[EV_RESAMPLE], h->ev[EV_QUERY]);
    h->timings[3] = elapsed(h->ev[h->stage_ev.query_skipped ? EV_RESAMPLE : EV_QUERY], h->ev[EV_RAYS]);
    h->timings[4] = elapsed(h->ev[EV_RAYS], h->ev[EV_SENSOR]);
    return MCL_OK;
}

// Phase 4: what every tail ends in, once the update's result block has been unpacked.
static void finish_update(mcl_engine *h, const Update &u)
{
    if (u.kld) kld_decide(h, u.keep);
    if (!u.fuse) recov_after(h, u.rec, u.keep, u.prev_sum_w, u.n);      // (a fused scan folds nothing into the averages)
    h->have_logw = true;
    h->weighted = true;
    h->have_steps = h->cfg.keep_ray_steps != 0 && !h->lf_on;
    if (u.resample_and_move) h->update_idx++;
    h->timings[5] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - u.t0).count();
    if (u.tiny) h->timings[3] = h->timings[5];
    h->ray_ms = h->ray_ms_is_graph_tail ? h->timings[3] : elapsed(h->ev[EV_K0], h->ev[EV_K1]);
}

static int do_update(mcl_engine_t *h, const double action[3], const float *obs, int32_t n_beams, const double *normals,
                     const double *uniforms, bool resample_and_move, int obs_stride = 1, bool fuse = false)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    h->set_epoch++;                         // (the labels of a clustering are void from here on)
    if (!ready(h, true)) return fail(h, MCL_ERR_NOT_READY, "map, beam angles and particles must be set first");
    if (!obs || n_beams != h->B || (resample_and_move && !action)) return fail(h, MCL_ERR_INVALID_ARG, "bad action/observation");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    Update u{action, obs, obs_stride, uniforms, resample_and_move, std::chrono::steady_clock::now()};     // (the rest: zero)
    u.fuse = fuse;
    h->weighted = false;                    // (until this update has formed its weights: finish_update)
    MCL_TRY(plan_update(h, u));
    const double *d_norm = nullptr, *d_uni = nullptr;
    if (resample_and_move) {
        if (normals) {
            HIPCHK(h, hipMemcpyAsync(h->d_inject, normals, (size_t)u.n * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
            d_norm = h->d_inject;
        }
        if (uniforms) {
            HIPCHK(h, hipMemcpyAsync(h->d_inject + (size_t)3 * h->cap, uniforms, (size_t)u.n * sizeof(double), hipMemcpyHostToDevice, h->stream));
            d_uni = h->d_inject + (size_t)3 * h->cap;
        }
    }
    if (!resample_and_move) HIPCHK(h, hipMemsetAsync(h->d_counters, 0, 4 * sizeof(unsigned long long), h->stream));   // else: the resampling kernel
    if (u.n != u.n_par) {
        // another size: nothing made for the old one is reused (captured graphs, the warm small-update paths, the previous
        // update's ordering layout, the cleared-word cache), as when the particles are set from outside
        graph_reset(h);
        h->far_fresh = true;
    }
    if (u.rec) h->far_fresh = true;        // injected children anywhere on the map: the ray stage plans as for a set from outside
    h->recov_cnt_slot = -1; h->recov_injected = 0;
    ray_handoff_void(h);                   // (written by this update's resampling launch, if it has one)
    if (!u.tiny) HIPCHK(h, hipEventRecord(h->ev[EV_START], h->stream));
    if (resample_and_move) MCL_TRY(launch_update_resample(h, u, d_norm, d_uni));
    if (!u.tiny && !u.resample_bound) HIPCHK(h, hipEventRecord(h->ev[EV_RESAMPLE], h->stream));
    MCL_TRY(u.tiny ? tail_tiny(h, u) : (u.graph_ok && graph_ready(h, u)) ? tail_graph(h, u) : tail_launches(h, u));
    finish_update(h, u);
    return MCL_OK;
}

int mcl_update(mcl_engine_t *h, const double action[3], const float *obs, int32_t n_beams, const double *normals_nx3,
               const double *uniforms_n)
{
    return do_update(h, action, obs, n_beams, normals_nx3, uniforms_n, true);
}

int mcl_sensor_update(mcl_engine_t *h, const float *obs, int32_t n_beams)
{
    return do_update(h, nullptr, obs, n_beams, nullptr, nullptr, false);
}

int mcl_sensor_update_fuse(mcl_engine_t *h, const float *obs, int32_t n_beams)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_UNSUPPORTED, "sensor_update_fuse: weight_mode LOG only");
    if (h->comm || h->in_group) return fail(h, MCL_ERR_UNSUPPORTED, "sensor_update_fuse is single-engine only (not with a communicator or in a device group)");
    if (!ready(h, true)) return fail(h, MCL_ERR_NOT_READY, "map, beam angles and particles must be set first");
    if (!obs || n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "bad action/observation");
    if (!h->weighted || !h->have_logw)
        return fail(h, MCL_ERR_NOT_READY, "sensor_update_fuse: the last weighting call (mcl_update*, mcl_sensor_update) was not on the current particle set");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    MCL_TRY(h->d_logw_prev.reserve(h, (size_t)h->cap));
    HIPCHK(h, hipMemcpyAsync(h->d_logw_prev, h->d_logw, (size_t)h->N * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return do_update(h, nullptr, obs, n_beams, nullptr, nullptr, false, 1, true);
}

int mcl_update_scan(mcl_engine_t *h, const double action[3], const float *ranges, int32_t n_ranges, int32_t angle_step)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!ranges || angle_step <= 0 || n_ranges <= 0) return fail(h, MCL_ERR_INVALID_ARG, "bad scan");
    int32_t nb = (n_ranges + angle_step - 1) / angle_step;            // cpp:317: i = 0, ANGLE_STEP, ...
    return do_update(h, action, ranges, nb, nullptr, nullptr, true, angle_step);
}

int mcl_get_planned_ray_kernel(const mcl_engine_t *h, int64_t n_particles, int32_t *kernel, const char **reason)
{
    if (!h || !kernel) return MCL_ERR_INVALID_ARG;
    if (!h->have_map || h->B <= 0) return MCL_ERR_NOT_READY;
    const int64_t n = n_particles > 0 ? n_particles : (h->have_particles ? h->N : h->cap);
    const char *why = "";
    *kernel = choose_ray_mode(h, n, false, &why);
    if (reason) *reason = why ? why : "";
    return MCL_OK;
}

// ---- odometry motion models and the Gaussian pose initialisation (the header's M1-M6 / G1) ----
int mcl_init_particles_gaussian(mcl_engine_t *h, const double mean[3], const double cov[9], int64_t n, int64_t first_global_index,
                                int64_t n_total)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    MCL_TRY(check_init(h, mean && cov, n, first_global_index, n_total));
    double L[6];
    if (const char *why = gaussian_factor(cov, L)) return fail(h, MCL_ERR_INVALID_ARG, why);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int c = h->cur;
    hipLaunchKernelGGL(mcl::k_init_gaussian, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, mean[0], mean[1], mean[2], L[0],
                       L[1], L[2], L[3], L[4], L[5], n, first_global_index, (uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32), h->init_idx,
                       h->d_x[c], h->d_y[c], h->d_th[c]);
    HIPCHK(h, hipGetLastError());
    return finish_init(h, n, n_total);
}

int mcl_init_particles_mixture(mcl_engine_t *h, int32_t n_components, const double *means, const double *covs, const int64_t *counts,
                               int64_t n, int64_t first_global_index, int64_t n_total)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    MCL_TRY(check_init(h, means && covs && counts, n, first_global_index, n_total));
    if (n_components < 1 || n_components > 4096) return fail(h, MCL_ERR_INVALID_ARG, "mixture init: n_components must be in [1, 4096]");
    if (first_global_index + n > n_total) return fail(h, MCL_ERR_INVALID_ARG, "mixture init: the shard ends beyond n_total");
    std::vector<mcl::MixComponent> comp((size_t)n_components);
    int64_t sum = 0;
    for (int c = 0; c < n_components; ++c) {
        const std::string who = "mixture init, component " + std::to_string(c) + ": ";
        if (counts[c] < 0 || counts[c] > n_total) return fail(h, MCL_ERR_INVALID_ARG, who + "its count must be in [0, n_total]");
        sum += counts[c];
        comp[(size_t)c].end = sum;
        for (int k = 0; k < 3; ++k) comp[(size_t)c].mean[k] = means[3 * c + k];
        if (const char *why = gaussian_factor(covs + 9 * (size_t)c, comp[(size_t)c].l)) return fail(h, MCL_ERR_INVALID_ARG, who + why);
    }
    if (sum != n_total) return fail(h, MCL_ERR_INVALID_ARG, "mixture init: the counts must add up to n_total");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    DevBuf<mcl::MixComponent> d_comp;
    MCL_TRY(d_comp.reserve(h, comp.size()));
    int rc = MCL_OK;
    if (hipMemcpy(d_comp, comp.data(), comp.size() * sizeof(mcl::MixComponent), hipMemcpyHostToDevice) != hipSuccess) rc = MCL_ERR_HIP;
    if (rc == MCL_OK) {
        const int c = h->cur;
        hipLaunchKernelGGL(mcl::k_init_mixture, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d_comp, n_components, n,
                           first_global_index, (uint32_t)h->cfg.seed, (uint32_t)(h->cfg.seed >> 32), h->init_idx, h->d_x[c], h->d_y[c], h->d_th[c]);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) rc = MCL_ERR_HIP;
    }
    if (rc != MCL_OK) return fail(h, rc, "mixture init: uploading the components or the draw failed");
    return finish_init(h, n, n_total);
}

int mcl_set_likelihood_field(mcl_engine_t *h, const mcl_likelihood_field_config_t *c)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (c) {
        MCL_TRY(refuse_shared(h, "the likelihood field"));
        if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_UNSUPPORTED, "the likelihood field needs weight_mode LOG");
        if (const char *why = lf_invalid(c)) return fail(h, MCL_ERR_INVALID_ARG, why);
        if (h->have_map && lf_cap(c, (float)h->res) < 0)
            return fail(h, MCL_ERR_INVALID_ARG, "likelihood field: K = ceil((max_occ_dist_m / resolution)^2) exceeds 65535 on this map");
    }
    // either way, what the beam model's updates keep between updates (captured graphs, the warm small-update paths, the ordering
    // layout, the cleared-word cache, the far-pass state) is dropped: the next update plans as after mcl_set_particles
    graph_reset(h);
    h->far_fresh = true;
    if (!c) {
        h->lf_on = false;
        h->bs_on = h->bs_have = false;       // (beam skipping cannot be on without the field)
        return MCL_OK;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->lf = *c;
    h->lf_on = true;
    h->lf_K = -1;
    if (h->have_map) {
        const int rc = lf_build(h);
        if (rc) { h->lf_on = false; h->bs_on = h->bs_have = false; return rc; }
    }
    return MCL_OK;
}

// ---------------------------------------------------------------------------------------------
// multi-GPU staging
// ---------------------------------------------------------------------------------------------
int mcl_device_ptr(mcl_engine_t *h, int32_t which, void **p)
{
    if (!h || !p) return MCL_ERR_INVALID_ARG;
    switch (which) {
    case MCL_BUF_X: *p = h->d_x[h->cur]; break;
    case MCL_BUF_Y: *p = h->d_y[h->cur]; break;
    case MCL_BUF_THETA: *p = h->d_th[h->cur]; break;
    case MCL_BUF_QWEIGHT: *p = h->d_q; break;
    case MCL_BUF_LOGW: *p = h->d_logw; break;
    case MCL_BUF_SCALARS: *p = h->d_scalars; break;
    default: return MCL_ERR_INVALID_ARG;
    }
    return MCL_OK;
}

int mcl_export_state(mcl_engine_t *h, double *d_x, double *d_y, double *d_theta, uint64_t *d_q)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t nb = (size_t)h->N * 8;
    const int c = h->cur;
    if (d_x) HIPCHK(h, hipMemcpyAsync(d_x, h->d_x[c], nb, hipMemcpyDeviceToDevice, h->stream));
    if (d_y) HIPCHK(h, hipMemcpyAsync(d_y, h->d_y[c], nb, hipMemcpyDeviceToDevice, h->stream));
    if (d_theta) HIPCHK(h, hipMemcpyAsync(d_theta, h->d_th[c], nb, hipMemcpyDeviceToDevice, h->stream));
    if (d_q) HIPCHK(h, hipMemcpyAsync(d_q, h->d_q, nb, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_export_records(mcl_engine_t *h, void *d_records)
{
    if (!h || !d_records) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int c = h->cur;
    const int64_t n = h->N;
    if (h->pack_valid[c]) {
        HIPCHK(h, hipMemcpyAsync(d_records, h->d_pack[c], (size_t)n * sizeof(double4), hipMemcpyDeviceToDevice, h->stream));
    } else {
        hipLaunchKernelGGL(mcl::k_pack_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_x[c], h->d_y[c], h->d_th[c], n,
                           reinterpret_cast<double4 *>(d_records));
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_export_records_at(mcl_engine_t *h, const int64_t *d_index, int64_t count, void *d_out)
{
    if (!h || count < 0 || (count > 0 && (!d_index || !d_out))) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    if (count == 0) return MCL_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int c = h->cur;
    const int64_t n = h->N;
    if (!h->pack_valid[c]) {
        hipLaunchKernelGGL(mcl::k_pack_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_x[c], h->d_y[c], h->d_th[c], n, h->d_pack[c]);
        h->pack_valid[c] = true;
    }
    hipLaunchKernelGGL(mcl::k_gather_records, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, h->d_pack[c], d_index, count, n,
                       reinterpret_cast<double4 *>(d_out));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_stage_distinct_parents(mcl_engine_t *h, const int32_t *d_parent, int64_t n_children, int64_t n_total, int64_t *d_distinct,
                               int32_t *d_slot, int64_t *count)
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h || !d_parent || !d_distinct || !d_slot || !count || n_children <= 0 || n_total <= 0) return MCL_ERR_INVALID_ARG;
    if (n_total > MCL_MAX_TOTAL_PARTICLES) return fail(h, MCL_ERR_INVALID_ARG, "n_total exceeds MCL_MAX_TOTAL_PARTICLES");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t nwords = (n_total + 31) / 32;
    MCL_TRY(h->d_bm.reserve(h, (size_t)nwords));
    MCL_TRY(h->d_bm_pop.reserve(h, (size_t)nwords));
    MCL_TRY(h->d_bm_pref.reserve(h, (size_t)nwords));
    MCL_TRY(reserve_scan_spine(h, nwords));
    HIPCHK(h, hipMemsetAsync(h->d_bm, 0, (size_t)nwords * 4, h->stream));
    hipLaunchKernelGGL(mcl::k_bm_mark, dim3((unsigned)((n_children + 255) / 256)), dim3(256), 0, h->stream, d_parent, n_children, n_total, h->d_bm);
    hipLaunchKernelGGL(mcl::k_bm_pop, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, h->stream, h->d_bm, nwords, h->d_bm_pop);
    MCL_TRY(scan_weights(h, h->d_bm_pop, h->d_bm_pref, nwords, 0, nullptr));
    h->blocktot_for = nullptr;                  // the spine now describes the bitmap's prefix, not a CDF
    hipLaunchKernelGGL(mcl::k_bm_expand, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, h->stream, h->d_bm, h->d_bm_pref, nwords, d_distinct);
    hipLaunchKernelGGL(mcl::k_bm_slot, dim3((unsigned)((n_children + 255) / 256)), dim3(256), 0, h->stream, d_parent, n_children, n_total, h->d_bm,
                       h->d_bm_pref, d_slot);
    HIPCHK(h, hipGetLastError());
    uint64_t c = 0;
    HIPCHK(h, hipMemcpyAsync(&c, h->d_bm_pref + (nwords - 1), 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *count = (int64_t)c;
    return MCL_OK;
}

// Launches the staged resample (+ motion) on the engine's stream; no synchronisation.  An index-only pass leaves the
// engine untouched; otherwise the children land in the other particle buffer, which becomes current.
int mcl_host::stage_resample_launch(mcl_engine_t *h, const ParentSource &src, const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total,
                                 int64_t child_first, int64_t n_children_total, const double action[3])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    h->set_epoch++;                         // (the labels of a clustering are void from here on)
    if (!ready(h, true)) return fail(h, MCL_ERR_NOT_READY, "map, beam angles and particles must be set first");
    const bool have_parents = src.records || src.n_per_rank > 0 || (src.px && src.py && src.pth) || src.idx_only_out || src.gcdf;
    if (!have_parents || (!d_cdf && !src.idx_in && !src.gcdf && !src.keep) || (!action && !src.idx_only_out) || n_parents <= 0 ||
        n_parents >= MCL_MAX_TOTAL_PARTICLES || n_children_total >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "bad stage_resample arguments (totals must stay below 2^27)");
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG)
        return fail(h, MCL_ERR_UNSUPPORTED, "the staged (sharded) flow needs weight_mode LOG");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t n = h->N;
    const bool index_only = src.idx_only_out != nullptr;
    if (!index_only) {
        HIPCHK(h, hipMemsetAsync(h->d_counters, 0, 4 * sizeof(unsigned long long), h->stream));
        HIPCHK(h, hipEventRecord(h->ev[EV_START], h->stream));
    }
    const int nx = h->cur ^ 1;
    mcl::ResampleArgs a{};
    a.px = src.px; a.py = src.py; a.pth = src.pth; a.q_total = q_total;
    resample_common_args(h, a, d_cdf, n_parents);
    a.ppack = reinterpret_cast<const double4 *>(src.records);
    for (int r = 0; r < mcl::kMaxShards; ++r) a.ppack_rank[r] = src.rank_records[r];
    a.n_per_rank = src.n_per_rank; a.self_rank = src.self_rank; a.remote_count = src.remote_count;
    a.idx_in = src.idx_in; a.index_only = index_only ? 1 : 0;
    a.cpack = h->d_pack[nx];
    if (src.gcdf) {
        a.ccdf = src.gcdf; a.ctop = src.gtop; a.n_compact = n_parents; a.cchunks = src.cchunks;
        a.ccap = src.cchunk_entries; a.cchunk_bytes = src.cchunk_entries * kCompactEntryBytes;
        a.cpack = nullptr;
    }
    a.idx_out = src.idx_in ? nullptr : h->d_idx;       // the global parents of an earlier index-only pass stay in d_idx
    a.n_children = n; a.child_first = child_first; a.n_children_total = n_children_total;
    if (action) motion_scalars(action, a.dt, a.v, a.w);
    a.do_resample = src.keep ? 0 : 1;
    a.idx_out_base = src.keep ? child_first : 0;
    ray_handoff_void(h);
    // as in mcl_update: the ray stage's per-particle constants, its zeroed scratch and (by the previous update's layout) the sort
    // keys come out of this kernel; the layout of these children is made on the second stream for the next update
    if (!index_only) resample_ray_extras(h, n, a);
    mcl::OdoArgs odo_cur{};
    const bool odo = !index_only && odo_args_of(h, action, odo_cur);       // (an index-only pass moves nothing)
    (void)launch_resample(h, dim3((unsigned)((n + 255) / 256)), 0, !index_only, a, nullptr, nullptr, nullptr, odo ? &odo_cur : nullptr);   // (bound: the staged flow reads EV_RESAMPLE itself)
    HIPCHK(h, hipGetLastError());
    if (a.pc_out) MCL_TRY(layout_mark(h, n));
    if (index_only) {
        HIPCHK(h, hipMemcpyAsync(src.idx_only_out, h->d_idx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
        h->have_idx = true;
        return MCL_OK;
    }
    h->cur = nx;
    h->pack_valid[nx] = a.cpack != nullptr;
    h->compact_used = src.gcdf != nullptr;
    h->guide_used = false;
    h->have_idx = true;
    h->have_logw = false;
    h->sp_valid = h->weighted = false;
    h->resampled_last = !src.keep;
    h->stage_kept = src.keep;              // mcl_stage_rays adds the previous update's log-weights (minus their maximum)
    h->update_idx++;
    return MCL_OK;
}

static int stage_resample_sync(mcl_engine_t *h, const ParentSource &src, const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total,
                               int64_t child_first, int64_t n_children_total, const double action[3])
{
    MCL_TRY(stage_resample_launch(h, src, d_cdf, n_parents, q_total, child_first, n_children_total, action));
    HIPCHK(h, hipStreamSynchronize(h->stream));           // the children (or the indices) are final: the host may export / gather them now
    return MCL_OK;
}

int mcl_stage_resample(mcl_engine_t *h, const double *d_px, const double *d_py, const double *d_pth, const uint64_t *d_cdf,
                       int64_t n_parents, uint64_t q_total, int64_t child_first, int64_t n_children_total, const double action[3])
{
    if (const int rc = refuse_stage(h)) return rc;
    ParentSource src; src.px = d_px; src.py = d_py; src.pth = d_pth;
    if (!d_px || !d_py || !d_pth) return h ? fail(h, MCL_ERR_INVALID_ARG, "bad stage_resample arguments") : MCL_ERR_INVALID_ARG;
    return stage_resample_sync(h, src, d_cdf, n_parents, q_total, child_first, n_children_total, action);
}

int mcl_stage_resample_records(mcl_engine_t *h, const void *d_records, const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total,
                               int64_t child_first, int64_t n_children_total, const double action[3])
{
    if (const int rc = refuse_stage(h)) return rc;
    ParentSource src; src.records = d_records;
    if (!d_records) return h ? fail(h, MCL_ERR_INVALID_ARG, "bad stage_resample arguments") : MCL_ERR_INVALID_ARG;
    return stage_resample_sync(h, src, d_cdf, n_parents, q_total, child_first, n_children_total, action);
}

int mcl_stage_resample_indices(mcl_engine_t *h, const uint64_t *d_cdf, int64_t n_parents, uint64_t q_total, int64_t child_first,
                               int64_t n_children_total, int32_t *d_parent_idx)
{
    if (const int rc = refuse_stage(h)) return rc;
    ParentSource src; src.idx_only_out = d_parent_idx;
    if (!d_parent_idx || !d_cdf) return h ? fail(h, MCL_ERR_INVALID_ARG, "bad stage_resample_indices arguments") : MCL_ERR_INVALID_ARG;
    return stage_resample_sync(h, src, d_cdf, n_parents, q_total, child_first, n_children_total, nullptr);
}

int mcl_stage_motion_records(mcl_engine_t *h, const void *d_records, int64_t n_records, const int32_t *d_record_of_child, int64_t child_first,
                             int64_t n_children_total, const double action[3])
{
    if (const int rc = refuse_stage(h)) return rc;
    ParentSource src; src.records = d_records; src.idx_in = d_record_of_child;
    if (!d_records || !d_record_of_child || n_records <= 0) return h ? fail(h, MCL_ERR_INVALID_ARG, "bad stage_motion_records arguments") : MCL_ERR_INVALID_ARG;
    return stage_resample_sync(h, src, nullptr, n_records, 0, child_first, n_children_total, action);
}

// ---- sharded sets: the shards exchange their compact lists instead of every weight --------------------------------
int mcl_host::export_compact_launch(mcl_engine_t *h, void *d_chunk, int64_t chunk_entries, int dst_device, hipStream_t stream)
{
    if (!h || !d_chunk || chunk_entries <= 0 || (chunk_entries & 63)) return MCL_ERR_INVALID_ARG;
    if (h->compact_n < 0 || h->compact_n > chunk_entries) return fail(h, MCL_ERR_NOT_READY, "no compact list of that size (mcl_get_compact_list)");
    if (h->compact_n == 0) return MCL_OK;
    unsigned char *c = static_cast<unsigned char *>(d_chunk);
    const size_t n = (size_t)h->compact_n, cap = (size_t)chunk_entries;
    const int src = h->cfg.device;
    HIPCHK(h, hipMemcpyPeerAsync(c, dst_device, h->d_ccdf, src, n * 8, stream));
    HIPCHK(h, hipMemcpyPeerAsync(c + cap * 8, dst_device, h->d_crec, src, n * 32, stream));
    HIPCHK(h, hipMemcpyPeerAsync(c + cap * 40, dst_device, h->d_cidx, src, n * 4, stream));
    return MCL_OK;
}

int mcl_export_compact(mcl_engine_t *h, void *d_chunk, int64_t chunk_entries)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    MCL_TRY(export_compact_launch(h, d_chunk, chunk_entries, h->cfg.device, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

// merge of the gathered chunks + staged resample from them, on the engine's stream; no synchronisation
int mcl_host::stage_resample_compact_launch(mcl_engine_t *h, const void *d_chunks, int32_t n_shards, int64_t chunk_entries, const int64_t *counts,
                                         const uint64_t *totals, int64_t n_per_shard, int32_t self_shard, int64_t child_first,
                                         int64_t n_children_total, const double action[3], unsigned long long *remote_count)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!d_chunks || !counts || !totals || n_shards <= 0 || n_shards > mcl::kMaxShards || chunk_entries <= 0 || (chunk_entries & 63) || n_per_shard <= 0 ||
        self_shard < 0 || self_shard >= n_shards)
        return fail(h, MCL_ERR_INVALID_ARG, "bad stage_resample_compact arguments");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    mcl::MergeArgs m{};
    m.chunks = static_cast<const unsigned char *>(d_chunks); m.chunk_bytes = chunk_entries * kCompactEntryBytes; m.ccap = chunk_entries; m.n_shards = n_shards;
    uint64_t off = 0;
    for (int r = 0; r < n_shards; ++r) {
        if (counts[r] < 0 || counts[r] > chunk_entries) return fail(h, MCL_ERR_INVALID_ARG, "a list is longer than its chunk");
        m.count[r] = (uint32_t)counts[r]; m.off[r] = off; m.tot[r] = counts[r] > 0 ? totals[r] : 0ull;
        off += m.tot[r];
    }
    if (off == 0) return fail(h, MCL_ERR_INVALID_ARG, "the lists carry no weight");
    const size_t total = (size_t)n_shards * (size_t)chunk_entries;
    if (total >= (size_t)MCL_MAX_TOTAL_PARTICLES) return fail(h, MCL_ERR_INVALID_ARG, "gathered lists exceed 2^27 entries");
    MCL_TRY(h->d_gcdf.reserve(h, total));
    MCL_TRY(h->d_gtop.reserve(h, total / 64 + 1));
    m.gcdf = h->d_gcdf; m.gtop = h->d_gtop;
    hipLaunchKernelGGL(mcl::k_compact_merge, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, m);
    HIPCHK(h, hipGetLastError());
    ParentSource src;
    src.cchunks = m.chunks; src.cchunk_entries = chunk_entries; src.gcdf = h->d_gcdf; src.gtop = h->d_gtop;
    src.n_per_rank = n_per_shard; src.self_rank = self_shard; src.remote_count = remote_count;
    return stage_resample_launch(h, src, nullptr, (int64_t)total, off, child_first, n_children_total, action);
}

int mcl_stage_resample_compact(mcl_engine_t *h, const void *d_chunks, int32_t n_shards, int64_t chunk_entries, const int64_t *counts,
                               const uint64_t *totals, int64_t n_per_shard, int32_t self_shard, int64_t child_first, int64_t n_children_total,
                               const double action[3])
{
    if (const int rc = refuse_stage(h)) return rc;
    MCL_TRY(stage_resample_compact_launch(h, d_chunks, n_shards, chunk_entries, counts, totals, n_per_shard, self_shard, child_first,
                                          n_children_total, action, nullptr));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_host::stage_rays_launch(mcl_engine_t *h, const float *obs, int32_t n_beams, bool force_skip, double *d_max_out)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!ready(h, true)) return fail(h, MCL_ERR_NOT_READY, "map, beam angles and particles must be set first");
    if (!obs || n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "bad observation");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int64_t n = h->N;
    const int c = h->cur;
    if (!force_skip) {
        MCL_TRY(prepare_observation(h, obs, 1));
        HIPCHK(h, hipEventRecord(h->ev[EV_QUERY], h->stream));
    } else {
        HIPCHK(h, hipMemsetAsync(h->d_counters, 0, 4 * sizeof(unsigned long long), h->stream));
    }
    if (!h->handoff.constants) ray_handoff_void(h);     // no staged resampling before this call: nothing prepared
    h->stage_ev.rays_bound = false;
    h->weighted = false;                    // (d_logw is rewritten by a staged stage: mcl_sensor_update_fuse has nothing to add to)
    MCL_TRY(launch_rays(h, h->d_x[c], h->d_y[c], h->d_th[c], n, force_skip));
    MCL_TRY(next_layout_launch(h, n));
    if (h->stage_kept) {
        add_carry(h, n);
        HIPCHK(h, hipEventRecord(h->ev[EV_RAYS], h->stream));
    } else if (!h->stage_ev.rays_bound) HIPCHK(h, hipEventRecord(h->ev[EV_RAYS], h->stream));
    if (!h->max_partials_ready)
        hipLaunchKernelGGL(mcl::k_reduce_max, dim3(mcl::kRedBlocks), dim3(mcl::kRedThreads), 0, h->stream, h->d_logw, n, h->d_maxpart);
    hipLaunchKernelGGL(mcl::k_final_max, dim3(1), dim3(mcl::kRedThreads), 0, h->stream, h->d_maxpart, mcl::kRedBlocks, h->d_scalars, d_max_out);
    h->max_partials_ready = false;
    HIPCHK(h, hipGetLastError());
    if (!d_max_out)          // (the device-ordered flows read the result block once, after the weights)
        HIPCHK(h, hipMemcpyAsync(h->h_result, h->d_result, kResultWords * 8, hipMemcpyDeviceToHost, h->stream));
    return MCL_OK;
}

// the host-side notes of a finished ray stage (its stream has been waited for)
void mcl_host::stage_rays_note(mcl_engine_t *h)
{
    h->have_logw = true;
    h->have_steps = h->cfg.keep_ray_steps != 0;
    h->timings[0] = elapsed(h->ev[EV_START], h->ev[EV_RESAMPLE]);
    h->timings[1] = 0.0;
    h->timings[2] = 0.0;
    h->timings[3] = elapsed(h->ev[EV_QUERY], h->ev[EV_RAYS]);
    h->ray_ms = elapsed(h->ev[EV_K0], h->ev[EV_K1]);
}

int mcl_host::stage_rays_finish(mcl_engine_t *h, const float *obs, int32_t n_beams)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    for (int attempt = 0; attempt < 2; ++attempt) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::memcpy(h->h_scalars, h->h_result, 8 * sizeof(double));       // [0] = local max log-weight (mcl_get_host_scalars)
        std::memcpy(h->h_counters, h->h_result + 8, 4 * sizeof(unsigned long long));
        h->h_fix_count = h->h_result[12];
        if (!fix_lists_overflowed(h) || attempt == 1) break;
        // work-list overflow (only with debug_force_exact at large sizes): once more with the self-contained k_rays_skip
        MCL_TRY(stage_rays_launch(h, obs, n_beams, true));
    }
    stage_rays_note(h);
    return MCL_OK;
}

int mcl_stage_rays(mcl_engine_t *h, const float *obs, int32_t n_beams)
{
    if (const int rc = refuse_stage(h)) return rc;
    MCL_TRY(stage_rays_launch(h, obs, n_beams, false));
    return stage_rays_finish(h, obs, n_beams);
}

int mcl_stage_propagate(mcl_engine_t *h, const double *d_px, const double *d_py, const double *d_pth, const uint64_t *d_cdf,
                        int64_t n_parents, uint64_t q_total, int64_t child_first, int64_t n_children_total,
                        const double action[3], const float *obs, int32_t n_beams)
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!obs || n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "bad observation");
    MCL_TRY(mcl_stage_resample(h, d_px, d_py, d_pth, d_cdf, n_parents, q_total, child_first, n_children_total, action));
    return mcl_stage_rays(h, obs, n_beams);
}

// d_global_max: the global maximum in device memory (the device-ordered flow: the log-weights need not have been seen by the
// host yet), else the host's value is staged
int mcl_host::stage_weights_launch(mcl_engine_t *h, double global_max_logw, const double *d_global_max)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    h->set_epoch++;                         // (the labels of a clustering are void from here on)
    if (!h->have_logw && !d_global_max) return MCL_ERR_NOT_READY;
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG)
        return fail(h, MCL_ERR_UNSUPPORTED, "the staged (sharded) flow needs weight_mode LOG");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (d_global_max) {
        hipLaunchKernelGGL(mcl::k_copy_double, dim3(1), dim3(1), 0, h->stream, d_global_max, h->d_scalars);
    } else {
        h->h_result[kResultStage] = 0;
        std::memcpy(&h->h_result[kResultStage], &global_max_logw, sizeof(double));   // pinned: stays valid until the copy has run
        HIPCHK(h, hipMemcpyAsync(h->d_scalars, &h->h_result[kResultStage], sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    MCL_TRY(weight_stats(h, true, h->d_scalars, true));        // (the scan below finishes the sums)
    // (adaptive resampling: the carry this wrote -- logw minus the GLOBAL maximum -- becomes current in mcl_stage_finish, once the
    //  host knows that the update is not redone from the ray stage on)
    // the shard's own CDF follows its new weights: mcl_sample_particles (visualize) and a later plain mcl_update search it
    MCL_TRY(close_sensor_stage(h, false));
    HIPCHK(h, hipMemcpyAsync(h->h_result, h->d_result, kResultWords * 8, hipMemcpyDeviceToHost, h->stream));
    return MCL_OK;
}

int mcl_host::stage_weights_finish(mcl_engine_t *h)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_result(h);
    h->timings[4] = elapsed(h->ev[EV_RAYS], h->ev[EV_SENSOR]);
    return layout_adopt(h, h->N);
}

int mcl_stage_weights(mcl_engine_t *h, double global_max_logw)
{
    if (const int rc = refuse_stage(h)) return rc;
    MCL_TRY(stage_weights_launch(h, global_max_logw));
    return stage_weights_finish(h);
}

// end of a staged update: the carry its weights stage wrote becomes the current one
void mcl_host::stage_commit_carry(mcl_engine_t *h)
{
    if (h->carry_pending) { h->carry_idx ^= 1; h->carry_valid = true; h->carry_pending = false; }
    h->stage_kept = false;
}

int mcl_stage_finish(mcl_engine_t *h, const double global_sums[5])
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h || !global_sums) return MCL_ERR_INVALID_ARG;
    for (int i = 0; i < 5; ++i) h->global_sums[i] = global_sums[i];
    stage_commit_carry(h);
    return MCL_OK;
}

// Adaptive resampling in a sharded set (E9).  The DECISION is the host's: keep the set when (sum w)^2 >= r / 1000 * N * sum w^2 over
// the WHOLE set (the sums of the previous update: five in the exchanged vector, sum w^2 at its end; r = resample_neff_permille),
// the same numbers on every shard.  mcl_stage_keep then takes the place of the exchange and the resampling: every particle is its
// own parent (no collective at all), the motion model is applied with the same random streams, and mcl_stage_rays adds the
// previous update's log-weights minus their global maximum, as mcl_update does.  Launch only (no wait).
int mcl_stage_keep(mcl_engine_t *h, int64_t child_first, int64_t n_children_total, const double action[3])
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h || !action) return MCL_ERR_INVALID_ARG;
    if (h->cfg.resample_neff_permille <= 0) return fail(h, MCL_ERR_UNSUPPORTED, "mcl_stage_keep needs resample_neff_permille > 0");
    if (!h->carry_valid) return fail(h, MCL_ERR_NOT_READY, "no log-weights of a previous update to carry");
    ParentSource src;
    const int c = h->cur;
    src.px = h->d_x[c]; src.py = h->d_y[c]; src.pth = h->d_th[c];
    src.keep = true;
    return stage_resample_launch(h, src, nullptr, h->N, 0, child_first, n_children_total, action);
}

// ---- the staged flow ordered on the device: nothing below waits for the stream except mcl_stage_complete ----------------
int mcl_stream_wait_external(mcl_engine_t *h, void *stream)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipEventRecord(h->ev_ext_in, static_cast<hipStream_t>(stream)));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_ext_in, 0));
    return MCL_OK;
}

int mcl_external_wait_stream(mcl_engine_t *h, void *stream)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipEventRecord(h->ev_ext_out, h->stream));
    HIPCHK(h, hipStreamWaitEvent(static_cast<hipStream_t>(stream), h->ev_ext_out, 0));
    return MCL_OK;
}

int mcl_export_compact_async(mcl_engine_t *h, void *d_chunk, int64_t chunk_entries)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    return export_compact_launch(h, d_chunk, chunk_entries, h->cfg.device, h->stream);
}

int mcl_stage_resample_compact_async(mcl_engine_t *h, const void *d_chunks, int32_t n_shards, int64_t chunk_entries, const int64_t *counts,
                                     const uint64_t *totals, int64_t n_per_shard, int32_t self_shard, int64_t child_first,
                                     int64_t n_children_total, const double action[3])
{
    if (const int rc = refuse_stage(h)) return rc;
    return stage_resample_compact_launch(h, d_chunks, n_shards, chunk_entries, counts, totals, n_per_shard, self_shard, child_first,
                                         n_children_total, action, nullptr);
}

int mcl_stage_rays_async(mcl_engine_t *h, const float *obs, int32_t n_beams, double *d_local_max)
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h || !d_local_max) return MCL_ERR_INVALID_ARG;
    MCL_TRY(stage_rays_launch(h, obs, n_beams, false, d_local_max));
    h->stage_async_rays = true;
    return MCL_OK;
}

int mcl_stage_weights_async(mcl_engine_t *h, const double *d_global_max, double *d_vec, int32_t n_shards, int32_t self_shard)
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h || !d_global_max || !d_vec || n_shards <= 0 || n_shards > mcl::kMaxShards || self_shard < 0 || self_shard >= n_shards)
        return MCL_ERR_INVALID_ARG;
    if (!h->stage_async_rays) return fail(h, MCL_ERR_NOT_READY, "mcl_stage_rays_async first");
    MCL_TRY(stage_weights_launch(h, 0.0, d_global_max));       // ends with the copy of the result block to pinned memory
    hipLaunchKernelGGL(mcl::k_stage_pack, dim3(1), dim3(64), 0, h->stream, h->d_result, d_vec, n_shards, self_shard, h->compact_pending ? 1 : 0,
                       (unsigned long long)h->compact_cap);
    HIPCHK(h, hipGetLastError());
    h->stage_async_weights = true;
    return MCL_OK;
}

int mcl_stage_complete(mcl_engine_t *h, const double global_sums[5], int32_t *redo)
{
    if (const int rc = refuse_stage(h)) return rc;
    if (!h || !global_sums || !redo) return MCL_ERR_INVALID_ARG;
    if (!h->stage_async_rays || !h->stage_async_weights) return fail(h, MCL_ERR_NOT_READY, "mcl_stage_rays_async and mcl_stage_weights_async first");
    h->stage_async_rays = h->stage_async_weights = false;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unpack_result(h);
    stage_rays_note(h);
    h->timings[4] = elapsed(h->ev[EV_RAYS], h->ev[EV_SENSOR]);
    MCL_TRY(layout_adopt(h, h->N));
    // more undecided rays than the fix-up lists hold (debug_force_exact at large sizes, a pathological map): the log-weights of
    // this update are incomplete.  The caller runs the ray stage again through mcl_stage_rays (which falls back to the
    // self-contained kernel) and the two exchanges after it; the children are untouched
    *redo = fix_lists_overflowed(h) ? 1 : 0;
    for (int i = 0; i < 5; ++i) h->global_sums[i] = global_sums[i];
    // (the carry of adaptive resampling is committed by mcl_stage_finish, which the host calls once the update stands)
    return MCL_OK;
}

int mcl_scan_weights(mcl_engine_t *h, const uint64_t *d_q, uint64_t *d_cdf, int64_t n, uint64_t offset)
{
    if (!h || !d_q || !d_cdf || n <= 0) return MCL_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    MCL_TRY(reserve_scan_spine(h, n));     // (sized for cap at mcl_create; a gathered array may be longer)
    MCL_TRY(scan_weights(h, d_q, d_cdf, n, offset, nullptr));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

// ---- the few kernels mcl_comm.hip / mcl_group.hip launch themselves (mcl_engine_internal.h): the kernels are compiled here only
namespace mcl_host {
void launch_copy_double(hipStream_t stream, const double *src, double *dst) { hipLaunchKernelGGL(mcl::k_copy_double, dim3(1), dim3(1), 0, stream, src, dst); }
void launch_set_double(hipStream_t stream, double *dst, double v) { hipLaunchKernelGGL(mcl::k_set_double, dim3(1), dim3(1), 0, stream, dst, v); }
void launch_spin_ms(hipStream_t stream, double ms) { hipLaunchKernelGGL(mcl::k_spin_ms, dim3(1), dim3(64), 0, stream, ms); }
void launch_stage_pack(hipStream_t stream, const unsigned long long *d_result, double *d_vec, int n_shards, int self, int listed, unsigned long long list_cap)
{
    hipLaunchKernelGGL(mcl::k_stage_pack, dim3(1), dim3(64), 0, stream, d_result, d_vec, n_shards, self, listed, list_cap);
}
void launch_pack_records(hipStream_t stream, const double *x, const double *y, const double *th, int64_t n, double4 *out)
{
    hipLaunchKernelGGL(mcl::k_pack_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, th, n, out);
}
int lf_used_beams(const mcl_engine *h, const float *obs, int stride, double2 *out, int32_t *idx, bool deskew)
{
    const double inv_res = 1.0 / h->res;
    int nb = 0;
    for (int j = 0; j < h->B; ++j) {
        const double r = (double)obs[(size_t)j * stride];
        if (!(r >= 0.0 && r < h->cfg.max_range_m)) continue;             // NaN, +-inf, negative, max range: no contribution
        if (idx) idx[nb] = j;
        if (deskew) out[nb++] = mcl_host::deskew_pair(r, h->ds_off[(size_t)j], h->ds_off[(size_t)h->B + j], h->ds_cs_host[(size_t)j], inv_res);
        else out[nb++] = make_double2(r * h->beam_cs_host[(size_t)j].x * inv_res, r * h->beam_cs_host[(size_t)j].y * inv_res);
    }
    return nb;
}
int launch_lfield_on(mcl_engine *h, const double *x, const double *y, const double *th, int64_t n, const double2 *d_beams, int nb,
                     double *logw)
{
    mcl::LfArgs a{};
    a.x = x; a.y = y; a.th = th; a.n = n;
    a.beams = d_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.logw = logw;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (h->lf_K < mcl::kLfLdsEntries)
        hipLaunchKernelGGL(mcl::k_lfield<true>, grid, dim3(256), (size_t)(h->lf_K + 1) * sizeof(float), h->stream, a);
    else
        hipLaunchKernelGGL(mcl::k_lfield<false>, grid, dim3(256), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}
void launch_group_max(hipStream_t stream, const mcl::GroupMaxArgs &a) { hipLaunchKernelGGL(mcl::k_group_max, dim3(1), dim3(1), 0, stream, a); }
}  // namespace mcl_host

// ---- sensor mount (mcl_set_sensor_mount).  Down here, behind every other launch of the unit: the kernels of
// mcl_mount.h are named last, so the code object keeps the kernels it had in the places they had.
namespace {

// The poses a sensor stage of n particles is handed: with no mount the ones it was given (nothing is launched, nothing reserved);
// with one, k_mount_poses on the stream -- in front of the stage's first kernel -- into the engine's scratch, and that scratch.
int sensor_poses(mcl_engine *h, const double *&x, const double *&y, const double *&th, int64_t n)
{
    h->last_mounted = h->mounted;
    if (!h->mounted) { h->sp_valid = false; return MCL_OK; }     // (this stage reads the base poses: the scratch is no stage's any more)
    if (h->d_sth.cap < (size_t)h->cap) {
        if (h->capturing) return fail(h, MCL_ERR_HIP, "sensor-pose buffers missing during capture (internal)");
        MCL_TRY(h->d_sx.reserve(h, (size_t)h->cap));
        MCL_TRY(h->d_sy.reserve(h, (size_t)h->cap));
        MCL_TRY(h->d_sth.reserve(h, (size_t)h->cap));
    }
    if (n < 1 || n > h->cap) return fail(h, MCL_ERR_INVALID_ARG, "sensor poses: particle count out of range (internal)");
    mcl::launch_mount_poses(h->stream, x, y, th, n, h->mount, h->d_sx, h->d_sy, h->d_sth);
    HIPCHK(h, hipGetLastError());
    x = h->d_sx; y = h->d_sy; th = h->d_sth;
    h->sp_valid = true; h->sp_n = n;
    return MCL_OK;
}

}  // namespace

static void add_prev_logw(mcl_engine *h, int64_t n)
{
    hipLaunchKernelGGL(mcl::k_add_logw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, h->d_logw.p, h->d_logw_prev.p, n);
    h->max_partials_ready = false;
}

// ---- per-beam sensor offsets (mcl_set_beam_offsets).  Behind the mount's launches: k_rays_deskew is named last.
namespace {

// The beam model's sensor stage with offsets on: the one kernel, on the sensor poses launch_rays formed, with the offsets' own directions
// and float angles (DS1) in place of the engine's, the scan's rows and the static table (no transposed table is read, no sweep table built).
void ray_kernel_deskew(mcl_engine *h, const RayPlan &p, mcl::RayArgs &a)
{
    a.beam_cs = h->d_ds_cs(); a.beam_angle = h->d_ds_angle();
    a.Ldirect = h->d_L; a.obs_idx = h->d_obs_idx;
    const dim3 g((unsigned)p.grid), b(mcl::kDeskewThreads);
    if (a.steps16) hipLaunchKernelGGL(mcl::k_rays_deskew<2>, g, b, 0, h->stream, a, h->d_ds_off());
    else if (a.steps) hipLaunchKernelGGL(mcl::k_rays_deskew<1>, g, b, 0, h->stream, a, h->d_ds_off());
    else hipLaunchKernelGGL(mcl::k_rays_deskew<0>, g, b, 0, h->stream, a, h->d_ds_off());
}

}  // namespace

int mcl_set_beam_offsets(mcl_engine_t *h, const double *offsets_colmajor, int32_t n_beams)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!offsets_colmajor) {                // off: the default.  Turning them off voids what was captured or handed off with them on, once
        if (h->ds_on) graph_reset(h);
        h->ds_on = false;
        return MCL_OK;
    }
    if (h->B <= 0 || h->beam_cs_host.empty()) return fail(h, MCL_ERR_NOT_READY, "beam offsets: set the beam angles first (mcl_set_beam_angles)");
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "beam offsets: n_beams does not match the beam angles");
    if (h->comm || h->in_group)
        return fail(h, MCL_ERR_UNSUPPORTED, "per-beam sensor offsets are single-engine only: this engine has a communicator or belongs to a device group");
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_UNSUPPORTED, "per-beam sensor offsets need weight_mode LOG: create the engine with MCL_WEIGHT_LOG");
    if (h->cfg.ray_kernel != MCL_RAYS_AUTO)
        return fail(h, MCL_ERR_UNSUPPORTED, "per-beam sensor offsets take a ray kernel of their own: create the engine with ray_kernel MCL_RAYS_AUTO");
    const size_t B = (size_t)h->B;
    for (size_t k = 0; k < 3 * B; ++k)
        if (!std::isfinite(offsets_colmajor[k])) return fail(h, MCL_ERR_INVALID_ARG, "beam offsets: every component (ox, oy, dtheta) must be finite");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // one block: [B double2: DS1's pairs | 3 B doubles: the table | B floats: a'], staged in pinned memory and uploaded in one copy
    const size_t words = mcl_host::deskew_block_words(B);
    if (h->d_ds.cap < words) {
        if (h->ds_on) { graph_reset(h); h->ds_on = false; }
        MCL_TRY(h->d_ds.reserve(h, words));
        MCL_TRY(h->h_ds.reserve(h, words));
    }
    h->ds_B = h->B;
    h->ds_off.assign(offsets_colmajor, offsets_colmajor + 3 * B);
    h->ds_cs_host.resize(B); h->ds_angle.resize(B);
    mcl_host::deskew_table(h->angles.data(), offsets_colmajor, h->B, h->ds_angle.data(), h->ds_cs_host.data());
    // (a stage that reads the block has been waited for by its update: the staging words are free; a second call before any update
    //  queues a second copy behind the first, and the last one written is the one the next stage reads)
    std::memcpy(h->h_ds.p, h->ds_cs_host.data(), B * sizeof(double2));
    std::memcpy(h->h_ds.p + 2 * B, h->ds_off.data(), 3 * B * sizeof(double));
    std::memcpy(h->h_ds.p + 5 * B, h->ds_angle.data(), B * sizeof(float));
    HIPCHK(h, hipMemcpyAsync(h->d_ds, h->h_ds, words * sizeof(double), hipMemcpyHostToDevice, h->stream));     // no host wait
    if (!h->ds_on) graph_reset(h);          // turning them on: the captured tails and the hand-off were made for the other ray stage
    h->ds_on = true;
    return MCL_OK;
}

int mcl_get_beam_offsets(const mcl_engine_t *h, double *offsets_colmajor, float *effective_angles, int32_t n_beams, int32_t *on)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (on) *on = h->ds_on ? 1 : 0;
    if (!offsets_colmajor && !effective_angles) return MCL_OK;
    if (h->B <= 0 || n_beams != h->B) return MCL_ERR_INVALID_ARG;
    const size_t B = (size_t)h->B;
    // off: a table of zeros and the beam angles themselves
    if (offsets_colmajor) for (size_t k = 0; k < 3 * B; ++k) offsets_colmajor[k] = h->ds_on ? h->ds_off[k] : 0.0;
    if (effective_angles) for (size_t j = 0; j < B; ++j) effective_angles[j] = h->ds_on ? h->ds_angle[j] : h->angles[j];
    return MCL_OK;
}
