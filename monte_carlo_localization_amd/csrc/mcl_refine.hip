// mcl_refine.hip -- mcl_refine_poses, mcl_refine_poses_beam (§4.18) and mcl_refine_poses_sequence (§4.23): the
// score of every pose of a dense window around each seed pose against one scan, under the likelihood-field model or under the
// beam model, or against a scan sequence joined by odometry under the likelihood-field model; per seed the best window pose, the
// weighted mean and the covariance.  Called outside the update: they read the beams and the map's tables, write
// only buffers of their own (struct mcl_refine) and leave every engine state as it was.
//
// A call, on the engine's stream:
//   (upload)              the M seeds and the scan (field: its used beams; beam model: its readings), from pinned staging
//   k_refine_score        field: one lane per window pose: the score volume (M x n_win)
//   k_refine_score_seq    field, S scans: the same lanes, every scan scored from where the odometry puts it, the S sums folded
//   k_refine_beam_rows    beam model: where the table row of every used beam starts
//   k_refine_beam_score   beam model: one wave per window pose casts and sums its beams: the score volume (2^22 poses a launch)
//   k_refine_reduce       one workgroup per seed: best pose (R3), moments (R4), the record
//   (copy)                the M records; one host wait.  The volume stays on the device for mcl_get_refine_scores.
#include "mcl_refine.h"
#include "mcl_side_buffers.h"

#include <algorithm>
#include <cstring>

using namespace mcl_rf;
using namespace mcl_side;
using mcl_host::fail;

// the buffers of the refinement, kept between calls and grown on demand
struct mcl_refine {
    DevBuf<double> d_seeds;                                     // 3 per seed
    HostBuf<double> h_seeds;
    DevBuf<mcl_refine_result_t> d_out;
    HostBuf<mcl_refine_result_t> h_out;
    DevBuf<double2> d_beams;
    HostBuf<double2> h_beams;
    HostBuf<float> h_obs;
    DevBuf<double> d_score;
    Volume volume;                                              // what d_score holds (of either call)
    // the beam model's (mcl_refine_poses_beam)
    DevBuf<float> d_obs;                                        // the scan
    DevBuf<uint32_t> d_row_base;                                // per used beam
    DevBuf<BeamHeader> d_hdr;
    HostBuf<BeamHeader> h_hdr;
    // the scan sequence's (mcl_refine_poses_sequence): the table of RS1 and where each scan's beams begin; d_beams / h_beams
    // then hold the S used-beam lists one after the other
    DevBuf<double> d_off;                                       // 3 per (seed, window heading, scan)
    HostBuf<double> h_off;
    DevBuf<int32_t> d_begin;                                    // MCL_SEARCH_MAX_SCANS + 1
    HostBuf<int32_t> h_begin;
    size_t device_bytes = 0;
};

namespace {

// room for M seeds, a volume of n_poses and a scan of B beams
int refine_alloc(mcl_engine *h, mcl_refine *r, size_t M, size_t n_poses, size_t B)
{
    SIDE_TRY(r->d_seeds.reserve(h, 3 * M, &r->device_bytes));
    SIDE_TRY(r->d_out.reserve(h, M, &r->device_bytes));
    SIDE_TRY(r->h_seeds.reserve(h, 3 * M));
    SIDE_TRY(r->h_out.reserve(h, M));
    SIDE_TRY(r->d_beams.reserve(h, B, &r->device_bytes));
    SIDE_TRY(r->h_beams.reserve(h, B));
    SIDE_TRY(r->h_obs.reserve(h, B));
    if (n_poses > r->d_score.cap) r->volume.n = 0;
    return r->d_score.reserve(h, n_poses, &r->device_bytes);
}

// refine_alloc with a beam list of S scans of B beams each (the staging of one scan's readings grows with it: S * B floats), and
// the table of `rows` triples (RS1) with the S + 1 begin offsets (RS3)
int refine_sequence_alloc(mcl_engine *h, mcl_refine *r, size_t M, size_t n_poses, size_t B, size_t S, size_t rows)
{
    SIDE_TRY(refine_alloc(h, r, M, n_poses, S * B));
    SIDE_TRY(r->d_off.reserve(h, 3 * rows, &r->device_bytes));
    SIDE_TRY(r->h_off.reserve(h, 3 * rows));
    SIDE_TRY(r->d_begin.reserve(h, (size_t)MCL_SEARCH_MAX_SCANS + 1, &r->device_bytes));
    return r->h_begin.reserve(h, (size_t)MCL_SEARCH_MAX_SCANS + 1);
}

// the same for the beam model: no used-beam pairs (the engine's directions serve), the scan, its rows and the counter instead
int refine_beam_alloc(mcl_engine *h, mcl_refine *r, size_t M, size_t n_poses, size_t B)
{
    SIDE_TRY(r->d_seeds.reserve(h, 3 * M, &r->device_bytes));
    SIDE_TRY(r->d_out.reserve(h, M, &r->device_bytes));
    SIDE_TRY(r->h_seeds.reserve(h, 3 * M));
    SIDE_TRY(r->h_out.reserve(h, M));
    SIDE_TRY(r->h_obs.reserve(h, B));
    SIDE_TRY(r->d_obs.reserve(h, B, &r->device_bytes));
    SIDE_TRY(r->d_row_base.reserve(h, B, &r->device_bytes));
    SIDE_TRY(r->d_hdr.reserve(h, 1, &r->device_bytes));
    SIDE_TRY(r->h_hdr.reserve(h, 1));
    if (n_poses > r->d_score.cap) r->volume.n = 0;
    return r->d_score.reserve(h, n_poses, &r->device_bytes);
}

// what R7 refuses of the config and the arguments, for both calls: c receives the config in force
int refine_args(mcl_engine *h, const mcl_refine_config_t *cfg, const double *seeds_colmajor, int32_t M, const float *obs,
                const mcl_refine_result_t *out, mcl_refine_config_t &c)
{
    if (cfg) c = *cfg; else mcl_default_refine_config(&c);
    if (const char *why = mcl_host::refine_invalid(&c)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!seeds_colmajor || !obs || !out) return fail(h, MCL_ERR_INVALID_ARG, "refine: seeds / obs / out is null");
    if (M < 1 || M > kMaxSeeds) return fail(h, MCL_ERR_INVALID_ARG, "refine: the number of seeds must be in [1, 4096]");
    for (int64_t i = 0; i < (int64_t)3 * M; ++i)
        if (!std::isfinite(seeds_colmajor[i])) return fail(h, MCL_ERR_INVALID_ARG, "refine: a seed has a non-finite component");
    return MCL_OK;
}

// the seeds to the device
int refine_seeds_upload(mcl_engine *h, mcl_refine *r, const double *seeds_colmajor, int32_t M)
{
    std::memcpy(r->h_seeds, seeds_colmajor, (size_t)3 * M * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(r->d_seeds, r->h_seeds, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return MCL_OK;
}

// R3 / R4 of the volume the stream has made by then, the M records back; the host wait of the call
int refine_reduce(mcl_engine *h, mcl_refine *r, const Args &a, int64_t n_poses, mcl_refine_result_t *out)
{
    hipLaunchKernelGGL(k_refine_reduce, dim3((unsigned)a.M), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(r->h_out, r->d_out, (size_t)a.M * sizeof(mcl_refine_result_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait
    r->volume = {h->map_epoch, n_poses};
    std::memcpy(out, r->h_out, (size_t)a.M * sizeof(mcl_refine_result_t));
    return MCL_OK;
}

}  // namespace

void refine_free(struct mcl_refine *r) { delete r; }

extern "C" {

int mcl_refine_poses(mcl_engine_t *h, const mcl_refine_config_t *cfg, const double *seeds_colmajor, int32_t M, const float *obs,
                     int32_t n_beams, mcl_refine_result_t *out, uint64_t stats[4])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    mcl_refine_config_t c;
    // arguments, then readiness (R7)
    SIDE_TRY(refine_args(h, cfg, seeds_colmajor, M, obs, out, c));
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "refine: no map is set");
    if (h->B <= 0 || h->beam_cs_host.empty()) return fail(h, MCL_ERR_NOT_READY, "refine: no beam angles are set");
    if (!h->lf_on || h->lf_K < 0 || !h->d_lf_D)
        return fail(h, MCL_ERR_NOT_READY, "refine: the likelihood-field model is off (mcl_set_likelihood_field; the refinement reads its field and table)");
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "refine: n_beams does not match the beam angles");
    const Window win = window_of(c, h->res);
    const int64_t n_poses = (int64_t)M * win.n_win;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "refine: seeds * window poses must stay below 2^27 (fewer seeds or a smaller window)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->rfn) h->rfn = new mcl_refine();
    mcl_refine *r = h->rfn;
    const int B = h->B;
    SIDE_TRY(refine_alloc(h, r, (size_t)M, (size_t)n_poses, (size_t)B));
    r->volume.n = 0;                                            // until this volume is whole

    SIDE_TRY(refine_seeds_upload(h, r, seeds_colmajor, M));
    const int nb = stage_used_beams(h, c.beam_stride, obs, r->h_obs, r->h_beams);                  // R2
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(r->d_beams, r->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));

    Args a{};
    a.seeds = r->d_seeds; a.M = M; a.win = win; a.n_total = (int32_t)n_poses;
    a.beams = r->d_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.score = r->d_score; a.out = r->d_out;
    const dim3 grid_score((unsigned)((n_poses + kThreads - 1) / kThreads));
    if (const size_t lds = lf_lds_bytes(h))
        hipLaunchKernelGGL(k_refine_score<true>, grid_score, dim3(kThreads), lds, h->stream, a);
    else
        hipLaunchKernelGGL(k_refine_score<false>, grid_score, dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    SIDE_TRY(refine_reduce(h, r, a, n_poses, out));
    if (stats) {
        stats[0] = (uint64_t)win.n_win; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)r->device_bytes;
    }
    return MCL_OK;
}

int mcl_refine_poses_beam(mcl_engine_t *h, const mcl_refine_config_t *cfg, const double *seeds_colmajor, int32_t M, const float *obs,
                          int32_t n_beams, mcl_refine_result_t *out, uint64_t stats[6])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    mcl_refine_config_t c;
    // arguments, then where it works, then readiness (RB6)
    SIDE_TRY(refine_args(h, cfg, seeds_colmajor, M, obs, out, c));
    SIDE_TRY(beam_model_check(h, "refine (beam model)", true));
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "refine: n_beams does not match the beam angles");
    const Window win = window_of(c, h->res);
    const int64_t n_poses = (int64_t)M * win.n_win;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "refine: seeds * window poses must stay below 2^27 (fewer seeds or a smaller window)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->rfn) h->rfn = new mcl_refine();
    mcl_refine *r = h->rfn;
    const int B = h->B;
    const int nb = (B + c.beam_stride - 1) / c.beam_stride;       // RB3: j = u * beam_stride < B
    SIDE_TRY(refine_beam_alloc(h, r, (size_t)M, (size_t)n_poses, (size_t)B));
    r->volume.n = 0;                                            // until this volume is whole

    SIDE_TRY(refine_seeds_upload(h, r, seeds_colmajor, M));
    std::memcpy(r->h_obs, obs, (size_t)B * sizeof(float));
    HIPCHK(h, hipMemcpyAsync(r->d_obs, r->h_obs, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(r->d_hdr, 0, sizeof(BeamHeader), h->stream));

    BeamArgs b{};
    fill_ray_args(h, b.ray);
    b.seeds = r->d_seeds; b.M = M; b.win = win; b.n_total = (int32_t)n_poses;
    b.obs = r->d_obs; b.beam_stride = c.beam_stride; b.nb = nb;
    b.row_base = r->d_row_base; b.L = h->d_L;
    b.score = r->d_score; b.hdr = r->d_hdr;
    hipLaunchKernelGGL(k_refine_beam_rows, dim3((unsigned)((nb + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, b);
    HIPCHK(h, hipGetLastError());
    for (int64_t p0 = 0; p0 < n_poses; p0 += kPosesPerLaunch) {   // a wave per pose, at most 2^30 threads per launch
        const int64_t n = std::min<int64_t>(n_poses - p0, kPosesPerLaunch);
        b.pose0 = (int32_t)p0;
        hipLaunchKernelGGL(k_refine_beam_score, dim3((unsigned)((n + kPosesPerBlock - 1) / kPosesPerBlock)), dim3(kThreads), 0, h->stream, b);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipMemcpyAsync(r->h_hdr, r->d_hdr, sizeof(BeamHeader), hipMemcpyDeviceToHost, h->stream));

    Args a{};                                                   // RB4: R3 / R4 as they are
    a.seeds = r->d_seeds; a.M = M; a.win = win; a.n_total = (int32_t)n_poses;
    a.score = r->d_score; a.out = r->d_out;
    SIDE_TRY(refine_reduce(h, r, a, n_poses, out));
    if (stats) {
        stats[0] = (uint64_t)win.n_win; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)r->device_bytes;
        stats[4] = (uint64_t)n_poses * (uint64_t)nb; stats[5] = (uint64_t)r->h_hdr->level3;
    }
    return MCL_OK;
}

int mcl_refine_poses_sequence(mcl_engine_t *h, const mcl_refine_config_t *cfg, const double *seeds_colmajor, int32_t M, const float *scans,
                              const double *rel, int32_t n_scans, int32_t n_beams, mcl_refine_result_t *out, uint64_t stats[5])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    mcl_refine_config_t c;
    // the sequence's own arguments, then everything mcl_refine_poses checks, then the size of the table (RS7)
    if (const char *why = mcl_host::refine_sequence_invalid(rel, n_scans)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!scans) return fail(h, MCL_ERR_INVALID_ARG, "refine: scans is null");
    SIDE_TRY(refine_args(h, cfg, seeds_colmajor, M, scans, out, c));
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "refine: no map is set");
    if (h->B <= 0 || h->beam_cs_host.empty()) return fail(h, MCL_ERR_NOT_READY, "refine: no beam angles are set");
    if (!h->lf_on || h->lf_K < 0 || !h->d_lf_D)
        return fail(h, MCL_ERR_NOT_READY, "refine: the likelihood-field model is off (mcl_set_likelihood_field; the refinement reads its field and table)");
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "refine: n_beams does not match the beam angles");
    const Window win = window_of(c, h->res);
    const int64_t n_poses = (int64_t)M * win.n_win;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "refine: seeds * window poses must stay below 2^27 (fewer seeds or a smaller window)");
    const int S = n_scans;
    const std::string rows_refused = mcl_host::refine_sequence_rows_refused(M, win.nt, S);
    if (!rows_refused.empty()) return fail(h, MCL_ERR_INVALID_ARG, rows_refused);
    const size_t rows = (size_t)M * (size_t)win.nt * (size_t)S;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->rfn) h->rfn = new mcl_refine();
    mcl_refine *r = h->rfn;
    const int B = h->B;
    SIDE_TRY(refine_sequence_alloc(h, r, (size_t)M, (size_t)n_poses, (size_t)B, (size_t)S, rows));
    r->volume.n = 0;                                            // until this volume is whole

    SIDE_TRY(refine_seeds_upload(h, r, seeds_colmajor, M));
    int nb = 0;                                                 // RS3: every scan's used beams, one list after the other
    for (int sc = 0; sc < S; ++sc) {
        r->h_begin[sc] = nb;
        nb += stage_used_beams(h, c.beam_stride, scans + (size_t)sc * (size_t)B, r->h_obs, r->h_beams + nb);
    }
    r->h_begin[S] = nb;
    mcl_host::refine_sequence_offsets(c.half_theta, c.step_theta_rad, seeds_colmajor, M, rel, S, r->h_off);       // RS1
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(r->d_beams, r->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(r->d_begin, r->h_begin, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(r->d_off, r->h_off, 3 * rows * sizeof(double), hipMemcpyHostToDevice, h->stream));

    SeqArgs q{};
    Args &a = q.a;
    a.seeds = r->d_seeds; a.M = M; a.win = win; a.n_total = (int32_t)n_poses;
    a.beams = r->d_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.score = r->d_score; a.out = r->d_out;
    q.off = r->d_off; q.beam_begin = r->d_begin; q.S = S;
    const dim3 grid_score((unsigned)((n_poses + kThreads - 1) / kThreads));
    if (const size_t lds = lf_lds_bytes(h))
        hipLaunchKernelGGL(k_refine_score_seq<true>, grid_score, dim3(kThreads), lds, h->stream, q);
    else
        hipLaunchKernelGGL(k_refine_score_seq<false>, grid_score, dim3(kThreads), 0, h->stream, q);
    HIPCHK(h, hipGetLastError());
    SIDE_TRY(refine_reduce(h, r, a, n_poses, out));              // RS5: R3 / R4 as they are, on the summed volume
    if (stats) {
        stats[0] = (uint64_t)win.n_win; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)r->device_bytes;
        stats[4] = (uint64_t)S;
    }
    return MCL_OK;
}

int mcl_get_refine_scores(mcl_engine_t *h, double *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    const mcl_refine *r = h->rfn;
    return read_volume(h, r ? &r->volume : nullptr, r ? r->d_score.p : nullptr, out, n, "no score volume: no refinement has run on this map",
                       "the volume has seeds x window poses entries");
}

int mcl_get_refine_bytes(const mcl_engine_t *h, uint64_t *bytes)
{
    if (!h || !bytes) return MCL_ERR_INVALID_ARG;
    *bytes = h->rfn ? (uint64_t)h->rfn->device_bytes : 0;
    return MCL_OK;
}

}  // extern "C"
