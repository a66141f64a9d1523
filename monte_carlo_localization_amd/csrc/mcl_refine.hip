// mcl_refine.hip -- mcl_refine_poses: the likelihood-field score of every pose of a dense window around each
// seed pose against one scan; per seed the best window pose, the weighted mean and the covariance.  Called outside the update: it
// reads the beams, the likelihood field and its table, writes only buffers of its own (struct mcl_refine) and leaves every engine
// state as it was.
//
// A call, on the engine's stream:
//   (upload)          the M seeds and the used beams of the scan, from pinned staging
//   k_refine_score    one lane per window pose: the score volume (M x n_win)
//   k_refine_reduce   one workgroup per seed: best pose (R3), moments (R4), the record
//   (copy)            the M records; one host wait.  The volume stays on the device for mcl_get_refine_scores.
#include "mcl_refine.h"

#include <cmath>
#include <cstring>

using namespace mcl_rf;

// the buffers of the refinement, kept between calls and grown on demand
struct mcl_refine {
    int64_t cap_seeds = 0;
    double *d_seeds = nullptr, *h_seeds = nullptr;              // 3 per seed
    mcl_refine_result_t *d_out = nullptr, *h_out = nullptr;
    int64_t cap_b = 0;
    double2 *d_beams = nullptr, *h_beams = nullptr;
    float *h_obs = nullptr;
    int64_t cap_poses = 0;
    double *d_score = nullptr;
    // the volume d_score holds: of which map, how many poses (0: none)
    unsigned long long volume_epoch = 0;
    int64_t volume_n = 0;
    size_t device_bytes = 0;
};

namespace {

using mcl_host::dfree;
using mcl_host::fail;

template <class T>
void hfree(T *&p)
{
    if (p) (void)hipHostFree(p);
    p = nullptr;
}

template <class T>
int grow_dev(mcl_engine *h, mcl_refine *r, T *&p, size_t want)
{
    dfree(p);
    HIPCHK(h, hipMalloc(&p, want * sizeof(T)));
    r->device_bytes += want * sizeof(T);
    return MCL_OK;
}

template <class T>
int grow_host(mcl_engine *h, T *&p, size_t want)
{
    hfree(p);
    HIPCHK(h, hipHostMalloc((void **)&p, want * sizeof(T)));
    return MCL_OK;
}

#define RFN_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// room for M seeds, a volume of n_poses and a scan of B beams
int refine_alloc(mcl_engine *h, mcl_refine *r, int64_t M, int64_t n_poses, int B)
{
    if (M > r->cap_seeds) {
        r->cap_seeds = 0;
        RFN_TRY(grow_dev(h, r, r->d_seeds, (size_t)3 * M));
        RFN_TRY(grow_dev(h, r, r->d_out, (size_t)M));
        RFN_TRY(grow_host(h, r->h_seeds, (size_t)3 * M));
        RFN_TRY(grow_host(h, r->h_out, (size_t)M));
        r->cap_seeds = M;
    }
    if (B > r->cap_b) {
        r->cap_b = 0;
        RFN_TRY(grow_dev(h, r, r->d_beams, (size_t)B));
        RFN_TRY(grow_host(h, r->h_beams, (size_t)B));
        RFN_TRY(grow_host(h, r->h_obs, (size_t)B));
        r->cap_b = B;
    }
    if (n_poses > r->cap_poses) {
        r->cap_poses = 0;
        r->volume_n = 0;
        RFN_TRY(grow_dev(h, r, r->d_score, (size_t)n_poses));
        r->cap_poses = n_poses;
    }
    return MCL_OK;
}

}  // namespace

void refine_free(struct mcl_refine *r)
{
    if (!r) return;
    dfree(r->d_seeds); dfree(r->d_out); dfree(r->d_beams); dfree(r->d_score);
    hfree(r->h_seeds); hfree(r->h_out); hfree(r->h_beams); hfree(r->h_obs);
    delete r;
}

extern "C" {

int mcl_refine_poses(mcl_engine_t *h, const mcl_refine_config_t *cfg, const double *seeds_colmajor, int32_t M, const float *obs,
                     int32_t n_beams, mcl_refine_result_t *out, uint64_t stats[4])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    mcl_refine_config_t c;
    if (cfg) c = *cfg; else mcl_default_refine_config(&c);
    // arguments, then readiness (R7)
    if (const char *why = mcl_host::refine_invalid(&c)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!seeds_colmajor || !obs || !out) return fail(h, MCL_ERR_INVALID_ARG, "refine: seeds / obs / out is null");
    if (M < 1 || M > kMaxSeeds) return fail(h, MCL_ERR_INVALID_ARG, "refine: the number of seeds must be in [1, 4096]");
    for (int64_t i = 0; i < (int64_t)3 * M; ++i)
        if (!std::isfinite(seeds_colmajor[i])) return fail(h, MCL_ERR_INVALID_ARG, "refine: a seed has a non-finite component");
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
    RFN_TRY(refine_alloc(h, r, M, n_poses, B));
    r->volume_n = 0;                                             // until this volume is whole

    std::memcpy(r->h_seeds, seeds_colmajor, (size_t)3 * M * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(r->d_seeds, r->h_seeds, (size_t)3 * M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // R2: the readings of the candidate beams, the others NaN (no contribution), through the update's own rule
    for (int j = 0; j < B; ++j) r->h_obs[j] = (j % c.beam_stride == 0) ? obs[j] : NAN;
    const int nb = mcl_host::lf_used_beams(h, r->h_obs, 1, r->h_beams);
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(r->d_beams, r->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));

    Args a{};
    a.seeds = r->d_seeds; a.M = M; a.win = win; a.n_total = (int32_t)n_poses;
    a.beams = r->d_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.score = r->d_score; a.out = r->d_out;
    const dim3 grid_score((unsigned)((n_poses + kThreads - 1) / kThreads));
    if (h->lf_K < mcl::kLfLdsEntries)
        hipLaunchKernelGGL(k_refine_score<true>, grid_score, dim3(kThreads), (size_t)(h->lf_K + 1) * sizeof(float), h->stream, a);
    else
        hipLaunchKernelGGL(k_refine_score<false>, grid_score, dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    hipLaunchKernelGGL(k_refine_reduce, dim3((unsigned)M), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(r->h_out, r->d_out, (size_t)M * sizeof(mcl_refine_result_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait
    r->volume_epoch = h->map_epoch;
    r->volume_n = n_poses;
    std::memcpy(out, r->h_out, (size_t)M * sizeof(mcl_refine_result_t));
    if (stats) {
        stats[0] = (uint64_t)win.n_win; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)r->device_bytes;
    }
    return MCL_OK;
}

int mcl_get_refine_scores(mcl_engine_t *h, double *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    const mcl_refine *r = h->rfn;
    if (!r || r->volume_n == 0 || r->volume_epoch != h->map_epoch || !h->have_map)
        return fail(h, MCL_ERR_NOT_READY, "no score volume: no refinement has run on this map");
    if (n != (size_t)r->volume_n) return fail(h, MCL_ERR_INVALID_ARG, "the volume has seeds x window poses entries");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(out, r->d_score, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_get_refine_bytes(const mcl_engine_t *h, uint64_t *bytes)
{
    if (!h || !bytes) return MCL_ERR_INVALID_ARG;
    *bytes = h->rfn ? (uint64_t)h->rfn->device_bytes : 0;
    return MCL_OK;
}

}  // extern "C"
