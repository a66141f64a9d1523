// mcl_side_buffers.h -- what the host code of the three read-only side calls shares (mcl_query.hip, mcl_search.hip, mcl_refine.hip):
// the owning buffer types (mcl_buffers.h) and the few steps more than one of the calls takes.  Host code only.
#pragma once
#include "mcl_engine_internal.h"
#include "mcl_lfield_core.h"
#include "mcl_ray_core.h"

#include <algorithm>
#include <cmath>

#define SIDE_TRY(call) MCL_TRY(call)

namespace mcl_side {

// the owning buffers (mcl_buffers.h) under the names the side calls use
using ::DevBuf;
using ::HostBuf;

// The used beams of a scan (search S3, refine R2) at `out`, through the update's own rule: the readings of every beam_stride-th
// beam, the others NaN (no contribution).  h_obs: B floats of staging.  Returns their number.
inline int stage_used_beams(const mcl_engine *h, int beam_stride, const float *obs, float *h_obs, double2 *out)
{
    for (int j = 0; j < h->B; ++j) h_obs[j] = (j % beam_stride == 0) ? obs[j] : NAN;
    return mcl_host::lf_used_beams(h, h_obs, 1, out);
}

// dynamic LDS of a kernel that stages the likelihood table there; 0: the table is too long, the kernel reads it from memory
inline size_t lf_lds_bytes(const mcl_engine *h)
{
    return h->lf_K < mcl::kLfLdsEntries ? (size_t)(h->lf_K + 1) * sizeof(float) : 0;
}

// What the ray functions (mcl_ray_core.h) read of the engine: the map, P, the beams, force_exact.  The rest of `m` stays as it is.
inline void fill_ray_args(const mcl_engine *h, mcl::RayArgs &m)
{
    m.B = h->B; m.P = h->P;
    m.beam_cs = h->d_beam_cs; m.beam_angle = h->d_angle;
    m.grid = h->d_grid; m.W = h->W; m.H = h->H;
    m.res = h->res; m.ox = h->ox; m.oy = h->oy;
    m.dist = h->d_dist; m.Wp = h->Wp; m.Hp = h->Hp; m.Wps = h->Wps;
    m.force_exact = h->cfg.debug_force_exact;
}

// workgroups (of 4 waves) of a kernel that gives every listed level-3 ray a wave, for a list that holds at most `waves` rays
// (the count is read on the device)
inline unsigned level3_grid(const mcl_engine *h, int64_t waves)
{
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)h->num_cu * 8));
}

// What refuses a call under the beam model after its arguments (B6 / RB6): where it works, then readiness.  `who` opens every
// message.  map_and_beams: false where the call's own argument check has asked for the map and the beam angles already.
inline int beam_model_check(mcl_engine *h, const std::string &who, bool map_and_beams)
{
    using mcl_host::fail;
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_INVALID_ARG, who + ": weight_mode LOG only");
    if (h->comm || h->in_group)
        return fail(h, MCL_ERR_UNSUPPORTED, who + ": single-engine only: this engine has a communicator or belongs to a device group");
    if (map_and_beams) {
        if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, who + ": no map is set");
        if (h->B <= 0 || !h->d_beam_cs || !h->d_angle) return fail(h, MCL_ERR_NOT_READY, who + ": no beam angles are set");
    }
    if (!h->d_L || !h->d_dist || !h->d_grid) return fail(h, MCL_ERR_NOT_READY, who + ": the map's tables are not built");
    return MCL_OK;
}

// the score volume a call left on the device: of which map, how many poses (0: none)
struct Volume {
    unsigned long long epoch = 0;
    int64_t n = 0;
};

// mcl_get_*_scores: the n doubles of volume v (null: the feature never ran) from d_score, or why not
inline int read_volume(mcl_engine *h, const Volume *v, const double *d_score, double *out, size_t n, const char *no_volume,
                       const char *wrong_size)
{
    if (!v || v->n == 0 || v->epoch != h->map_epoch || !h->have_map) return mcl_host::fail(h, MCL_ERR_NOT_READY, no_volume);
    if (n != (size_t)v->n) return mcl_host::fail(h, MCL_ERR_INVALID_ARG, wrong_size);
    return read_back(h, {{out, d_score, n * sizeof(double)}});
}

}  // namespace mcl_side
