// mcl_side_buffers.h -- what the host code of the three read-only side calls shares (mcl_query.hip, mcl_search.hip, mcl_refine.hip):
// the owning buffer types (mcl_buffers.h) and the few steps more than one of the calls takes.  Host code only.
#pragma once
#include "mcl_engine_internal.h"
#include "mcl_lfield_core.h"

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
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(out, d_score, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

}  // namespace mcl_side
