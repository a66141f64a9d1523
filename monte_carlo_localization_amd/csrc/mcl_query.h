// mcl_query.h -- the pose query (mcl_query_scans / mcl_score_poses): the expected scan of K poses that are not
// particles, and how well a scan supports each of them.  The arguments of its kernels and the kernels themselves; only
// mcl_query.hip includes it.  A ray's step index comes from the functions the update's own ray stage calls (mcl_ray_core.h), so a
// query and a particle at the same pose agree bit for bit.
#pragma once
#include "mcl_device_math.h"
#include "mcl_engine_internal.h"
#include "mcl_ray_core.h"

namespace mcl_qry {

constexpr int kThreads = 256;
constexpr int32_t kMaxPoses = 65536;
constexpr unsigned long long kListCap = 1ull << 20;   // level-3 rays of a call that get a wave each (more: marched by their own lane)
constexpr uint32_t kObsInvalid = 0x80000000u;          // flag of a beam that is not valid (Q4) beside its table row

using Header = mcl::Level3Header;   // what the kernels count; copied to the host at the end of a call

struct Args {
    mcl::RayArgs ray;               // the map, P, B, the beam directions and angles, force_exact: what trace_fp64 / march_exact read
    const double *x, *y, *th;       // K poses
    int32_t K;
    uint16_t *steps;                // K x B, pose-major
    float *ranges;                  // the same in metres (Q2), or null
    float miss_range;               // MAX_RANGE_METERS as a float (cpp:649)
    unsigned long long *list;       // ray indices k * B + j waiting for the literal march
    unsigned long long list_cap;
    Header *hdr;
    // the score
    const float *obs;               // B readings
    uint32_t *obs_row;              // per beam: its table row (E2), kObsInvalid set when the beam is not valid
    const float *L;                 // [row][step], P + 1 columns: the engine's static table
    const double *lf_logw;          // likelihood field on: the K log-likelihoods k_lfield left, else null
    int32_t tol_steps;
    mcl_pose_score_t *out;
};

__device__ __forceinline__ void store_ray(const Args &a, uint32_t ray, int r)
{
    a.steps[ray] = (uint16_t)r;
    if (a.ranges) a.ranges[ray] = r < a.ray.P ? (float)((double)r * a.ray.res) : a.miss_range;      // cpp:635 / 644 / 649
}

// One lane per ray (k, j), ray index k * B + j: 64 consecutive beams of a pose (or of two) per wave, so the lanes of a wave walk
// near-identical rays.  Levels 2 and 3 exactly as k_rays_fix runs them on the isotropic field: fp64 positions with the guard,
// the literal march where the guard says so, where the pose is not sane, or with debug_force_exact.  Level-3 rays go to the list
// (k_query_exact gives each a wave); beyond its capacity the lane marches itself.
__global__ __launch_bounds__(kThreads) void k_query_rays(Args a)
{
    const mcl::RayArgs &m = a.ray;
    const uint32_t ray = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (ray >= (uint32_t)a.K * (uint32_t)m.B) return;
    const uint32_t k = ray / (uint32_t)m.B;
    const int j = (int)(ray - k * (uint32_t)m.B);
    const double4 pci = mcl::particle_constants(a.x[k], a.y[k], a.th[k], m.ox, m.oy, m.res);
    const double2 cs = m.beam_cs[j];
    const double ux = pci.x * cs.x - pci.y * cs.y, uy = pci.y * cs.x + pci.x * cs.y;
    const mcl::RayOrigin o = mcl::ray_origin(m, pci.z, pci.w);
    int r = m.P;
    uint32_t amb = o.amb0;
    unsigned np = 0;
    if (o.sane)
        r = mcl::trace_fp64<false, false>(m, nullptr, 0, mcl::kOriginBase, o.p0x, o.p0y, ux, uy, mcl::first_skip(m, o, m.dist), amb, np);
    if (mcl::takes_literal_march(m, o.sane, amb)) {
        if (mcl::level3_append(a.hdr, a.list, a.list_cap, (unsigned long long)ray)) return;
        r = mcl::march_exact(m, a.x[k], a.y[k], a.th[k] + (double)m.beam_angle[j]);
        atomicAdd(&a.hdr->level3, 1ull);
    }
    store_ray(a, ray, r);
}

// Level 3 for the listed rays: the literal march of cast_ray (cpp:611-650), one WAVE per ray (mcl::wave_march_exact_dir).
__global__ __launch_bounds__(kThreads) void k_query_exact(Args a)
{
    const mcl::RayArgs &m = a.ray;
    const int lane = threadIdx.x & 63;
    const unsigned long long wave_id = ((unsigned long long)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * kThreads) >> 6;
    const unsigned long long n = mcl::level3_listed(a.hdr, a.list_cap);
    unsigned long long done = 0;
    for (unsigned long long e = wave_id; e < n; e += nwaves) {
        const uint32_t ray = (uint32_t)a.list[e];
        const uint32_t k = ray / (uint32_t)m.B;
        const int j = (int)(ray - k * (uint32_t)m.B);
        const double angle = a.th[k] + (double)m.beam_angle[j];
        const double dx = cos(angle) * m.res, dy = sin(angle) * m.res;
        const int r = mcl::wave_march_exact_dir(m, a.x[k], a.y[k], dx, dy, lane);
        if (lane == 0) { store_ray(a, ray, r); ++done; }
    }
    if (lane == 0 && done) atomicAdd(&a.hdr->level3, done);
}

// the scan's table rows (E2) and which beams are valid (Q4: a finite reading whose row is below P)
__global__ __launch_bounds__(kThreads) void k_query_obs(Args a)
{
    const int j = (int)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
    if (j >= a.ray.B) return;
    const float o = a.obs[j];
    const int row = mcl::obs_index_of(o, a.ray.res, a.ray.P);
    const bool valid = o - o == 0.0f && row < a.ray.P;                // (o - o is NaN for NaN and +-inf)
    a.obs_row[j] = (uint32_t)row | (valid ? 0u : kObsInvalid);
}

// One wave per pose: lane l takes beams l, l + 64, ... in order -- the table gather and its fp64 sum (Q3: fixed lane strides,
// then a fixed butterfly), and the three counts (Q4) by ballot and popcount.
__global__ __launch_bounds__(kThreads) void k_query_score(Args a)
{
    const int lane = threadIdx.x & 63;
    const int k = (int)((blockIdx.x * (uint32_t)kThreads + threadIdx.x) >> 6);
    if (k >= a.K) return;                                               // (whole waves leave together)
    const int B = a.ray.B, P = a.ray.P, tw = P + 1;
    const uint16_t *st = a.steps + (size_t)k * B;
    double acc = 0.0;
    int n_valid = 0, n_agree = 0, n_miss = 0;
    for (int j0 = 0; j0 < B; j0 += 64) {
        const int j = j0 + lane;
        bool valid = false, agree = false, miss = false;
        if (j < B) {
            const uint32_t e = a.obs_row[j];
            const int row = (int)(e & ~kObsInvalid), r = (int)st[j];
            valid = !(e & kObsInvalid);
            const int diff = row > r ? row - r : r - row;
            agree = valid && diff <= a.tol_steps;
            miss = r == P;
            if (!a.lf_logw) acc += (double)a.L[(size_t)row * tw + r];
        }
        n_valid += __popcll(__ballot(valid));
        n_agree += __popcll(__ballot(agree));
        n_miss += __popcll(__ballot(miss));
    }
    acc = mcl::wave_sum(acc);
    if (lane == 0) {
        mcl_pose_score_t s;
        s.log_likelihood = a.lf_logw ? a.lf_logw[k] : acc;
        s.n_valid = n_valid; s.n_agree = n_agree; s.n_miss = n_miss; s.reserved = 0;
        a.out[k] = s;
    }
}

}  // namespace mcl_qry
