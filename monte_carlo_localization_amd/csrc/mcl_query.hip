// mcl_query.hip -- mcl_query_scans / mcl_score_poses: the expected scan of K poses that are not particles and
// how well a scan supports each of them.  Called outside the update: it reads the map, the beams and the static tables, writes
// only buffers of its own (struct mcl_query) and leaves every engine state as it was.
//
// A call, on the engine's stream:
//   (copy)         the poses (and the scan) from pinned staging
//   k_mount_poses  (a sensor mount set) the poses given are base poses: every kernel below reads the sensors'
//   k_query_rays   one lane per ray: levels 2 and 3 of the ray stage on the isotropic field; level-3 rays are listed
//   k_query_exact  one wave per listed ray: the literal march
//   k_query_obs    (score) table row and validity of every beam
//   k_lfield       (score, likelihood field on) the K log-likelihoods, through the update's own kernel on the query's buffers
//   k_query_score  (score) one wave per pose: the table sum in a fixed order, the three counts
//   (copy)         the results; one host wait
#include "mcl_query.h"
#include "mcl_side_buffers.h"
#include "mcl_mount.h"

#include <algorithm>
#include <cstring>

using namespace mcl_qry;
using namespace mcl_side;
using mcl_host::fail;

// the buffers of the query, kept between calls and grown with K, B and K * B
struct mcl_query {
    DevBuf<double> d_pose;                      // 3 K: x, y, theta columns
    HostBuf<double> h_pose;
    DevBuf<double> d_pose_s;                    // 3 K: their sensor poses (only with a mount; mcl_mount_poses)
    DevBuf<double> d_org_pose, d_org;           // mcl_beam_origins: 3 K sensor poses in, 2 K B origins out, and their pinned staging
    HostBuf<double> h_org_pose, h_org;
    DevBuf<uint16_t> d_steps;
    DevBuf<float> d_ranges;
    DevBuf<unsigned long long> d_list;
    DevBuf<Header> d_hdr;
    HostBuf<Header> h_hdr;
    DevBuf<float> d_obs;
    HostBuf<float> h_obs;
    DevBuf<uint32_t> d_obs_row;
    DevBuf<double2> d_lf_beams;
    HostBuf<double2> h_lf_beams;
    DevBuf<double> d_lf_logw;
    DevBuf<mcl_pose_score_t> d_out;
    HostBuf<mcl_pose_score_t> h_out;
    unsigned long long last_level3 = 0;
    size_t device_bytes = 0;
};

namespace {

// room for K poses of B beams; ranges / the score's buffers only for a call that wants them.  (device_bytes counts what was ever
// asked of the device: a diagnostic, mcl_get_query_counters.)
int query_alloc(mcl_engine *h, mcl_query *q, size_t K, size_t B, bool want_ranges, bool score)
{
    size_t *bytes = &q->device_bytes;
    const size_t rays = K * B;
    SIDE_TRY(q->d_hdr.reserve(h, 1, bytes));
    SIDE_TRY(q->h_hdr.reserve(h, 1));
    SIDE_TRY(q->d_pose.reserve(h, 3 * K, bytes));
    SIDE_TRY(q->h_pose.reserve(h, 3 * K));
    SIDE_TRY(q->d_steps.reserve(h, rays, bytes));
    SIDE_TRY(q->d_list.reserve(h, (size_t)std::min<unsigned long long>(rays, kListCap), bytes));
    if (want_ranges) SIDE_TRY(q->d_ranges.reserve(h, rays, bytes));
    if (!score) return MCL_OK;
    SIDE_TRY(q->d_obs.reserve(h, B, bytes));
    SIDE_TRY(q->h_obs.reserve(h, B));
    SIDE_TRY(q->d_obs_row.reserve(h, B, bytes));
    // what only a score needs is as large as the poses / the scan have room: grown here when they have grown since, in any call
    const size_t room_k = q->d_pose.cap / 3, room_b = q->d_obs.cap;
    SIDE_TRY(q->d_out.reserve(h, room_k, bytes));
    SIDE_TRY(q->h_out.reserve(h, room_k));
    if (h->lf_on) {
        SIDE_TRY(q->d_lf_beams.reserve(h, room_b, bytes));
        SIDE_TRY(q->h_lf_beams.reserve(h, room_b));
        SIDE_TRY(q->d_lf_logw.reserve(h, room_k, bytes));
    }
    return MCL_OK;
}

// what both calls check, in the order of Q6: arguments, then readiness
int query_check(mcl_engine *h, const double *poses, int32_t K, const char *who)
{
    if (!poses) return fail(h, MCL_ERR_INVALID_ARG, std::string(who) + ": poses is null");
    if (K < 1 || K > kMaxPoses) return fail(h, MCL_ERR_INVALID_ARG, std::string(who) + ": K must be in [1, 65536]");
    if (!h->have_map || h->B <= 0 || !h->d_beam_cs) return fail(h, MCL_ERR_NOT_READY, std::string(who) + ": map and beam angles must be set first");
    if (h->B > 65535) return fail(h, MCL_ERR_UNSUPPORTED, std::string(who) + ": more than 65535 beams");
    return MCL_OK;
}

// the poses to the device, the rays cast: d_steps (and d_ranges) hold the K x B results when the stream gets there
int query_cast(mcl_engine *h, mcl_query *q, Args &a, const double *poses, int32_t K, bool want_ranges)
{
    std::memcpy(q->h_pose, poses, (size_t)3 * K * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(q->d_pose, q->h_pose, (size_t)3 * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(q->d_hdr, 0, sizeof(Header), h->stream));
    fill_ray_args(h, a.ray);
    a.x = q->d_pose; a.y = q->d_pose + K; a.th = q->d_pose + 2 * (size_t)K;
    if (h->mounted) {
        SIDE_TRY(q->d_pose_s.reserve(h, q->d_pose.cap, &q->device_bytes));
        double *sx = q->d_pose_s, *sy = q->d_pose_s + K, *sth = q->d_pose_s + 2 * (size_t)K;
        mcl::launch_mount_poses(h->stream, a.x, a.y, a.th, K, h->mount, sx, sy, sth);
        HIPCHK(h, hipGetLastError());
        a.x = sx; a.y = sy; a.th = sth;
    }
    a.K = K;
    a.steps = q->d_steps;
    a.ranges = want_ranges ? q->d_ranges : nullptr;
    a.miss_range = (float)h->cfg.max_range_m;
    a.list = q->d_list; a.list_cap = (unsigned long long)q->d_list.cap;
    a.hdr = q->d_hdr;
    const int64_t rays = (int64_t)K * h->B;
    hipLaunchKernelGGL(k_query_rays, dim3((unsigned)((rays + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    // one wave per listed ray, as many as the list can hold at this size
    const unsigned grid_exact = level3_grid(h, std::min<int64_t>(rays, (int64_t)q->d_list.cap));
    hipLaunchKernelGGL(k_query_exact, dim3(grid_exact), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

int query_finish(mcl_engine *h, mcl_query *q)
{
    HIPCHK(h, hipMemcpyAsync(q->h_hdr, q->d_hdr, sizeof(Header), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait
    q->last_level3 = q->h_hdr->level3;
    return MCL_OK;
}

}  // namespace

void query_free(struct mcl_query *q) { delete q; }

extern "C" {

int mcl_query_scans(mcl_engine_t *h, const double *poses_colmajor, int32_t K, float *ranges_m, uint16_t *steps)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    SIDE_TRY(query_check(h, poses_colmajor, K, "query_scans"));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->qry) h->qry = new mcl_query();
    mcl_query *q = h->qry;
    SIDE_TRY(query_alloc(h, q, (size_t)K, (size_t)h->B, ranges_m != nullptr, false));
    Args a{};
    SIDE_TRY(query_cast(h, q, a, poses_colmajor, K, ranges_m != nullptr));
    const size_t rays = (size_t)K * h->B;
    if (ranges_m) HIPCHK(h, hipMemcpyAsync(ranges_m, q->d_ranges, rays * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (steps) HIPCHK(h, hipMemcpyAsync(steps, q->d_steps, rays * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
    return query_finish(h, q);
}

int mcl_score_poses(mcl_engine_t *h, const double *poses_colmajor, int32_t K, const float *obs, int32_t n_beams, int32_t tol_steps,
                    mcl_pose_score_t *out)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!obs || !out) return fail(h, MCL_ERR_INVALID_ARG, "score_poses: obs / out is null");
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_INVALID_ARG, "score_poses: weight_mode LOG only (mcl_query_scans works in PRODUCT mode)");
    SIDE_TRY(query_check(h, poses_colmajor, K, "score_poses"));
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "score_poses: n_beams does not match the beam angles");
    if (tol_steps < 0 || tol_steps > h->P) return fail(h, MCL_ERR_INVALID_ARG, "score_poses: tol_steps must be in [0, MAX_RANGE_PX]");
    const bool lf = h->lf_on;
    if (lf && (h->lf_K < 0 || !h->d_lf_D)) return fail(h, MCL_ERR_NOT_READY, "score_poses: the likelihood field of this map is not built");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->qry) h->qry = new mcl_query();
    mcl_query *q = h->qry;
    SIDE_TRY(query_alloc(h, q, (size_t)K, (size_t)h->B, false, true));
    Args a{};
    SIDE_TRY(query_cast(h, q, a, poses_colmajor, K, false));
    const int B = h->B;
    std::memcpy(q->h_obs, obs, (size_t)B * sizeof(float));
    HIPCHK(h, hipMemcpyAsync(q->d_obs, q->h_obs, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    a.obs = q->d_obs; a.obs_row = q->d_obs_row;
    a.L = h->d_L;
    a.tol_steps = tol_steps;
    a.out = q->d_out;
    hipLaunchKernelGGL(k_query_obs, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    if (lf) {
        const int nb = mcl_host::lf_used_beams(h, q->h_obs, 1, q->h_lf_beams);
        if (nb > 0)
            HIPCHK(h, hipMemcpyAsync(q->d_lf_beams, q->h_lf_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
        SIDE_TRY(mcl_host::launch_lfield_on(h, a.x, a.y, a.th, K, q->d_lf_beams, nb, q->d_lf_logw));
        a.lf_logw = q->d_lf_logw;
    }
    hipLaunchKernelGGL(k_query_score, dim3((unsigned)((K + 3) / 4)), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(q->h_out, q->d_out, (size_t)K * sizeof(mcl_pose_score_t), hipMemcpyDeviceToHost, h->stream));
    SIDE_TRY(query_finish(h, q));
    std::memcpy(out, q->h_out, (size_t)K * sizeof(mcl_pose_score_t));
    return MCL_OK;
}

int mcl_mount_poses(mcl_engine_t *h, const double *poses_colmajor, int64_t k, double *out_colmajor)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!poses_colmajor || !out_colmajor) return fail(h, MCL_ERR_INVALID_ARG, "mount_poses: poses / out is null");
    if (k < 1 || k > kMaxPoses) return fail(h, MCL_ERR_INVALID_ARG, "mount_poses: k must be in [1, 65536]");
    const size_t K = (size_t)k;
    if (!h->mounted) {                          // no mount: the sensor is the base
        std::memmove(out_colmajor, poses_colmajor, 3 * K * sizeof(double));
        return MCL_OK;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->qry) h->qry = new mcl_query();
    mcl_query *q = h->qry;
    SIDE_TRY(q->d_pose.reserve(h, 3 * K, &q->device_bytes));
    SIDE_TRY(q->h_pose.reserve(h, 3 * K));
    SIDE_TRY(q->d_pose_s.reserve(h, q->d_pose.cap, &q->device_bytes));
    std::memcpy(q->h_pose, poses_colmajor, 3 * K * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(q->d_pose, q->h_pose, 3 * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    mcl::launch_mount_poses(h->stream, q->d_pose, q->d_pose + K, q->d_pose + 2 * K, k, h->mount, q->d_pose_s, q->d_pose_s + K, q->d_pose_s + 2 * K);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(q->h_pose, q->d_pose_s, 3 * K * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(out_colmajor, q->h_pose, 3 * K * sizeof(double));
    return MCL_OK;
}

// DS2 for k given sensor poses and the engine's table of per-beam offsets: one lane per (pose, beam), the pose's
// sincos per lane (nothing against a read-back), frame_point as k_rays_deskew calls it: the metric origin, also for a garbage heading,
// whose ray k_rays_deskew starts from a NaN pixel position and marches literally from here.  Buffers of its own.
static __global__ __launch_bounds__(256) void k_beam_origins(const double *__restrict__ x, const double *__restrict__ y,
                                                             const double *__restrict__ th, int64_t k, int B, const double *__restrict__ off,
                                                             double *__restrict__ ox, double *__restrict__ oy)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= k * B) return;
    const int64_t i = e / B;
    const int j = (int)(e - i * B);
    double s, c;
    sincos(th[i], &s, &c);
    double xb, yb;
    mcl::frame_point(x[i], y[i], s, c, off ? off[j] : 0.0, off ? off[(size_t)B + j] : 0.0, xb, yb);
    ox[e] = xb; oy[e] = yb;
}

int mcl_beam_origins(mcl_engine_t *h, const double *sensor_poses_colmajor, int64_t k, double *xy)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!sensor_poses_colmajor || !xy) return fail(h, MCL_ERR_INVALID_ARG, "beam_origins: poses / xy is null");
    if (k < 1 || k > kMaxPoses) return fail(h, MCL_ERR_INVALID_ARG, "beam_origins: k must be in [1, 65536]");
    if (h->B <= 0) return fail(h, MCL_ERR_NOT_READY, "beam_origins: no beam angles are set");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->qry) h->qry = new mcl_query();
    mcl_query *q = h->qry;
    const size_t K = (size_t)k, KB = K * (size_t)h->B;
    SIDE_TRY(q->d_org_pose.reserve(h, 3 * K, &q->device_bytes));
    SIDE_TRY(q->h_org_pose.reserve(h, 3 * K));
    SIDE_TRY(q->d_org.reserve(h, 2 * KB, &q->device_bytes));
    SIDE_TRY(q->h_org.reserve(h, 2 * KB));
    std::memcpy(q->h_org_pose, sensor_poses_colmajor, 3 * K * sizeof(double));
    HIPCHK(h, hipMemcpyAsync(q->d_org_pose, q->h_org_pose, 3 * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_beam_origins, dim3((unsigned)((KB + 255) / 256)), dim3(256), 0, h->stream, q->d_org_pose.p, q->d_org_pose.p + K,
                       q->d_org_pose.p + 2 * K, k, h->B, h->ds_on ? h->d_ds_off() : (const double *)nullptr, q->d_org.p, q->d_org.p + KB);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(q->h_org, q->d_org, 2 * KB * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(xy, q->h_org, 2 * KB * sizeof(double));
    return MCL_OK;
}

int mcl_get_query_counters(const mcl_engine_t *h, uint64_t out[2])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    out[0] = h->qry ? h->qry->last_level3 : 0;
    out[1] = h->qry ? (uint64_t)h->qry->device_bytes : 0;
    return MCL_OK;
}

}  // extern "C"
