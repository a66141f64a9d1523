// Odometry motion models (mcl_set_motion_model; include/mcl_hip_engine.h M1-M6) and the Gaussian pose
// initialisation (G1).  Included by mcl_kernels.h: the per-child step below is the body the odometry forms of the resampling
// kernel run instead of the reference's bicycle arc, and the one mcl_host_motion_sample runs on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcl {

// What an update with MCL_MOTION_DIFF / MCL_MOTION_OMNI hands its resampling kernel beside ResampleArgs (whose layout stays as it
// is): the model and the six per-update scalars of mcl_host_motion_scalars, out[0..5].
//   DIFF: s = {rot1, trans, rot2, sigma1, sigma_t, sigma2}      OMNI: s = {bearing, trans, rot, sigma_t, sigma_r, sigma_s}
struct OdoArgs {
    int model;                        // 1 DIFF, 2 OMNI (wave-uniform: one kernel, one uniform branch)
    int pad;
    double s[6];
};

// M5: the child of pose (x, y, th) with the normals (n0, n1, n2); th comes back NOT normalised (the caller's normalize_angle).
// One sincos, no division, no atan2.
__host__ __device__ __forceinline__ void odo_step(const OdoArgs &o, double &x, double &y, double &th, double n0, double n1, double n2)
{
    double sn, cs;
    if (o.model == 1) {
        const double r1 = o.s[0] - o.s[3] * n0;
        const double t = o.s[1] - o.s[4] * n1;
        const double r2 = o.s[2] - o.s[5] * n2;
        sincos(th + r1, &sn, &cs);
        x = x + t * cs;
        y = y + t * sn;
        th = th + (r1 + r2);
    } else {
        const double t = o.s[1] + o.s[3] * n0;
        const double r = o.s[2] + o.s[4] * n1;
        const double s = o.s[5] * n2;
        sincos(o.s[0] + th, &sn, &cs);
        x = x + (t * cs + s * sn);
        y = y + (t * sn - s * cs);
        th = th + r;
    }
}

}  // namespace mcl
