// mcl_mount.h -- the sensor mount (mcl_set_sensor_mount): the sensor's pose of a base pose, on the device, and the
// one-line kernel of mcl_sensor_update_fuse.  Included by mcl_engine.hip (the sensor stages of an update) and mcl_query.hip (the
// pose query and mcl_mount_poses); the host's statement of the same rule is mcl_host_sensor_mount (mcl_host_math.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mcl_ray_core.h"

namespace mcl {

// SM2, the only statement of it on the device: fp64, in this order, no contraction (the library is built with -ffp-contract=off);
// the heading is one rounded add and is not wrapped.  Non-finite inputs give what these operations give.
__device__ __forceinline__ void mount_pose(double x, double y, double th, double mx, double my, double mth, double &xs, double &ys,
                                           double &ths)
{
    double s, c;
    sincos(th, &s, &c);
    frame_point(x, y, s, c, mx, my, xs, ys);
    ths = th + mth;
}

// One pose per lane, three fp64 columns in and three out (48 bytes per pose, consecutive lanes on consecutive addresses); no LDS,
// no atomics; lanes beyond n do nothing.  The grid is sized from n (launch_mount_poses).  (static, like k_add_logw: the header
// is part of two translation units of one library, each of which gets its own copy.)
static __global__ __launch_bounds__(256) void k_mount_poses(const double *__restrict__ x, const double *__restrict__ y,
                                                     const double *__restrict__ th, int64_t n, double mx, double my, double mth,
                                                     double *__restrict__ xs, double *__restrict__ ys, double *__restrict__ ths)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double ox, oy, oth;
    mount_pose(x[i], y[i], th[i], mx, my, mth, ox, oy, oth);
    xs[i] = ox; ys[i] = oy; ths[i] = oth;
}

// mcl_sensor_update_fuse: logw_i <- prev_i + logw_i, one rounded fp64 add, prev the left operand (k_add_carry adds its operand on
// the right; IEEE addition gives the same bits either way, and -inf stays -inf -- this kernel states the order the rule is written in)
[[maybe_unused]] static __global__ void k_add_logw(double *__restrict__ logw, const double *__restrict__ prev, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) logw[i] = prev[i] + logw[i];
}

// n >= 1 poses on `stream`; the output columns must not overlap the input's
inline void launch_mount_poses(hipStream_t stream, const double *x, const double *y, const double *th, int64_t n, const double m[3],
                               double *xs, double *ys, double *ths)
{
    hipLaunchKernelGGL(k_mount_poses, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, th, n, m[0], m[1], m[2], xs, ys, ths);
}

}  // namespace mcl
