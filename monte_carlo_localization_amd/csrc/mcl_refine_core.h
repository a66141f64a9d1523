// mcl_refine_core.h -- the arithmetic of the pose refinement (mcl_refine_poses, DESIGN.md §4.14, rules R1 / R3 / R4 of
// include/mcl_hip_engine.h) that the device (mcl_refine.h) and the host restatement (mcl_host_refine_*, mcl_host_math.hip) share:
// the window's geometry, the order of R3 and the step from R4's ten sums to a result record.  No kernels here.
#pragma once
#include "../../include/mcl_hip_engine.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mcl_rf {

constexpr int kThreads = 256;                  // lanes of a reduction workgroup == partial sums of R4
constexpr int kSums = 10;                      // S, 3 first moments, 6 second moments (00 01 02 11 12 22)
constexpr int32_t kMaxWindow = 32768, kMaxSeeds = 4096;

// the window of a config on a map of resolution `res` (R1); ny == nx
struct Window {
    int32_t half_xy, half_theta, nx, nt, n_win;
    double sx, st;                              // the steps: sx formed once, here, on the host
};

inline Window window_of(const mcl_refine_config_t &c, double res)
{
    Window w{};
    w.half_xy = c.half_xy; w.half_theta = c.half_theta;
    w.nx = 2 * c.half_xy + 1; w.nt = 2 * c.half_theta + 1;
    w.n_win = w.nx * w.nx * w.nt;
    w.sx = c.step_xy_cells * res; w.st = c.step_theta_rad;
    return w;
}

// window index -> integer offsets from the window centre
__host__ __device__ inline void offsets(const Window &g, int32_t w, int32_t &dx, int32_t &dy, int32_t &dt)
{
    const int32_t row = w / g.nx;
    const int32_t it = row / g.nx;
    dx = w - row * g.nx - g.half_xy;
    dy = row - it * g.nx - g.half_xy;
    dt = it - g.half_theta;
}

// a window coordinate: the multiply and the add each rounded, never one fma (R1)
__host__ __device__ inline double coord(double c0, int32_t d, double step)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(c0, __dmul_rn((double)d, step));
#else
    const double t = (double)d * step;         // (the unit is compiled with -ffp-contract=off)
    return c0 + t;
#endif
}

// R3: is (sa, qa, wa) better than (sb, qb, wb)?  Scores are finite or -inf, never NaN.
__host__ __device__ inline bool better(double sa, int32_t qa, int32_t wa, double sb, int32_t qb, int32_t wb)
{
    if (sa != sb) return sa > sb;
    if (qa != qb) return qa < qb;
    return wa < wb;
}

// the weight of a window pose and its ten terms about the best pose (R4), added to `acc`
__host__ __device__ inline void accumulate(const Window &g, int32_t w, double s, double sb, int32_t bx, int32_t by, int32_t bt, double acc[kSums])
{
    int32_t dx, dy, dt;
    offsets(g, w, dx, dy, dt);
    const double wi = s == -__builtin_inf() ? 0.0 : exp(s - sb);
    const double ux = (double)(dx - bx), uy = (double)(dy - by), ut = (double)(dt - bt);
    acc[0] += wi;
    acc[1] += wi * ux; acc[2] += wi * uy; acc[3] += wi * ut;
    acc[4] += wi * (ux * ux); acc[5] += wi * (ux * uy); acc[6] += wi * (ux * ut);
    acc[7] += wi * (uy * uy); acc[8] += wi * (uy * ut); acc[9] += wi * (ut * ut);
}

// from the best pose (window index wb, score sb), the centre's score and the ten sums to the record of one seed (R3 / R4)
__host__ __device__ inline void finish(const Window &g, double x0, double y0, double t0, int32_t wb, double sb, double s_centre,
                                       const double sums[kSums], mcl_refine_result_t *out)
{
    int32_t bx, by, bt;
    offsets(g, wb, bx, by, bt);
    const double step[3] = {g.sx, g.sx, g.st};
    out->best[0] = coord(x0, bx, g.sx); out->best[1] = coord(y0, by, g.sx); out->best[2] = coord(t0, bt, g.st);
    out->best_log_likelihood = sb;
    out->seed_log_likelihood = s_centre;
    out->best_index = wb;
    const double S = sums[0];
    double m[3] = {0.0, 0.0, 0.0}, C[3][3] = {};
    if (S > 0.0) {                              // (a void seed: m = 0, C = 0)
        for (int a = 0; a < 3; ++a) m[a] = sums[1 + a] / S;
        int k = 4;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b, ++k) {
                const double mm = m[a] * m[b];
                C[a][b] = C[b][a] = sums[k] / S - mm;
            }
    }
    for (int a = 0; a < 3; ++a) {
        const double d = step[a] * m[a];
        out->mean[a] = out->best[a] + d;
        for (int b = a; b < 3; ++b) {
            const double ss = step[a] * step[b];
            double v = ss * C[a][b];
            if (a == b) v = v + ss / 12.0;
            out->cov[3 * a + b] = out->cov[3 * b + a] = v;
        }
    }
    out->weight_sum = S;
}

}  // namespace mcl_rf
