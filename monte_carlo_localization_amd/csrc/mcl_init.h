// mcl_init.h -- the particle initialisers (k_init_pose / _gaussian / _mixture / _global), k_fill, and k_obs_build_lt, the per-scan
// table of the basic and legacy ray kernels.
#pragma once

namespace mcl {

// Particle initialisation on the device.  Philox streams 5/6 (pose cloud) and 7 (global).
//   pose cloud, cpp:390-398: x = pose_x + n0*0.5, y = pose_y + n1*0.5, theta = wrap(pose_t + n2*0.4)
//   global, cpp:433-441:     cell = free[floor(u*n_free)], x = col*res + ox, y = row*res + oy, theta = u2*2pi
__global__ __launch_bounds__(256) void k_init_pose(double px, double py, double pt, int64_t n, int64_t first, uint32_t seed_lo,
                                                  uint32_t seed_hi, uint32_t init_idx, double *__restrict__ x,
                                                  double *__restrict__ y, double *__restrict__ th)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t g = (uint64_t)(first + i);
    const double TWO_M53 = 1.0 / 9007199254740992.0;
    const double TWO_PI = 2.0 * 3.14159265358979323846;
    u32x4 o = philox4x32((uint32_t)g, init_idx, 5u, (uint32_t)(g >> 32), seed_lo, seed_hi);
    double u1 = (double)(bits53(o.v[0], o.v[1]) + 1) * TWO_M53;
    double u2 = (double)bits53(o.v[2], o.v[3]) * TWO_M53;
    double rad = sqrt(-2.0 * log(u1));
    double n0 = rad * cos(TWO_PI * u2), n1 = rad * sin(TWO_PI * u2);
    o = philox4x32((uint32_t)g, init_idx, 6u, (uint32_t)(g >> 32), seed_lo, seed_hi);
    u1 = (double)(bits53(o.v[0], o.v[1]) + 1) * TWO_M53;
    u2 = (double)bits53(o.v[2], o.v[3]) * TWO_M53;
    double n2 = sqrt(-2.0 * log(u1)) * cos(TWO_PI * u2);
    x[i] = px + n0 * 0.5;
    y[i] = py + n1 * 0.5;
    th[i] = normalize_angle(pt + n2 * 0.4);
}

// the three normals of particle g of an initialisation (k_init_pose's draw: streams 5 and 6, the init counter)
__device__ __forceinline__ void init_normals(uint64_t g, uint32_t init_idx, uint32_t seed_lo, uint32_t seed_hi, double &n0, double &n1,
                                             double &n2)
{
    normals3(g, init_idx, 5u, 6u, seed_lo, seed_hi, n0, n1, n2);
}

// mcl_init_particles_gaussian (G1): k_init_pose's draw with the lower Cholesky factor of the covariance as six scalars
__global__ __launch_bounds__(256) void k_init_gaussian(double px, double py, double pt, double l00, double l10, double l11, double l20,
                                                      double l21, double l22, int64_t n, int64_t first, uint32_t seed_lo,
                                                      uint32_t seed_hi, uint32_t init_idx, double *__restrict__ x,
                                                      double *__restrict__ y, double *__restrict__ th)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double n0, n1, n2;
    init_normals((uint64_t)(first + i), init_idx, seed_lo, seed_hi, n0, n1, n2);
    x[i] = px + l00 * n0;
    y[i] = py + (l10 * n0 + l11 * n1);
    th[i] = normalize_angle(pt + (l20 * n0 + l21 * n1 + l22 * n2));
}

// mcl_init_particles_mixture: G1 per component.  Particle g belongs to the component whose prefix range holds g: the first c with
// g < end[c] (end = the inclusive prefix sums of the counts, so an empty component is never chosen).
struct MixComponent {
    double mean[3];
    double l[6];            // L00, L10, L11, L20, L21, L22
    int64_t end;
};
__global__ __launch_bounds__(256) void k_init_mixture(const MixComponent *__restrict__ comp, int n_comp, int64_t n, int64_t first,
                                                     uint32_t seed_lo, uint32_t seed_hi, uint32_t init_idx, double *__restrict__ x,
                                                     double *__restrict__ y, double *__restrict__ th)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t g = first + i;
    int lo = 0, hi = n_comp - 1;          // (g < end[n_comp - 1] = n_total)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (g < comp[mid].end) hi = mid; else lo = mid + 1;
    }
    const MixComponent m = comp[lo];
    double n0, n1, n2;
    init_normals((uint64_t)g, init_idx, seed_lo, seed_hi, n0, n1, n2);
    x[i] = m.mean[0] + m.l[0] * n0;
    y[i] = m.mean[1] + (m.l[1] * n0 + m.l[2] * n1);
    th[i] = normalize_angle(m.mean[2] + (m.l[3] * n0 + m.l[4] * n1 + m.l[5] * n2));
}

__global__ __launch_bounds__(256) void k_init_global(const uint32_t *__restrict__ free_cells, uint64_t n_free, int W, double res,
                                                    double ox, double oy, int64_t n, int64_t first, uint32_t seed_lo,
                                                    uint32_t seed_hi, uint32_t init_idx, double *__restrict__ x,
                                                    double *__restrict__ y, double *__restrict__ th)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t g = (uint64_t)(first + i);
    u32x4 o = philox4x32((uint32_t)g, init_idx, 7u, (uint32_t)(g >> 32), seed_lo, seed_hi);
    uint64_t k = bits53(o.v[0], o.v[1]);
    uint64_t pick = __umul64hi(k << 11, n_free);            // floor(k/2^53 * n_free)
    uint32_t cell = free_cells[pick];
    int row = (int)(cell / (uint32_t)W), col = (int)(cell - (uint32_t)row * (uint32_t)W);
    x[i] = col * res + ox;                                   // cpp:438
    y[i] = row * res + oy;                                   // cpp:439
    th[i] = (double)bits53(o.v[2], o.v[3]) * (1.0 / 9007199254740992.0) * (2.0 * 3.14159265358979323846);
}

__global__ void k_fill(double *__restrict__ p, int64_t n, double v)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// per-update transposed log table: Lt[d * bpad + j] = L[obs_idx[j] * (P+1) + d], straight from the raw ranges (every thread
// derives its beam's table row; row 0's threads also publish obs_idx for the kernels that read it).
// Ltr holds the same rows in reverse order (row rho = P - d), the form k_rays_cell indexes with "samples left"
__global__ void k_obs_build_lt(const float *__restrict__ obs, double res, int P, const float *__restrict__ L, int B, int bpad,
                               int32_t *__restrict__ obs_idx, float *__restrict__ Lt, float *__restrict__ Ltr)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int d = blockIdx.y, tw = P + 1;
    if (j >= bpad) return;
    float v = 0.f;
    if (j < B) {
        const int oi = obs_index_of(obs[j], res, P);
        if (d == 0) obs_idx[j] = oi;
        v = L[(size_t)oi * tw + d];
    }
    Lt[(size_t)d * bpad + j] = v;
    Ltr[(size_t)(tw - 1 - d) * bpad + j] = v;
}

}  // namespace mcl
