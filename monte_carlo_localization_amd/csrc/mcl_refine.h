// mcl_refine.h -- the pose refinement (mcl_refine_poses): the likelihood-field score of every pose of a dense
// window around each seed pose, and per seed the best pose, the weighted mean and the covariance of its window.  The arguments of
// its kernels and the kernels themselves; only mcl_refine.hip includes it.  A score comes from the per-beam arithmetic of k_lfield
// (mcl_lfield_core.h), so a window pose and a queried pose at the same place agree bit for bit.
#pragma once
#include "mcl_engine_internal.h"
#include "mcl_lfield_core.h"
#include "mcl_refine_core.h"

namespace mcl_rf {

struct Args {
    const double *seeds;            // M x 3 column-major
    int32_t M;
    Window win;
    int32_t n_total;                // M * n_win (< 2^27)
    // the scan and the field
    const double2 *beams;           // the used beams in beam order (R2)
    int nb;
    const uint16_t *D;              // H x W, row-major
    int W, H;
    double ox, oy, inv_res;
    const float *lf;                // K + 1 entries
    int K;
    double *score;                  // M x n_win: score[m * n_win + w]
    mcl_refine_result_t *out;       // M records
};

// One lane per window pose i = m * n_win + w, ix fastest: the lanes of a wave are neighbouring sub-cell positions of one heading
// (or of two, where a row of the window ends), so for one beam their end points fall into the same few cells of D.  The pose is
// formed from the seed (R1); the per-lane sincos is nothing against the beams.  The beam index is wave-uniform, its pair read
// from a uniform address.  The in-order fp64 sum of LF5 per lane.  LDS_TABLE as in k_lfield.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_refine_score(Args a)
{
    extern __shared__ float s_lf[];
    const float *lf = a.lf;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_lf[k] = a.lf[k];
        __syncthreads();
        lf = s_lf;
    }
    const int32_t i = (int32_t)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
    if (i >= a.n_total) return;
    const int32_t m = i / a.win.n_win, w = i - m * a.win.n_win;
    int32_t dx, dy, dt;
    offsets(a.win, w, dx, dy, dt);
    const double x = coord(a.seeds[m], dx, a.win.sx);
    const double y = coord(a.seeds[(size_t)a.M + m], dy, a.win.sx);
    const double th = coord(a.seeds[(size_t)2 * a.M + m], dt, a.win.st);
    double s, c;
    sincos(th, &s, &c);
    const double px = mcl::lf_cell_coord(x, a.ox, a.inv_res), py = mcl::lf_cell_coord(y, a.oy, a.inv_res);
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < a.nb; ++j)
        acc += (double)mcl::lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
    a.score[i] = acc;
}

// One workgroup per seed.  Pass 1: every lane keeps the best (R3) of its window poses l, l + 256, ...; a tree over the lanes finds
// the window's (the order is total: any association gives the same pose).  Pass 2: every lane adds R4's ten terms of the same
// poses in ascending order, a fixed tree adds the 256 partial sums; lane 0 writes the record.
__global__ __launch_bounds__(kThreads) void k_refine_reduce(Args a)
{
    __shared__ double s_sum[kSums][kThreads];
    __shared__ double s_s[kThreads];
    __shared__ int32_t s_q[kThreads], s_w[kThreads];
    const int32_t m = (int32_t)blockIdx.x, l = (int32_t)threadIdx.x;
    const int32_t n_win = a.win.n_win;
    const double *score = a.score + (size_t)m * (size_t)n_win;

    double bs = -__builtin_inf();
    int32_t bq = 0x7fffffff, bw = 0x7fffffff;                  // worse than every pose (the lanes beyond a small window keep it)
    for (int32_t w = l; w < n_win; w += kThreads) {
        int32_t dx, dy, dt;
        offsets(a.win, w, dx, dy, dt);
        const int32_t q = dx * dx + dy * dy + dt * dt;
        const double s = score[w];
        if (better(s, q, w, bs, bq, bw)) { bs = s; bq = q; bw = w; }
    }
    s_s[l] = bs; s_q[l] = bq; s_w[l] = bw;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (l < st && better(s_s[l + st], s_q[l + st], s_w[l + st], s_s[l], s_q[l], s_w[l])) {
            s_s[l] = s_s[l + st]; s_q[l] = s_q[l + st]; s_w[l] = s_w[l + st];
        }
        __syncthreads();
    }
    const double sb = s_s[0];
    const int32_t wb = s_w[0];
    int32_t bx, by, bt;
    offsets(a.win, wb, bx, by, bt);

    double acc[kSums];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    for (int32_t w = l; w < n_win; w += kThreads) accumulate(a.win, w, score[w], sb, bx, by, bt, acc);
#pragma unroll
    for (int k = 0; k < kSums; ++k) s_sum[k][l] = acc[k];
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if (l < st) {
#pragma unroll
            for (int k = 0; k < kSums; ++k) s_sum[k][l] += s_sum[k][l + st];
        }
        __syncthreads();
    }
    if (l == 0) {
        double sums[kSums];
#pragma unroll
        for (int k = 0; k < kSums; ++k) sums[k] = s_sum[k][0];
        const int32_t wc = (a.win.half_theta * a.win.nx + a.win.half_xy) * a.win.nx + a.win.half_xy;
        finish(a.win, a.seeds[m], a.seeds[(size_t)a.M + m], a.seeds[(size_t)2 * a.M + m], wb, sb, score[wc], sums, &a.out[m]);
    }
}

}  // namespace mcl_rf
