// mcl_lfield.h -- the likelihood-field ("endpoint") sensor model (mcl_set_likelihood_field): the exact integer
// distance field of the map and k_lfield, which turns every particle's beam end points into its log-weight.  Included by
// mcl_engine.hip only; the per-beam arithmetic is mcl_lfield_core.h's, shared with the lattice search.
#pragma once
#include "mcl_lfield_core.h"

namespace mcl {

// Column pass of LF1: g[c] = |dy| to the nearest occupied cell (> 50) of the same column, exact below `reach`, else `reach`
// (reach^2 >= K: a capped value only makes sums >= K, which the row pass clamps to K anyway).  One thread per cell, early exit.
__global__ __launch_bounds__(256) void k_lf_cols(const int8_t *__restrict__ grid, int W, int H, int reach, uint16_t *__restrict__ g)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)W * H) return;
    const int y = (int)(c / W), x = (int)(c - (int64_t)y * W);
    int d = reach;
    for (int k = 0; k < reach; ++k) {
        const bool up = y - k >= 0 && grid[(size_t)(y - k) * W + x] > 50;
        const bool dn = y + k < H && grid[(size_t)(y + k) * W + x] > 50;
        if (up || dn) { d = k; break; }
        if (y - k < 0 && y + k >= H) break;
    }
    g[c] = (uint16_t)d;
}

// Row pass: D[c] = min(K, min over |dx| < reach of dx^2 + g[x + dx]^2) in integers, exact (LF1); stops once dx^2 >= the best.
__global__ __launch_bounds__(256) void k_lf_rows(const uint16_t *__restrict__ g, int W, int H, int reach, int K, uint16_t *__restrict__ D)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)W * H) return;
    const int y = (int)(c / W), x = (int)(c - (int64_t)y * W);
    const uint16_t *row = g + (size_t)y * W;
    int best = K;
    for (int dx = 0; dx < reach && dx * dx < best; ++dx) {
        if (x - dx >= 0) { const int v = row[x - dx]; best = min(best, dx * dx + v * v); }
        if (x + dx < W) { const int v = row[x + dx]; best = min(best, dx * dx + v * v); }
    }
    D[c] = (uint16_t)best;
}

struct LfArgs {
    const double *x, *y, *th;
    int64_t n;
    const double2 *beams;          // the used beams of the scan in beam order (LF3): (r_j cos a_j / res, r_j sin a_j / res)
    int nb;
    const uint16_t *D;             // H x W, row-major
    int W, H;
    double ox, oy, inv_res;
    const float *lf;               // K + 1 entries
    int K;
    double *logw;
};

// One particle per lane, the beams in order: logw_i = sum_j (double)Lf[D[cell_ij]] (LF5), the in-order fp64 sum bit for bit.  The
// beam index is wave-uniform, so its pair is read from a uniform address; per beam: four fp64 FMAs, two floors, the bounds test,
// two conversions, one 2-byte gather from D, the table read and an fp64 add.  LDS_TABLE: Lf is staged in LDS (K < kLfLdsEntries).
template <bool LDS_TABLE>
__global__ __launch_bounds__(256) void k_lfield(LfArgs a)
{
    extern __shared__ float s_lf[];
    const float *lf = a.lf;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += 256) s_lf[k] = a.lf[k];
        __syncthreads();
        lf = s_lf;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double s, c;
    sincos(a.th[i], &s, &c);
    // the particle in cell units; the end point of beam j is (px + c u_j - s v_j, py + s u_j + c v_j) (LF4, the rotation form)
    const double px = lf_cell_coord(a.x[i], a.ox, a.inv_res), py = lf_cell_coord(a.y[i], a.oy, a.inv_res);
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < a.nb; ++j) {
        acc += (double)lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
    }
    a.logw[i] = acc;
}

}  // namespace mcl
