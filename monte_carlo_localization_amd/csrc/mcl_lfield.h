// mcl_lfield.h -- the likelihood-field ("endpoint") sensor model (mcl_set_likelihood_field): the exact integer
// distance field of the map and k_lfield, which turns every particle's beam end points into its log-weight; and the three kernels
// of an update with beam skipping (§4.24).  Included by mcl_engine.hip only; the per-beam arithmetic is mcl_lfield_core.h's,
// shared with the lattice search.
#pragma once
#include "../../include/mcl_hip_engine.h"
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

// ---- beam skipping (mcl_set_beam_skip): a counting pass, the plan, a second summing pass over the kept beams
// The per-workgroup counter row of k_lfield_agree lives in LDS up to this many used beams (8 KiB), and only while the staged
// table and the row together stay within k_lfield's largest request (kLfLdsEntries words, 32 KiB: five workgroups per CU as
// before); beyond either, one global atomic per wave per beam.
constexpr int kBsLdsBeams = 2048;
// The counting pass is persistent: at most this many workgroups per CU (the 32 waves a CU holds), each walking tiles of 256
// particles, so that the counter rows are flushed once per workgroup and not once per tile.
constexpr int kBsWorkgroupsPerCu = 8;

struct BsCountArgs {
    unsigned int *cnt;             // nb counters, zeroed in-stream before the launch
    int64_t tiles;                 // ceil(n / 256)
    uint32_t ka;                   // BS1
    int cnt_off;                   // the LDS counter row starts at this word (behind the staged table)
};

// Pass 1: k_lfield's lanes and loop -- one particle per lane, the beams in order, the full LF5 sum to logw -- and per beam the
// agreement bit D < Ka (BS1): one ballot and population count per wave, added by one lane to the workgroup's LDS counter row
// (LDS_CNT) or straight to the global counter.  Lanes beyond n carry a NaN position -- every end point off the map, no load, no
// agreement -- and take part in the barriers.  The row is flushed once, by contiguous lanes to contiguous counters.
template <bool LDS_TABLE, bool LDS_CNT>
__global__ __launch_bounds__(256) void k_lfield_agree(LfArgs a, BsCountArgs b)
{
    extern __shared__ float s_lf[];
    const float *lf = a.lf;
    unsigned int *s_cnt = reinterpret_cast<unsigned int *>(s_lf + b.cnt_off);
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += 256) s_lf[k] = a.lf[k];
        lf = s_lf;
    }
    if constexpr (LDS_CNT)
        for (int j = threadIdx.x; j < a.nb; j += 256) s_cnt[j] = 0u;
    if constexpr (LDS_TABLE || LDS_CNT) __syncthreads();
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    const bool first_lane = (threadIdx.x & 63) == 0;
    for (int64_t tile = blockIdx.x; tile < b.tiles; tile += gridDim.x) {
        const int64_t i = tile * 256 + threadIdx.x;
        const bool live = i < a.n;
        double s = 0.0, c = 1.0, px = NAN, py = NAN;
        if (live) {
            sincos(a.th[i], &s, &c);
            px = lf_cell_coord(a.x[i], a.ox, a.inv_res);
            py = lf_cell_coord(a.y[i], a.oy, a.inv_res);
        }
        double acc = 0.0;
        // the wave's agreement count of beam j, added by its first lane
        auto count = [&](int j, uint32_t d) {
            const unsigned long long agree = __ballot(d < b.ka);
            if (first_lane && agree) {
                const unsigned int k = (unsigned int)__popcll(agree);
                if constexpr (LDS_CNT)
                    __hip_atomic_fetch_add(&s_cnt[j], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                else
                    __hip_atomic_fetch_add(&b.cnt[j], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        };
        // four beams at a time by hand (the ballot keeps the compiler from unrolling as it does in k_lfield): four gathers in
        // flight, then the adds in beam order
        int j = 0;
        for (; j + 4 <= a.nb; j += 4) {
            uint32_t d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = lf_beam_dist(a.beams[j + u], s, c, px, py, W, H, a.W, a.D);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += (double)(d[u] == kLfOffMap ? off : lf[d[u]]);
#pragma unroll
            for (int u = 0; u < 4; ++u) count(j + u, d[u]);
        }
        for (; j < a.nb; ++j) {
            const uint32_t d = lf_beam_dist(a.beams[j], s, c, px, py, W, H, a.W, a.D);
            acc += (double)(d == kLfOffMap ? off : lf[d]);
            count(j, d);
        }
        if (live) a.logw[i] = acc;
    }
    if constexpr (LDS_CNT) {
        __syncthreads();
        for (int j = threadIdx.x; j < a.nb; j += 256) {
            const unsigned int k = s_cnt[j];
            if (k) __hip_atomic_fetch_add(&b.cnt[j], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

struct BsPlanArgs {
    const unsigned int *cnt;       // nb counts (BS2)
    const double2 *beams;          // the used beams
    int nb;
    int64_t n, min_count;          // BS3, formed on the host
    int min_skipped, ka;           // BS4, BS1
    uint8_t *kept;                 // nb: 1 summed, 2 skipped
    double2 *beams_kept;           // the kept beams in beam order
    mcl_beam_skip_state_t *st;
};

// The plan, one workgroup: n_skipped by a block reduction, BS4, then the kept beams' pairs compacted in beam order (a ballot
// scan per 256 beams behind a running base) and the state record.
__global__ __launch_bounds__(256) void k_lf_skip_plan(BsPlanArgs p)
{
    __shared__ int s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int mine = 0;
    for (int j = threadIdx.x; j < p.nb; j += 256) mine += (int64_t)p.cnt[j] < p.min_count;
    for (int o = 32; o; o >>= 1) mine += __shfl_down(mine, o);
    if (lane == 0) s_wave[wave] = mine;
    __syncthreads();
    const int n_skipped = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    const bool all = n_skipped >= p.min_skipped;
    __syncthreads();
    int base = 0;
    for (int j0 = 0; j0 < p.nb; j0 += 256) {
        const int j = j0 + (int)threadIdx.x;
        const bool in = j < p.nb;
        const bool keep = in && (all || (int64_t)p.cnt[j] >= p.min_count);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) pos += s_wave[w];
        base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        if (in) p.kept[j] = keep ? 1 : 2;
        if (keep) p.beams_kept[pos] = p.beams[j];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        mcl_beam_skip_state_t st;
        st.n_particles = p.n; st.min_count = p.min_count;
        st.n_used = p.nb; st.n_kept = base; st.n_skipped = n_skipped; st.min_skipped = p.min_skipped;
        st.integrate_all = all ? 1 : 0; st.ka = p.ka;
        *p.st = st;
    }
}

// Pass 2: k_lfield over the compacted list (a.beams), its beam count read from the state record.  Nothing skipped: every
// workgroup returns at once and pass 1's sums stand; else logw is overwritten with the in-order sum over the kept beams (BS5).
template <bool LDS_TABLE>
__global__ __launch_bounds__(256) void k_lfield_kept(LfArgs a, const mcl_beam_skip_state_t *__restrict__ st)
{
    extern __shared__ float s_lf[];
    const int nb = st->n_kept;
    if (nb == st->n_used) return;
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
    const double px = lf_cell_coord(a.x[i], a.ox, a.inv_res), py = lf_cell_coord(a.y[i], a.oy, a.inv_res);
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < nb; ++j) {
        acc += (double)lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
    }
    a.logw[i] = acc;
}

}  // namespace mcl
