// mcl_refine.h -- the pose refinement (mcl_refine_poses; mcl_refine_poses_beam, §4.18): the score of every pose
// of a dense window around each seed pose, and per seed the best pose, the weighted mean and the covariance of its window.  The
// arguments of its kernels and the kernels themselves; only mcl_refine.hip includes it.  A likelihood-field score comes from the
// per-beam arithmetic of k_lfield (mcl_lfield_core.h), a beam-model score from the ray functions the update and the pose
// query call (mcl_ray_core.h), so a window pose and a queried pose at the same place agree bit for bit under either model.
#pragma once
#include "mcl_device_math.h"
#include "mcl_engine_internal.h"
#include "mcl_lfield_core.h"
#include "mcl_ray_core.h"
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

// what k_refine_beam_score counts (stats only: never part of a score)
struct BeamHeader {
    unsigned long long level3;      // rays the literal march decided
};

struct BeamArgs {
    mcl::RayArgs ray;               // the map, P, the beam directions and angles, force_exact: what trace_fp64 and the march read
    const double *seeds;            // M x 3 column-major
    int32_t M;
    Window win;
    int32_t n_total;                // M * n_win (< 2^27)
    int32_t pose0;                  // first pose of this launch of k_refine_beam_score (kPosesPerLaunch)
    const float *obs;               // B readings
    int32_t beam_stride, nb;        // nb = used beams: j = u * beam_stride, u < nb
    uint32_t *row_base;             // per used beam: row_j * (P + 1), where its row of L starts (RB3)
    const float *L;                 // [row][step], P + 1 columns: the engine's static table
    double *score;                  // M x n_win
    BeamHeader *hdr;
};

// Flagged lanes of a round from which every one of them marches its own ray (march_exact, 64 rays at once) instead of the wave
// marching them one after the other (mcl::wave_march_exact_dir).  The wave's march costs about 270 instruction slots per ray whatever its
// length, a lane's about 60 per step of the longest flagged ray: they break even at (longest ray) / 4.5 flagged lanes, 9 to 50
// for rays of 40 to 240 steps.  Measured on whole-wave rounds: any value from 1 to 32 gives the same time, 11
// times shorter than the wave's march alone.
constexpr int kLaneMarchMin = 16;

// k_refine_beam_score: a wave per pose, so a workgroup holds four poses, and a launch at most 2^22 of them: 2^30 threads, below
// the 2^32 threads a grid may have.  The 2^27 - 1 poses R7 allows take 32 launches on the stream.
constexpr int kPosesPerBlock = kThreads / 64;
constexpr int32_t kPosesPerLaunch = 1 << 22;

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

// The refinement over a scan sequence (mcl_refine_poses_sequence): Args as above -- beams holds the S used-beam
// lists one after the other, nb their total -- and what joins the scans.
struct SeqArgs {
    Args a;
    const double *off;              // M x nt x S triples (ax, ay, theta_s), formed on the host (RS1)
    const int32_t *beam_begin;      // S + 1: scan s owns beams[beam_begin[s] .. beam_begin[s + 1])
    int S;
};

// k_refine_score's decomposition: one lane per window pose i = m * n_win + w, ix fastest.  A wave may straddle two headings or two
// seeds, so the row (m, it) of the table is per lane: per (lane, scan) one 24-byte triple, one sincos and two cell coordinates
// (RS2), nothing against the beams.  The bounds of a scan's beam list and every beam's pair are wave-uniform.  k_search_score_seq's
// loop: the scans outside, the beams inside; one accumulator per scan -- the in-order sum of LF5, what k_lfield gives for the pose
// of RS2 -- folded into the total in scan order (RS4).  Lf is staged once per workgroup, not once per scan.  Stores score[i] alone.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_refine_score_seq(SeqArgs q)
{
    extern __shared__ float s_lf[];
    const Args &a = q.a;
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
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    const double *o = q.off + ((size_t)m * (size_t)a.win.nt + (size_t)(dt + a.win.half_theta)) * (size_t)q.S * 3;
    double total = 0.0;
    for (int sc = 0; sc < q.S; ++sc, o += 3) {
        double s, c;
        sincos(o[2], &s, &c);
        const double px = mcl::lf_cell_coord(__dadd_rn(x, o[0]), a.ox, a.inv_res), py = mcl::lf_cell_coord(__dadd_rn(y, o[1]), a.oy, a.inv_res);
        const int j1 = q.beam_begin[sc + 1];
        double acc = 0.0;
#pragma unroll 4
        for (int j = q.beam_begin[sc]; j < j1; ++j)
            acc += (double)mcl::lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
        total += acc;
    }
    a.score[i] = total;
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

// ---- under the beam model (RB1-RB6) ------------------------------------------------------------------------------------------

// Once per call: where the table row (E2) of every used beam starts.  Every reading has a row: NaN, +-inf and readings out of
// range land where E4 puts them.
__global__ __launch_bounds__(kThreads) void k_refine_beam_rows(BeamArgs a)
{
    const int u = (int)(blockIdx.x * (uint32_t)kThreads + threadIdx.x);
    if (u >= a.nb) return;
    const int row = mcl::obs_index_of(a.obs[(size_t)u * a.beam_stride], a.ray.res, a.ray.P);
    a.row_base[u] = (uint32_t)row * (uint32_t)(a.ray.P + 1);
}

// One WAVE per window pose i = m * n_win + w, four poses per workgroup; lane l takes the used beams u = l, l + 64, ... (RB3: Q3's
// order).  The pose (R1), its constants, its start cell and the skip distance there are the same in all 64 lanes; neighbouring
// lanes walk neighbouring beams from that cell, the pose query's access pattern.  A round: every lane walks its beam at level 2
// (k_query_rays' arithmetic: fp64 positions on the isotropic field, the guard) and the lanes whose ray wants the literal march
// are balloted.  Few of them: the wave marches them one after the other (mcl::wave_march_exact_dir).  Many (kLaneMarchMin; a pose on
// a cell edge flags all 64): each marches its own ray (mcl::march_exact).  Both are cast_ray's additions in its order.  Then every lane
// gathers its table entry and adds it in fp64.  No step is ever stored.  The butterfly joins the 64 lane sums; lane 0 writes
// the score.
__global__ __launch_bounds__(kThreads) void k_refine_beam_score(BeamArgs a)
{
    const mcl::RayArgs &m = a.ray;
    const int lane = threadIdx.x & 63;
    // (the pose index from the block index, not from a global thread index: M * n_win waves may be 2^33 threads)
    const int32_t i = a.pose0 + (int32_t)(blockIdx.x * (uint32_t)kPosesPerBlock + (threadIdx.x >> 6));
    if (i >= a.n_total) return;                                         // (whole waves leave together)
    const int32_t sm = i / a.win.n_win, w = i - sm * a.win.n_win;
    int32_t dx, dy, dt;
    offsets(a.win, w, dx, dy, dt);
    const double x = coord(a.seeds[sm], dx, a.win.sx);
    const double y = coord(a.seeds[(size_t)a.M + sm], dy, a.win.sx);
    const double th = coord(a.seeds[(size_t)2 * a.M + sm], dt, a.win.st);
    const double4 pci = mcl::particle_constants(x, y, th, m.ox, m.oy, m.res);
    const mcl::RayOrigin o = mcl::ray_origin(m, pci.z, pci.w);
    // (a ray bound for the march anyway needs no walk; from a pose on a cell edge the walk can only lower amb)
    const bool walk = !mcl::takes_literal_march(m, o.sane, o.amb0);
    const int s_first = mcl::first_skip(m, o, m.dist);
    double acc = 0.0;
    unsigned n3 = 0;
    for (int u0 = 0; u0 < a.nb; u0 += 64) {
        const int u = u0 + lane;
        const bool live = u < a.nb;
        const int j = live ? u * a.beam_stride : 0;
        int r = m.P;
        bool exact = false;
        if (live) {
            uint32_t amb = o.amb0;
            if (walk) {
                const double2 cs = m.beam_cs[j];
                const double ux = pci.x * cs.x - pci.y * cs.y, uy = pci.y * cs.x + pci.x * cs.y;
                unsigned np = 0;
                r = mcl::trace_fp64<false, false>(m, nullptr, 0, mcl::kOriginBase, o.p0x, o.p0y, ux, uy, s_first, amb, np);
            }
            exact = mcl::takes_literal_march(m, o.sane, amb);
        }
        unsigned long long todo = __ballot(exact);
        const int n_exact = __popcll(todo);
        n3 += (unsigned)n_exact;
        if (n_exact >= kLaneMarchMin) {                              // (wave-uniform) many: every flagged lane marches its own ray
            if (exact) r = mcl::march_exact(m, x, y, th + (double)m.beam_angle[j]);
            todo = 0;
        }
        while (todo) {                                                  // (wave-uniform: every lane is in every march)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int jj = __shfl(j, src);
            const double angle = th + (double)m.beam_angle[jj];
            const int rr = mcl::wave_march_exact_dir(m, x, y, cos(angle) * m.res, sin(angle) * m.res, lane);
            if (lane == src) r = rr;
        }
        if (live) acc += (double)a.L[(size_t)a.row_base[u] + (size_t)r];
    }
    acc = mcl::wave_sum(acc);                                             // Q3's butterfly: every lane ends with the same bits
    if (lane == 0) {
        a.score[i] = acc;
        if (n3) atomicAdd(&a.hdr->level3, (unsigned long long)n3);
    }
}

}  // namespace mcl_rf
