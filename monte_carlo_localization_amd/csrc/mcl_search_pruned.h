// mcl_search_pruned.h -- the global search with exact pruning (mcl_global_search_pruned): the lattice of
// mcl_global_search cut into S x S blocks of positions, an upper bound U of every (block, heading) pair's scores that holds as
// bits (P1 - P3), and the scores of the pairs whose bound says they might matter.  The arguments of its kernels and the kernels
// themselves; only mcl_search.hip includes it, after mcl_search.h.  A score comes from lf_beam_value in k_search_score's order, so
// it is mcl_global_search's bit for bit.  The same over a scan sequence (mcl_global_search_sequence_pruned, §4.21, PS1 - PS5): the
// bound and the block scores summed over the scans in k_search_score_seq's order; the ranking, the marking and the decision are
// shared.
#pragma once
#include "mcl_search.h"

namespace mcl_prune {

using mcl_srch::kNoCandidate;
using mcl_srch::kThreads;
using mcl_srch::score_key;

constexpr uint32_t kNoIndex = ~0u;              // the index of a store entry that holds no pose: sorts after every pose's

// ---- P2: the pooled field.  Dp[(y + w - 1) * Wp + (x + w - 1)], Wp = W + w - 1, for low corners x in [-(w - 1), W - 1] (y
// likewise): the minimum of D' over the w x w window whose low corner is (x, y), D' = D inside the map and K outside.  Two
// separable passes, rows then columns, one thread per output cell (as k_lf_cols / k_lf_rows).
// Row pass: R[y * Wp + xs] = min over dx < w of D'(xs - (w - 1) + dx, y), for the map's rows y.
__global__ __launch_bounds__(256) void k_lf_pool_rows(const uint16_t *__restrict__ D, int W, int H, int K, int w, uint16_t *__restrict__ R)
{
    const int Wp = W + w - 1;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)Wp * H) return;
    const int y = (int)(c / Wp), xs = (int)(c - (int64_t)y * Wp);
    const uint16_t *row = D + (size_t)y * W;
    int best = K;
    for (int dx = 0; dx < w; ++dx) {
        const int x = xs - (w - 1) + dx;
        if (x >= 0 && x < W) best = min(best, (int)row[x]);
    }
    R[c] = (uint16_t)best;
}

// Column pass: Dp[ys * Wp + xs] = min over dy < w of R'(ys - (w - 1) + dy, xs), R' = R on the map's rows and K off them.
__global__ __launch_bounds__(256) void k_lf_pool_cols(const uint16_t *__restrict__ R, int W, int H, int K, int w, uint16_t *__restrict__ Dp)
{
    const int Wp = W + w - 1, Hp = H + w - 1;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= (int64_t)Wp * Hp) return;
    const int ys = (int)(c / Wp), xs = (int)(c - (int64_t)ys * Wp);
    int best = K;
    for (int dy = 0; dy < w; ++dy) {
        const int y = ys - (w - 1) + dy;
        if (y >= 0 && y < H) best = min(best, (int)R[(size_t)y * Wp + xs]);
    }
    Dp[c] = (uint16_t)best;
}

// what a round reports to the host
struct Round {
    uint64_t c_key;                 // the key of the max_hits-th best provisional candidate, kNoCandidate when there are fewer
    uint32_t stop;                  // nothing is unscored, or c is strictly above the bound of the first unscored pair
    uint32_t next;                  // the first rank whose U is below c, n_pairs when there is none; 0 when there is no c
};

struct Args {
    // the lattice and the headings of the search (mcl_srch::Args)
    const double2 *xy;
    const int32_t *pmap;            // ny x nx: (iy, ix) -> position, -1: no position
    const double *theta;
    int32_t n_pos, n_head, nx, ny;
    // P1: the live blocks in row-major order of (by, bx)
    int32_t S, n_blocks, nbx;       // positions per block side, live blocks, block columns
    uint32_t n_pairs;               // n_head * n_blocks; pair = k * n_blocks + b
    uint32_t groups_per_heading;    // ceil(n_blocks / 256)
    const double4 *corner;          // per live block: (x_lo, y_lo, x_hi, y_hi), the cell centres of S1 of its first and last
                                    // lattice column and row (clipped to the lattice)
    const int2 *blk;                // per live block: (bx, by)
    const int32_t *bmap;            // nby x nbx: (by, bx) -> live block, -1: none
    // the scan, the field and its pooled form
    const double2 *beams;
    int nb;
    const uint16_t *D;
    int W, H;
    double ox, oy, inv_res;
    const float *lf;                // K + 1 entries
    const float *ub;                // K + 1 entries: Ub[k] = max over j >= k of Lf[j]
    int K;
    const uint16_t *Dp;             // (H + w - 1) x (W + w - 1)
    int w;
    // the bounds and their order
    double *U;                      // per pair
    uint64_t *ukey;                 // per pair: score_key(U), before the sort
    uint32_t *upair;                // per pair: its number, before the sort
    const uint64_t *ukey_sorted;    // after it: U descending, ties by pair
    const uint32_t *pair_sorted;
    uint32_t *rank;                 // per pair: its place in that order.  The slot map: a pair of rank r < n_scored has its S * S
                                    // scores at store[r * S * S], a pair of a higher rank has none
    unsigned long long *guard;      // beam terms that fell back to Ub[0] (P3)
    // the rounds
    double *store;
    uint32_t r0, r1;                // k_search_score_block: the ranks [r0, r1) are scored
    uint32_t n_scored;              // k_search_mark_block, k_search_decide: the ranks [0, n_scored) have scores
    int nms;
    uint64_t *ckey;                 // per store entry: its sort key, kNoCandidate for none
    uint32_t *cval;                 // per store entry: the pose's index, kNoIndex where the entry holds no pose
    unsigned long long *count;      // provisional candidates
    uint32_t max_hits;
    Round *round;
};

// P3.  One lane per pair, a workgroup = 256 consecutive live blocks at ONE heading (k_search_score's decomposition): the heading,
// its sine and cosine and every beam's pair are uniform over the workgroup, and for one beam the low corners of neighbouring
// lanes are neighbouring cells of Dp (blocks of one block row: S * stride_cells apart).  Per beam the two nested fmas and the
// floors of lf_beam_value at both corners of the block; both are monotone in px and py, so every pose of the block has its end
// point's cell inside [lo, hi] in each axis.  With hi - lo < w in both axes that cell lies in the window of low corner lo and the
// term is Ub[Dp[lo]]; otherwise (NaN included) Ub[0].  U is the in-order fp64 sum of the terms from +0.0, as the score is.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_search_bound(Args a)
{
    extern __shared__ float s_ub[];
    const float *ub = a.ub;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_ub[k] = a.ub[k];
        __syncthreads();
        ub = s_ub;
    }
    const uint32_t k = blockIdx.x / a.groups_per_heading;
    const uint32_t b = (blockIdx.x - k * a.groups_per_heading) * (uint32_t)kThreads + threadIdx.x;
    if (b >= (uint32_t)a.n_blocks) return;
    double s, c;
    sincos(a.theta[k], &s, &c);
    const double4 q = a.corner[b];
    const double px0 = mcl::lf_cell_coord(q.x, a.ox, a.inv_res), py0 = mcl::lf_cell_coord(q.y, a.oy, a.inv_res);
    const double px1 = mcl::lf_cell_coord(q.z, a.ox, a.inv_res), py1 = mcl::lf_cell_coord(q.w, a.oy, a.inv_res);
    const double w = (double)a.w, xmin = (double)(1 - a.w), W = (double)a.W, H = (double)a.H;
    const int Wp = a.W + a.w - 1;
    const float top = ub[0], off = ub[a.K];
    double acc = 0.0;
    unsigned fell = 0;
#pragma unroll 2
    for (int j = 0; j < a.nb; ++j) {
        const double2 bm = a.beams[j];
        const double lx = floor(fma(c, bm.x, fma(-s, bm.y, px0))), ly = floor(fma(s, bm.x, fma(c, bm.y, py0)));
        const double hx = floor(fma(c, bm.x, fma(-s, bm.y, px1))), hy = floor(fma(s, bm.x, fma(c, bm.y, py1)));
        float v = top;
        if (hx - lx < w && hy - ly < w) {                                   // (false for NaN)
            v = off;                                                        // a window wholly off the map in either axis: K
            if (lx >= xmin && lx < W && ly >= xmin && ly < H)
                v = ub[a.Dp[(size_t)((int)ly + a.w - 1) * (size_t)Wp + (size_t)((int)lx + a.w - 1)]];
        } else {
            ++fell;
        }
        acc += (double)v;
    }
    const uint32_t pair = k * (uint32_t)a.n_blocks + b;
    a.U[pair] = acc;
    a.ukey[pair] = score_key(acc);
    a.upair[pair] = pair;
    if (fell) atomicAdd(a.guard, (unsigned long long)fell);
}

// the inverse of the sorted order: rank[pair_sorted[r]] = r
__global__ __launch_bounds__(kThreads) void k_search_rank(Args a)
{
    const uint32_t r = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (r < a.n_pairs) a.rank[a.pair_sorted[r]] = r;
}

// The lattice position of lane l of live block b: l = ly * S + lx is lattice cell (bx * S + lx, by * S + ly); -1 where the block has
// none there.
__device__ __forceinline__ int32_t block_position(const Args &a, uint32_t b, uint32_t l)
{
    const int2 at = a.blk[b];
    const int ly = (int)l / a.S, lx = (int)l - ly * a.S;
    const int ix = at.x * a.S + lx, iy = at.y * a.S + ly;
    if (ly >= a.S || ix >= a.nx || iy >= a.ny) return -1;
    return a.pmap[(size_t)iy * (size_t)a.nx + (size_t)ix];
}

// One WAVE per pair of the ranks [r0, r1), one lane per lattice position of its block (S * S <= 64); a workgroup = 4 pairs.  The
// pair is the wave's, so the heading, its sine and cosine and every beam's pair arrive by scalar loads as in k_search_score, and
// the lanes of one block row read cells stride_cells apart.  The loop is k_search_score's, so a score is mcl_global_search's bit
// for bit.  Lanes without a position write -inf and take no part in the loop.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_search_score_block(Args a)
{
    extern __shared__ float s_lf[];
    const float *lf = a.lf;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_lf[k] = a.lf[k];
        __syncthreads();
        lf = s_lf;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = a.r0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)(kThreads / 64) + (threadIdx.x >> 6)));
    if (r >= a.r1) return;
    const uint32_t SS = (uint32_t)(a.S * a.S);
    if (lane >= SS) return;
    const uint32_t pair = a.pair_sorted[r];
    const uint32_t k = pair / (uint32_t)a.n_blocks, b = pair - k * (uint32_t)a.n_blocks;
    const int32_t p = block_position(a, b, lane);
    double acc = -__builtin_inf();
    if (p >= 0) {
        double s, c;
        sincos(a.theta[k], &s, &c);
        const double2 q = a.xy[p];
        const double px = mcl::lf_cell_coord(q.x, a.ox, a.inv_res), py = mcl::lf_cell_coord(q.y, a.oy, a.inv_res);
        const double W = (double)a.W, H = (double)a.H;
        const float off = lf[a.K];
        acc = 0.0;
#pragma unroll 4
        for (int j = 0; j < a.nb; ++j)
            acc += (double)mcl::lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
    }
    a.store[(size_t)r * SS + lane] = acc;
}

// ---- the pruned search over a scan sequence (mcl_global_search_sequence_pruned): Args as above -- beams holds the
// S used-beam lists one after the other, nb their total -- and what joins the scans (mcl_srch::SeqArgs' three)
struct SeqArgs {
    Args a;
    const double *off;              // n_head x n_scans triples (ax_ks, ay_ks, theta_ks), formed on the host (SQ1)
    const int32_t *beam_begin;      // n_scans + 1: scan s owns beams[beam_begin[s] .. beam_begin[s + 1])
    int n_scans;
};

// PS3.  k_search_bound's decomposition: one lane per pair, a workgroup = 256 consecutive live blocks at ONE heading.  For one
// (heading, scan) the triple of SQ1, the sine and cosine of theta_ks, the bounds of the beam list and every beam's pair are uniform
// over the workgroup (scalar loads, addressed from blockIdx and the loop counters alone).  Both corners of the block get the
// displacement by SQ2's one rounded add each, which is monotone, so every pose of the block has its scan pose between the shifted
// corners; from there a beam's term is k_search_bound's, and for one beam neighbouring lanes still read neighbouring windows of
// Dp: the displacement is the same for all of them.  The scans outside, the beams inside; one accumulator per scan -- the in-order
// fp64 sum of the terms from +0.0 -- folded into the total in scan order, as SQ4 folds the scores.  Ub is staged once per
// workgroup, not once per scan.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_search_bound_seq(SeqArgs q)
{
    extern __shared__ float s_ub[];
    const Args &a = q.a;
    const float *ub = a.ub;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_ub[k] = a.ub[k];
        __syncthreads();
        ub = s_ub;
    }
    const uint32_t k = blockIdx.x / a.groups_per_heading;
    const uint32_t b = (blockIdx.x - k * a.groups_per_heading) * (uint32_t)kThreads + threadIdx.x;
    if (b >= (uint32_t)a.n_blocks) return;
    const double4 cn = a.corner[b];
    const double w = (double)a.w, xmin = (double)(1 - a.w), W = (double)a.W, H = (double)a.H;
    const int Wp = a.W + a.w - 1;
    const float top = ub[0], off = ub[a.K];
    const double *o = q.off + (size_t)k * (size_t)q.n_scans * 3;
    double total = 0.0;
    unsigned fell = 0;
    for (int sc = 0; sc < q.n_scans; ++sc, o += 3) {
        double s, c;
        sincos(o[2], &s, &c);
        const double px0 = mcl::lf_cell_coord(cn.x + o[0], a.ox, a.inv_res), py0 = mcl::lf_cell_coord(cn.y + o[1], a.oy, a.inv_res);
        const double px1 = mcl::lf_cell_coord(cn.z + o[0], a.ox, a.inv_res), py1 = mcl::lf_cell_coord(cn.w + o[1], a.oy, a.inv_res);
        const int j1 = q.beam_begin[sc + 1];
        double acc = 0.0;
#pragma unroll 2
        for (int j = q.beam_begin[sc]; j < j1; ++j) {
            const double2 bm = a.beams[j];
            const double lx = floor(fma(c, bm.x, fma(-s, bm.y, px0))), ly = floor(fma(s, bm.x, fma(c, bm.y, py0)));
            const double hx = floor(fma(c, bm.x, fma(-s, bm.y, px1))), hy = floor(fma(s, bm.x, fma(c, bm.y, py1)));
            float v = top;
            if (hx - lx < w && hy - ly < w) {                               // (false for NaN)
                v = off;                                                    // a window wholly off the map in either axis: K
                if (lx >= xmin && lx < W && ly >= xmin && ly < H)
                    v = ub[a.Dp[(size_t)((int)ly + a.w - 1) * (size_t)Wp + (size_t)((int)lx + a.w - 1)]];
            } else {
                ++fell;
            }
            acc += (double)v;
        }
        total += acc;
    }
    const uint32_t pair = k * (uint32_t)a.n_blocks + b;
    a.U[pair] = total;
    a.ukey[pair] = score_key(total);
    a.upair[pair] = pair;
    if (fell) atomicAdd(a.guard, (unsigned long long)fell);
}

// PS4.  k_search_score_block's decomposition: one WAVE per pair of the ranks [r0, r1), one lane per lattice position of its block;
// the pair is the wave's, so the triples of SQ1, their sines and cosines, the beam lists' bounds and every beam's pair arrive by
// scalar loads.  The loop is k_search_score_seq's, so a score is mcl_global_search_sequence's bit for bit.  Lanes without a
// position write -inf and take no part in the loop.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_search_score_block_seq(SeqArgs q)
{
    extern __shared__ float s_lf[];
    const Args &a = q.a;
    const float *lf = a.lf;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_lf[k] = a.lf[k];
        __syncthreads();
        lf = s_lf;
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = a.r0 + (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (uint32_t)(kThreads / 64) + (threadIdx.x >> 6)));
    if (r >= a.r1) return;
    const uint32_t SS = (uint32_t)(a.S * a.S);
    if (lane >= SS) return;
    const uint32_t pair = a.pair_sorted[r];
    const uint32_t k = pair / (uint32_t)a.n_blocks, b = pair - k * (uint32_t)a.n_blocks;
    const int32_t p = block_position(a, b, lane);
    double total = -__builtin_inf();
    if (p >= 0) {
        const double2 xy = a.xy[p];
        const double W = (double)a.W, H = (double)a.H;
        const float off = lf[a.K];
        const double *o = q.off + (size_t)k * (size_t)q.n_scans * 3;
        total = 0.0;
        for (int sc = 0; sc < q.n_scans; ++sc, o += 3) {
            double s, c;
            sincos(o[2], &s, &c);
            const double px = mcl::lf_cell_coord(xy.x + o[0], a.ox, a.inv_res), py = mcl::lf_cell_coord(xy.y + o[1], a.oy, a.inv_res);
            const int j1 = q.beam_begin[sc + 1];
            double acc = 0.0;
#pragma unroll 4
            for (int j = q.beam_begin[sc]; j < j1; ++j)
                acc += (double)mcl::lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
            total += acc;
        }
    }
    a.store[(size_t)r * SS + lane] = total;
}

// S5 over the scored pairs, through the slot map: one lane per store entry e = r * S * S + l of the ranks [0, n_scored).  The
// neighbours are k_search_mark's; one whose pair has no scores counts as worse.  Every entry gets its sort key and its pose's
// index (kNoCandidate and kNoIndex where it holds no pose); the candidates are counted per wave.
__global__ __launch_bounds__(kThreads) void k_search_mark_block(Args a)
{
    const uint32_t SS = (uint32_t)(a.S * a.S);
    const uint64_t n = (uint64_t)a.n_scored * SS;
    const uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool cand = false;
    if (e < n) {
        const uint32_t r = (uint32_t)(e / SS), l = (uint32_t)(e - (uint64_t)r * SS);
        const uint32_t pair = a.pair_sorted[r];
        const int k = (int)(pair / (uint32_t)a.n_blocks);
        const uint32_t b = pair - (uint32_t)k * (uint32_t)a.n_blocks;
        const int32_t p = block_position(a, b, l);
        uint64_t key = kNoCandidate;
        uint32_t idx = kNoIndex;
        if (p >= 0) {
            const uint64_t i = (uint64_t)k * (uint64_t)a.n_pos + (uint64_t)p;
            const double s = a.store[e];
            cand = s > -__builtin_inf();
            if (cand && a.nms) {
                const int2 at = a.blk[b];
                const int ly = (int)l / a.S, lx = (int)l - ly * a.S;
                const int ix = at.x * a.S + lx, iy = at.y * a.S + ly;
                for (int dk = -1; dk <= 1 && cand; ++dk) {
                    const int kk = mcl_srch::wrap_heading(k + dk, a.n_head);
                    for (int dy = -1; dy <= 1; ++dy) {
                        const int jy = iy + dy;
                        if (jy < 0 || jy >= a.ny) continue;
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int jx = ix + dx;
                            if (jx < 0 || jx >= a.nx) continue;
                            const int32_t q = a.pmap[(size_t)jy * (size_t)a.nx + (size_t)jx];
                            if (q < 0) continue;
                            const uint64_t j = (uint64_t)kk * (uint64_t)a.n_pos + (uint64_t)q;
                            if (j == i) continue;
                            const int qy = jy / a.S, qx = jx / a.S;
                            const int32_t nb = a.bmap[(size_t)qy * (size_t)a.nbx + (size_t)qx];     // (live: it holds q)
                            const uint32_t nr = a.rank[(uint32_t)kk * (uint32_t)a.n_blocks + (uint32_t)nb];
                            if (nr >= a.n_scored) continue;                                         // unscored: worse
                            const double t = a.store[(size_t)nr * SS + (size_t)((jy - qy * a.S) * a.S + (jx - qx * a.S))];
                            if (!(s > t || (s == t && i < j))) cand = false;
                        }
                    }
                }
            }
            key = cand ? score_key(s) : kNoCandidate;
            idx = (uint32_t)i;
        }
        a.ckey[e] = key;
        a.cval[e] = idx;
    }
    const unsigned long long found = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(a.count, (unsigned long long)__popcll(found));
}

// Steps 5 and 6 after the candidates' sort (ckey: ascending, so the best first): c, whether the call stops, and the first rank
// with U < c -- in keys, the first with a key above c's -- by bisection of the sorted bounds (0 while there are fewer than max_hits
// candidates: the doubling of P4 alone decides).  One thread.
__global__ void k_search_decide(Args a)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t n = (uint64_t)a.n_scored * (uint64_t)(a.S * a.S);
    const uint64_t c_key = (uint64_t)a.max_hits <= n ? a.ckey[a.max_hits - 1] : kNoCandidate;
    uint32_t lo = 0, hi = c_key == kNoCandidate ? 0 : a.n_pairs;            // (fewer than max_hits candidates: no c, no such rank)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.ukey_sorted[mid] > c_key) hi = mid; else lo = mid + 1;
    }
    Round out;
    out.c_key = c_key;
    out.stop = (a.n_scored >= a.n_pairs || c_key < a.ukey_sorted[a.n_scored]) ? 1u : 0u;
    out.next = lo;
    *a.round = out;
}

}  // namespace mcl_prune
