// mcl_search.h -- the global search (mcl_global_search; over a scan sequence: §4.15): the likelihood-field score of
// every pose of a regular lattice over the map's free cells, and which of them are hits.  The arguments of its kernels and the kernels themselves; only
// mcl_search.hip includes it.  A score comes from the per-beam arithmetic of k_lfield (mcl_lfield_core.h), so a lattice pose and
// a particle (or a queried pose) at the same place agree bit for bit.
#pragma once
#include "mcl_engine_internal.h"
#include "mcl_lfield_core.h"

namespace mcl_srch {

constexpr int kThreads = 256;
constexpr uint64_t kNoCandidate = ~0ull;        // sort key of a pose that is no candidate: after every candidate's

struct Args {
    // the lattice: positions in row-major order of (iy, ix) (S1), headings (S2)
    const double2 *xy;              // n_pos cell centres, formed on the host
    const int2 *lat;                // n_pos lattice coordinates (ix, iy)
    const int32_t *pmap;            // ny x nx, row-major: (iy, ix) -> position, -1: no position
    const double *theta;            // n_head headings
    int32_t n_pos, n_head, nx, ny;
    uint32_t blocks_per_heading;    // ceil(n_pos / 256)
    // the scan and the field
    const double2 *beams;           // the used beams in beam order (S3)
    int nb;
    const uint16_t *D;              // H x W, row-major
    int W, H;
    double ox, oy, inv_res;
    const float *lf;                // K + 1 entries
    int K;
    double *score;                  // n_head x n_pos: score[k * n_pos + p]; the streamed search: a ring of planes (below)
    // Which headings a launch scores and where they go.  Workgroups of heading slot b score the LINEAR heading hh = head0 + b:
    // heading hh mod n_head (hh = -1 is heading n_head - 1, hh = n_head is heading 0), into plane (hh + 1) % ring of `score`,
    // or with ring == 0 into plane hh.  The unstreamed searches: head0 = 0, ring = 0 -- the plane is the heading.
    int32_t head0, ring;
    // the hits
    int nms;
    uint64_t *key;                  // per pose: its sort key (ascending keys = better poses first), kNoCandidate for none
    uint32_t *val;                  // per pose: its index
    unsigned long long *count;      // candidates
};

// Ascending order of the key == descending order of the score.  A score is finite or -inf here and never -0.0 (an in-order sum
// that starts at +0.0), so equal scores have equal keys; `s + 0.0` states the latter.
__device__ __forceinline__ uint64_t score_key(double s)
{
    const uint64_t b = (uint64_t)__double_as_longlong(s + 0.0);
    const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~asc;
}

// a linear heading in [-1, n_head] as a heading (ST2's wrap neighbours), and the plane of `score` that holds it
__device__ __forceinline__ int32_t wrap_heading(int32_t hh, int32_t n_head)
{
    return hh < 0 ? hh + n_head : (hh >= n_head ? hh - n_head : hh);
}
__device__ __forceinline__ uint32_t ring_plane(int32_t hh, int32_t ring)
{
    return ring ? (uint32_t)(hh + 1) % (uint32_t)ring : (uint32_t)hh;
}

// One lane per pose, a workgroup = 256 consecutive positions at ONE heading: the heading, its sine and cosine and every beam's
// pair are uniform over the workgroup, and for one beam the end points of neighbouring lanes are neighbouring cells of the
// field (same row of the lattice: stride_cells apart).  The in-order fp64 sum of LF5 per lane.  LDS_TABLE as in k_lfield.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_search_score(Args a)
{
    extern __shared__ float s_lf[];
    const float *lf = a.lf;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_lf[k] = a.lf[k];
        __syncthreads();
        lf = s_lf;
    }
    const uint32_t b = blockIdx.x / a.blocks_per_heading;
    const uint32_t p = (blockIdx.x - b * a.blocks_per_heading) * (uint32_t)kThreads + threadIdx.x;
    if (p >= (uint32_t)a.n_pos) return;
    const int32_t hh = a.head0 + (int32_t)b;
    const uint32_t k = (uint32_t)wrap_heading(hh, a.n_head), plane = ring_plane(hh, a.ring);
    double s, c;
    sincos(a.theta[k], &s, &c);
    const double2 q = a.xy[p];
    const double px = mcl::lf_cell_coord(q.x, a.ox, a.inv_res), py = mcl::lf_cell_coord(q.y, a.oy, a.inv_res);
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    double acc = 0.0;
#pragma unroll 4
    for (int j = 0; j < a.nb; ++j)
        acc += (double)mcl::lf_beam_value(a.beams[j], s, c, px, py, W, H, a.W, a.D, lf, off);
    a.score[(size_t)plane * (size_t)a.n_pos + p] = acc;
}

// The search over a scan sequence (mcl_global_search_sequence): Args as above -- beams holds the S used-beam lists
// one after the other, nb their total -- and what joins the scans.
struct SeqArgs {
    Args a;
    const double *off;              // n_head x S triples (ax_ks, ay_ks, theta_ks), formed on the host (SQ1)
    const int32_t *beam_begin;      // S + 1: scan s owns beams[beam_begin[s] .. beam_begin[s + 1])
    int S;
};

// k_search_score's decomposition: one lane per lattice pose, a workgroup = 256 consecutive positions at ONE heading.  For one
// (heading, scan) the triple of SQ1, the sine and cosine of theta_ks, the bounds of the beam list and every beam's pair are uniform
// over the workgroup (scalar loads, addressed from blockIdx and the loop counters alone), and for one beam neighbouring lanes still
// read neighbouring cells of the field: the displacement is the same for all of them.  The scans outside, the beams inside; one
// accumulator per scan -- the in-order sum of LF5, what k_lfield gives for the pose of SQ2 -- folded into the total in scan order
// (SQ4).  Lf is staged once per workgroup, not once per scan.
template <bool LDS_TABLE>
__global__ __launch_bounds__(kThreads) void k_search_score_seq(SeqArgs q)
{
    extern __shared__ float s_lf[];
    const Args &a = q.a;
    const float *lf = a.lf;
    if constexpr (LDS_TABLE) {
        for (int k = threadIdx.x; k <= a.K; k += kThreads) s_lf[k] = a.lf[k];
        __syncthreads();
        lf = s_lf;
    }
    const uint32_t b = blockIdx.x / a.blocks_per_heading;
    const uint32_t p = (blockIdx.x - b * a.blocks_per_heading) * (uint32_t)kThreads + threadIdx.x;
    if (p >= (uint32_t)a.n_pos) return;
    const int32_t hh = a.head0 + (int32_t)b;
    const uint32_t k = (uint32_t)wrap_heading(hh, a.n_head), plane = ring_plane(hh, a.ring);
    const double2 xy = a.xy[p];
    const double W = (double)a.W, H = (double)a.H;
    const float off = lf[a.K];
    const double *o = q.off + (size_t)k * (size_t)q.S * 3;
    double total = 0.0;
    for (int sc = 0; sc < q.S; ++sc, o += 3) {
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
    a.score[(size_t)plane * (size_t)a.n_pos + p] = total;
}

// One lane per pose i = k * n_pos + p: is it a candidate (S5)?  With nms, a pose must be better -- a higher score, or the same
// score and a lower index -- than each of its up to 26 lattice neighbours (positions one lattice step away in ix / iy, headings
// k - 1, k, k + 1 modulo n_head; with one or two headings the wrap lands on the pose itself or twice on the same neighbour, which
// changes nothing).  Every pose gets its sort key and its index; the candidates are counted per wave.
__global__ __launch_bounds__(kThreads) void k_search_mark(Args a)
{
    const uint64_t n_poses = (uint64_t)a.n_pos * (uint64_t)a.n_head;
    const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool cand = false;
    if (i < n_poses) {
        const int k = (int)(i / (uint64_t)a.n_pos);
        const int p = (int)(i - (uint64_t)k * (uint64_t)a.n_pos);
        const double s = a.score[i];
        cand = s > -__builtin_inf();
        if (cand && a.nms) {
            const int2 at = a.lat[p];
            for (int dk = -1; dk <= 1 && cand; ++dk) {
                int kk = k + dk;
                kk = kk < 0 ? kk + a.n_head : (kk >= a.n_head ? kk - a.n_head : kk);
                for (int dy = -1; dy <= 1; ++dy) {
                    const int jy = at.y + dy;
                    if (jy < 0 || jy >= a.ny) continue;
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int jx = at.x + dx;
                        if (jx < 0 || jx >= a.nx) continue;
                        const int32_t q = a.pmap[(size_t)jy * (size_t)a.nx + (size_t)jx];
                        if (q < 0) continue;
                        const uint64_t j = (uint64_t)kk * (uint64_t)a.n_pos + (uint64_t)q;
                        if (j == i) continue;
                        const double t = a.score[j];
                        if (!(s > t || (s == t && i < j))) cand = false;
                    }
                }
            }
        }
        a.key[i] = cand ? score_key(s) : kNoCandidate;
        a.val[i] = (uint32_t)i;
    }
    const unsigned long long found = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(a.count, (unsigned long long)__popcll(found));
}

// ---- the streamed search (mcl_global_search_streamed): the volume in slabs of headings through a ring of planes
// what the slabs of one call hand on, on the device; slab t reads state[t & 1] and writes state[(t + 1) & 1]
struct SlabState {
    unsigned long long run_n;       // entries of the running list (ST3): min(max_hits, candidates merged so far)
    unsigned long long compacted;   // candidates compacted so far, over all slabs
};

struct SlabArgs {
    Args a;                         // a.score: the ring; a.key: the slab's keys (per slab pose); a.count: all candidates of the call
    int32_t head_lo, g;             // the slab marks headings [head_lo, head_lo + g)
    int32_t wrap;                   // 1: one slab holds every heading (plane = heading, neighbours wrap inside the ring)
    uint64_t max_hits;
    const SlabState *in;
    SlabState *out;
    uint32_t *flag;                 // per slab pose: 1 when the pose is compacted
    const uint32_t *pos;            // the exclusive scan of flag
    // the running list and, behind it, this slab's candidates: (key, 64-bit index), what the stable sort merges
    uint64_t *ckey, *cidx;
    unsigned long long *seg;        // {0, run_n + this slab's compacted candidates}: the one segment the sort works on
};

// k_search_mark over one slab: one lane per pose of the slab's g headings, i = (k - head_lo) * n_pos + p.  The score and those of
// the up to 26 neighbours come from the ring: linear heading hh = k + dk in [-1, n_head] sits in plane (hh + 1) % ring (with
// `wrap`: heading hh mod n_head sits in plane hh mod n_head), and stands for heading hh mod n_head when indices are compared, so
// S5 holds as it stands, with one or two headings too.  A candidate is compacted unless the running list is full and the
// candidate is no better than its last entry: every index of this slab is higher than every index in the list, so a tie loses.
__global__ __launch_bounds__(kThreads) void k_search_mark_slab(SlabArgs q)
{
    const Args &a = q.a;
    const uint64_t n_slab = (uint64_t)a.n_pos * (uint64_t)q.g;
    const uint64_t li = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    bool cand = false;
    if (li < n_slab) {
        const int dk0 = (int)(li / (uint64_t)a.n_pos);
        const int p = (int)(li - (uint64_t)dk0 * (uint64_t)a.n_pos);
        const int k = q.head_lo + dk0;
        const uint64_t i = (uint64_t)k * (uint64_t)a.n_pos + (uint64_t)p;
        const double s = a.score[(size_t)ring_plane(k, a.ring) * (size_t)a.n_pos + (size_t)p];
        cand = s > -__builtin_inf();
        if (cand && a.nms) {
            const int2 at = a.lat[p];
            for (int dk = -1; dk <= 1 && cand; ++dk) {
                const int hh = k + dk;
                const int kk = wrap_heading(hh, a.n_head);
                const size_t plane = (size_t)ring_plane(q.wrap ? kk : hh, a.ring) * (size_t)a.n_pos;
                for (int dy = -1; dy <= 1; ++dy) {
                    const int jy = at.y + dy;
                    if (jy < 0 || jy >= a.ny) continue;
                    for (int dx = -1; dx <= 1; ++dx) {
                        const int jx = at.x + dx;
                        if (jx < 0 || jx >= a.nx) continue;
                        const int32_t n = a.pmap[(size_t)jy * (size_t)a.nx + (size_t)jx];
                        if (n < 0) continue;
                        const uint64_t j = (uint64_t)kk * (uint64_t)a.n_pos + (uint64_t)n;
                        if (j == i) continue;
                        const double t = a.score[plane + (size_t)n];
                        if (!(s > t || (s == t && i < j))) cand = false;
                    }
                }
            }
        }
        const uint64_t key = cand ? score_key(s) : kNoCandidate;
        a.key[li] = key;
        bool take = cand && q.max_hits > 0;
        if (take && q.in->run_n >= q.max_hits) take = key < q.ckey[q.max_hits - 1];
        q.flag[li] = take ? 1u : 0u;
    }
    const unsigned long long found = __ballot(cand);
    if ((threadIdx.x & 63) == 0 && found) atomicAdd(a.count, (unsigned long long)__popcll(found));
}

// The flagged poses of the slab, in index order, behind the running list: (key, 64-bit index).  The lane of the slab's last pose
// knows how many there are: it closes the sort's segment and hands the counts on.
__global__ __launch_bounds__(kThreads) void k_search_compact(SlabArgs q)
{
    const Args &a = q.a;
    const uint64_t n_slab = (uint64_t)a.n_pos * (uint64_t)q.g;
    const uint64_t li = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (li >= n_slab) return;
    const unsigned long long run_n = q.in->run_n;
    const uint32_t f = q.flag[li], at = q.pos[li];
    if (f) {
        q.ckey[run_n + at] = a.key[li];
        q.cidx[run_n + at] = (uint64_t)q.head_lo * (uint64_t)a.n_pos + li;
    }
    if (li == n_slab - 1) {
        const unsigned long long c = (unsigned long long)at + f, all = run_n + c;
        q.seg[0] = 0;
        q.seg[1] = all;
        q.out->run_n = all < q.max_hits ? all : q.max_hits;
        q.out->compacted = q.in->compacted + c;
    }
}

}  // namespace mcl_srch
