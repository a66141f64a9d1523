// mcl_search_beam.h -- the global search under the beam model (mcl_global_search_beam, DESIGN.md §4.17, rules B1-B6 of
// include/mcl_hip_engine.h): the arguments of its kernels and the kernels themselves; only mcl_search.hip includes it.  All
// headings of a lattice position share that position's rays: a tile of T positions gets a table R[m * T + t] of E3's step at
// the M grid angles (k_beam_table, k_beam_table_exact), and a pose's score is a sum of table entries of the scan's rows
// (k_beam_rows, k_beam_score).  A step comes from the functions the update's ray stage calls (mcl_ray_core.h), at level 3 with
// the direction the host formed (B2), so a table entry is bit for bit cast_ray's step at that origin and grid angle.
#pragma once
#include "mcl_engine_internal.h"
#include "mcl_ray_core.h"

namespace mcl_sbeam {

constexpr int kThreads = 256;

using Header = mcl::Level3Header;   // what the table kernels count: `listed` of this tile, `level3` of the whole call

struct Args {
    mcl::RayArgs ray;               // the map, P, force_exact: what trace_fp64 and the march read
    // the tile: positions [pos0, pos0 + count) of the lattice, count <= T
    const double2 *xy;              // the lattice's cell centres (S1)
    const double2 *dir;             // M pairs (cos phi_m, sin phi_m), formed on the host in double (B2)
    int32_t M, T, pos0, count;
    uint32_t blocks_per_row;        // ceil(count / 256): the workgroups of one angle (table) or one heading (score)
    void *tab;                      // T x M entries, angle-major: R[m * T + t]; uint8_t when P <= 255, else uint16_t
    uint32_t *list;                 // flagged rays m * T + t waiting for the literal march
    unsigned long long list_cap;
    Header *hdr;
    // the scan
    const float *obs;               // B readings
    int32_t B, beam_stride, nb;     // nb = used beams: j = u * beam_stride, u < nb
    const float *L;                 // [row][step], P + 1 columns: the engine's static table
    float *lobs;                    // nb x (P + 1): Lobs[u][r] = L[row_{j_u}][r]
    // the score
    int32_t n_pos, n_head, heading_step;
    double *score;                  // n_head x n_pos
};

// One lane per (tile position t, angle m), a workgroup = 256 consecutive positions at ONE angle: a wave is 64 neighbouring
// origins with one direction, so its rays are near-identical and its store is 64 consecutive entries.  Levels 2 and 3 as
// k_query_rays runs them, with the uploaded direction.  Flagged rays go to the list
// (k_beam_table_exact gives each a wave); beyond its capacity the lane marches itself.
template <class E>
__global__ __launch_bounds__(kThreads) void k_beam_table(Args a)
{
    const mcl::RayArgs &m = a.ray;
    const uint32_t mi = blockIdx.x / a.blocks_per_row;
    const uint32_t t = (blockIdx.x - mi * a.blocks_per_row) * (uint32_t)kThreads + threadIdx.x;
    if (mi >= (uint32_t)a.M || t >= (uint32_t)a.count) return;
    const double2 q = a.xy[(size_t)a.pos0 + t];
    const double2 u = a.dir[mi];
    const mcl::RayOrigin o = mcl::ray_origin(m, (q.x - m.ox) / m.res, (q.y - m.oy) / m.res);
    int r = m.P;
    uint32_t amb = o.amb0;
    unsigned np = 0;
    if (o.sane && m.force_exact != 1)                      // (a ray bound for the list anyway needs no walk)
        r = mcl::trace_fp64<false, false>(m, nullptr, 0, mcl::kOriginBase, o.p0x, o.p0y, u.x, u.y, mcl::first_skip(m, o, m.dist), amb, np);
    const uint32_t ray = mi * (uint32_t)a.T + t;
    if (mcl::takes_literal_march(m, o.sane, amb)) {
        if (mcl::level3_append(a.hdr, a.list, a.list_cap, ray)) return;
        r = mcl::march_exact_dir(m, q.x, q.y, u.x * m.res, u.y * m.res);
        atomicAdd(&a.hdr->level3, 1ull);
    }
    static_cast<E *>(a.tab)[ray] = (E)r;
}

// Level 3 for the listed rays: one WAVE per ray (mcl::wave_march_exact_dir).
template <class E>
__global__ __launch_bounds__(kThreads) void k_beam_table_exact(Args a)
{
    const mcl::RayArgs &m = a.ray;
    const int lane = threadIdx.x & 63;
    const unsigned long long wave_id = ((unsigned long long)blockIdx.x * kThreads + threadIdx.x) >> 6;
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * kThreads) >> 6;
    const unsigned long long n = mcl::level3_listed(a.hdr, a.list_cap);
    unsigned long long done = 0;
    for (unsigned long long e = wave_id; e < n; e += nwaves) {
        const uint32_t ray = a.list[e];
        const uint32_t mi = ray / (uint32_t)a.T, t = ray - mi * (uint32_t)a.T;
        // (never taken: the list holds what k_beam_table put there.  `ray` is the same in all 64 lanes, so the wave leaves the
        //  iteration together and the march below has the whole wave)
        if (mi >= (uint32_t)a.M || t >= (uint32_t)a.count) continue;
        const double2 q = a.xy[(size_t)a.pos0 + t];
        const double2 u = a.dir[mi];
        const int r = mcl::wave_march_exact_dir(m, q.x, q.y, u.x * m.res, u.y * m.res, lane);
        if (lane == 0) { static_cast<E *>(a.tab)[ray] = (E)r; ++done; }
    }
    if (lane == 0 && done) atomicAdd(&a.hdr->level3, done);
}

// Once per call: the table rows of the scan's used beams, Lobs[u][r] = L[row_{j_u}][r] with row from E2 (obs_index_of: NaN,
// +-inf and readings out of range land where E4 puts them).  One lane per entry.
__global__ __launch_bounds__(kThreads) void k_beam_rows(Args a)
{
    const int tw = a.ray.P + 1;
    const uint32_t i = blockIdx.x * (uint32_t)kThreads + threadIdx.x;
    if (i >= (uint32_t)a.nb * (uint32_t)tw) return;
    const uint32_t u = i / (uint32_t)tw, r = i - u * (uint32_t)tw;
    const int row = mcl::obs_index_of(a.obs[(size_t)u * a.beam_stride], a.ray.res, a.ray.P);
    a.lobs[i] = a.L[(size_t)row * tw + r];
}

// The hot path.  One lane per pose of the tile, a workgroup = 256 consecutive tile positions at ONE heading (the headings of a
// position block are consecutive workgroups: they read the same columns of the table).  The grid angle of beam j at heading
// k, m = (k s + j) mod M, is uniform over the workgroup and advances by beam_stride per used beam; per beam a wave reads 64
// consecutive table entries and gathers 4 bytes of Lobs[u][.] -- neighbouring origins have neighbouring steps.  The fp64 sum
// runs in beam order from +0.0 (B3), one lane per pose, straight into the volume.
template <class E>
__global__ __launch_bounds__(kThreads) void k_beam_score(Args a)
{
    const uint32_t pb = blockIdx.x / (uint32_t)a.n_head, k = blockIdx.x - pb * (uint32_t)a.n_head;
    const uint32_t t = pb * (uint32_t)kThreads + threadIdx.x;
    if (pb >= a.blocks_per_row || t >= (uint32_t)a.count) return;
    const uint32_t M = (uint32_t)a.M, step_m = (uint32_t)a.beam_stride % M;
    const int tw = a.ray.P + 1;
    const E *col = static_cast<const E *>(a.tab) + t;
    const float *lobs = a.lobs;
    uint32_t m = (uint32_t)(((uint64_t)k * (uint64_t)a.heading_step) % M);
    double acc = 0.0;
#pragma unroll 8
    for (int u = 0; u < a.nb; ++u) {
        const uint32_t r = col[(size_t)m * (size_t)a.T];
        acc += (double)lobs[r];
        lobs += tw;
        m += step_m;
        m = m >= M ? m - M : m;
    }
    a.score[(size_t)k * (size_t)a.n_pos + (size_t)a.pos0 + t] = acc;
}

}  // namespace mcl_sbeam
