// mcl_rays_deskew.h -- the beam model's sensor stage while per-beam sensor offsets are on (mcl_set_beam_offsets):
// every beam of a particle has its own origin (DS2), so none of the kernels built on one origin per particle can take the stage.
// One kernel, one launch: no LDS window, no ordering, no work lists, no fix-up pass.  Named last in mcl_kernels.h, so the code
// object keeps its other kernels where they were.
#pragma once

namespace mcl {

constexpr int kDeskewThreads = 256;
constexpr int kDeskewWaves = kDeskewThreads / 64;
// flagged lanes of a round from which each marches its own ray: k_refine_beam_score's threshold (mcl_refine.h says how it was found)
constexpr int kDeskewLaneMarchMin = 16;

// The march's per-step displacement (cos, sin of the ray's angle times the resolution: march_exact's expressions), out of line: inlined,
// the constants of the fp64 cosine and sine are hoisted in front of the round loop and crowd the kernel's arguments out of the SGPRs.
// (static: the header's one including unit gets its own copy, and a second one or a relocatable-device-code build would get no duplicate)
static __device__ __attribute__((noinline)) double2 deskew_displacement(double angle, double res)
{
    return make_double2(cos(angle) * res, sin(angle) * res);
}

// One WAVE per particle i, four particles per workgroup; lane l takes beams l, l + 64, ... (Q3's order).  `a` is the stage's RayArgs
// with the SENSOR poses in x / y / th, the table of the offsets in beam_cs / beam_angle (DS1's pairs and float angles a', not the
// engine's own), the scan's rows in obs_idx and the static table in Ldirect; `off` is the 3 x B column-major table (ox, oy, dtheta).
// The particle's sincos once per wave, as particle_constants takes it.  Per lane and beam: the origin (DS2: frame_point's four
// multiply-adds), its pixel position, ray_origin, the level-2 walk on the isotropic field (k_query_rays' arithmetic), and a ballot
// of the lanes whose ray wants the literal march.  Few of them: the wave marches them one after the other (wave_march_exact_dir);
// from kDeskewLaneMarchMin on each marches its own (march_exact_dir) -- k_refine_beam_score's rule and threshold; one site forms the
// displacement of both (deskew_displacement).  Both are cast_ray's additions in its order from (x_ij, y_ij) at th + (double)a'_j
// (DS3).  Then the gather from L, the fp64 add and the butterfly (DS4); lane 0 writes the log-weight.  A step is stored only where
// the engine keeps ray steps.
// KEEP: 0 no step is stored, 1 8-bit steps, 2 16-bit steps (P > 255) -- the store's pointer is the only one of the three the kernel holds.
template <int KEEP>
__global__ __launch_bounds__(kDeskewThreads) void k_rays_deskew(RayArgs a, const double *__restrict__ off)
{
    const int lane = threadIdx.x & 63;
    // (the particle from the block index, not from a global thread index: 4M particles are 2^28 threads, the capacity has no bound)
    const int64_t i = (int64_t)blockIdx.x * kDeskewWaves + (threadIdx.x >> 6);
    if (i >= a.n) return;                                               // (whole waves leave together)
    const double xs = a.x[i], ys = a.y[i], th = a.th[i];
    double s, c;
    sincos(th, &s, &c);
    const bool heading_ok = th == th && fabs(th) < 1e6;
    const int tw = a.P + 1;
    double acc = 0.0;
    unsigned n3 = 0;
    for (int j0 = 0; j0 < a.B; j0 += 64) {
        const int j = j0 + lane;
        const bool live = j < a.B;
        int r = a.P;
        bool exact = false;
        double xb = 0.0, yb = 0.0;
        if (live) {
            frame_point(xs, ys, s, c, off[j], off[(size_t)a.B + j], xb, yb);
            const double2 px = pixel_position(xb, yb, heading_ok, a.ox, a.oy, a.res);
            const RayOrigin o = ray_origin(a, px.x, px.y);
            uint32_t amb = o.amb0;
            // (a ray bound for the march anyway needs no walk; from an origin on a cell edge the walk can only lower amb)
            if (!takes_literal_march(a, o.sane, o.amb0)) {
                const double2 cs = a.beam_cs[j];
                const double ux = c * cs.x - s * cs.y, uy = s * cs.x + c * cs.y;
                unsigned np = 0;
                r = trace_fp64<false, false>(a, nullptr, 0, kOriginBase, o.p0x, o.p0y, ux, uy, first_skip(a, o, a.dist), amb, np);
            }
            exact = takes_literal_march(a, o.sane, amb);
        }
        unsigned long long todo = __ballot(exact);
        const int n_exact = __popcll(todo);
        n3 += (unsigned)n_exact;
        // (one place takes the cosine and the sine for both forms of the march: the lane's own beam, or the beam of the lane whose turn it is)
        const bool own = n_exact >= kDeskewLaneMarchMin;               // (wave-uniform) many: every flagged lane marches its own ray
        while (todo) {                                                  // (wave-uniform: every lane is in every march)
            const int src = __ffsll((long long)todo) - 1;
            const int jj = own ? (live ? j : 0) : __shfl(j, src);
            const double angle = th + (double)a.beam_angle[jj];
            const double2 d = deskew_displacement(angle, a.res);
            const double dx = d.x, dy = d.y;
            if (own) {
                if (exact) r = march_exact_dir(a, xb, yb, dx, dy);
                todo = 0;
            } else {
                const int rr = wave_march_exact_dir(a, __shfl(xb, src), __shfl(yb, src), dx, dy, lane);
                if (lane == src) r = rr;
                todo &= todo - 1;
            }
        }
        if (live) {
            acc += (double)a.Ldirect[(size_t)a.obs_idx[j] * tw + r];
            if (KEEP == 1) a.steps[(size_t)i * a.B + j] = (uint8_t)r;
            if (KEEP == 2) a.steps16[(size_t)i * a.B + j] = (uint16_t)r;
        }
    }
    acc = wave_sum(acc);                                                // Q3's butterfly
    if (lane == 0) {
        a.logw[i] = acc;
        if (n3) atomicAdd(&a.counters[0], (unsigned long long)n3);
    }
}

}  // namespace mcl
