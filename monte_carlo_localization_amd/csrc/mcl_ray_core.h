// mcl_ray_core.h -- the one statement of what decides a ray's step index (E3) at levels 2 and 3, and an observation's table row
// (E2): the arguments, the origin set-up of the fp64 walk, the walk, the rule that sends a ray to the literal march, that march
// by a lane and by a wave, and the list of rays waiting for it.  The update's ray kernels (mcl_kernels.h) and the side calls
// (mcl_query.h, mcl_search_beam.h, mcl_refine.h) call these functions, so a particle and a queried pose at the same place get
// the same bits.  Device functions only, no kernels: every translation unit with device code may include it.
#pragma once
#include "mcl_types.h"

namespace mcl {

// per-particle constants of the ray stage: (cos, sin, pixel x, pixel y); a garbage heading gets a NaN pixel position (the
// pair fails every window test and is marched literally)
__device__ __forceinline__ double4 particle_constants(double x, double y, double t, double ox, double oy, double res)
{
    double s, c;
    sincos(t, &s, &c);
    const bool heading_ok = t == t && fabs(t) < 1e6;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    return make_double4(c, s, heading_ok ? (x - ox) / res : nanv, heading_ok ? (y - oy) / res : nanv);
}

// The same constants in two steps, for an update whose ordering gather finishes them (the radix path: k_resample_* writes the
// heading form, k_sort_gather makes the full form of it): (heading, 0, pixel x, pixel y) with particle_constants' pixel position ...
__device__ __forceinline__ double4 particle_heading_record(double x, double y, double t, double ox, double oy, double res)
{
    const bool heading_ok = t == t && fabs(t) < 1e6;
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    return make_double4(t, 0.0, heading_ok ? (x - ox) / res : nanv, heading_ok ? (y - oy) / res : nanv);
}
// ... and particle_constants' sincos of the same argument: the bits of particle_constants(x, y, t, ..)
__device__ __forceinline__ double4 particle_constants_of(const double4 &rec)
{
    double s, c;
    sincos(rec.x, &s, &c);
    return make_double4(c, s, rec.z, rec.w);
}

// particle_constants' pixel position alone, for a caller that took the sincos of the heading once for many positions (k_rays_deskew)
__device__ __forceinline__ double2 pixel_position(double x, double y, bool heading_ok, double ox, double oy, double res)
{
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    return make_double2(heading_ok ? (x - ox) / res : nanv, heading_ok ? (y - oy) / res : nanv);
}

// The point (mx, my) of a frame at (x, y) whose heading has the sine s and the cosine c: SM2's position (mount_pose, mcl_mount.h) and
// DS2's beam origin, the one statement of both.  fp64, in this order, no contraction.
__device__ __forceinline__ void frame_point(double x, double y, double s, double c, double mx, double my, double &xs, double &ys)
{
    xs = x + (c * mx - s * my);
    ys = y + (s * mx + c * my);
}

// lidarCB's downsampled range -> table row of a beam, cpp:549-554, 570, 573 (NaN -> 0)
__device__ __forceinline__ int obs_index_of(float obs, double res, int P)
{
    float px = (float)((double)obs / res);
    if (px > (float)P) px = (float)P;
    float r = roundf(px);
    int idx;
    if (r != r) idx = 0;
    else if (r <= -2147483648.0f) idx = 0;
    else idx = (int)r;
    idx = idx > P ? P : idx;
    idx = idx < 0 ? 0 : idx;
    return idx;
}

struct RayArgs {
    const double *x, *y, *th;      // particles (this launch's)
    const double4 *pc;             // per particle (cos th, sin th, (x-ox)/res, (y-oy)/res), k_particle_prep
    const short4 *qr;              // per particle quadrant ranges of its beams (k_rays_quad), k_particle_prep
    const double4 *pcs;            // k_rays_cell: pc in cell-sorted order (k_sort_scatter)
    const uint32_t *perm;          // k_rays_cell: sorted slot -> particle index
    const double *ths;             // k_rays_cell: heading in cell-sorted order
    const double2 *slice_mean;     // k_rays_cell: mean pixel position of every slice of the sorted order (k_slice_means)
    const uint8_t *distw;          // k_rays_cell: kWedges wedge fields (mcl_wedge.h), field k at distw + k * distw_stride
    size_t distw_stride;
    const uint8_t *distg;          // k_rays_sweep<.., GLOBAL>: the same fields mirrored per quadrant, with a two-cell ring of stop bytes around the
    size_t distg_stride;           //   padded grid and a tail of stop rows: mirrored padded cell (y, x) of field k at distg + k * distg_stride +
    int distg_pitch;               //   (y + 2) * distg_pitch + (x + 2); distg is the START of the allocation (every offset the kernel forms is >= 0)
    int qside;                     // k_rays_quad: window side in cells (1 byte per cell)
    int nslices;                   // k_rays_quad: particle slices; grid = 4 * nslices
    unsigned long long *fix_list;  // k_rays_quad -> k_rays_fix: (particle << 16 | beam) of undecided rays
    unsigned long long *fix_count; // per workgroup of k_rays_quad (stride 8 words): entries appended (> fix_cap: overflow)
    unsigned long long fix_cap;    // capacity of one workgroup's segment
    int fix_segments;              // number of segments = workgroups of k_rays_quad
    unsigned long long *exact_list;   // k_rays_fix -> k_rays_exact: rays that need the literal march (level 3)
    unsigned long long *exact_count;  // entries appended (beyond exact_cap: marched inline by k_rays_fix)
    unsigned long long exact_cap;
    uint8_t *far_flags;            // [particle][quadrant]: pair does not fit its quadrant window -> k_rays_far
    unsigned long long *work_counter;  // k_rays_quad: next (slice, quadrant) item
    unsigned long long *dbg;       // optional [workgroup][4]: start, end (s_memrealtime, 100 MHz), HW_ID, XCC_ID
    int64_t n;
    int B, bpad, P;
    const double2 *beam_cs;        // (cos a_j, sin a_j) of (double)angle_f32[j], host fp64
    const double2 *beam_csx;       // k_rays_sweep: the same with beam_margin virtual beams before beam 0 and after beam B - 1 (entry j + beam_margin)
    int beam_pad, beam_margin;     // beams of a full wedge up to which a scan-edge lane is padded with virtual beams (0: never); see k_rays_sweep
    const double2 *beam_csi;       // k_rays_sweep<.., REC>: (cos, sin) of the GRID angle a0 + j inc of every table column (entry j + beam_margin)
    const double *beam_err;        //   and the beam's own offset from it, a_j - (a0 + j inc) (0 for virtual beams and padding): ltd_cols entries
    double rec_k;                  //   2 cos(inc): the three-term recurrence of the turned direction (MCL_SW_STEP_REC)
    const float *beam_angle;       // float angles (MARCH path uses theta + (double)angle)
    double beam_a0, beam_inv_inc;  // first angle and beams per radian (k_rays_cell's guess of a wedge's first beam)
    double beam_alast;             // last angle: (double)beam_angle[B - 1]
    const float *Lt;               // (P+1) x bpad
    const float *Ltr;              // the same with the rows reversed (row P - d)
    const double *Ltd;             // k_rays_sweep: fp64 table indexed by samples left + kSwUnder (mcl_rays_sweep.h), ltd_cols columns
    int ltd_cols;
    int sweep_g;                   // k_rays_sweep: wedges per work item
    int split16;                   // k_rays_sweep: passes of 9..16 chunks are handed out in halves too (small launches)
    const int4 *items;             // k_rays_sweep: work items (first unit, units, wedge group, run), big first (guided schedule)
    const int4 *centres;           // k_rays_sweep: per run of units (window centre as a padded cell x, y; first unit; units), k_sweep_plan
    int nitems;
    const int *nitems_ptr;          // k_rays_sweep: number of work items, written by k_sweep_plan
    const double4 *unit_sums;      // k_rays_sweep: per unit of the sorted order (sum px, sum py, count, -) and its bounding box, k_unit_sums
    const uint32_t *unit_begin;    // k_rays_sweep: first slot of every unit, one entry past the last (k_unit_table)
    uint32_t *far_list;            // k_rays_sweep -> k_rays_far: slots with at least one flagged quadrant (appended once each), or null
    unsigned long long *far_count; // entries in far_list
    const uint32_t *far_sorted;    // k_rays_skip<.., FAR>: the flagged slots in ascending (= spatial) order, k_far_scatter
    const unsigned long long *far_min;   // the windowed far pass runs when *far_count >= *far_min ... (k_rays_far: when below)
    int far_windowed;              // k_rays_far: 1 = a windowed far pass was launched beside it (stand down when it runs)
    int slot_space;                // 1: fix-list entries, far flags and `logw` are indexed by sorted slot (k_rays_sweep), and the
                                   // per-particle constants of k_rays_fix / k_rays_far come from pcs / ths; perm gives the particle
    double *logw;                  // out
    uint8_t *steps;                // out N*B or null
    uint16_t *steps16;             // the same as 16-bit entries, for maps whose range exceeds 255 px (k_rays_march / k_rays_skip)
    // map
    const int8_t *grid; int W, H;
    double res, ox, oy;
    const uint8_t *dist;           // padded distance field Hp x Wps bytes (0 = stop), cap 255
    const float *Ldirect;          // k_rays_skip, small updates: the static table L[row][step] read through obs_idx (no per-update
    const int32_t *obs_idx;        //   transposed copy is built); null = use Lt
    const uint8_t *dist4;          // the same field as nibbles min(d, 15), two cells per byte, Hp x Wps/2 bytes (k_rays_skip's window)
    const uint8_t *distq[4];       // directional fields per quadrant (k_rays_quad, k_rays_far)
    int Wp, Hp, Wps;
    int tw_cells;                  // LDS window side (multiple of 8)
    unsigned long long *counters;  // [0] exact-fallback rays, [1] particles off-window, [2] probes
    int force_exact;
};

// the fp64 positions of levels 2 and 3 (the three precision levels are described at k_rays_skip, mcl_rays_basic.h)
// fp64 fixed-point extraction: t = p + kMagic puts floor(p)+2^19 in the low 20 bits of the high
// dword and the fraction (2^-32 units, biased by +4) in the low dword; lo < kGuard <=> within 2^-30 px.
constexpr double kMagic = 1572864.0 + 0x1p-30;   // 1.5 * 2^20 + 2^-30
constexpr uint32_t kGuard = 8u;
constexpr int kCellBase = 1 << 19;

// Level 3: the literal restatement of cast_ray (cpp:611-650) on the int8 grid, with its per-step displacement given; returns the
// step index (0..P-1) or P for "no hit within MAX_RANGE_PX samples".  The displacement form exists for directions the host
// formed (the global search under the beam model, rule B2): the products of the host's cosine and sine with the resolution,
// so the additions are the oracle's additions.
__device__ __forceinline__ int march_exact_dir(const RayArgs &a, double x, double y, double dx, double dy)
{
    double cx = x, cy = y;
    for (int step = 0; step < a.P; ++step) {
        cx += dx;
        cy += dy;
        int gx = (int)((cx - a.ox) / a.res);
        int gy = (int)((cy - a.oy) / a.res);
        if (gx < 0 || gx >= a.W || gy < 0 || gy >= a.H) return step;
        if (a.grid[(size_t)gy * a.W + gx] > 50) return step;
    }
    return a.P;
}

// the same with the cosine and the sine of an angle taken on the device
__device__ __forceinline__ int march_exact(const RayArgs &a, double x, double y, double angle)
{
    return march_exact_dir(a, x, y, cos(angle) * a.res, sin(angle) * a.res);
}

// The same march by a whole WAVE.  Lane l accumulates `current += d` l + 1 times exactly as the reference's single accumulator
// does (the same additions in the same order, so the same bits), then the 64 lanes test 64 consecutive samples at once; the
// first stop wins.  Every argument but `lane` is wave-uniform and all 64 lanes must be here; every lane gets the result.  (Only
// the displacement form: a caller with an angle forms cos(angle) * res, sin(angle) * res BEFORE it loads x and y, which
// otherwise stay in registers across the cosine and the sine.)
__device__ __forceinline__ int wave_march_exact_dir(const RayArgs &a, double x, double y, double dx, double dy, int lane)
{
    double cx = x, cy = y;
    for (int t = 0; t <= lane; ++t) { cx += dx; cy += dy; }            // sample lane + 1 of the sequential accumulation
    for (int s0 = 0; s0 < a.P; s0 += 64) {
        const int step = s0 + lane;
        bool hit = false;
        if (step < a.P) {
            const int gx = (int)((cx - a.ox) / a.res), gy = (int)((cy - a.oy) / a.res);
            hit = gx < 0 || gx >= a.W || gy < 0 || gy >= a.H || a.grid[(size_t)gy * a.W + gx] > 50;
        }
        const unsigned long long hits = __ballot(hit);
        if (hits) return s0 + (__ffsll((long long)hits) - 1);
        for (int t = 0; t < 64; ++t) { cx += dx; cy += dy; }            // 64 samples further
    }
    return a.P;
}

// fp64 skipping march of one ray, on the LDS nibble window (LDSWIN) or on the global byte field.
template <bool LDSWIN, bool COUNT>
__device__ __forceinline__ int trace_fp64(const RayArgs &a, const unsigned char *ldsb, int strideB, int base, double p0x, double p0y,
                                          double ux, double uy, int s0, uint32_t &amb, unsigned &np, const uint8_t *field = nullptr,
                                          bool wedge_coded = false)
{
    const uint8_t *gf = field ? field : a.dist;
    int s = s0, r = a.P;
    if (s > a.P) return r;
    while (true) {
        double sd = (double)s;
        double tx = __builtin_fma(sd, ux, p0x);
        double ty = __builtin_fma(sd, uy, p0y);
        uint32_t lox = (uint32_t)__double2loint(tx), loy = (uint32_t)__double2loint(ty);
        int cx = (__double2hiint(tx) & 0xFFFFF) - base;
        int cy = (__double2hiint(ty) & 0xFFFFF) - base;
        uint32_t mlo = lox < loy ? lox : loy;
        amb = amb < mlo ? amb : mlo;
        int d;
        if (LDSWIN) {
            uint32_t byte = ldsb[cy * strideB + (cx >> 1)];
            d = (byte >> ((cx & 1) * 4)) & 15;
        } else {
            d = ((unsigned)cx < (unsigned)a.Wp && (unsigned)cy < (unsigned)a.Hp) ? gf[(size_t)cy * a.Wps + cx] : 0;
            if (wedge_coded) d = d == 255 ? 0 : d;        // a wedge field (mcl_wedge.h) as the windows hold it: 0xFF = stop, skips 1..127
        }
        if (COUNT) ++np;
        if (d == 0) { r = s - 1; break; }
        s += d;
        if (s > a.P) break;
    }
    return r;
}

// Where the fp64 walk of a ray from pixel position (px, py) starts: padded global coordinates shifted by 2^18, so `base` of
// trace_fp64 is kOriginBase.  Outside the window of +-200000 px (NaN included) the position is not `sane`: the ray is marched
// literally, amb0 is 0, `inside` is false and the cell means nothing.  (No branch on `sane` here: k_rays_fix keeps its registers.)
constexpr int kOriginBase = kCellBase + 262144;
struct RayOrigin {
    double p0x, p0y;               // the position as trace_fp64 takes it
    uint32_t amb0;                 // min of the two fractions: what the walk's `amb` starts from
    int cx, cy;                    // the start cell in the padded field
    bool sane, inside;             // inside: the start cell lies in the padded field
};
__device__ __forceinline__ RayOrigin ray_origin(const RayArgs &a, double px, double py)
{
    RayOrigin o;
    o.sane = (px > -200000.0) && (px < 200000.0) && (py > -200000.0) && (py < 200000.0);
    o.p0x = (px + 1.0 + 262144.0) + kMagic; o.p0y = (py + 1.0 + 262144.0) + kMagic;
    const uint32_t lox = (uint32_t)__double2loint(o.p0x), loy = (uint32_t)__double2loint(o.p0y);
    o.cx = (__double2hiint(o.p0x) & 0xFFFFF) - kOriginBase; o.cy = (__double2hiint(o.p0y) & 0xFFFFF) - kOriginBase;
    o.amb0 = o.sane ? (lox < loy ? lox : loy) : 0u;
    o.inside = o.sane && (unsigned)o.cx < (unsigned)a.Wp && (unsigned)o.cy < (unsigned)a.Hp;
    return o;
}

// the first sample of the walk (trace_fp64's s0): the skip the caller's own field allows at the start cell, at least 1
__device__ __forceinline__ int first_skip(const RayArgs &a, const RayOrigin &o, const uint8_t *field, bool wedge_coded = false)
{
    int d = o.inside ? field[(size_t)o.cy * a.Wps + o.cx] : 0;
    if (wedge_coded && d == 255) d = 0;
    return d > 1 ? d : 1;
}

// this ray takes the literal march: `amb` is what the walk left (the origin's amb0 where none ran)
__device__ __forceinline__ bool takes_literal_march(const RayArgs &a, bool sane, uint32_t amb)
{
    return !sane || amb < kGuard || a.force_exact == 1;
}

// The side calls' list of rays waiting for the literal march, a wave each.  E: the entry, a ray index of the call.
struct Level3Header {
    unsigned long long listed;      // rays appended to the list (may exceed its capacity: those were marched inline)
    unsigned long long level3;      // rays the literal march decided
};

// true: the ray is on the list.  false: the list is full, the lane marches its ray itself and counts it in level3.
template <class E>
__device__ __forceinline__ bool level3_append(Level3Header *hdr, E *list, unsigned long long cap, E ray)
{
    const unsigned long long slot = atomicAdd(&hdr->listed, 1ull);
    if (slot >= cap) return false;
    list[slot] = ray;
    return true;
}

// entries on the list, for a later kernel (an earlier kernel's atomics: plain loads see them)
__device__ __forceinline__ unsigned long long level3_listed(const Level3Header *hdr, unsigned long long cap)
{
    const unsigned long long n = hdr->listed;
    return n > cap ? cap : n;
}

}  // namespace mcl
