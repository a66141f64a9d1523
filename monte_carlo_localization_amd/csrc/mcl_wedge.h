// mcl_wedge.h — direction-binned skip fields ("wedge fields"), shared by the host code and the kernels.
//
// skip_k(c) bounds how far the fixed-step march (cast_ray, cpp:611-650) may jump from a sample inside cell c
// when the ray's direction angle lies in wedge k = [2*pi*k/K, 2*pi*(k+1)/K]:
//     skip_k(c) = floor( min over stop cells t REACHABLE from c in wedge k of gap(c, t) ) + 1,
// gap(c,t)^2 = max(|dx|-1,0)^2 + max(|dy|-1,0)^2 as for the isotropic field (mcl_host_math.hip).  A sample p in
// the half-open square of c and a later sample p + s*u (u in the wedge) inside the square of t differ by a
// vector of the wedge that lies in the OPEN square (t - c) + (-1,1)^2, so t is reachable only if that open
// square meets the closed wedge.  The wedge is the intersection of two half-planes n1.v >= 0, n2.v >= 0 inside
// one quadrant; an open square o + (-1,1)^2 meets {n.v >= 0} iff n.o + |nx| + |ny| > 0, and it meets the
// quadrant iff sx*ox >= 0 and sy*oy >= 0.  Testing the three conditions separately keeps a superset of the
// reachable cells (corners near the apex), which is the safe direction.  Walls beside a ray no longer shorten
// its jumps; with K = 16 the benchmark input needs 3.9 probes per ray instead of 5.2 with quadrant fields.
// That is the EUCLIDEAN rule (wedge_skip_cell, mcl_host_skip_field_wedge).  What mcl_set_map builds is the TIGHT rule further down
// (wedge_skip_cell_tight): the same candidate cells, each bounded by the distance travelled inside the wedge.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define MCL_HD __host__ __device__
#else
#define MCL_HD
#endif

namespace mcl {

#ifndef MCL_KWEDGES
#define MCL_KWEDGES 16                   // (a build with another count is an experiment: include/mcl_hip_engine.h says 16)
#endif
constexpr int kWedges = MCL_KWEDGES;     // direction bins per turn (a power of two, multiple of 4)
constexpr int kWedgeShift = kWedges == 8 ? 1 : kWedges == 16 ? 2 : kWedges == 32 ? 3 : 4;   // log2(kWedges / 4): bin -> quadrant
static_assert(kWedges == (4 << kWedgeShift), "kWedges must be 8, 16, 32 or 64");
constexpr int kWedgeR = 255;             // offsets searched per axis: gaps beyond 254 are capped anyway

struct WedgeRow { int16_t xa, xb; };     // reachable offsets ox in row oy: xa..xb (none when xa > xb)

// rows[oy + kWedgeR] for oy = -kWedgeR..kWedgeR.  For every row the reachable ox form one interval (the three
// conditions are convex); it is found by testing every ox.
inline void wedge_rows(int k, WedgeRow *rows)
{
    const double two_pi = 6.283185307179586476925286766559;
    const double a0 = two_pi * k / kWedges, a1 = two_pi * (k + 1) / kWedges;
    const double n1x = -std::sin(a0), n1y = std::cos(a0);      // left of the lower edge
    const double n2x = std::sin(a1), n2y = -std::cos(a1);      // right of the upper edge
    const double e1 = std::fabs(n1x) + std::fabs(n1y), e2 = std::fabs(n2x) + std::fabs(n2y);
    const int q = k >> kWedgeShift;
    const int sx = (q == 0 || q == 3) ? 1 : -1, sy = (q == 0 || q == 1) ? 1 : -1;
    for (int oy = -kWedgeR; oy <= kWedgeR; ++oy) {
        int xa = 1, xb = 0;
        bool any = false;
        for (int ox = -kWedgeR; ox <= kWedgeR; ++ox) {
            // 1e-9: the sums are either exactly zero in real arithmetic (square touches the edge: not reachable)
            // or larger than 1e-3 for |o| <= 255, so rounding cannot move a reachable offset below the threshold
            const bool in = sx * ox >= 0 && sy * oy >= 0 && (n1x * ox + n1y * oy + e1 > 1e-9) && (n2x * ox + n2y * oy + e2 > 1e-9);
            if (in) { if (!any) { xa = ox; any = true; } xb = ox; }
        }
        rows[oy + kWedgeR].xa = (int16_t)xa;
        rows[oy + kWedgeR].xb = (int16_t)xb;
    }
}

// nxt[y*Wp + x]: smallest x' >= x with stop(x', y), Wp when there is none; prv: largest x' <= x, -1 when none.
// Cells outside the padded grid are stops (cpp:632-636).
MCL_HD inline int wedge_skip_cell(const int32_t *nxt, const int32_t *prv, int Wp, int Hp, int x, int y, const WedgeRow *rows)
{
    if (nxt[(size_t)y * Wp + x] == x) return 0;                // a stop cell
    int64_t best = (int64_t)1 << 40;
    for (int d = 0; d <= kWedgeR; ++d) {
        const int64_t gy = d > 1 ? d - 1 : 0;
        if (gy * gy >= best) break;
        for (int sgn = (d == 0 ? 1 : -1); sgn <= 1; sgn += 2) {
            const int oy = sgn * d;
            const WedgeRow r = rows[oy + kWedgeR];
            if (r.xa > r.xb) continue;
            const int yy = y + oy, lo = x + r.xa, hi = x + r.xb;
            const bool row_in = yy >= 0 && yy < Hp;
            int ox = 1 << 20;                                   // smallest |ox| of a reachable stop in this row
            if (r.xa <= 0 && r.xb >= 0) {                       // the interval contains ox = 0: look both ways
                const int xr = row_in ? nxt[(size_t)yy * Wp + x] : x;
                const int xl = row_in ? prv[(size_t)yy * Wp + x] : x;
                if (xr <= hi) ox = xr - x;
                if (xl >= lo && x - xl < ox) ox = x - xl;
            } else if (r.xa > 0) {                              // strictly to the right
                const int xr = (!row_in || lo >= Wp) ? lo : nxt[(size_t)yy * Wp + lo];
                if (xr <= hi) ox = xr - x;
            } else {                                            // strictly to the left
                const int xl = (!row_in || hi < 0) ? hi : prv[(size_t)yy * Wp + hi];
                if (xl >= lo) ox = x - xl;
            }
            if (ox < (1 << 20)) {
                const int64_t gx = ox > 1 ? ox - 1 : 0;
                const int64_t g2 = gx * gx + gy * gy;
                if (g2 < best) best = g2;
            }
        }
    }
    if (best >= (int64_t)254 * 254) return 255;
    int64_t rt = (int64_t)sqrt((double)best);
    while (rt * rt > best) --rt;
    while ((rt + 1) * (rt + 1) <= best) ++rt;
    return (int)(rt + 1);
}

// ---- the tight rule: bound a jump by the distance travelled INSIDE the wedge ---------------------------------------------------
//
// gap(c,t) is attained between the two nearest points of the cell squares.  For a stop cell that straddles an edge of the wedge
// the direction joining them lies outside the wedge: no ray of the wedge travels that short way (a wall beside a ray).  With
// o = t - c let
//     D_k(o) = distance from the origin to  closure(o + (-1,1)^2)  ∩  closed wedge k,
//     skip_k(c) = floor( min over the same candidate stop cells t of D_k(t - c) ) + 1.
// Why this is safe: a sample p in the half-open square of c and a later sample p + s*u (u a unit vector of the wedge, s the number
// of samples in between) inside the square of t differ by v = s*u, a vector of the wedge in the OPEN square o + (-1,1)^2, and
// |v| = s.  The closed intersection is convex and does not contain the origin (else D = 0 and nothing is claimed), so its nearest
// point is unique and lies on its boundary: either on the boundary of the square, or on an edge ray of the wedge inside the square
// -- and along a ray from the origin the distance grows, so that point is where the edge ray ENTERS the closed square, again a
// boundary point of the square.  v lies in the open square, so v is not that point and |v| > D strictly: s >= floor(D) + 1 even
// when D is an integer.  The nearest point is therefore one of
//   * the square's own nearest point to the origin, if it lies in the wedge (then D = gap: today's value), or
//   * the entry point of one of the two edge rays into the closed square (slab test; the edge directions are unit vectors, so
//     the ray parameter is the distance),
// and D is the minimum over those that exist.  Where none exists -- the three separate conditions of wedge_rows admit a few
// offsets next to the apex that the wedge does not truly meet -- the value stays gap's.  D >= gap always (the intersection is a
// subset of the square); the result is clamped from below by today's value so rounding can never make a skip shorter.
// Margins (the safe direction is the smaller skip): D is evaluated for the wedge WIDENED by kWedgeWiden = 1e-7 rad on both
// sides, and kWedgeSlack = 1e-6 px is taken off before the floor.  beam_wedge bins th + angle in fp64 (|th| < 1e6: 2.4e-10 rad of
// rounding at most, and the ray's own direction comes from the same sum), the edge directions below carry 1e-16, and the few
// flops of wedge_tight_value lose less than 1e-12 px at |o| <= 255: both margins are larger by three orders of magnitude or
// more.  The direction error of the 32-bit walk (level 1) is not covered here and need not be: a walk whose samples all lie
// outside the guard band reads the same cells as the exact ray, and the others are re-run.
// What reads these fields: the walks of k_rays_sweep (LDS windows, the ringed global copies, the hybrid of both) and k_rays_fix's
// fp64 re-trace, each with the field of the ray's own beam_wedge bin, so the geometry above is theirs.  Where they may READ does
// not depend on the bytes: a walk ends when the skip exceeds the samples left (or its window budget), skips stay capped at 127 as
// stored, and the window / tail bounds are arithmetic on samples left (sweep_global_layout below) -- also for the
// virtual beams that pad a scan-edge wedge and may point outside it: they can skip over a wall their field does not know of,
// but they add zero table columns and advance by no more samples than any other ray.
// Along a row of offsets the value is non-decreasing in |ox| over the reachable interval, which is what lets the search look at
// the nearest stop of a row only: for |oy| >= 2 the wedge cut by the row's strip has its nearest point to the origin at its
// smallest |x| (the strip's near line meets the steeper edge there), dist(origin, that set ∩ {x}) is convex in x, and the minimum
// of a convex function over the sliding window [ox-1, ox+1] does not decrease once the window has reached the minimiser; for
// |oy| <= 1 the strip holds the origin and the value is gap's.  The final max with today's (monotone) value keeps that order.
// tests/test_wedge_tight.py enumerates every row for |o| <= 255 and all wedges, on the compiled arithmetic of the host twin.
// That the kernel computes the same bytes (both are built without contraction; the kernel takes its stop cells from the uploaded
// isotropic field, the twin from the grid) is what tests/test_gpu_ray_tables.py checks: the device's fields read back
// (mcl_get_wedge_fields) against the twin's, byte for byte, under both rules.
constexpr double kWedgeWiden = 1e-7;     // rad, each side
constexpr double kWedgeSlack = 1e-6;     // px, before the floor

struct WedgeCone {                       // the widened wedge: unit edge directions, their reciprocals, inward normals' signs folded in
    double ax, ay, bx, by;               // lower edge (angle a0 - widen), upper edge (a1 + widen)
    double iax, iay, ibx, iby;           // 1 / component (inf where a component is zero: the slab test handles it)
};

inline WedgeCone wedge_cone(int k)
{
    const double two_pi = 6.283185307179586476925286766559;
    const double a0 = two_pi * k / kWedges - kWedgeWiden, a1 = two_pi * (k + 1) / kWedges + kWedgeWiden;
    WedgeCone w;
    w.ax = std::cos(a0); w.ay = std::sin(a0); w.bx = std::cos(a1); w.by = std::sin(a1);
    w.iax = 1.0 / w.ax; w.iay = 1.0 / w.ay; w.ibx = 1.0 / w.bx; w.iby = 1.0 / w.by;
    return w;
}

// distance along the unit ray (ex, ey) from the origin to its entry into the closed square [lx, hx] x [ly, hy]; < 0: no entry
MCL_HD inline double wedge_ray_entry(double ex, double ey, double iex, double iey, double lx, double hx, double ly, double hy)
{
    double t0 = 0.0, t1 = 1e30;
    if (ex == 0.0) { if (lx > 0.0 || hx < 0.0) return -1.0; }
    else { const double p = lx * iex, q = hx * iex; t0 = fmax(t0, fmin(p, q)); t1 = fmin(t1, fmax(p, q)); }
    if (ey == 0.0) { if (ly > 0.0 || hy < 0.0) return -1.0; }
    else { const double p = ly * iey, q = hy * iey; t0 = fmax(t0, fmin(p, q)); t1 = fmin(t1, fmax(p, q)); }
    return t0 <= t1 ? t0 : -1.0;
}

MCL_HD inline int wedge_isqrt(int64_t v)
{
    int64_t rt = (int64_t)sqrt((double)v);
    while (rt * rt > v) --rt;
    while ((rt + 1) * (rt + 1) <= v) ++rt;
    return (int)rt;
}

// the skip a stop cell at offset (ox, oy) allows under the tight rule, uncapped: max(floor(gap) + 1, floor(D - slack) + 1)
MCL_HD inline int wedge_tight_value(const WedgeCone &w, int ox, int oy)
{
    const int ax = ox < 0 ? -ox : ox, ay = oy < 0 ? -oy : oy;
    const int gx = ax > 1 ? ax - 1 : 0, gy = ay > 1 ? ay - 1 : 0;
    const int base = wedge_isqrt((int64_t)gx * gx + (int64_t)gy * gy) + 1;
    if (gx == 0 && gy == 0) return base;                                    // the closed square holds the origin: D = 0
    const double nx = ox < 0 ? -(double)gx : (double)gx, ny = oy < 0 ? -(double)gy : (double)gy;   // the square's nearest point
    if (w.ax * ny - w.ay * nx >= 0.0 && nx * w.by - ny * w.bx >= 0.0) return base;                 // ... lies in the wedge: D = gap
    const double lx = ox - 1.0, hx = ox + 1.0, ly = oy - 1.0, hy = oy + 1.0;
    const double ta = wedge_ray_entry(w.ax, w.ay, w.iax, w.iay, lx, hx, ly, hy);
    const double tb = wedge_ray_entry(w.bx, w.by, w.ibx, w.iby, lx, hx, ly, hy);
    double D = -1.0;
    if (ta >= 0.0) D = ta;
    if (tb >= 0.0 && (D < 0.0 || tb < D)) D = tb;
    if (D < 0.0) return base;                                               // admitted by the superset test only: keep gap
    const int v = (int)floor(D - kWedgeSlack) + 1;
    return v > base ? v : base;
}

// wedge_skip_cell under the tight rule: the same rows, intervals and nearest stops; a row at distance d cannot give less than d
// (D >= gap >= d - 1), which is the early exit.  Where a row's interval holds ox = 0 both neighbours are evaluated (the value
// is not symmetric in ox).
MCL_HD inline int wedge_skip_cell_tight(const int32_t *nxt, const int32_t *prv, int Wp, int Hp, int x, int y, const WedgeRow *rows,
                                        const WedgeCone &w)
{
    if (nxt[(size_t)y * Wp + x] == x) return 0;                // a stop cell
    int best = 255;
    for (int d = 0; d <= kWedgeR; ++d) {
        if (d >= best) break;
        for (int sgn = (d == 0 ? 1 : -1); sgn <= 1; sgn += 2) {
            const int oy = sgn * d;
            const WedgeRow r = rows[oy + kWedgeR];
            if (r.xa > r.xb) continue;
            const int yy = y + oy, lo = x + r.xa, hi = x + r.xb;
            const bool row_in = yy >= 0 && yy < Hp;
            int oxr = 1 << 20, oxl = 1 << 20;                   // offsets of the nearest reachable stop to the right (>= 0) / left (as -oxl)
            if (r.xa <= 0 && r.xb >= 0) {
                const int xr = row_in ? nxt[(size_t)yy * Wp + x] : x;
                const int xl = row_in ? prv[(size_t)yy * Wp + x] : x;
                if (xr <= hi) oxr = xr - x;
                if (xl >= lo) oxl = x - xl;
            } else if (r.xa > 0) {
                const int xr = (!row_in || lo >= Wp) ? lo : nxt[(size_t)yy * Wp + lo];
                if (xr <= hi) oxr = xr - x;
            } else {
                const int xl = (!row_in || hi < 0) ? hi : prv[(size_t)yy * Wp + hi];
                if (xl >= lo) oxl = x - xl;
            }
            // (a stop whose gap alone reaches `best` cannot lower it: no need to look at its D)
            const int64_t gy = d > 1 ? d - 1 : 0, lim = (int64_t)(best - 1) * (best - 1);
            if (oxr < (1 << 20)) {
                const int64_t gx = oxr > 1 ? oxr - 1 : 0;
                if (gx * gx + gy * gy < lim) { const int v = wedge_tight_value(w, oxr, oy); if (v < best) best = v; }
            }
            if (oxl < (1 << 20) && oxl != 0) {
                const int64_t gx = oxl > 1 ? oxl - 1 : 0;
                if (gx * gx + gy * gy < lim) { const int v = wedge_tight_value(w, -oxl, oy); if (v < best) best = v; }
            }
        }
    }
    return best;
}

// Layout of the sixteen mirrored, ringed wedge fields k_rays_sweep<.., GLOBAL> probes in place (mcl_rays_sweep.h, k_ring_field),
// and the proof obligation that goes with it: the kernel forms the byte offset  row * pitch + column  from the START of the
// allocation, with column = k * stride + cell column.  A walk of field k starts in a cell of the ringed grid (row < Hp + 4,
// column < Wp + 4 <= pitch), runs towards +x, +y only and advances by at most P samples of at most one cell per axis in total
// (a skip larger than the samples left ends the walk before the jump is made; the start's fraction and the guard bias add
// less than one more cell), so the largest offset it can form is
//   k * stride + (Hp + 4 + P) * pitch + (Wp + 4 + P)   =  sweep_global_max_offset(k)
// which must lie inside field k's own stride (rows of stop bytes behind the ringed grid: the tail), and the whole allocation
// below 2^32 (the offset is a 32-bit VGPR); the multiplicands of the kernel's v_mad_u32_u24 (row, pitch) must fit 24 bits.
struct SweepGlobalLayout { bool ok; int pitch; int rows; size_t stride, alloc; };
inline SweepGlobalLayout sweep_global_layout(int Wp, int Hp, int P)
{
    SweepGlobalLayout g{};
    g.pitch = (Wp + 4 + 63) & ~63;
    const int tail = P + 2 + (P + 4 + g.pitch - 1) / g.pitch;        // rows the walk can run past the ringed grid, column overflow included
    g.rows = Hp + 4 + tail;
    g.stride = (size_t)g.rows * (size_t)g.pitch;
    g.alloc = g.stride * (size_t)kWedges;
    g.ok = g.alloc < ((size_t)1 << 32) && g.rows + P < (1 << 24) && g.pitch < (1 << 24) && P >= 1;
    return g;
}
inline size_t sweep_global_max_offset(const SweepGlobalLayout &g, int Wp, int Hp, int P, int k)
{
    return (size_t)k * g.stride + (size_t)(Hp + 4 + P) * (size_t)g.pitch + (size_t)(Wp + 4 + P);
}

}  // namespace mcl
