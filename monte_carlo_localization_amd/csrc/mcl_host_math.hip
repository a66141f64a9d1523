// mcl_host_math.hip -- the host arithmetic of the engine: everything that neither calls HIP nor touches a mcl_engine.  The tables and
// fields built here are defined bit for bit (compiled with the flags of the other units: -ffp-contract=off), and the mcl_host_*
// entry points of the ABI (include/mcl_hip_engine.h) hand them to the tests as they are.  No kernels: mcl_kernels.h is not included;
// the few __host__ __device__ rules shared with the kernels live in mcl_types.h (kld_bin), mcl_motion.h (odo_step) and mcl_wedge.h.
#include "mcl_host_math.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "mcl_motion.h"
#include "mcl_refine_core.h"
#include "mcl_wedge.h"
#include "mcl_sort_key.h"
#include "mcl_compact_guide.h"

namespace mcl_host {

// What the sensor model's fields must satisfy for the table to be a probability table (null: they do).  The reference does not
// check them; here a NaN or a zero row would reach every log-weight (E5).
const char *bad_sensor_fields(const mcl_config_t &c)
{
    const double z[4] = {c.z_hit, c.z_short, c.z_max, c.z_rand};
    for (double v : z)
        if (!std::isfinite(v) || v < 0.0) return "bad config (z_hit, z_short, z_max and z_rand must be finite and >= 0)";
    if (z[0] == 0.0 && z[1] == 0.0 && z[2] == 0.0 && z[3] == 0.0) return "bad config (z_hit, z_short, z_max and z_rand are all 0)";
    if (!std::isfinite(c.sigma_hit) || !(c.sigma_hit > 0.0)) return "bad config (sigma_hit must be finite and > 0)";
    return nullptr;
}

// cpp:233-292, restated; column-major (d*(tw)+r).
void build_sensor_table(const mcl_config_t &c, int P, std::vector<double> &t)
{
    const int tw = P + 1;
    t.assign((size_t)tw * tw, 0.0);
    for (int d = 0; d < tw; ++d) {
        double norm = 0.0;
        for (int r = 0; r < tw; ++r) {
            double prob = 0.0;
            double z = (double)(r - d);
            prob += c.z_hit * std::exp(-(z * z) / (2.0 * c.sigma_hit * c.sigma_hit)) / (c.sigma_hit * std::sqrt(2.0 * M_PI));
            if (r < d) prob += 2.0 * c.z_short * (d - r) / (double)d;
            if (r == P) prob += c.z_max;
            if (r < P) prob += c.z_rand * 1.0 / (double)P;
            norm += prob;
            t[(size_t)d * tw + r] = prob;
        }
        if (norm > 0)
            for (int r = 0; r < tw; ++r) t[(size_t)d * tw + r] /= norm;
    }
}

// Padded stop grid + skip-distance field.
// Padded cell (xp,yp), xp in [0,W], yp in [0,H], stands for reference cell (max(xp-1,0), max(yp-1,0)):
// the reference truncates toward zero (cpp:628-629), so pixel coordinates in (-1,0) read cell 0.
// Everything outside the padded grid is "stop" (map boundary, cpp:632-636).
//
// skip(c) = how far the fixed-step march may jump from a sample inside cell c without being able to
// land in a stop cell earlier.  Samples are exactly one pixel apart along the ray, so sample k+j lies at
// Euclidean distance j from sample k; it can be inside stop cell t only if j >= dist(p_k, t) >= gap(c, t),
// the distance between the two (closed) cell squares, with equality only for p_k on the boundary of c
// (such samples are caught by the kernel's boundary guard).  Hence skip(c) = floor(min_t gap(c,t)) + 1.
// gap^2(c,t) = max(|dx|-1,0)^2 + max(|dy|-1,0)^2 is the squared centre distance from c to the 3x3
// dilation of t, so one exact integer squared-EDT (Felzenszwalb & Huttenlocher lower envelopes) of the
// dilated stop set gives it.  Stop cells get 0; values are capped at 255.
static void edt_1d(const int64_t *f, int n, int64_t *d, int *v, double *z)
{
    const int64_t INF = (int64_t)1 << 40;
    int k = 0;
    v[0] = 0; z[0] = -1e30; z[1] = 1e30;
    for (int q = 1; q < n; ++q) {
        if (f[q] >= INF) continue;
        while (true) {
            if (f[v[k]] >= INF) { v[k] = q; z[k] = -1e30; z[k + 1] = 1e30; break; }
            double s = ((double)(f[q] + (int64_t)q * q) - (double)(f[v[k]] + (int64_t)v[k] * v[k])) / (2.0 * q - 2.0 * v[k]);
            if (s <= z[k]) { --k; if (k < 0) { k = 0; v[0] = q; z[0] = -1e30; z[1] = 1e30; break; } continue; }
            ++k; v[k] = q; z[k] = s; z[k + 1] = 1e30;
            break;
        }
    }
    k = 0;
    for (int q = 0; q < n; ++q) {
        while (z[k + 1] < q) ++k;
        int64_t dq = (int64_t)(q - v[k]);
        d[q] = (f[v[k]] >= INF) ? INF : dq * dq + f[v[k]];
    }
}

void build_distance_field(const int8_t *grid, int W, int H, int Wp, int Hp, int Wps, std::vector<uint8_t> &dist)
{
    // work grid = padded grid plus a one-cell stop border on every side
    const int Ww = Wp + 2, Hw = Hp + 2;
    std::vector<uint8_t> stop((size_t)Hw * Ww, 1), dil((size_t)Hw * Ww, 0);
    for (int yp = 0; yp < Hp; ++yp)
        for (int xp = 0; xp < Wp; ++xp) {
            int gx = std::max(xp - 1, 0), gy = std::max(yp - 1, 0);
            stop[(size_t)(yp + 1) * Ww + xp + 1] = grid[(size_t)gy * W + gx] > 50;
        }
    for (int y = 0; y < Hw; ++y)
        for (int x = 0; x < Ww; ++x) {
            if (!stop[(size_t)y * Ww + x]) continue;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    int yy = y + dy, xx = x + dx;
                    if (yy >= 0 && yy < Hw && xx >= 0 && xx < Ww) dil[(size_t)yy * Ww + xx] = 1;
                }
        }
    const int64_t INF = (int64_t)1 << 40;
    std::vector<int64_t> g((size_t)Hw * Ww);
    const int nmax = std::max(Ww, Hw);
    std::vector<int64_t> f(nmax), d(nmax);
    std::vector<int> v(nmax + 1);
    std::vector<double> z(nmax + 2);
    for (int x = 0; x < Ww; ++x) {            // columns
        for (int y = 0; y < Hw; ++y) f[y] = dil[(size_t)y * Ww + x] ? 0 : INF;
        edt_1d(f.data(), Hw, d.data(), v.data(), z.data());
        for (int y = 0; y < Hw; ++y) g[(size_t)y * Ww + x] = d[y];
    }
    dist.assign((size_t)Hp * Wps, 0);
    for (int y = 1; y <= Hp; ++y) {           // rows
        for (int x = 0; x < Ww; ++x) f[x] = g[(size_t)y * Ww + x];
        edt_1d(f.data(), Ww, d.data(), v.data(), z.data());
        for (int x = 1; x <= Wp; ++x) {
            int val = 0;
            if (!stop[(size_t)y * Ww + x]) {
                int64_t g2 = d[x];
                int64_t r = (int64_t)std::sqrt((double)g2);
                while (r * r > g2) --r;
                while ((r + 1) * (r + 1) <= g2) ++r;
                val = (int)std::min<int64_t>(r + 1, 255);
            }
            dist[(size_t)(y - 1) * Wps + (x - 1)] = (uint8_t)val;
        }
    }
}

// Directional skip field for k_rays_quad, quadrant q = (sx, sy): a ray whose direction has sign sx in x and sy
// in y can only ever enter cells t with sx*(t_x - c_x) >= 0 and sy*(t_y - c_y) >= 0, so only those stop cells
// bound the jump: skip_q(c) = floor(min over forward stop cells t of gap(c, t)) + 1, gap as in
// build_distance_field.  Walls beside or behind a ray no longer shorten its jumps (-30 % probes on the
// benchmark input).  Exact integer arithmetic: per row the forward x-gap h to the next stop, then per column
// a one-sided squared distance transform (lower envelope of parabolas, sources only ahead of the query).
void build_directional_field(const int8_t *grid, int W, int H, int Wp, int Hp, int Wps, int sx, int sy, std::vector<uint8_t> &dist)
{
    const int64_t INF = (int64_t)1 << 40;
    // stop(xf, yf) in "forward" coordinates: xf = sx > 0 ? xp : Wp-1-xp, same for y
    auto stop_at = [&](int xf, int yf) -> bool {
        int xp = sx > 0 ? xf : Wp - 1 - xf, yp = sy > 0 ? yf : Hp - 1 - yf;
        int gx = std::max(xp - 1, 0), gy = std::max(yp - 1, 0);
        return grid[(size_t)gy * W + gx] > 50;
    };
    // h[yf][xf]: gap in x to the nearest stop at x' >= xf in the same row (the cell just outside the grid is a stop)
    std::vector<int32_t> h((size_t)(Hp + 1) * Wp);
    for (int yf = 0; yf < Hp; ++yf) {
        int nxt = Wp;
        for (int xf = Wp - 1; xf >= 0; --xf) {
            if (stop_at(xf, yf)) nxt = xf;
            h[(size_t)yf * Wp + xf] = std::max(nxt - xf - 1, 0);
        }
    }
    for (int xf = 0; xf < Wp; ++xf) h[(size_t)Hp * Wp + xf] = 0;      // the row beyond the grid is all stop
    dist.assign((size_t)Hp * Wps, 0);
    std::vector<int> vp(Hp + 2);          // envelope: source positions (in r = decreasing-y order)
    std::vector<double> z(Hp + 3);
    std::vector<int64_t> hg(Hp + 2);      // heights of the sources
    for (int xf = 0; xf < Wp; ++xf) {
        // g2(yf) = min( h(yf)^2 , min over p >= yf of (p - yf)^2 + h(p+1)^2 ): sources p = Hp-1 .. 0 arrive in
        // decreasing p, i.e. increasing r = Hp-1-p; the query sits at the newest source's position.
        int k = -1;
        for (int yf = Hp - 1; yf >= 0; --yf) {
            const int r = Hp - 1 - yf;
            const int64_t hv = h[(size_t)(yf + 1) * Wp + xf];
            const int64_t fh = hv * hv;
            // insert parabola (r, fh)
            while (true) {
                if (k < 0) { k = 0; vp[0] = r; hg[0] = fh; z[0] = -1e30; z[1] = 1e30; break; }
                double sI = ((double)(fh + (int64_t)r * r) - (double)(hg[k] + (int64_t)vp[k] * vp[k])) / (2.0 * r - 2.0 * vp[k]);
                if (sI <= z[k]) { --k; continue; }
                ++k; vp[k] = r; hg[k] = fh; z[k] = sI; z[k + 1] = 1e30;
                break;
            }
            // query at r: the parabola whose interval contains r
            int kk = k;
            while (z[kk] > (double)r) --kk;
            int64_t dq = (int64_t)(r - vp[kk]);
            int64_t g2 = dq * dq + hg[kk];
            // exactness of the envelope near interval ends: also try the neighbours
            if (kk > 0) { int64_t d2 = (int64_t)(r - vp[kk - 1]); g2 = std::min(g2, d2 * d2 + hg[kk - 1]); }
            if (kk < k) { int64_t d2 = (int64_t)(r - vp[kk + 1]); g2 = std::min(g2, d2 * d2 + hg[kk + 1]); }
            const int64_t hs = h[(size_t)yf * Wp + xf];
            g2 = std::min(g2, hs * hs);
            int val = 0;
            if (!stop_at(xf, yf)) {
                int64_t rt = (int64_t)std::sqrt((double)g2);
                while (rt * rt > g2) --rt;
                while ((rt + 1) * (rt + 1) <= g2) ++rt;
                val = (int)std::min<int64_t>(rt + 1, 255);
            }
            int xp = sx > 0 ? xf : Wp - 1 - xf, yp = sy > 0 ? yf : Hp - 1 - yf;
            dist[(size_t)yp * Wps + xp] = (uint8_t)val;
        }
    }
    (void)INF; (void)H;
}

// Which cells of which table a changed stop cell can alter.  Grid cell (gx, gy) is padded cell (gx + 1, gy + 1),
// and grid row / column 0 also feeds padded row / column 0.  A skip value is min(floor(gap) + 1, 255): a stop cell changes it only
// where its gap is below 254, and gap >= |offset| - 1 per axis (isotropic: the dilated cell is one nearer, the centre distance
// one more), so the offsets that matter are at most kMapPatchReach per axis -- on every side for the isotropic field, on the side
// the rays come from for a quadrant field and the wedge fields of that quadrant.  The likelihood field is capped at K <= reach^2.
bool map_patch_plan(int W, int H, const int32_t b[4], int lf_reach, MapPatchPlan &p)
{
    if (W <= 0 || H <= 0 || b[2] < b[0] || b[3] < b[1] || b[2] < 0 || b[3] < 0 || b[0] >= W || b[1] >= H) return false;
    const int gx0 = std::max(b[0], 0), gy0 = std::max(b[1], 0), gx1 = std::min(b[2], W - 1), gy1 = std::min(b[3], H - 1);
    const int px0 = gx0 == 0 ? 0 : gx0 + 1, py0 = gy0 == 0 ? 0 : gy0 + 1, px1 = gx1 + 1, py1 = gy1 + 1;      // the padded stop cells
    const int R = kMapPatchReach;
    p.win[0] = std::max(px0 - R, 0); p.win[1] = std::max(py0 - R, 0); p.win[2] = std::min(px1 + R, W); p.win[3] = std::min(py1 + R, H);
    static const int qsx[4] = {1, -1, -1, 1}, qsy[4] = {1, 1, -1, -1};
    for (int q = 0; q < 4; ++q) {
        p.quad[q][0] = qsx[q] > 0 ? p.win[0] : px0; p.quad[q][2] = qsx[q] > 0 ? px1 : p.win[2];
        p.quad[q][1] = qsy[q] > 0 ? p.win[1] : py0; p.quad[q][3] = qsy[q] > 0 ? py1 : p.win[3];
    }
    if (lf_reach > 0) {
        p.lf[0] = (int32_t)std::max<int64_t>((int64_t)gx0 - lf_reach, 0); p.lf[1] = (int32_t)std::max<int64_t>((int64_t)gy0 - lf_reach, 0);
        p.lf[2] = (int32_t)std::min<int64_t>((int64_t)gx1 + lf_reach, W - 1); p.lf[3] = (int32_t)std::min<int64_t>((int64_t)gy1 + lf_reach, H - 1);
    } else {
        p.lf[0] = p.lf[1] = 0; p.lf[2] = p.lf[3] = -1;
    }
    return true;
}

// cpp:452-471
void motion_scalars(const double action[3], double &dt, double &v, double &w)
{
    dt = 0.01; v = 0.0; w = 0.0;
    double fd = action[0], ad = action[2];
    if (std::abs(fd) > 0.001) {
        if (std::abs(fd) < 0.1) dt = std::abs(fd) / 1.0;
        else dt = std::abs(fd) / 5.0;
        dt = std::max(0.001, std::min(dt, 0.1));
        v = fd / dt;
    }
    if (std::abs(ad) > 0.001) w = ad / dt;
}

// The 32-bit offset of a systematic resampling draw, one per update: word 0 of Philox-4x32-10 stream 3, counter (0, update_idx, 3, 0),
// key (seed_lo, seed_hi) -- the host's one restatement of philox4x32 (mcl_device_math.h).
uint32_t systematic_offset(uint32_t seed_lo, uint32_t seed_hi, uint32_t update_idx)
{
    uint32_t c0 = 0, c1 = update_idx, c2 = 3, c3 = 0, k0 = seed_lo, k1 = seed_hi;
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// ---- KLD-adaptive particle count (mcl_set_kld)
// why a KLD configuration is refused (null: it is not); cap > 0: the engine's max_particles
const char *kld_invalid(const mcl_kld_config_t *k, int64_t cap)
{
    if (!(k->min_particles >= 1 && k->min_particles <= k->max_particles)) return "KLD: need 1 <= min_particles <= max_particles";
    if (k->max_particles >= MCL_MAX_TOTAL_PARTICLES) return "KLD: max_particles must stay below 2^27";
    if (cap > 0 && k->max_particles > cap) return "KLD: max_particles exceeds the engine's max_particles";
    if (!(std::isfinite(k->err) && k->err > 0.0)) return "KLD: err must be finite and positive";
    if (!(std::isfinite(k->z) && k->z >= 0.0)) return "KLD: z must be finite and non-negative";
    if (!(std::isfinite(k->bin_x_m) && k->bin_x_m > 0.0 && std::isfinite(k->bin_y_m) && k->bin_y_m > 0.0))
        return "KLD: bin sizes must be finite and positive";
    if (k->n_theta_bins < 1) return "KLD: n_theta_bins must be >= 1";
    if (k->round_to < 1) return "KLD: round_to must be >= 1";
    if (k->shrink_permille < 0 || k->shrink_permille > 1000) return "KLD: shrink_permille must be in [0, 1000]";
    if (k->reserved != 0) return "KLD: reserved must be 0";
    return nullptr;
}

// the bin grid over a W x H map (false: more than 2^31 bits)
bool kld_grid(const mcl_kld_config_t *k, uint32_t W, uint32_t H, float res, int64_t &nx, int64_t &ny, uint64_t &bits)
{
    const double fx = std::ceil((double)W * (double)res / k->bin_x_m), fy = std::ceil((double)H * (double)res / k->bin_y_m);
    if (!(fx >= 1.0 && fy >= 1.0 && fx * fy * (double)k->n_theta_bins + 1.0 <= 2147483648.0)) return false;
    nx = (int64_t)fx; ny = (int64_t)fy;
    bits = (uint64_t)(nx * ny * k->n_theta_bins) + 1;
    return true;
}

mcl::KldArgs kld_args_of(const mcl_kld_config_t *k, int64_t nx, int64_t ny, double ox, double oy)
{
    mcl::KldArgs a{};
    a.ox = ox; a.oy = oy;
    a.inv_bx = 1.0 / k->bin_x_m; a.inv_by = 1.0 / k->bin_y_m;
    a.th_scale = (double)k->n_theta_bins / (2.0 * 3.14159265358979323846);
    a.nx = (uint32_t)nx; a.ny = (uint32_t)ny; a.nth = (uint32_t)k->n_theta_bins;
    a.nx_d = (double)nx; a.ny_d = (double)ny;
    a.nth_d = (double)k->n_theta_bins; a.inv_nth = 1.0 / (double)k->n_theta_bins;
    a.outside = (uint32_t)(nx * ny * k->n_theta_bins);
    return a;
}

int64_t kld_target(const mcl_kld_config_t *k, int64_t bins, int64_t n_current)
{
    int64_t target = k->max_particles;
    if (bins > 1) {
        const double km1 = (double)(bins - 1);
        const double a = 2.0 / (9.0 * km1);
        const double b = 1.0 - a + std::sqrt(a) * k->z;
        const double n = std::ceil(km1 / (2.0 * k->err) * (b * b * b));
        if (n < (double)k->max_particles) {            // (rounding up and clamping cannot go below max from there)
            const int64_t r = k->round_to, ni = n > 0.0 ? (int64_t)n : 0;
            target = std::min(std::max((ni + r - 1) / r * r, k->min_particles), k->max_particles);
        }
    }
    if (target <= n_current && target * 1000 >= n_current * (int64_t)k->shrink_permille) return n_current;
    return target;
}

int64_t compact_chunk_entries(int64_t longest)
{
    return std::max<int64_t>(64, (longest + 63) & ~(int64_t)63);
}

// ---- recovery by random-particle injection (mcl_set_recovery): host double throughout
const char *recov_invalid(const mcl_recovery_config_t *c)
{
    if (!(std::isfinite(c->alpha_slow) && std::isfinite(c->alpha_fast) && c->alpha_slow > 0.0 && c->alpha_slow < c->alpha_fast &&
          c->alpha_fast <= 1.0))
        return "recovery: need 0 < alpha_slow < alpha_fast <= 1";
    if (c->per_beam != 0 && c->per_beam != 1) return "recovery: per_beam must be 0 or 1";
    if (c->reserved != 0) return "recovery: reserved must be 0";
    return nullptr;
}

static double recov_logaddexp(double a, double b)
{
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    if (hi == -INFINITY) return -INFINITY;
    return hi + std::log1p(std::exp(lo - hi));
}

// l of one update: m + log(sum_w) - log(denom), -inf for m = -inf, divided by the beam count with per_beam
double recov_likelihood(const mcl_recovery_config_t &c, double max_logw, double sum_w, double denom, int n_beams)
{
    double l = max_logw == -INFINITY ? -INFINITY : max_logw + std::log(sum_w) - std::log(denom);
    if (c.per_beam) l = l / (double)n_beams;
    return l;
}

// folds l into (S, F) (NaN: unset); a NaN l changes nothing
void recov_fold(const mcl_recovery_config_t &c, double &S, double &F, double l)
{
    if (std::isnan(l)) return;
    S = std::isnan(S) ? l : recov_logaddexp(S + std::log1p(-c.alpha_slow), l + std::log(c.alpha_slow));
    F = std::isnan(F) ? l : recov_logaddexp(F + std::log1p(-c.alpha_fast), l + std::log(c.alpha_fast));
}

double recov_p(double S, double F)
{
    if (std::isnan(S) || std::isnan(F) || S == -INFINITY) return 0.0;
    const double p = 1.0 - std::exp(F - S);
    return p > 0.0 ? (p < 1.0 ? p : 1.0) : 0.0;
}

uint64_t recov_threshold(double p) { return (uint64_t)(p * 9007199254740992.0); }     // floor(p * 2^53), p in [0, 1]

// ---- likelihood-field sensor model (mcl_set_likelihood_field): the field on the device, the table in host double
const char *lf_invalid(const mcl_likelihood_field_config_t *c)
{
    const double z[2] = {c->z_hit, c->z_rand};
    for (double v : z)
        if (!std::isfinite(v) || v < 0.0) return "likelihood field: z_hit and z_rand must be finite and >= 0";
    if (z[0] == 0.0 && z[1] == 0.0) return "likelihood field: z_hit and z_rand are both 0";
    if (!(std::isfinite(c->sigma_hit_m) && c->sigma_hit_m > 0.0)) return "likelihood field: sigma_hit_m must be finite and > 0";
    if (!(std::isfinite(c->max_occ_dist_m) && c->max_occ_dist_m > 0.0)) return "likelihood field: max_occ_dist_m must be finite and > 0";
    if (c->reserved[0] != 0 || c->reserved[1] != 0) return "likelihood field: reserved must be 0";
    return nullptr;
}

// K = ceil((max_occ_dist / res)^2) (LF1), res the float resolution widened; -1 above 65535 (D is uint16)
int lf_cap(const mcl_likelihood_field_config_t *c, float resolution)
{
    const double q = c->max_occ_dist_m / (double)resolution;
    const double k = std::ceil(q * q);
    return k <= 65535.0 ? (int)k : -1;
}

// LF2: Lf[k] for 0 <= k < K, Lf[K] at the distance max_occ_dist_m; log(0) = -inf
void lf_table(const mcl_config_t &cfg, const mcl_likelihood_field_config_t &c, double res, int K, std::vector<float> &t)
{
    t.resize((size_t)K + 1);
    const double res2 = res * res, den = 2.0 * c.sigma_hit_m * c.sigma_hit_m, rnd = c.z_rand / cfg.max_range_m;
    const double inv_squash = 1.0 / cfg.squash_factor;
    for (int k = 0; k <= K; ++k) {
        const double e = k < K ? std::exp(-((double)k * res2) / den) : std::exp(-(c.max_occ_dist_m * c.max_occ_dist_m) / den);
        t[(size_t)k] = (float)(std::log(c.z_hit * e + rnd) * inv_squash);
    }
}

// ---- beam skipping (mcl_set_beam_skip): the integer thresholds of an update, formed once on the host
const char *bs_invalid(const mcl_beam_skip_config_t *c)
{
    if (!(std::isfinite(c->distance_m) && c->distance_m > 0.0)) return "beam skipping: distance_m must be finite and > 0";
    if (!(c->threshold >= 0.0 && c->threshold <= 1.0)) return "beam skipping: threshold must lie in [0, 1]";
    if (!(std::isfinite(c->error_threshold) && c->error_threshold >= 0.0)) return "beam skipping: error_threshold must be finite and >= 0";
    if (c->reserved[0] != 0 || c->reserved[1] != 0) return "beam skipping: reserved must be 0";
    return nullptr;
}

// BS1: Ka = ceil((distance_m / res)^2), K's expression; held at 65536 (every D is below it, the off-map sentinel is not)
int bs_ka(const mcl_beam_skip_config_t *c, float resolution)
{
    const double q = c->distance_m / (double)resolution;
    const double k = std::ceil(q * q);
    return k < 65536.0 ? (int)k : 65536;
}

// BS3: the least c in [1, n + 1] with (double)c / (double)n > threshold (c / n does not decrease with c, and (n + 1) / n > 1)
int64_t bs_min_count(double threshold, int64_t n)
{
    const double dn = (double)n;
    int64_t c = (int64_t)std::floor(threshold * dn);
    c = std::min(std::max<int64_t>(c, 1), n + 1);
    while (c <= n && !((double)c / dn > threshold)) ++c;
    while (c > 1 && (double)(c - 1) / dn > threshold) --c;
    return c;
}

// BS4: the least s >= 0 with (double)s >= error_threshold * (double)n_used, held at n_used + 1
int32_t bs_min_skipped(double error_threshold, int32_t n_used)
{
    const double x = error_threshold * (double)n_used;
    if (x > (double)n_used) return n_used + 1;
    int64_t s = (int64_t)std::ceil(x);
    while (s > 0 && (double)(s - 1) >= x) --s;
    while ((double)s < x) ++s;
    return (int32_t)std::min<int64_t>(s, (int64_t)n_used + 1);
}

// LF1 on the host: exact squared distances from the lower envelopes of edt_1d (columns, then rows), clamped to K
static void lf_field_host(const int8_t *grid, int W, int H, int K, uint16_t *out)
{
    const int64_t INF = (int64_t)1 << 40;
    const int n = std::max(W, H);
    std::vector<int64_t> f((size_t)n), d((size_t)n), col((size_t)W * H);
    std::vector<int> v((size_t)n);
    std::vector<double> z((size_t)n + 1);
    for (int x = 0; x < W; ++x) {
        for (int y = 0; y < H; ++y) f[(size_t)y] = grid[(size_t)y * W + x] > 50 ? 0 : INF;
        edt_1d(f.data(), H, d.data(), v.data(), z.data());
        for (int y = 0; y < H; ++y) col[(size_t)y * W + x] = d[(size_t)y];
    }
    for (int y = 0; y < H; ++y) {
        edt_1d(col.data() + (size_t)y * W, W, d.data(), v.data(), z.data());
        for (int x = 0; x < W; ++x) out[(size_t)y * W + x] = (uint16_t)std::min<int64_t>(d[(size_t)x], K);
    }
}

// ---- sensor mount (mcl_set_sensor_mount): SM1
bool mount_valid(const double mount[3])
{
    return std::isfinite(mount[0]) && std::isfinite(mount[1]) && std::isfinite(mount[2]) && std::fabs(mount[2]) <= 2.0 * M_PI;
}

// ---- per-beam sensor offsets (mcl_set_beam_offsets): DS1
void deskew_table(const float *angles, const double *offsets_colmajor, int32_t n_beams, float *effective_angles, double2 *cs)
{
    for (int32_t j = 0; j < n_beams; ++j) {
        const float af = (float)((double)angles[j] + offsets_colmajor[2 * (size_t)n_beams + j]);
        const double a = (double)af;                                   // cpp:533 widens the float angle
        if (effective_angles) effective_angles[j] = af;
        if (cs) cs[j] = make_double2(std::cos(a), std::sin(a));
    }
}

// ---- odometry motion models and the Gaussian pose initialisation (the header's M1-M6 / G1) ----
const char *motion_invalid(const mcl_motion_config_t *c)
{
    if (c->model != MCL_MOTION_REFERENCE && c->model != MCL_MOTION_DIFF && c->model != MCL_MOTION_OMNI) return "motion model: unknown model";
    if (c->reserved != 0) return "motion model: reserved must be 0";
    const double v[7] = {c->alpha1, c->alpha2, c->alpha3, c->alpha4, c->alpha5, c->floor_trans_m, c->floor_rot_rad};
    for (double e : v)
        if (!std::isfinite(e) || e < 0.0) return "motion model: the alphas and floors must be finite and >= 0";
    return nullptr;
}

static double odo_norm(double z) { return std::atan2(std::sin(z), std::cos(z)); }
static double odo_adiff(double a, double b)
{
    const double PI = 3.14159265358979323846;
    a = odo_norm(a); b = odo_norm(b);
    const double d1 = a - b;
    double d2 = 2.0 * PI - std::fabs(d1);
    if (d1 > 0.0) d2 = -d2;
    return std::fabs(d1) < std::fabs(d2) ? d1 : d2;
}

// mcl_device_math.h's normalize_angle on the host
static double host_normalize_angle(double a)
{
    const double PI = 3.14159265358979323846;
    int it = 0;
    while (a > PI && it < 64) { a -= 2.0 * PI; ++it; }
    while (a < -PI && it < 128) { a += 2.0 * PI; ++it; }
    if (it >= 64 && (a > PI || a < -PI)) a = std::remainder(a, 2.0 * PI);
    return a;
}

// ---- the global search (mcl_global_search): its config check, lattice (S1) and headings (S2)
const char *search_invalid(const mcl_search_config_t *c)
{
    if (c->stride_cells < 1) return "global search: stride_cells must be >= 1";
    if (c->n_headings < 1) return "global search: n_headings must be >= 1";
    if (c->beam_stride < 1) return "global search: beam_stride must be >= 1";
    if (c->nms != 0 && c->nms != 1) return "global search: nms must be 0 or 1";
    for (int i = 0; i < 4; ++i)
        if (c->reserved[i] != 0) return "global search: reserved must be 0";
    return nullptr;
}

int64_t search_lattice(int stride, const int8_t *data, int W, int H, double res, double ox, double oy, std::vector<uint32_t> *cells,
                       std::vector<double> *xy, std::vector<int32_t> *lat, std::vector<int32_t> *pmap, int &nx, int &ny)
{
    const int64_t h0 = stride / 2;
    nx = h0 < W ? (int)(((int64_t)W - 1 - h0) / stride + 1) : 0;       // columns h0 + ix * stride < W
    ny = h0 < H ? (int)(((int64_t)H - 1 - h0) / stride + 1) : 0;
    if (pmap) pmap->assign((size_t)nx * (size_t)ny, -1);
    int64_t np = 0;
    for (int iy = 0; iy < ny; ++iy) {
        const int64_t row = h0 + (int64_t)iy * stride;
        for (int ix = 0; ix < nx; ++ix) {
            const int64_t col = h0 + (int64_t)ix * stride;
            if (data[(size_t)row * (size_t)W + (size_t)col] != 0) continue;         // the free rule of mcl_init_global
            if (cells) cells->push_back((uint32_t)(row * W + col));
            if (xy) {
                xy->push_back(ox + ((double)col + 0.5) * res);       // the cell centre; the multiply and the add each rounded
                xy->push_back(oy + ((double)row + 0.5) * res);
            }
            if (lat) { lat->push_back(ix); lat->push_back(iy); }
            if (pmap) (*pmap)[(size_t)iy * (size_t)nx + (size_t)ix] = (int32_t)np;
            ++np;
        }
    }
    return np;
}

void search_headings(int n_headings, double *theta)
{
    const double step = 3.14159265358979323846 / (double)n_headings;     // formed once
    for (int64_t k = 0; k < n_headings; ++k) theta[k] = (double)(2 * k - (int64_t)n_headings) * step;
}

// ---- the search under the beam model (mcl_global_search_beam): the angle grid of B1 and the tiles of B5
std::string search_beam_grid(const float *angles, int n_beams, int n_headings, SearchBeamGrid &g)
{
    constexpr double kTwoPi = 6.283185307179586, kPi = 3.141592653589793;
    g = SearchBeamGrid{};
    if (!angles || n_beams < 1) return "beam search: no beam angles";
    if (n_headings < 1) return "beam search: n_headings must be >= 1";
    const int64_t B = n_beams;
    const double a0 = (double)angles[0];
    int64_t M = n_headings;                                              // one beam: the headings are the grid
    if (B >= 2) {
        const double inc = ((double)angles[B - 1] - a0) / (double)(B - 1);
        if (!(inc > 0.0)) return "beam search: the beam angles must ascend (increment (a_last - a_first) / (B - 1) > 0)";
        const double turns = kTwoPi / inc;
        if (!(turns < 16384.5)) return "beam search: the angle grid M = round(2 pi / increment) must be at most 16384";
        M = std::llround(turns);
    }
    if (M > 16384) return "beam search: the angle grid M = round(2 pi / increment) must be at most 16384";
    g.M = (int32_t)M;
    g.delta = kTwoPi / (double)M;
    g.phi0 = a0 - kPi;
    double worst = 0.0;
    bool finite = true;
    for (int64_t j = 0; j < B; ++j) {
        const double dev = std::fabs((double)angles[j] - (a0 + (double)j * g.delta));
        if (!(dev == dev)) finite = false;
        else if (dev > worst) worst = dev;
    }
    g.max_dev = finite ? worst : std::nan("");
    if (B > M) return "beam search: more beams than grid angles (B <= M = round(2 pi / increment): the scan spans more than a turn)";
    if (M % n_headings != 0) return "beam search: n_headings must divide the angle grid M = " + std::to_string(M);
    g.heading_step = (int32_t)(M / n_headings);
    if (!finite || !(worst <= 4e-6)) return "beam search: the beam angles are not evenly spaced on the grid of 2 pi / M (a deviation above 4e-6 rad)";
    return std::string();
}

void search_beam_angles(const SearchBeamGrid &g, double *phi)
{
    for (int64_t m = 0; m < g.M; ++m) phi[m] = g.phi0 + (double)m * g.delta;
}

std::string search_beam_tiles(int64_t n_positions, int32_t M, int32_t max_range_px, uint64_t budget_bytes, SearchBeamTiles &t)
{
    t = SearchBeamTiles{};
    if (n_positions < 1 || n_positions >= MCL_MAX_TOTAL_PARTICLES || M < 1 || M > 16384 || max_range_px < 1 || max_range_px > 65535)
        return "beam search: no tile plan for these sizes";
    t.entry_bytes = max_range_px <= 255 ? 1 : 2;
    const uint64_t budget = budget_bytes ? budget_bytes : kSearchBeamDefaultBudget;
    const uint64_t per_position = (uint64_t)M * (uint64_t)t.entry_bytes;
    uint64_t T = budget / per_position / 256 * 256;
    if (T < 256)
        return "beam search: table_budget_bytes holds fewer than 256 positions' rays (" + std::to_string(256 * per_position) + " bytes needed)";
    T = std::min<uint64_t>(T, ((uint64_t)n_positions + 255) / 256 * 256);       // no larger than the lattice
    T = std::min<uint64_t>(T, (1ull << 31) / (uint64_t)M / 256 * 256);         // a tile's ray index stays below 2^31
    t.T = (int64_t)T;
    t.tiles = (n_positions + t.T - 1) / t.T;
    return std::string();
}

// ---- the search over a scan sequence (mcl_global_search_sequence): what it refuses of rel, and SQ1
const char *search_sequence_invalid(const double *rel, int n_scans)
{
    static_assert(MCL_SEARCH_MAX_SCANS == 16, "the message below names the limit");
    if (n_scans < 1 || n_scans > MCL_SEARCH_MAX_SCANS) return "global search: n_scans must be in [1, 16] (MCL_SEARCH_MAX_SCANS)";
    if (!rel) return "global search: rel is null";
    for (int i = 0; i < 3 * n_scans; ++i)
        if (!std::isfinite(rel[i])) return "global search: rel has an entry that is not finite";
    return nullptr;
}

void search_sequence_offsets(int n_headings, const double *theta, const double *rel, int n_scans, double *out)
{
    for (int k = 0; k < n_headings; ++k) {
        const double ck = std::cos(theta[k]), sk = std::sin(theta[k]);
        for (int s = 0; s < n_scans; ++s) {
            const double dx = rel[3 * s], dy = rel[3 * s + 1];
            double *o = out + ((size_t)k * (size_t)n_scans + (size_t)s) * 3;
            o[0] = ck * dx - sk * dy;                  // each product rounded, then the difference (contraction is off)
            o[1] = sk * dx + ck * dy;
            o[2] = theta[k] + rel[3 * s + 2];
        }
    }
}

// ---- the streamed search (mcl_global_search_streamed): the plan of ST2 / ST4 / ST5
SearchSlabPlan search_slab_bytes(int64_t n_positions, int32_t G)
{
    SearchSlabPlan p;
    const uint64_t np = (uint64_t)n_positions;
    p.G = G;
    p.slab_poses = (uint64_t)G * np;
    p.ring_bytes = ((uint64_t)G + 2) * np * sizeof(double);             // the ring of G + 2 score planes
    p.flag_bytes = p.slab_poses * sizeof(uint32_t);                     // the slab's flags,
    p.pos_bytes = p.slab_poses * sizeof(uint32_t);                      // their scan,
    p.key_bytes = p.slab_poses * sizeof(uint64_t);                      // the slab's keys
    p.list_entries = kSearchListHits + p.slab_poses;                    // the running list, behind it the slab's candidates:
    p.list_bytes = 2 * p.list_entries * 2 * sizeof(uint64_t);           //   (key, index), twice (the sort goes from one to the other)
    p.scratch_bytes = (256u << 10) + (p.slab_poses >> 4);               // what the scan and the sort may ask for
    p.bytes = p.ring_bytes + p.flag_bytes + p.pos_bytes + p.key_bytes + p.list_bytes + p.scratch_bytes;
    return p;
}

std::string search_slabs(const mcl_search_config_t *c, const mcl_search_stream_config_t *sc, int64_t n_positions, int32_t n_scans,
                         SearchSlabPlan &plan)
{
    if (const char *why = search_invalid(c)) return why;
    for (int i = 0; i < 5; ++i)
        if (sc->reserved[i] != 0) return "streamed search: reserved must be 0";
    if (sc->slab_headings < 0) return "streamed search: slab_headings must be >= 0";
    if (n_scans < 1 || n_scans > MCL_SEARCH_MAX_SCANS) return "global search: n_scans must be in [1, 16] (MCL_SEARCH_MAX_SCANS)";
    if (n_positions < 1) return "streamed search: n_positions must be >= 1";
    const int64_t n = c->n_headings;
    if (n_positions >= MCL_MAX_TOTAL_PARTICLES || n_positions * n >= ((int64_t)1 << 40))
        return "streamed search: n_positions * n_headings must stay below 2^40 (and n_positions below 2^27)";
    const uint64_t budget = sc->budget_bytes ? sc->budget_bytes : kSearchStreamDefaultBudget;
    const auto st4 = [&](int64_t G) { return (G + 2) * n_positions < MCL_MAX_TOTAL_PARTICLES; };
    const auto fits = [&](int64_t G) { return st4(G) && search_slab_bytes(n_positions, (int32_t)G).bytes <= budget; };
    int64_t G = std::min<int64_t>(sc->slab_headings, n);                // a G above n_headings is n_headings: one slab
    if (G > 0) {
        if (!st4(G)) return "streamed search: (slab_headings + 2) * n_positions must stay below 2^27 (fewer headings per slab)";
    } else if (fits(1)) {
        int64_t lo = 1, hi = n;                                         // the largest G in [1, n] that fits: both bounds are monotone
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo + 1) / 2;
            if (fits(mid)) lo = mid; else hi = mid - 1;
        }
        G = lo;
    } else {
        G = 1;
        if (!st4(G)) return "streamed search: 3 * n_positions must stay below 2^27 (a larger stride_cells)";
    }
    const SearchSlabPlan p = search_slab_bytes(n_positions, (int32_t)G);
    if (p.bytes > budget)
        return "streamed search: slabs of " + std::to_string(G) + " heading" + (G > 1 ? "s" : "") + " need " + std::to_string(p.bytes) +
               " bytes, the budget is " + std::to_string(budget) + " bytes";
    plan = p;
    plan.n_slabs = (int32_t)((n + G - 1) / G);
    return std::string();
}

// ---- the search with exact pruning (mcl_global_search_pruned): the blocks of P1, the pooled field and the bound
// table of P2, the rounds of P4
const char *search_prune_invalid(const mcl_search_config_t *c, const mcl_search_prune_config_t *pc)
{
    if (pc->block != 2 && pc->block != 4 && pc->block != 8) return "pruned search: block must be 2, 4 or 8";
    if (pc->first_pairs < 0) return "pruned search: first_pairs must be >= 0";
    for (int i = 0; i < 6; ++i)
        if (pc->reserved[i] != 0) return "pruned search: reserved must be 0";
    if ((int64_t)(pc->block - 1) * (int64_t)c->stride_cells + 2 > 65536) return "pruned search: the window (block - 1) * stride_cells + 2 must be at most 65536 cells";
    return nullptr;
}

void search_blocks(int S, int stride, const int32_t *pmap, int nx, int ny, SearchBlocks &out)
{
    out = SearchBlocks{};
    out.S = S;
    out.w = (S - 1) * stride + 2;
    out.nbx = (nx + S - 1) / S;
    out.nby = (ny + S - 1) / S;
    out.bmap.assign((size_t)out.nbx * (size_t)out.nby, -1);
    for (int by = 0; by < out.nby; ++by)
        for (int bx = 0; bx < out.nbx; ++bx) {
            int32_t held = 0;
            for (int iy = by * S; iy < std::min(ny, by * S + S); ++iy)
                for (int ix = bx * S; ix < std::min(nx, bx * S + S); ++ix)
                    if (pmap[(size_t)iy * (size_t)nx + (size_t)ix] >= 0) ++held;
            if (!held) continue;
            out.bmap[(size_t)by * (size_t)out.nbx + (size_t)bx] = out.n_blocks++;
            out.blk.push_back(bx); out.blk.push_back(by); out.blk.push_back(held);
        }
}

// rows, then columns, as the device's two passes
void lf_pool(const uint16_t *D, int W, int H, int K, int w, uint16_t *out)
{
    const int Wp = W + w - 1, Hp = H + w - 1;
    std::vector<uint16_t> R((size_t)Wp * (size_t)H);
    for (int y = 0; y < H; ++y)
        for (int xs = 0; xs < Wp; ++xs) {
            int best = K;
            for (int x = std::max(0, xs - (w - 1)); x <= std::min(W - 1, xs); ++x) best = std::min(best, (int)D[(size_t)y * W + x]);
            R[(size_t)y * Wp + xs] = (uint16_t)best;
        }
    for (int ys = 0; ys < Hp; ++ys)
        for (int xs = 0; xs < Wp; ++xs) {
            int best = K;
            for (int y = std::max(0, ys - (w - 1)); y <= std::min(H - 1, ys); ++y) best = std::min(best, (int)R[(size_t)y * Wp + xs]);
            out[(size_t)ys * Wp + xs] = (uint16_t)best;
        }
}

void search_bound_table(const float *lf, int K, float *ub)
{
    float m = lf[K];
    for (int k = K; k >= 0; --k) {
        if (lf[k] > m) m = lf[k];
        ub[k] = m;
    }
}

int64_t search_prune_next(const mcl_search_prune_config_t &pc, int64_t pairs, int64_t n_scored, int64_t first_below_c)
{
    if (n_scored <= 0) {
        const int64_t first = pc.first_pairs > 0 ? (int64_t)pc.first_pairs : std::max<int64_t>(1024, pairs / 64);
        return std::min(first, pairs);
    }
    const int64_t twice = n_scored > pairs / 2 ? pairs : std::min(2 * n_scored, pairs);
    return std::max(std::min(first_below_c, pairs), twice);
}

// ---- the pose refinement (mcl_refine_poses): its config check (R7)
const char *refine_invalid(const mcl_refine_config_t *c)
{
    if (c->half_xy < 0 || c->half_theta < 0) return "refine: half_xy and half_theta must be >= 0";
    if (!(std::isfinite(c->step_xy_cells) && c->step_xy_cells > 0.0)) return "refine: step_xy_cells must be finite and > 0";
    if (!(std::isfinite(c->step_theta_rad) && c->step_theta_rad > 0.0)) return "refine: step_theta_rad must be finite and > 0";
    if (c->beam_stride < 1) return "refine: beam_stride must be >= 1";
    for (int i = 0; i < 3; ++i)
        if (c->reserved[i] != 0) return "refine: reserved must be 0";
    // n_win = (2 half_xy + 1)^2 (2 half_theta + 1) <= 32768, without overflow
    if (c->half_xy > 90 || c->half_theta > 16383) return "refine: the window must have at most 32768 poses";
    const int64_t nx = 2 * (int64_t)c->half_xy + 1, nt = 2 * (int64_t)c->half_theta + 1;
    if (nx * nx * nt > mcl_rf::kMaxWindow) return "refine: the window must have at most 32768 poses";
    return nullptr;
}

// ---- the refinement over a scan sequence (mcl_refine_poses_sequence): what RS7 refuses of rel and of the
// table's size, and RS1
const char *refine_sequence_invalid(const double *rel, int n_scans)
{
    static_assert(MCL_SEARCH_MAX_SCANS == 16, "the message below names the limit");
    if (n_scans < 1 || n_scans > MCL_SEARCH_MAX_SCANS) return "refine: n_scans must be in [1, 16] (MCL_SEARCH_MAX_SCANS)";
    if (!rel) return "refine: rel is null";
    for (int i = 0; i < 3 * n_scans; ++i)
        if (!std::isfinite(rel[i])) return "refine: rel has an entry that is not finite";
    return nullptr;
}

std::string refine_sequence_rows_refused(int64_t M, int64_t nt, int64_t S)
{
    if (M * nt * S <= (int64_t)MCL_REFINE_SEQ_MAX_ROWS) return std::string();
    return "refine: the offset table would have " + std::to_string(M * nt * S) + " rows (" + std::to_string(M) + " seeds x " +
           std::to_string(nt) + " window headings x " + std::to_string(S) + " scans), more than MCL_REFINE_SEQ_MAX_ROWS = " +
           std::to_string((int64_t)MCL_REFINE_SEQ_MAX_ROWS);
}

void refine_sequence_offsets(int32_t half_theta, double step_theta, const double *seeds_colmajor, int32_t M, const double *rel, int n_scans,
                             double *out)
{
    const int32_t nt = 2 * half_theta + 1;
    for (int32_t m = 0; m < M; ++m)
        for (int32_t it = 0; it < nt; ++it) {
            const double th = mcl_rf::coord(seeds_colmajor[(size_t)2 * (size_t)M + (size_t)m], it - half_theta, step_theta);     // R1's heading
            const double c = std::cos(th), s = std::sin(th);
            double *o = out + ((size_t)m * (size_t)nt + (size_t)it) * (size_t)n_scans * 3;
            for (int sc = 0; sc < n_scans; ++sc, o += 3) {
                const double dx = rel[3 * sc], dy = rel[3 * sc + 1];
                o[0] = c * dx - s * dy;                    // each product rounded, then the difference (contraction is off)
                o[1] = s * dx + c * dy;
                o[2] = th + rel[3 * sc + 2];
            }
        }
}

// G1: the lower Cholesky factor of a symmetric positive semi-definite 3 x 3 matrix (row-major), L = {L00, L10, L11, L20, L21, L22}
const char *gaussian_factor(const double cov[9], double L[6])
{
    double amax = 0.0, dmax = 0.0;
    for (int i = 0; i < 9; ++i) {
        if (!std::isfinite(cov[i])) return "gaussian init: the covariance must be finite";
        amax = std::max(amax, std::fabs(cov[i]));
    }
    for (int i = 0; i < 3; ++i) {
        dmax = std::max(dmax, cov[4 * i]);
        for (int j = 0; j < i; ++j)
            if (std::fabs(cov[3 * i + j] - cov[3 * j + i]) > 1e-12 * amax) return "gaussian init: the covariance must be symmetric";
    }
    const double tol = 1e-12 * dmax;
    double l[3][3] = {};
    for (int j = 0; j < 3; ++j) {
        double p = cov[4 * j];
        for (int k = 0; k < j; ++k) p -= l[j][k] * l[j][k];
        if (std::fabs(p) <= tol) continue;               // a zero pivot: the column stays zero
        if (p < 0.0) return "gaussian init: the covariance must be positive semi-definite";
        l[j][j] = std::sqrt(p);
        for (int i = j + 1; i < 3; ++i) {
            double v = cov[3 * i + j];
            for (int k = 0; k < j; ++k) v -= l[i][k] * l[j][k];
            l[i][j] = v / l[j][j];
        }
    }
    L[0] = l[0][0]; L[1] = l[1][0]; L[2] = l[1][1]; L[3] = l[2][0]; L[4] = l[2][1]; L[5] = l[2][2];
    return nullptr;
}

// P1 / P2 of mcl_set_recovery_proposal: every component checked (its covariance by G1's own function), then the thresholds
// t_k = floor((s_k / s_M) 2^53) of the in-order prefix sums, the last one 2^53.  Nothing is written unless everything is fine.
std::string recov_proposal(int32_t M, const double *means, const double *covs, const double *weights, uint64_t *thresholds, double *factors)
{
    if (M < 1 || M > kRecovProposalMax) return "recovery proposal: n_components must be in [1, 4096]";
    if (!means || !covs) return "recovery proposal: null means or covariances";
    double total = 0.0;
    for (int32_t c = 0; c < M; ++c) {
        const std::string who = "recovery proposal, component " + std::to_string(c) + ": ";
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(means[3 * (size_t)c + k])) return who + "the mean must be finite";
        double L[6];
        if (const char *why = gaussian_factor(covs + 9 * (size_t)c, L)) return who + why;
        const double w = weights ? weights[c] : 1.0;
        if (!std::isfinite(w) || w < 0.0) return who + "the weight must be finite and >= 0";
        total += w;
    }
    if (!std::isfinite(total) || !(total > 0.0)) return "recovery proposal: the sum of the weights must be finite and > 0";
    double s = 0.0;
    for (int32_t c = 0; c < M; ++c) {
        s += weights ? weights[c] : 1.0;
        if (thresholds) thresholds[c] = c == M - 1 ? (1ull << 53) : (uint64_t)std::floor((s / total) * 9007199254740992.0);
        if (factors) {
            double *f = factors + 9 * (size_t)c;
            for (int k = 0; k < 3; ++k) f[k] = means[3 * (size_t)c + k];
            (void)gaussian_factor(covs + 9 * (size_t)c, f + 3);
        }
    }
    return std::string();
}

}  // namespace mcl_host

using namespace mcl_host;

extern "C" {

void mcl_default_config(mcl_config_t *c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->max_particles = 2000;       // cpp:24, yaml:6
    c->device = 0;
    c->seed = 0;
    c->max_range_m = 12.0;         // cpp:27
    c->z_hit = 0.80; c->z_short = 0.01; c->z_max = 0.07; c->z_rand = 0.12; c->sigma_hit = 8.0;   // cpp:30-34
    c->squash_factor = 2.2;        // cpp:26
    c->motion_dispersion_x = 0.05; c->motion_dispersion_y = 0.025; c->motion_dispersion_theta = 0.25;   // cpp:35-37
    c->resample_mode = MCL_RESAMPLE_MULTINOMIAL;
    c->weight_mode = MCL_WEIGHT_LOG;
    c->ray_kernel = MCL_RAYS_AUTO;
}

int mcl_host_sensor_table(const mcl_config_t *cfg, int32_t P, double *out, size_t n)
{
    if (!cfg || !out || P < 1 || n != (size_t)(P + 1) * (P + 1) || bad_sensor_fields(*cfg)) return MCL_ERR_INVALID_ARG;
    std::vector<double> t;
    build_sensor_table(*cfg, P, t);
    std::memcpy(out, t.data(), n * sizeof(double));
    return MCL_OK;
}

int mcl_host_skip_field_dir(const int8_t *data, uint32_t width, uint32_t height, int32_t quadrant, uint8_t *out, size_t n)
{
    if (!data || !out || width == 0 || height == 0 || quadrant < 0 || quadrant > 3 || n != (size_t)(width + 1) * (height + 1))
        return MCL_ERR_INVALID_ARG;
    static const int qsx[4] = {1, -1, -1, 1}, qsy[4] = {1, 1, -1, -1};
    const int Wp = (int)width + 1, Hp = (int)height + 1, Wps = (Wp + 7) & ~7;
    std::vector<uint8_t> d;
    build_directional_field(data, (int)width, (int)height, Wp, Hp, Wps, qsx[quadrant], qsy[quadrant], d);
    for (int y = 0; y < Hp; ++y) std::memcpy(out + (size_t)y * Wp, d.data() + (size_t)y * Wps, Wp);
    return MCL_OK;
}

static int host_wedge_field(const int8_t *data, uint32_t width, uint32_t height, int32_t wedge, uint8_t *out, size_t n, bool tight);

int mcl_host_skip_field_wedge(const int8_t *data, uint32_t width, uint32_t height, int32_t wedge, uint8_t *out, size_t n)
{
    return host_wedge_field(data, width, height, wedge, out, n, false);
}

int mcl_host_skip_field_wedge_tight(const int8_t *data, uint32_t width, uint32_t height, int32_t wedge, uint8_t *out, size_t n)
{
    return host_wedge_field(data, width, height, wedge, out, n, true);
}

int mcl_host_wedge_tight_table(int32_t wedge, int32_t *values, uint8_t *reachable, size_t n)
{
    const int S = 2 * mcl::kWedgeR + 1;
    if (wedge < 0 || wedge >= mcl::kWedges || !values || !reachable || n != (size_t)S * S) return MCL_ERR_INVALID_ARG;
    std::vector<mcl::WedgeRow> rows(S);
    mcl::wedge_rows(wedge, rows.data());
    const mcl::WedgeCone cone = mcl::wedge_cone(wedge);
    for (int oy = -mcl::kWedgeR; oy <= mcl::kWedgeR; ++oy)
        for (int ox = -mcl::kWedgeR; ox <= mcl::kWedgeR; ++ox) {
            const size_t i = (size_t)(oy + mcl::kWedgeR) * S + (size_t)(ox + mcl::kWedgeR);
            const mcl::WedgeRow r = rows[oy + mcl::kWedgeR];
            reachable[i] = (ox >= r.xa && ox <= r.xb) ? 1 : 0;
            values[i] = mcl::wedge_tight_value(cone, ox, oy);
        }
    return MCL_OK;
}

static int host_wedge_field(const int8_t *data, uint32_t width, uint32_t height, int32_t wedge, uint8_t *out, size_t n, bool tight)
{
    if (!data || !out || width == 0 || height == 0 || wedge < 0 || wedge >= mcl::kWedges || n != (size_t)(width + 1) * (height + 1))
        return MCL_ERR_INVALID_ARG;
    const int W = (int)width, H = (int)height, Wp = W + 1, Hp = H + 1;
    std::vector<int32_t> nxt((size_t)Wp * Hp), prv((size_t)Wp * Hp);
    for (int y = 0; y < Hp; ++y) {
        auto stop = [&](int x) { return data[(size_t)std::max(y - 1, 0) * W + std::max(x - 1, 0)] > 50; };
        int last = -1;
        for (int x = 0; x < Wp; ++x) { if (stop(x)) last = x; prv[(size_t)y * Wp + x] = last; }
        int next = Wp;
        for (int x = Wp - 1; x >= 0; --x) { if (stop(x)) next = x; nxt[(size_t)y * Wp + x] = next; }
    }
    std::vector<mcl::WedgeRow> rows(2 * mcl::kWedgeR + 1);
    mcl::wedge_rows(wedge, rows.data());
    const mcl::WedgeCone cone = mcl::wedge_cone(wedge);
    for (int y = 0; y < Hp; ++y)
        for (int x = 0; x < Wp; ++x)
            out[(size_t)y * Wp + x] = (uint8_t)(tight ? mcl::wedge_skip_cell_tight(nxt.data(), prv.data(), Wp, Hp, x, y, rows.data(), cone)
                                                      : mcl::wedge_skip_cell(nxt.data(), prv.data(), Wp, Hp, x, y, rows.data()));
    return MCL_OK;
}

int mcl_host_skip_field(const int8_t *data, uint32_t width, uint32_t height, uint8_t *out, size_t n)
{
    if (!data || !out || width == 0 || height == 0 || n != (size_t)(width + 1) * (height + 1)) return MCL_ERR_INVALID_ARG;
    const int Wp = (int)width + 1, Hp = (int)height + 1, Wps = (Wp + 7) & ~7;
    std::vector<uint8_t> d;
    build_distance_field(data, (int)width, (int)height, Wp, Hp, Wps, d);
    for (int y = 0; y < Hp; ++y) std::memcpy(out + (size_t)y * Wp, d.data() + (size_t)y * Wps, Wp);
    return MCL_OK;
}

int mcl_host_sweep_global_layout(uint32_t width, uint32_t height, int32_t max_range_px, int64_t out[6])
{
    if (!out || width == 0 || height == 0 || max_range_px < 1) return MCL_ERR_INVALID_ARG;
    const int Wp = (int)width + 1, Hp = (int)height + 1;
    const mcl::SweepGlobalLayout g = mcl::sweep_global_layout(Wp, Hp, max_range_px);
    out[0] = g.ok ? 1 : 0; out[1] = g.pitch; out[2] = g.rows; out[3] = (int64_t)g.stride; out[4] = (int64_t)g.alloc;
    out[5] = (int64_t)mcl::sweep_global_max_offset(g, Wp, Hp, max_range_px, mcl::kWedges - 1);
    return MCL_OK;
}

int mcl_host_map_patch_plan(uint32_t map_w, uint32_t map_h, const int32_t stop_bbox[4], int32_t lf_reach, int32_t window[4], int32_t lf_window[4])
{
    if (!stop_bbox || !window || !lf_window || map_w == 0 || map_h == 0 || map_w > 200000 || map_h > 200000) return MCL_ERR_INVALID_ARG;
    MapPatchPlan p;
    if (!map_patch_plan((int)map_w, (int)map_h, stop_bbox, lf_reach, p)) return MCL_ERR_INVALID_ARG;
    std::memcpy(window, p.win, sizeof(p.win));
    std::memcpy(lf_window, p.lf, sizeof(p.lf));
    return MCL_OK;
}

int mcl_host_sort_key(const int32_t bbox[7], const int32_t *tilemap, int32_t ntx_abs, uint32_t width, uint32_t height,
                      const double *px, const double *py, const double *theta, int64_t n, int64_t n_layout, int32_t fine, uint32_t *keys)
{
    if (!bbox || !px || !py || !theta || !keys || n < 0 || n_layout < 0 || width == 0 || height == 0 || fine < 0 || (fine & 15) > mcl::kSortMaxFine || fine >= 8 << 4)
        return MCL_ERR_INVALID_ARG;
    const int Wp = (int)width + 1, Hp = (int)height + 1;
    const int hx = Wp * mcl::kSortSub - 1, hy = Hp * mcl::kSortSub - 1;
    // a box inside the padded grid (an empty one holds no particle to key), and with numbered tiles a map for every tile of it
    if (bbox[0] < 0 || bbox[1] < 0 || bbox[2] > hx || bbox[3] > hy || bbox[0] > bbox[2] || bbox[1] > bbox[3]) return MCL_ERR_INVALID_ARG;
    if (bbox[5] != 0 && (!tilemap || ntx_abs < (hx >> 5) + 1 || bbox[4] < 0)) return MCL_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i) {
        const double gx = px[i] * mcl::kSortSub, gy = py[i] * mcl::kSortSub;        // (what the ordering kernels hand sort_key, term for term)
        keys[i] = mcl::sort_key(bbox, tilemap, ntx_abs, mcl::cell_of(gx, hx), mcl::cell_of(gy, hy), theta[i], n_layout, gx - floor(gx), gy - floor(gy), fine);
    }
    return MCL_OK;
}

int mcl_host_compact_guide(const uint64_t *ccdf, int64_t n_compact, uint64_t q_total, int32_t m, uint32_t *guide, size_t n_guide,
                           int32_t *s_out, uint32_t *bmax_out, int64_t *n_written)
{
    if (!ccdf || n_compact <= 0 || n_compact > 0xffffffffll || m < mcl::kGuideLog2Min || m > mcl::kGuideLog2Max || ccdf[n_compact - 1] != q_total)
        return MCL_ERR_INVALID_ARG;
    const int s = mcl::guide_shift(q_total, m);
    const uint32_t bmax = mcl::guide_bmax(q_total, s);
    if (s_out) *s_out = s;
    if (bmax_out) *bmax_out = bmax;
    if (!guide) return MCL_OK;
    if (n_guide != (size_t)bmax + 1) return MCL_ERR_INVALID_ARG;
    int64_t written = 0;
    uint64_t prev = 0;
    for (int64_t p = 0; p < n_compact; ++p) {                 // the scan's rule, entry by entry: every owner writes its own range
        const uint64_t c = ccdf[p];
        if (c <= prev) return MCL_ERR_INVALID_ARG;            // (a list entry carries weight: the CDF is strictly increasing)
        uint32_t b0, b1;
        mcl::guide_owner_range(c, c - prev, s, (uint32_t)p, b0, b1);
        for (uint32_t b = b0; b < b1; ++b) { guide[b] = (uint32_t)p; ++written; }
        prev = c;
    }
    if (n_written) *n_written = written;
    return MCL_OK;
}

int mcl_host_compact_search(const uint64_t *ccdf, int64_t n_compact, const uint32_t *guide, size_t n_guide, int32_t s, uint32_t bmax,
                            const uint64_t *thr, int64_t n, int64_t *pos)
{
    if (!ccdf || !guide || !thr || !pos || n < 0 || n_compact <= 0 || n_compact > 0xffffffffll || s < 0 || s > 63 || n_guide < (size_t)bmax + 2)
        return MCL_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; ++i) pos[i] = (int64_t)mcl::compact_guide_search(ccdf, (uint32_t)n_compact, guide, s, bmax, thr[i]);
    return MCL_OK;
}

void mcl_default_kld_config(mcl_kld_config_t *k)
{
    if (!k) return;
    *k = mcl_kld_config_t{};
    k->min_particles = 256; k->max_particles = 4194304;
    k->err = 0.01; k->z = 2.326;
    k->bin_x_m = 0.5; k->bin_y_m = 0.5;
    k->n_theta_bins = 36; k->round_to = 256; k->shrink_permille = 800;
}

int mcl_host_kld_bins(const double *x, const double *y, const double *th, int64_t n, uint32_t width, uint32_t height,
                      float resolution, double origin_x, double origin_y, const mcl_kld_config_t *k, int64_t *bins)
{
    if (!k || !bins || n < 0 || (n > 0 && (!x || !y || !th)) || width == 0 || height == 0 || !(resolution > 0.0f) ||
        !std::isfinite(resolution) || kld_invalid(k, 0))
        return MCL_ERR_INVALID_ARG;
    int64_t nx = 0, ny = 0;
    uint64_t nbits = 0;
    if (!kld_grid(k, width, height, resolution, nx, ny, nbits)) return MCL_ERR_INVALID_ARG;
    const mcl::KldArgs a = kld_args_of(k, nx, ny, origin_x, origin_y);
    std::vector<uint32_t> b((size_t)n);
    for (int64_t i = 0; i < n; ++i) b[(size_t)i] = mcl::kld_bin(a, x[i], y[i], th[i]);
    std::sort(b.begin(), b.end());
    *bins = (int64_t)(std::unique(b.begin(), b.end()) - b.begin());
    return MCL_OK;
}

int mcl_host_kld_target(const mcl_kld_config_t *k, int64_t bins, int64_t n_current, int64_t *n_next)
{
    if (!k || !n_next || n_current < 0 || n_current >= MCL_MAX_TOTAL_PARTICLES || kld_invalid(k, 0)) return MCL_ERR_INVALID_ARG;
    *n_next = kld_target(k, bins, n_current);
    return MCL_OK;
}

int mcl_compact_chunk_bytes(int64_t chunk_entries, int64_t *bytes)
{
    if (!bytes || chunk_entries <= 0 || (chunk_entries & 63)) return MCL_ERR_INVALID_ARG;
    *bytes = chunk_entries * kCompactEntryBytes;
    return MCL_OK;
}

void mcl_default_motion_config(mcl_motion_config_t *c)
{
    if (!c) return;
    *c = mcl_motion_config_t{};
    c->model = MCL_MOTION_DIFF;
    c->alpha1 = c->alpha2 = c->alpha3 = c->alpha4 = c->alpha5 = 0.2;
}

int mcl_host_motion_scalars(const mcl_motion_config_t *c, const double action[3], double out[8])
{
    if (!c || !action || !out || motion_invalid(c) || c->model == MCL_MOTION_REFERENCE) return MCL_ERR_INVALID_ARG;
    const double PI = 3.14159265358979323846;
    const double dx = action[0], dy = action[1], dth = action[2];
    const double trans = std::sqrt(dx * dx + dy * dy);
    const double ft2 = c->floor_trans_m * c->floor_trans_m, fr2 = c->floor_rot_rad * c->floor_rot_rad;
    const double t2 = trans * trans;
    if (c->model == MCL_MOTION_DIFF) {
        const double rot1 = trans < 0.01 ? 0.0 : std::atan2(dy, dx);
        const double rot2 = odo_adiff(dth, rot1);
        const double r1n = std::fmin(std::fabs(odo_adiff(rot1, 0.0)), std::fabs(odo_adiff(rot1, PI)));
        const double r2n = std::fmin(std::fabs(odo_adiff(rot2, 0.0)), std::fabs(odo_adiff(rot2, PI)));
        out[0] = rot1; out[1] = trans; out[2] = rot2;
        out[3] = std::sqrt(c->alpha1 * (r1n * r1n) + c->alpha2 * t2 + fr2);
        out[4] = std::sqrt(c->alpha3 * t2 + c->alpha4 * (r1n * r1n) + c->alpha4 * (r2n * r2n) + ft2);
        out[5] = std::sqrt(c->alpha1 * (r2n * r2n) + c->alpha2 * t2 + fr2);
    } else {
        const double rot = dth, r2 = rot * rot;
        out[0] = std::atan2(dy, dx); out[1] = trans; out[2] = rot;
        out[3] = std::sqrt(c->alpha3 * t2 + c->alpha1 * r2 + ft2);
        out[4] = std::sqrt(c->alpha4 * r2 + c->alpha2 * t2 + fr2);
        out[5] = std::sqrt(c->alpha1 * r2 + c->alpha5 * t2 + ft2);
    }
    out[6] = 0.0; out[7] = 0.0;
    return MCL_OK;
}

int mcl_host_motion_sample(const mcl_motion_config_t *c, const double action[3], const double *xyz, const double *normals, int64_t n,
                           double *out)
{
    if (!xyz || !normals || !out || n < 0) return MCL_ERR_INVALID_ARG;
    double s[8];
    const int rc = mcl_host_motion_scalars(c, action, s);
    if (rc) return rc;
    mcl::OdoArgs o{};
    o.model = c->model;
    for (int i = 0; i < 6; ++i) o.s[i] = s[i];
    for (int64_t m = 0; m < n; ++m) {
        double x = xyz[m], y = xyz[n + m], th = xyz[2 * n + m];
        mcl::odo_step(o, x, y, th, normals[3 * m], normals[3 * m + 1], normals[3 * m + 2]);
        out[m] = x; out[n + m] = y; out[2 * n + m] = host_normalize_angle(th);
    }
    return MCL_OK;
}

int mcl_host_gaussian_factor(const double cov[9], double L[6])
{
    if (!cov || !L) return MCL_ERR_INVALID_ARG;
    return gaussian_factor(cov, L) ? MCL_ERR_INVALID_ARG : MCL_OK;
}

void mcl_default_recovery_config(mcl_recovery_config_t *c)
{
    if (!c) return;
    *c = mcl_recovery_config_t{};
    c->alpha_slow = 0.001; c->alpha_fast = 0.1; c->per_beam = 1;
}

int mcl_host_recovery_proposal(int32_t n_components, const double *means, const double *covs, const double *weights,
                               uint64_t *thresholds, double *factors)
{
    return recov_proposal(n_components, means, covs, weights, thresholds, factors).empty() ? MCL_OK : MCL_ERR_INVALID_ARG;
}

int mcl_host_recovery_step(const mcl_recovery_config_t *c, const double in[2], int32_t reset, double max_logw, double sum_w,
                           double denom, int32_t n_beams, double out[2], double *p_next)
{
    if (!c || !in || !out || recov_invalid(c) || !(denom > 0.0) || n_beams < 1) return MCL_ERR_INVALID_ARG;
    double S = reset ? NAN : in[0], F = reset ? NAN : in[1];
    recov_fold(*c, S, F, recov_likelihood(*c, max_logw, sum_w, denom, n_beams));
    out[0] = S; out[1] = F;
    if (p_next) *p_next = recov_p(S, F);
    return MCL_OK;
}

void mcl_default_likelihood_field_config(mcl_likelihood_field_config_t *c)
{
    if (!c) return;
    *c = mcl_likelihood_field_config_t{};
    c->z_hit = 0.5; c->z_rand = 0.5; c->sigma_hit_m = 0.2; c->max_occ_dist_m = 2.0;   // AMCL's defaults
}

int mcl_host_likelihood_field(const int8_t *data, uint32_t width, uint32_t height, float resolution,
                              const mcl_likelihood_field_config_t *c, uint16_t *out, size_t n)
{
    if (!data || !out || !c || width == 0 || height == 0 || width > 200000 || height > 200000 || !(resolution > 0.0f) ||
        !std::isfinite(resolution) || lf_invalid(c) || n != (size_t)width * height)
        return MCL_ERR_INVALID_ARG;
    const int K = lf_cap(c, resolution);
    if (K < 0) return MCL_ERR_INVALID_ARG;
    lf_field_host(data, (int)width, (int)height, K, out);
    return MCL_OK;
}

int mcl_host_likelihood_table(const mcl_config_t *cfg, const mcl_likelihood_field_config_t *c, float resolution, float *out,
                              size_t n, int32_t *K)
{
    if (!cfg || !c || !(resolution > 0.0f) || !std::isfinite(resolution) || lf_invalid(c)) return MCL_ERR_INVALID_ARG;
    if (!(std::isfinite(cfg->max_range_m) && cfg->max_range_m > 0.0 && std::isfinite(cfg->squash_factor) && cfg->squash_factor > 0.0))
        return MCL_ERR_INVALID_ARG;
    const int k = lf_cap(c, resolution);
    if (k < 0) return MCL_ERR_INVALID_ARG;
    if (K) *K = k;
    if (!out) return MCL_OK;
    if (n != (size_t)k + 1) return MCL_ERR_INVALID_ARG;
    std::vector<float> t;
    lf_table(*cfg, *c, (double)resolution, k, t);
    std::memcpy(out, t.data(), n * sizeof(float));
    return MCL_OK;
}

void mcl_default_beam_skip_config(mcl_beam_skip_config_t *c)
{
    if (!c) return;
    *c = mcl_beam_skip_config_t{};
    c->distance_m = 0.5; c->threshold = 0.3; c->error_threshold = 0.9;                // AMCL's defaults
}

static bool bs_host_args_ok(const mcl_beam_skip_config_t *c, int64_t n_particles, int32_t n_used)
{
    return c && !bs_invalid(c) && n_particles >= 1 && n_particles <= 0x7fffffff && n_used >= 0 && n_used < 0x7fffffff;
}

int mcl_host_beam_skip_thresholds(const mcl_beam_skip_config_t *c, float resolution, int64_t n_particles, int32_t n_used,
                                  int32_t *ka, int64_t *min_count, int32_t *min_skipped)
{
    if (!bs_host_args_ok(c, n_particles, n_used) || !(resolution > 0.0f) || !std::isfinite(resolution)) return MCL_ERR_INVALID_ARG;
    if (ka) *ka = bs_ka(c, resolution);
    if (min_count) *min_count = bs_min_count(c->threshold, n_particles);
    if (min_skipped) *min_skipped = bs_min_skipped(c->error_threshold, n_used);
    return MCL_OK;
}

int mcl_host_beam_skip_plan(const mcl_beam_skip_config_t *c, const uint32_t *counts_used, int32_t n_used, int64_t n_particles,
                            uint8_t *kept_used, int32_t *n_skipped, int32_t *integrate_all)
{
    if (!bs_host_args_ok(c, n_particles, n_used) || (!counts_used && n_used > 0)) return MCL_ERR_INVALID_ARG;
    const int64_t min_count = bs_min_count(c->threshold, n_particles);
    int32_t skipped = 0;
    for (int32_t j = 0; j < n_used; ++j) skipped += (int64_t)counts_used[j] < min_count;
    const int all = skipped >= bs_min_skipped(c->error_threshold, n_used);
    if (kept_used)
        for (int32_t j = 0; j < n_used; ++j) kept_used[j] = all || (int64_t)counts_used[j] >= min_count ? 1 : 2;
    if (n_skipped) *n_skipped = skipped;
    if (integrate_all) *integrate_all = all;
    return MCL_OK;
}

void mcl_default_search_config(mcl_search_config_t *c)
{
    if (!c) return;
    *c = mcl_search_config_t{};
    c->stride_cells = 2; c->n_headings = 72; c->beam_stride = 1; c->nms = 1;
}

int mcl_host_search_lattice(const mcl_search_config_t *c, const int8_t *data, uint32_t width, uint32_t height, float resolution,
                            double origin_x, double origin_y, uint32_t *cells, double *xy, size_t n, int64_t *n_positions)
{
    if (!c || search_invalid(c) || !data || !n_positions || width == 0 || height == 0 || width > 200000 || height > 200000 ||
        !(resolution > 0.0f) || !std::isfinite(resolution))
        return MCL_ERR_INVALID_ARG;
    std::vector<uint32_t> vc;
    std::vector<double> vxy;
    int nx = 0, ny = 0;
    const int64_t np = search_lattice(c->stride_cells, data, (int)width, (int)height, (double)resolution, origin_x, origin_y,
                                      cells ? &vc : nullptr, xy ? &vxy : nullptr, nullptr, nullptr, nx, ny);
    *n_positions = np;
    if (!cells && !xy) return MCL_OK;
    if (n != (size_t)np) return MCL_ERR_INVALID_ARG;
    if (cells && np) std::memcpy(cells, vc.data(), (size_t)np * sizeof(uint32_t));
    if (xy && np) std::memcpy(xy, vxy.data(), (size_t)np * 2 * sizeof(double));
    return MCL_OK;
}

int mcl_host_search_headings(const mcl_search_config_t *c, double *theta, size_t n)
{
    if (!c || search_invalid(c) || !theta || n != (size_t)c->n_headings) return MCL_ERR_INVALID_ARG;
    search_headings(c->n_headings, theta);
    return MCL_OK;
}

int mcl_host_search_sequence_offsets(const mcl_search_config_t *c, const double *rel, int32_t n_scans, double *out, size_t n)
{
    if (!c || search_invalid(c) || search_sequence_invalid(rel, n_scans) || !out || n != (size_t)c->n_headings * (size_t)n_scans * 3)
        return MCL_ERR_INVALID_ARG;
    std::vector<double> theta((size_t)c->n_headings);
    search_headings(c->n_headings, theta.data());
    search_sequence_offsets(c->n_headings, theta.data(), rel, n_scans, out);
    return MCL_OK;
}

int mcl_host_search_beam_grid(const float *angles, int32_t n_beams, int32_t n_headings, int32_t *M, int32_t *heading_step, double *delta,
                              double *max_dev, double *phi, size_t n_phi)
{
    SearchBeamGrid g;
    const std::string why = search_beam_grid(angles, n_beams, n_headings, g);
    if (max_dev) *max_dev = g.max_dev;                                  // (what was measured, refused or not)
    if (!why.empty()) return MCL_ERR_INVALID_ARG;
    if (phi && n_phi != (size_t)g.M) return MCL_ERR_INVALID_ARG;
    if (M) *M = g.M;
    if (heading_step) *heading_step = g.heading_step;
    if (delta) *delta = g.delta;
    if (phi) search_beam_angles(g, phi);
    return MCL_OK;
}

void mcl_default_search_stream_config(mcl_search_stream_config_t *c)
{
    if (!c) return;
    *c = mcl_search_stream_config_t{};
}

int mcl_host_search_slabs(const mcl_search_config_t *c, const mcl_search_stream_config_t *sc, int64_t n_positions, int32_t n_scans,
                          int32_t *slab_headings, int32_t *n_slabs, uint64_t *bytes)
{
    if (!c) return MCL_ERR_INVALID_ARG;
    mcl_search_stream_config_t d;
    mcl_default_search_stream_config(&d);
    SearchSlabPlan plan;
    if (!search_slabs(c, sc ? sc : &d, n_positions, n_scans, plan).empty()) return MCL_ERR_INVALID_ARG;
    if (slab_headings) *slab_headings = plan.G;
    if (n_slabs) *n_slabs = plan.n_slabs;
    if (bytes) *bytes = plan.bytes;
    return MCL_OK;
}

void mcl_default_search_prune_config(mcl_search_prune_config_t *c)
{
    if (!c) return;
    *c = mcl_search_prune_config_t{};
    c->block = 8; c->first_pairs = 0;
}

int mcl_host_search_blocks(const mcl_search_config_t *c, const mcl_search_prune_config_t *pc, const int8_t *data, uint32_t width,
                           uint32_t height, int32_t *n_blocks, int32_t *w, int32_t *nbx, int32_t *nby, int32_t *blocks, size_t n)
{
    mcl_search_prune_config_t d;
    mcl_default_search_prune_config(&d);
    if (!pc) pc = &d;
    if (!c || search_invalid(c) || search_prune_invalid(c, pc) || !data || width == 0 || height == 0 || width > 200000 || height > 200000)
        return MCL_ERR_INVALID_ARG;
    std::vector<int32_t> pmap;
    int nx = 0, ny = 0;
    search_lattice(c->stride_cells, data, (int)width, (int)height, 1.0, 0.0, 0.0, nullptr, nullptr, nullptr, &pmap, nx, ny);
    SearchBlocks b;
    search_blocks(pc->block, c->stride_cells, pmap.data(), nx, ny, b);
    if (n_blocks) *n_blocks = b.n_blocks;
    if (w) *w = b.w;
    if (nbx) *nbx = b.nbx;
    if (nby) *nby = b.nby;
    if (!blocks) return MCL_OK;
    if (n != (size_t)b.n_blocks) return MCL_ERR_INVALID_ARG;
    if (n) std::memcpy(blocks, b.blk.data(), n * 3 * sizeof(int32_t));
    return MCL_OK;
}

int mcl_host_lf_pool(const uint16_t *D, uint32_t width, uint32_t height, int32_t K, int32_t w, uint16_t *out, size_t n)
{
    if (!D || !out || width == 0 || height == 0 || width > 200000 || height > 200000 || K < 0 || K > 65535 || w < 1 || w > 65536 ||
        n != ((size_t)width + (size_t)w - 1) * ((size_t)height + (size_t)w - 1))
        return MCL_ERR_INVALID_ARG;
    lf_pool(D, (int)width, (int)height, K, w, out);
    return MCL_OK;
}

int mcl_host_search_bound_table(const float *lf, int32_t K, float *ub)
{
    if (!lf || !ub || K < 0 || K > 65535) return MCL_ERR_INVALID_ARG;
    search_bound_table(lf, K, ub);
    return MCL_OK;
}

int mcl_host_search_prune_next(const mcl_search_prune_config_t *pc, int64_t pairs, int64_t n_scored, int64_t first_below_c, int64_t *n_next)
{
    mcl_search_prune_config_t d;
    mcl_default_search_prune_config(&d);
    if (!pc) pc = &d;
    if (!n_next || pairs < 1 || n_scored < 0 || n_scored > pairs || first_below_c < 0 || pc->first_pairs < 0) return MCL_ERR_INVALID_ARG;
    *n_next = search_prune_next(*pc, pairs, n_scored, first_below_c);
    return MCL_OK;
}

int mcl_host_relative_poses(const double *odom, int32_t n_scans, int32_t anchor, double *rel)
{
    if (!odom || !rel || n_scans < 1 || anchor < 0 || anchor >= n_scans) return MCL_ERR_INVALID_ARG;
    for (int64_t i = 0; i < 3 * (int64_t)n_scans; ++i)
        if (!std::isfinite(odom[i])) return MCL_ERR_INVALID_ARG;
    const double PI = 3.14159265358979323846;
    const double xa = odom[3 * (size_t)anchor], ya = odom[3 * (size_t)anchor + 1], ta = odom[3 * (size_t)anchor + 2];
    const double ca = std::cos(ta), sa = std::sin(ta);
    for (int32_t s = 0; s < n_scans; ++s) {
        double *r = rel + 3 * (size_t)s;
        if (s == anchor) { r[0] = r[1] = r[2] = 0.0; continue; }
        const double ex = odom[3 * (size_t)s] - xa, ey = odom[3 * (size_t)s + 1] - ya;
        r[0] = ca * ex + sa * ey;
        r[1] = ca * ey - sa * ex;
        double d = std::remainder(odom[3 * (size_t)s + 2] - ta, 2.0 * PI);      // [-pi, pi]
        if (d <= -PI) d += 2.0 * PI;                                              // (-pi, pi]
        r[2] = d;
    }
    return MCL_OK;
}

void mcl_default_refine_config(mcl_refine_config_t *c)
{
    if (!c) return;
    *c = mcl_refine_config_t{};
    c->half_xy = 4; c->half_theta = 10; c->step_xy_cells = 0.5; c->step_theta_rad = 3.14159265358979323846 / 360.0; c->beam_stride = 1;
}

static bool refine_host_args_ok(const mcl_refine_config_t *c, const double seed[3], float resolution)
{
    return c && !refine_invalid(c) && seed && resolution > 0.0f && std::isfinite(resolution) && std::isfinite(seed[0]) &&
           std::isfinite(seed[1]) && std::isfinite(seed[2]);
}

int mcl_host_refine_window(const mcl_refine_config_t *c, const double seed[3], float resolution, double *poses, size_t n_win)
{
    if (!refine_host_args_ok(c, seed, resolution) || !poses) return MCL_ERR_INVALID_ARG;
    const mcl_rf::Window g = mcl_rf::window_of(*c, (double)resolution);
    if (n_win != (size_t)g.n_win) return MCL_ERR_INVALID_ARG;
    for (int32_t w = 0; w < g.n_win; ++w) {
        int32_t dx, dy, dt;
        mcl_rf::offsets(g, w, dx, dy, dt);
        poses[3 * (size_t)w] = mcl_rf::coord(seed[0], dx, g.sx);
        poses[3 * (size_t)w + 1] = mcl_rf::coord(seed[1], dy, g.sx);
        poses[3 * (size_t)w + 2] = mcl_rf::coord(seed[2], dt, g.st);
    }
    return MCL_OK;
}

// k_refine_reduce on the host: the same order of R3, the same 256 partial sums and tree of R4
int mcl_host_refine_reduce(const mcl_refine_config_t *c, const double seed[3], float resolution, const double *scores, size_t n_win,
                           mcl_refine_result_t *out)
{
    if (!refine_host_args_ok(c, seed, resolution) || !scores || !out) return MCL_ERR_INVALID_ARG;
    const mcl_rf::Window g = mcl_rf::window_of(*c, (double)resolution);
    if (n_win != (size_t)g.n_win) return MCL_ERR_INVALID_ARG;
    for (int32_t w = 0; w < g.n_win; ++w)
        if (std::isnan(scores[w]) || scores[w] == INFINITY) return MCL_ERR_INVALID_ARG;
    int32_t wb = 0, qb = 0;
    for (int32_t w = 0; w < g.n_win; ++w) {
        int32_t dx, dy, dt;
        mcl_rf::offsets(g, w, dx, dy, dt);
        const int32_t q = dx * dx + dy * dy + dt * dt;
        if (w == 0 || mcl_rf::better(scores[w], q, w, scores[wb], qb, wb)) { wb = w; qb = q; }
    }
    int32_t bx, by, bt;
    mcl_rf::offsets(g, wb, bx, by, bt);
    std::vector<double> part((size_t)mcl_rf::kSums * mcl_rf::kThreads, 0.0);
    for (int l = 0; l < mcl_rf::kThreads; ++l) {
        double acc[mcl_rf::kSums] = {};
        for (int32_t w = l; w < g.n_win; w += mcl_rf::kThreads) mcl_rf::accumulate(g, w, scores[w], scores[wb], bx, by, bt, acc);
        for (int k = 0; k < mcl_rf::kSums; ++k) part[(size_t)k * mcl_rf::kThreads + l] = acc[k];
    }
    for (int st = mcl_rf::kThreads / 2; st > 0; st >>= 1)
        for (int l = 0; l < st; ++l)
            for (int k = 0; k < mcl_rf::kSums; ++k) part[(size_t)k * mcl_rf::kThreads + l] += part[(size_t)k * mcl_rf::kThreads + l + st];
    double sums[mcl_rf::kSums];
    for (int k = 0; k < mcl_rf::kSums; ++k) sums[k] = part[(size_t)k * mcl_rf::kThreads];
    const int32_t wc = (g.half_theta * g.nx + g.half_xy) * g.nx + g.half_xy;
    mcl_rf::finish(g, seed[0], seed[1], seed[2], wb, scores[wb], scores[wc], sums, out);
    return MCL_OK;
}

int mcl_host_refine_sequence_offsets(const mcl_refine_config_t *c, const double *seeds_colmajor, int32_t M, const double *rel,
                                     int32_t n_scans, double *out, size_t n)
{
    mcl_refine_config_t d;
    mcl_default_refine_config(&d);
    if (!c) c = &d;
    if (refine_invalid(c) || !seeds_colmajor || M < 1 || M > mcl_rf::kMaxSeeds || refine_sequence_invalid(rel, n_scans) || !out)
        return MCL_ERR_INVALID_ARG;
    for (int64_t i = 0; i < (int64_t)3 * M; ++i)
        if (!std::isfinite(seeds_colmajor[i])) return MCL_ERR_INVALID_ARG;
    const int64_t nt = 2 * (int64_t)c->half_theta + 1;
    if (!refine_sequence_rows_refused(M, nt, n_scans).empty()) return MCL_ERR_INVALID_ARG;
    if (n != (size_t)M * (size_t)nt * (size_t)n_scans * 3) return MCL_ERR_INVALID_ARG;
    refine_sequence_offsets(c->half_theta, c->step_theta_rad, seeds_colmajor, M, rel, n_scans, out);
    return MCL_OK;
}

// ---- sensor mount on the host: SM2 with the host's libm, its inverse, and the covariance through either
int mcl_host_sensor_mount(const double mount[3], const double *poses_colmajor, int64_t n, double *out_colmajor)
{
    if (!mount || !mount_valid(mount) || !poses_colmajor || !out_colmajor || n < 1) return MCL_ERR_INVALID_ARG;
    const double mx = mount[0], my = mount[1], mth = mount[2];
    for (int64_t i = 0; i < n; ++i) {
        const double x = poses_colmajor[i], y = poses_colmajor[n + i], th = poses_colmajor[2 * n + i];
        const double s = std::sin(th), c = std::cos(th);
        out_colmajor[i] = x + (c * mx - s * my);
        out_colmajor[n + i] = y + (s * mx + c * my);
        out_colmajor[2 * n + i] = th + mth;
    }
    return MCL_OK;
}

int mcl_host_sensor_unmount(const double mount[3], const double *poses_colmajor, int64_t n, double *out_colmajor)
{
    if (!mount || !mount_valid(mount) || !poses_colmajor || !out_colmajor || n < 1) return MCL_ERR_INVALID_ARG;
    const double mx = mount[0], my = mount[1], mth = mount[2];
    for (int64_t i = 0; i < n; ++i) {
        const double xs = poses_colmajor[i], ys = poses_colmajor[n + i], ths = poses_colmajor[2 * n + i];
        const double th = ths - mth;
        const double s = std::sin(th), c = std::cos(th);
        out_colmajor[i] = xs - (c * mx - s * my);
        out_colmajor[n + i] = ys - (s * mx + c * my);
        out_colmajor[2 * n + i] = th;
    }
    return MCL_OK;
}

int mcl_host_sensor_mount_cov(const double mount[3], const double pose[3], const double cov9[9], int to_base, double out9[9])
{
    if (!mount || !mount_valid(mount) || !pose || !cov9 || !out9 || (to_base != 0 && to_base != 1)) return MCL_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(pose[k])) return MCL_ERR_INVALID_ARG;
    for (int k = 0; k < 9; ++k) if (!std::isfinite(cov9[k])) return MCL_ERR_INVALID_ARG;
    // the Jacobian of SM2 at a base pose, or of its inverse at a sensor pose: the identity but for the heading column
    const double th = to_base ? pose[2] - mount[2] : pose[2];
    const double s = std::sin(th), c = std::cos(th);
    const double jx = to_base ? (s * mount[0] + c * mount[1]) : -(s * mount[0] + c * mount[1]);
    const double jy = to_base ? -(c * mount[0] - s * mount[1]) : (c * mount[0] - s * mount[1]);
    const double J[9] = {1.0, 0.0, jx, 0.0, 1.0, jy, 0.0, 0.0, 1.0};
    double JS[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) JS[r * 3 + q] = J[r * 3 + 0] * cov9[0 * 3 + q] + J[r * 3 + 1] * cov9[1 * 3 + q] + J[r * 3 + 2] * cov9[2 * 3 + q];
    double o[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) o[r * 3 + q] = JS[r * 3 + 0] * J[q * 3 + 0] + JS[r * 3 + 1] * J[q * 3 + 1] + JS[r * 3 + 2] * J[q * 3 + 2];
    for (int k = 0; k < 9; ++k) out9[k] = o[k];
    return MCL_OK;
}

// ---- per-beam sensor offsets on the host: the constant-twist table (DM1, DM2) and the setter's table formation
int mcl_host_scan_motion_offsets(const double motion[3], const double mount[3], const double *t, double t_ref, int32_t n_beams,
                                 double *offsets_colmajor)
{
    if (!motion || !offsets_colmajor || n_beams < 1 || !std::isfinite(t_ref)) return MCL_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) if (!std::isfinite(motion[k])) return MCL_ERR_INVALID_ARG;
    if (mount && !mount_valid(mount)) return MCL_ERR_INVALID_ARG;
    if (t) for (int32_t j = 0; j < n_beams; ++j) if (!std::isfinite(t[j])) return MCL_ERR_INVALID_ARG;
    const double u = motion[0], v = motion[1], w = motion[2];
    const size_t B = (size_t)n_beams;
    for (int32_t j = 0; j < n_beams; ++j) {
        const double tj = t ? t[j] : (n_beams > 1 ? (double)j / (double)(n_beams - 1) : 0.0);
        // DM1: the base's pose at t_j in its frame at t_ref, a constant twist integrated over tau
        const double tau = tj - t_ref, th = tau * w;
        double A, Bc;
        if (std::fabs(th) < 1e-8) { A = 1.0 - th * th / 6.0; Bc = th / 2.0; }
        else { A = std::sin(th) / th; Bc = (1.0 - std::cos(th)) / th; }
        double d[3] = {tau * (A * u - Bc * v) + 0.0, tau * (Bc * u + A * v) + 0.0, th + 0.0};      // (+ 0.0: a zero twist gives +0, whatever tau's sign)
        if (mount) {
            // DM2: o = m^-1 o Delta o m -- the sensor's pose under Delta (mcl_host_sensor_mount's lines), then into the frame of the
            // sensor at t_ref: the base pose of the sensor pose m seen from the origin is the inverse composition (.._unmount's lines)
            const double mx = mount[0], my = mount[1], mth = mount[2];
            const double s = std::sin(d[2]), c = std::cos(d[2]);
            const double xs = d[0] + (c * mx - s * my), ys = d[1] + (s * mx + c * my);
            // m^-1 applied on the left: translate by -m's position, turn by -mtheta
            const double sm = std::sin(mth), cm = std::cos(mth);
            const double ex = xs - mx, ey = ys - my;
            d[0] = (cm * ex + sm * ey) + 0.0;
            d[1] = (cm * ey - sm * ex) + 0.0;
            // (the heading component: (theta + mtheta) - mtheta is theta whatever the mount)
        }
        offsets_colmajor[j] = d[0]; offsets_colmajor[B + j] = d[1]; offsets_colmajor[2 * B + j] = d[2];
    }
    return MCL_OK;
}

int mcl_host_beam_offset_table(const float *angles, const double *offsets_colmajor, int32_t n_beams, float *effective_angles, double *dirs)
{
    if (!angles || !offsets_colmajor || n_beams < 1 || (!effective_angles && !dirs)) return MCL_ERR_INVALID_ARG;
    const size_t B = (size_t)n_beams;
    for (size_t k = 0; k < 3 * B; ++k) if (!std::isfinite(offsets_colmajor[k])) return MCL_ERR_INVALID_ARG;
    std::vector<float> af(B);
    std::vector<double2> cs(B);
    deskew_table(angles, offsets_colmajor, n_beams, af.data(), cs.data());
    for (size_t j = 0; j < B; ++j) {
        if (effective_angles) effective_angles[j] = af[j];
        if (dirs) { dirs[j] = cs[j].x; dirs[B + j] = cs[j].y; }
    }
    return MCL_OK;
}

int mcl_host_beam_offset_pairs(const float *ranges, const double *offsets_colmajor, const double *dirs, int32_t n_beams, double resolution,
                               double *pairs)
{
    if (!ranges || !offsets_colmajor || !dirs || !pairs || n_beams < 1 || !(resolution > 0.0) || !std::isfinite(resolution)) return MCL_ERR_INVALID_ARG;
    const size_t B = (size_t)n_beams;
    const double inv_res = 1.0 / resolution;
    for (size_t j = 0; j < B; ++j) {
        const double2 p = deskew_pair((double)ranges[j], offsets_colmajor[j], offsets_colmajor[B + j], make_double2(dirs[j], dirs[B + j]), inv_res);
        pairs[j] = p.x; pairs[B + j] = p.y;
    }
    return MCL_OK;
}

}  // extern "C"
