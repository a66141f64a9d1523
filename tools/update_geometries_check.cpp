// update_geometries_check.cpp -- the host functions the filter's stages share with their tests, over the nine map geometries of
// tests/side_geometries.py: mcl_host_kld_bins (the bin rule of DESIGN.md §4.7) at the default bins, bins of one cell and bins
// larger than the map, and the block plan and pooled field of the pruned search (rules P1 / P2 of DESIGN.md §4.20) for strides
// 1 .. 3 and block sides 2, 4, 8.  A stand-alone host program for a sanitizer build: no device is opened.  Build it together
// with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/update_geometries_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o update_geometries_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <set>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d (%s): %s\n", __LINE__, geo_name, #cond); ++failures; } } while (0)

struct Geo { const char *name; int W, H; float res; double ox, oy; };
// the family's (W, H, resolution, origin): tests/test_side_geometries_host.py holds the Python family to the same table
static const Geo GEOS[9] = {
    {"narrow", 37, 301, 0.05f, -1.0, -7.0},         {"wide", 517, 23, 0.05f, -12.0, -0.5},
    {"coarse", 64, 48, 0.25f, -8.0, -6.0},          {"fine", 150, 110, 0.02f, -1.5, -1.1},
    {"spielberg_res", 120, 90, 0.05796f, -3.37, 1.91}, {"far_origin", 120, 90, 0.05f, 4096.3, -8191.7},
    {"tiny", 9, 7, 0.05f, 0.0, 0.0},                {"open", 80, 60, 0.05f, -2.0, -1.5},
    {"one_free", 40, 30, 0.05f, -1.0, -0.75},
};
static const char *geo_name = "";

// the bin rule of include/mcl_hip_engine.h restated: one subtract, one multiply, floor; the heading's turn wraps
static int64_t bins_ref(const std::vector<double> &x, const std::vector<double> &y, const std::vector<double> &th, const Geo &g,
                        const mcl_kld_config_t &k, int64_t *nx_out, int64_t *ny_out)
{
    const double res = (double)g.res;
    const double nx = std::ceil((double)g.W * res / k.bin_x_m), ny = std::ceil((double)g.H * res / k.bin_y_m);
    const double ibx = 1.0 / k.bin_x_m, iby = 1.0 / k.bin_y_m, scale = (double)k.n_theta_bins / (2.0 * M_PI);
    std::set<int64_t> seen;
    for (size_t i = 0; i < x.size(); ++i) {
        const double fx = std::floor((x[i] - g.ox) * ibx), fy = std::floor((y[i] - g.oy) * iby);
        if (!(fx >= 0 && fx < nx && fy >= 0 && fy < ny && std::fabs(th[i]) < 1e9)) {
            seen.insert((int64_t)nx * (int64_t)ny * k.n_theta_bins);
            continue;
        }
        int64_t t = (int64_t)std::floor((th[i] + M_PI) * scale) % k.n_theta_bins;
        if (t < 0) t += k.n_theta_bins;
        seen.insert((t * (int64_t)ny + (int64_t)fy) * (int64_t)nx + (int64_t)fx);
    }
    *nx_out = (int64_t)nx;
    *ny_out = (int64_t)ny;
    return (int64_t)seen.size();
}

// P2 by brute force
static std::vector<uint16_t> pool_ref(const std::vector<uint16_t> &D, int W, int H, int K, int w)
{
    const int Wp = W + w - 1, Hp = H + w - 1;
    std::vector<uint16_t> out((size_t)Wp * Hp);
    for (int ys = 0; ys < Hp; ++ys)
        for (int xs = 0; xs < Wp; ++xs) {
            int best = K;
            for (int y = std::max(0, ys - (w - 1)); y <= std::min(H - 1, ys); ++y)
                for (int x = std::max(0, xs - (w - 1)); x <= std::min(W - 1, xs); ++x) best = std::min(best, (int)D[(size_t)y * W + x]);
            out[(size_t)ys * Wp + xs] = (uint16_t)best;
        }
    return out;
}

// an outer wall with a gap, two inner walls where the map is large enough, a few unknown cells; open: nothing; one_free: one cell
static std::vector<int8_t> grid_of(const Geo &g, int which)
{
    const int W = g.W, H = g.H;
    std::vector<int8_t> d((size_t)W * H, 0);
    if (which == 7) return d;
    if (which == 8) {
        std::fill(d.begin(), d.end(), (int8_t)100);
        d[(size_t)13 * W + 19] = 0;
        return d;
    }
    for (int x = 0; x < W; ++x) d[x] = d[(size_t)(H - 1) * W + x] = 100;
    for (int y = 0; y < H; ++y) d[(size_t)y * W] = d[(size_t)y * W + W - 1] = 100;
    d[W / 4] = 0;
    if (W >= 20 && H >= 20) {
        for (int x = W / 6; x < 7 * W / 12; ++x) d[(size_t)(H / 3) * W + x] = 100;
        for (int y = H / 3; y < 5 * H / 6; ++y) d[(size_t)y * W + 7 * W / 10] = 100;
        d[(size_t)(2 * H / 3) * W + 2] = d[(size_t)(2 * H / 3) * W + 3] = -1;
    }
    return d;
}

int main()
{
    for (int gi = 0; gi < 9; ++gi) {
        const Geo &g = GEOS[gi];
        geo_name = g.name;
        const double res = (double)g.res;
        const std::vector<int8_t> data = grid_of(g, gi);

        // ---- the bin rule: a pose in every cell's centre, every map edge and grid edge by +-1 ulp and +-1 bin, headings at the
        // turn's ends
        for (int form = 0; form < 3; ++form) {
            mcl_kld_config_t k;
            mcl_default_kld_config(&k);
            if (form == 1) k.bin_x_m = k.bin_y_m = res;
            if (form == 2) k.bin_x_m = k.bin_y_m = 2.0 * std::max(g.W, g.H) * res;
            std::vector<double> x, y, th;
            for (int r = 0; r < g.H; ++r)
                for (int c = 0; c < g.W; ++c) {
                    x.push_back(g.ox + (c + 0.5) * res);
                    y.push_back(g.oy + (r + 0.5) * res);
                    th.push_back(0.1);
                }
            int64_t nx = 0, ny = 0, got = -1;
            const size_t n_cells = x.size();
            int64_t want = bins_ref(x, y, th, g, k, &nx, &ny);
            CHECK(mcl_host_kld_bins(x.data(), y.data(), th.data(), (int64_t)x.size(), g.W, g.H, g.res, g.ox, g.oy, &k, &got) == MCL_OK);
            CHECK(got == want);
            if (form == 0 && gi == 6) CHECK(nx == 1 && ny == 1 && got == 1);          // tiny: 0.45 m x 0.35 m in one 0.5 m bin
            if (form == 1) CHECK(nx >= g.W && nx <= g.W + 1 && ny >= g.H && ny <= g.H + 1 && got == (int64_t)n_cells);
            if (form == 2) CHECK(nx == 1 && ny == 1 && got == 1);
            const double ex[3] = {g.ox, g.ox + g.W * res, g.ox + (double)nx * k.bin_x_m};
            const double ey[3] = {g.oy, g.oy + g.H * res, g.oy + (double)ny * k.bin_y_m};
            const double ths[5] = {M_PI, -M_PI, std::nextafter(M_PI, 0.0), std::nextafter(-M_PI, 0.0), 0.0};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b)
                    for (int u = 0; u < 5; ++u)
                        for (int v = 0; v < 5; ++v) {
                            const double xs[5] = {ex[a], std::nextafter(ex[a], -INFINITY), std::nextafter(ex[a], INFINITY), ex[a] - k.bin_x_m, ex[a] + k.bin_x_m};
                            const double ys[5] = {ey[b], std::nextafter(ey[b], -INFINITY), std::nextafter(ey[b], INFINITY), ey[b] - k.bin_y_m, ey[b] + k.bin_y_m};
                            x.assign(1, xs[u]);
                            y.assign(1, ys[v]);
                            // alone with an inside pose: one bin if it is that pose's, else two
                            x.push_back(g.ox + 0.5 * res);
                            y.push_back(g.oy + 0.5 * res);
                            th.assign(2, ths[(u + v) % 5]);
                            want = bins_ref(x, y, th, g, k, &nx, &ny);
                            CHECK(mcl_host_kld_bins(x.data(), y.data(), th.data(), 2, g.W, g.H, g.res, g.ox, g.oy, &k, &got) == MCL_OK);
                            CHECK(got == want);
                        }
        }

        // ---- the likelihood field, the block plan and the pooled field
        mcl_likelihood_field_config_t lc;
        mcl_default_likelihood_field_config(&lc);
        std::vector<uint16_t> D((size_t)g.W * g.H);
        CHECK(mcl_host_likelihood_field(data.data(), g.W, g.H, g.res, &lc, D.data(), D.size()) == MCL_OK);
        const int K = (int)*std::max_element(D.begin(), D.end());              // (a stand-in for LF1's K: at least every entry)
        for (int stride = 1; stride <= 3; ++stride)
            for (int S : {2, 4, 8}) {
                mcl_search_config_t c;
                mcl_search_prune_config_t pc;
                mcl_default_search_config(&c);
                mcl_default_search_prune_config(&pc);
                c.stride_cells = stride;
                pc.block = S;
                int32_t n = -1, w = -1, nbx = -1, nby = -1;
                CHECK(mcl_host_search_blocks(&c, &pc, data.data(), g.W, g.H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_OK);
                const int h0 = stride / 2, lx = (g.W - 1 - h0) / stride + 1, ly = (g.H - 1 - h0) / stride + 1;
                CHECK(w == (S - 1) * stride + 2 && nbx == (lx + S - 1) / S && nby == (ly + S - 1) / S && n >= 1 && n <= nbx * nby);
                std::vector<int32_t> blk((size_t)n * 3);
                CHECK(mcl_host_search_blocks(&c, &pc, data.data(), g.W, g.H, &n, &w, &nbx, &nby, blk.data(), (size_t)n) == MCL_OK);
                // the plan by its definition: the lattice cells of each block that are free, blocks in row-major order
                std::vector<int32_t> ref;
                for (int by = 0; by < nby; ++by)
                    for (int bx = 0; bx < nbx; ++bx) {
                        int held = 0;
                        for (int iy = by * S; iy < std::min(ly, by * S + S); ++iy)
                            for (int ix = bx * S; ix < std::min(lx, bx * S + S); ++ix)
                                held += data[(size_t)(h0 + iy * stride) * g.W + (h0 + ix * stride)] == 0;
                        if (held) { ref.push_back(bx); ref.push_back(by); ref.push_back(held); }
                    }
                CHECK(blk == ref);
                if (gi == 8) CHECK(n == 1 && blk[2] == 1);
                if (gi == 6 && stride == 3 && S >= 4) CHECK(n == 1 && nbx == 1 && nby == 1);       // a 3 x 2 lattice in one block
                const size_t np = (size_t)(g.W + w - 1) * (g.H + w - 1);
                std::vector<uint16_t> out(np);
                CHECK(mcl_host_lf_pool(D.data(), g.W, g.H, K, w, out.data(), np) == MCL_OK);
                CHECK(out == pool_ref(D, g.W, g.H, K, w));
            }
    }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
