// refine_sequence_check.cpp -- the host side of mcl_refine_poses_sequence (rules RS1 / RS7): the offset table over
// its boundary and refusal cases, as a stand-alone host program for a sanitizer build: no device is opened.  Build it together
// with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/refine_sequence_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o refine_sequence_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"
#include "../monte_carlo_localization_amd/csrc/mcl_host_math.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// the table of a config with a guard double behind it: MCL_OK, the guard untouched, the call with n - 1 refused
static std::vector<double> table(const mcl_refine_config_t &c, const std::vector<double> &seeds, int M, const std::vector<double> &rel, int S)
{
    const size_t nt = 2 * (size_t)c.half_theta + 1, n = (size_t)M * nt * (size_t)S * 3;
    std::vector<double> off(n + 1, 77.0);
    CHECK(mcl_host_refine_sequence_offsets(&c, seeds.data(), M, rel.data(), S, off.data(), n) == MCL_OK);
    CHECK(off[n] == 77.0);
    CHECK(mcl_host_refine_sequence_offsets(&c, seeds.data(), M, rel.data(), S, off.data(), n - 1) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_refine_sequence_offsets(&c, seeds.data(), M, rel.data(), S, off.data(), n + 1) == MCL_ERR_INVALID_ARG);
    return off;
}

int main()
{
    mcl_refine_config_t c;
    mcl_default_refine_config(&c);

    // ---- M = nt = S = 1: one triple
    {
        c.half_theta = 0;
        const std::vector<double> seed = {1.0, 2.0, 0.3}, rel = {-0.5, 0.13, 0.2};
        const std::vector<double> off = table(c, seed, 1, rel, 1);
        const double ck = std::cos(0.3), sk = std::sin(0.3);
        CHECK(off[0] == ck * -0.5 - sk * 0.13 && off[1] == sk * -0.5 + ck * 0.13 && off[2] == 0.3 + 0.2);
    }

    // ---- every S up to 16, several seeds, half_theta 0 and more: the last triple written and nothing behind it; the anchor's row
    // (a zero rel) is the window heading bit for bit with no displacement, of either sign
    for (int ht : {0, 1, 10}) {
        c.half_theta = ht;
        const int M = 3, nt = 2 * ht + 1;
        const std::vector<double> seeds = {0.5, -3.0, 1e6, 0.25, 7.0, -1.0, -0.0, 3.0, -2.5};       // column-major: x, y, theta
        for (int S = 1; S <= MCL_SEARCH_MAX_SCANS; ++S) {
            std::vector<double> rel((size_t)S * 3);
            for (int s = 0; s < S; ++s) { rel[3 * s] = -0.5 * (S - 1 - s); rel[3 * s + 1] = 0.13 * (S - 1 - s); rel[3 * s + 2] = s == S - 1 ? 0.0 : 0.3; }
            const std::vector<double> off = table(c, seeds, M, rel, S);
            for (int m = 0; m < M; ++m)
                for (int it = 0; it < nt; ++it) {
                    const double t = (double)(it - ht) * c.step_theta_rad, th = seeds[(size_t)2 * M + m] + t;
                    const double *last = &off[(((size_t)m * nt + it) * S + (size_t)(S - 1)) * 3];
                    CHECK(last[2] == th && last[0] == 0.0 && last[1] == 0.0);
                    if (S > 1) {
                        const double *first = &off[(((size_t)m * nt + it) * S) * 3];
                        const double dx = rel[0], dy = rel[1], ck = std::cos(th), sk = std::sin(th);
                        CHECK(first[0] == ck * dx - sk * dy && first[1] == sk * dx + ck * dy && first[2] == th + 0.3);
                        CHECK(std::fabs(std::hypot(first[0], first[1]) - std::hypot(dx, dy)) < 1e-9);
                    }
                }
        }
    }

    // ---- the row cap: exactly met and exceeded by one (the rule itself: nt is odd, so M nt S never is 2^21 through the call), the
    // largest and the smallest tables the call's other bounds allow on either side of it
    {
        const int64_t cap = MCL_REFINE_SEQ_MAX_ROWS;
        CHECK(cap == 1 << 21);
        CHECK(mcl_host::refine_sequence_rows_refused(4096, 32, 16).empty());                       // == cap
        CHECK(mcl_host::refine_sequence_rows_refused(cap, 1, 1).empty());
        CHECK(!mcl_host::refine_sequence_rows_refused(cap + 1, 1, 1).empty());
        CHECK(!mcl_host::refine_sequence_rows_refused(4096, 32767, 16).empty());                   // the largest product: no overflow
        const std::string why = mcl_host::refine_sequence_rows_refused(9, 32767, 16);
        CHECK(why.find("2097152") != std::string::npos && why.find("9 seeds") != std::string::npos &&
              why.find("32767 window headings") != std::string::npos && why.find("16 scans") != std::string::npos);
        CHECK(mcl_host::refine_sequence_rows_refused(4096, 21, 16).empty());                       // 1 376 256
        c.half_xy = 0; c.half_theta = 16383;
        const std::vector<double> seeds(3 * 9, 0.25), rel(3 * 16, 0.0);
        std::vector<double> big((size_t)4 * 32767 * 16 * 3 + 1, 77.0);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds.data(), 4, rel.data(), 16, big.data(), big.size() - 1) == MCL_OK);    // 2 097 088 rows
        CHECK(big[big.size() - 1] == 77.0 && big[big.size() - 2] == 0.25 + 16383.0 * c.step_theta_rad);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds.data(), 5, rel.data(), 16, big.data(), (size_t)5 * 32767 * 16 * 3) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds.data(), 9, rel.data(), 16, big.data(), (size_t)9 * 32767 * 16 * 3) == MCL_ERR_INVALID_ARG);
    }

    // ---- every refusal
    {
        mcl_default_refine_config(&c);
        c.half_theta = 1;
        double seeds[6] = {0.0, 1.0, 2.0, 3.0, 0.1, 0.2}, rel[3 * (MCL_SEARCH_MAX_SCANS + 1)] = {0.0}, out[2 * 3 * (MCL_SEARCH_MAX_SCANS + 1) * 3];
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, 2, out, 36) == MCL_OK);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, 0, out, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, -1, out, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, MCL_SEARCH_MAX_SCANS + 1, out, (size_t)18 * (MCL_SEARCH_MAX_SCANS + 1)) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 0, rel, 2, out, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, -1, rel, 2, out, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 4097, rel, 2, out, (size_t)4097 * 18) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, nullptr, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, nullptr, 2, out, 36) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, 2, nullptr, 36) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(nullptr, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);      // the defaults: nt = 21
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
            for (int i = 0; i < 6; ++i) {
                const double keep = rel[i];
                rel[i] = bad;
                CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
                rel[i] = keep;
                const double keep_seed = seeds[i];
                seeds[i] = bad;
                CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
                seeds[i] = keep_seed;
            }
        }
        mcl_refine_config_t b = c;
        b.half_theta = -1;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        b = c; b.half_xy = -1;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        b = c; b.step_theta_rad = 0.0;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        b = c; b.step_xy_cells = NAN;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        b = c; b.beam_stride = 0;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        b = c; b.reserved[2] = 1;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, 36) == MCL_ERR_INVALID_ARG);
        b = c; b.half_xy = 0; b.half_theta = 16384;
        CHECK(mcl_host_refine_sequence_offsets(&b, seeds, 2, rel, 2, out, (size_t)2 * 32769 * 2 * 3) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_refine_sequence_offsets(&c, seeds, 2, rel, 2, out, 36) == MCL_OK);
    }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
