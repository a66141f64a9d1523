// scan_deskew_check.cpp -- mcl_host_scan_motion_offsets (rules DM1 / DM2) and the setter's host-side table
// formation (mcl_host_beam_offset_table: DS1; mcl_host_beam_offset_pairs: DS5's pairs) over their boundary cases and refusals, as a
// stand-alone host program for a sanitizer build: no device is opened.  Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/scan_deskew_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o scan_deskew_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
static uint32_t bitsf(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

// DM1 / DM2 restated: the statement the function is held to (tests/deskew_ref.py's, in C)
static void statement(const double mo[3], const double *m, double tau, double o[3])
{
    const double th = tau * mo[2];
    double A, Bc;
    if (std::fabs(th) < 1e-8) { A = 1.0 - th * th / 6.0; Bc = th / 2.0; }
    else { A = std::sin(th) / th; Bc = (1.0 - std::cos(th)) / th; }
    o[0] = tau * (A * mo[0] - Bc * mo[1]) + 0.0; o[1] = tau * (Bc * mo[0] + A * mo[1]) + 0.0; o[2] = th + 0.0;
    if (!m) return;
    const double s = std::sin(o[2]), c = std::cos(o[2]);
    const double xs = o[0] + (c * m[0] - s * m[1]), ys = o[1] + (s * m[0] + c * m[1]);
    const double sm = std::sin(m[2]), cm = std::cos(m[2]);
    const double ex = xs - m[0], ey = ys - m[1];
    o[0] = (cm * ex + sm * ey) + 0.0; o[1] = (cm * ey - sm * ex) + 0.0;
}

int main()
{
    const double mounts[4][3] = {{0.27, 0.0, 0.0}, {-0.4, 0.3, 2.5}, {0.1, -0.2, M_PI}, {0.1, -0.2, -M_PI}};        // (two turned by pi)
    const double motions[5][3] = {{0.175, 0.0, 0.0}, {0.1, -0.05, 0.0}, {0.0, 0.0, 0.12}, {0.175, 0.02, 0.12}, {-0.2, 0.04, -0.09}};
    const double t_refs[3] = {0.0, 0.5, 1.0};
    const int32_t sizes[4] = {1, 2, 61, 1081};

    // DM1 / DM2 against the statement, stamps defaulted and given, every mount and no mount, B = 1 among the sizes
    for (int32_t B : sizes) {
        std::vector<double> got(3 * (size_t)B), again(3 * (size_t)B), t((size_t)B);
        for (int32_t j = 0; j < B; ++j) t[j] = B > 1 ? (double)j / (double)(B - 1) : 0.0;
        for (const auto &mo : motions)
            for (double t_ref : t_refs)
                for (int mi = -1; mi < 4; ++mi) {
                    const double *m = mi < 0 ? nullptr : mounts[mi];
                    CHECK(mcl_host_scan_motion_offsets(mo, m, nullptr, t_ref, B, got.data()) == MCL_OK);
                    CHECK(mcl_host_scan_motion_offsets(mo, m, t.data(), t_ref, B, again.data()) == MCL_OK);
                    for (int32_t j = 0; j < B; ++j) {
                        double want[3];
                        statement(mo, m, t[j] - t_ref, want);
                        for (int k = 0; k < 3; ++k) {
                            CHECK(bits(got[(size_t)k * B + j]) == bits(want[k]));          // the same operations by the same libm
                            CHECK(bits(again[(size_t)k * B + j]) == bits(got[(size_t)k * B + j]));
                        }
                        CHECK(bits(got[2 * (size_t)B + j]) == bits((t[j] - t_ref) * mo[2] + 0.0));   // the heading: theta whatever the mount
                    }
                }
    }

    // a zero twist: a table of +0.0, whatever the mount, the stamps and the reference time
    {
        const double zero[3] = {0.0, -0.0, 0.0};
        std::vector<double> got(3 * 61);
        for (double t_ref : t_refs)
            for (int mi = -1; mi < 4; ++mi) {
                CHECK(mcl_host_scan_motion_offsets(zero, mi < 0 ? nullptr : mounts[mi], nullptr, t_ref, 61, got.data()) == MCL_OK);
                for (double v : got) CHECK(bits(v) == 0);
            }
    }

    // the series branch on both sides of 1e-8, either sign, and exactly at it
    {
        const double w = 1e-3, mo[3] = {0.175, 0.02, w};
        const double th[11] = {0.0, 0.5e-8, -0.5e-8, 0.99e-8, -0.99e-8, 1e-8, -1e-8, 1.01e-8, -1.01e-8, 2e-8, -2e-8};
        double t[11], got[33];
        for (int j = 0; j < 11; ++j) t[j] = th[j] / w;
        CHECK(mcl_host_scan_motion_offsets(mo, nullptr, t, 0.0, 11, got) == MCL_OK);
        for (int j = 0; j < 11; ++j) {
            double want[3];
            statement(mo, nullptr, t[j], want);
            for (int k = 0; k < 3; ++k) CHECK(bits(got[k * 11 + j]) == bits(want[k]));
            // either branch is the small-angle limit tau (u - theta v / 2) to first order in theta; beyond the series 1 - cos theta is
            // formed of a cosine that rounds to 1 within 2^-53, so Bc is within 2^-53 / |theta| <= 1.2e-8 of theta / 2
            CHECK(std::fabs(got[j] - t[j] * (mo[0] - 0.5 * th[j] * mo[1])) <= std::fabs(t[j]) * (std::ldexp(std::fabs(mo[0]), -50) + 1.2e-8 * std::fabs(mo[1])));
        }
    }

    // DS1: one add in double, one rounding to float; the pair of the widened float; zero offsets give the angles back
    {
        const int32_t B = 61;
        std::vector<float> ang(B), eff(B);
        std::vector<double> off(3 * B), dirs(2 * B), pairs(2 * B);
        for (int32_t j = 0; j < B; ++j) ang[j] = (float)(-2.356194490192345 + j * (4.71238898038469 / 60.0));
        CHECK(mcl_host_scan_motion_offsets(motions[3], mounts[1], nullptr, 1.0, B, off.data()) == MCL_OK);
        CHECK(mcl_host_beam_offset_table(ang.data(), off.data(), B, eff.data(), dirs.data()) == MCL_OK);
        for (int32_t j = 0; j < B; ++j) {
            const float want = (float)((double)ang[j] + off[2 * B + j]);
            CHECK(bitsf(eff[j]) == bitsf(want));
            CHECK(bits(dirs[j]) == bits(std::cos((double)want)) && bits(dirs[B + j]) == bits(std::sin((double)want)));
        }
        std::vector<float> only(B);
        CHECK(mcl_host_beam_offset_table(ang.data(), off.data(), B, only.data(), nullptr) == MCL_OK);      // either output alone
        CHECK(mcl_host_beam_offset_table(ang.data(), off.data(), B, nullptr, dirs.data()) == MCL_OK);
        for (int32_t j = 0; j < B; ++j) CHECK(bitsf(only[j]) == bitsf(eff[j]));
        std::vector<double> zeros(3 * B, 0.0);
        CHECK(mcl_host_beam_offset_table(ang.data(), zeros.data(), B, eff.data(), nullptr) == MCL_OK);
        for (int32_t j = 0; j < B; ++j) CHECK(bitsf(eff[j]) == bitsf(ang[j]));
        // DS5: ((ox + r c') / res, (oy + r s') / res) through the reciprocal; readings of 0, NaN and +inf give what the operations give
        std::vector<float> r(B);
        for (int32_t j = 0; j < B; ++j) r[j] = 0.25f * (float)j;
        r[3] = NAN; r[4] = INFINITY; r[5] = 0.0f;
        const double res = (double)0.05f, inv = 1.0 / res;
        CHECK(mcl_host_beam_offset_pairs(r.data(), off.data(), dirs.data(), B, res, pairs.data()) == MCL_OK);
        for (int32_t j = 0; j < B; ++j) {
            const double wx = (off[j] + (double)r[j] * dirs[j]) * inv, wy = (off[B + j] + (double)r[j] * dirs[B + j]) * inv;
            CHECK((std::isnan(wx) && std::isnan(pairs[j])) || bits(pairs[j]) == bits(wx));
            CHECK((std::isnan(wy) && std::isnan(pairs[B + j])) || bits(pairs[B + j]) == bits(wy));
        }
        // one beam
        const double one_off[3] = {0.1, -0.05, 0.02};
        float one_eff;
        double one_dirs[2], one_pair[2];
        CHECK(mcl_host_beam_offset_table(ang.data(), one_off, 1, &one_eff, one_dirs) == MCL_OK);
        CHECK(bitsf(one_eff) == bitsf((float)((double)ang[0] + 0.02)));
        CHECK(mcl_host_beam_offset_pairs(r.data() + 8, one_off, one_dirs, 1, res, one_pair) == MCL_OK);
        CHECK(bits(one_pair[0]) == bits((0.1 + (double)r[8] * one_dirs[0]) * inv));

        // refusals of the table formation
        std::vector<double> bad = off;
        bad[B + 7] = NAN;
        CHECK(mcl_host_beam_offset_table(ang.data(), bad.data(), B, eff.data(), dirs.data()) == MCL_ERR_INVALID_ARG);
        bad[B + 7] = 0.0; bad[2 * B] = -INFINITY;
        CHECK(mcl_host_beam_offset_table(ang.data(), bad.data(), B, eff.data(), dirs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_table(nullptr, off.data(), B, eff.data(), dirs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_table(ang.data(), nullptr, B, eff.data(), dirs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_table(ang.data(), off.data(), 0, eff.data(), dirs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_table(ang.data(), off.data(), B, nullptr, nullptr) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_pairs(nullptr, off.data(), dirs.data(), B, res, pairs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_pairs(r.data(), off.data(), dirs.data(), B, 0.0, pairs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_pairs(r.data(), off.data(), dirs.data(), B, NAN, pairs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_pairs(r.data(), off.data(), dirs.data(), -1, res, pairs.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_offset_pairs(r.data(), off.data(), dirs.data(), B, res, nullptr) == MCL_ERR_INVALID_ARG);
    }

    // refusals of the constant-twist rule: non-finite inputs, a mount SM1 refuses, null pointers, n_beams < 1
    {
        const double ok[3] = {0.175, 0.02, 0.12};
        double out[3 * 61], t[61];
        for (int j = 0; j < 61; ++j) t[j] = j / 60.0;
        const double nonfinite[3] = {NAN, INFINITY, -INFINITY};
        for (double v : nonfinite) {
            for (int k = 0; k < 3; ++k) {
                double mo[3] = {ok[0], ok[1], ok[2]}, m[3] = {0.1, 0.2, 0.3};
                mo[k] = v;
                CHECK(mcl_host_scan_motion_offsets(mo, nullptr, nullptr, 1.0, 61, out) == MCL_ERR_INVALID_ARG);
                m[k] = v;
                CHECK(mcl_host_scan_motion_offsets(ok, m, nullptr, 1.0, 61, out) == MCL_ERR_INVALID_ARG);
            }
            CHECK(mcl_host_scan_motion_offsets(ok, nullptr, nullptr, v, 61, out) == MCL_ERR_INVALID_ARG);
            double tb[61];
            std::memcpy(tb, t, sizeof t);
            tb[60] = v;
            CHECK(mcl_host_scan_motion_offsets(ok, nullptr, tb, 1.0, 61, out) == MCL_ERR_INVALID_ARG);
        }
        const double wide[3] = {0.0, 0.0, std::nextafter(2.0 * M_PI, 7.0)};
        CHECK(mcl_host_scan_motion_offsets(ok, wide, nullptr, 1.0, 61, out) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_scan_motion_offsets(nullptr, nullptr, nullptr, 1.0, 61, out) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_scan_motion_offsets(ok, nullptr, nullptr, 1.0, 61, nullptr) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_scan_motion_offsets(ok, nullptr, nullptr, 1.0, 0, out) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_scan_motion_offsets(ok, nullptr, nullptr, 1.0, -5, out) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_scan_motion_offsets(ok, nullptr, t, 0.5, 61, out) == MCL_OK);
    }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
