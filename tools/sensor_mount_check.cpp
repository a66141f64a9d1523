// sensor_mount_check.cpp -- mcl_host_sensor_mount, mcl_host_sensor_unmount and mcl_host_sensor_mount_cov (rules
// SM1 / SM2) over their boundary cases and refusals, as a stand-alone host program for a sanitizer build: no device is opened.
// Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/sensor_mount_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o sensor_mount_check
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

// a fixed sequence in [0, 1): no library generator, the same poses everywhere
static double unit(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); }

// the bound of tests/test_sensor_mount_host.py: three roundings and a libm sincos within 1 ulp, about 4x in hand
static double bound(const double m[3], double coord) { return std::ldexp(std::fabs(coord) + std::fabs(m[0]) + std::fabs(m[1]), -50); }

int main()
{
    const double two_pi = 2.0 * M_PI;
    const int64_t n = 1000;
    std::vector<double> p(3 * n), s(3 * n), b(3 * n);
    uint64_t seed = 12345;
    for (int64_t i = 0; i < n; ++i) {
        p[i] = -60.0 + 120.0 * unit(seed);
        p[n + i] = -45.0 + 90.0 * unit(seed);
        p[2 * n + i] = -M_PI + two_pi * unit(seed);
    }
    p[2 * n + 0] = M_PI; p[2 * n + 1] = -M_PI; p[2 * n + 2] = 0.0; p[2 * n + 3] = -0.0;

    // the zero mount, either sign of zero: the identity, bit for bit, both ways
    const double zeros[2][3] = {{0.0, 0.0, 0.0}, {-0.0, 0.0, -0.0}};
    for (const auto &z : zeros) {
        CHECK(mcl_host_sensor_mount(z, p.data(), n, s.data()) == MCL_OK);
        CHECK(mcl_host_sensor_unmount(z, p.data(), n, b.data()) == MCL_OK);
        for (int64_t i = 0; i < 2 * n; ++i) CHECK(s[i] == p[i] && b[i] == p[i]);
        for (int64_t i = 2 * n; i < 3 * n; ++i) CHECK(s[i] == p[i] && b[i] == p[i]);
    }

    // SM2 against its statement, and unmount o mount, for the mounts of the tests and mtheta = +-2 pi (accepted)
    const double mounts[5][3] = {{0.27, 0.0, 0.0}, {-0.4, 0.3, 2.5}, {0.0, 0.0, -M_PI}, {0.1, -0.2, two_pi}, {0.1, -0.2, -two_pi}};
    for (const auto &m : mounts) {
        CHECK(mcl_host_sensor_mount(m, p.data(), n, s.data()) == MCL_OK);
        CHECK(mcl_host_sensor_unmount(m, s.data(), n, b.data()) == MCL_OK);
        for (int64_t i = 0; i < n; ++i) {
            const double x = p[i], y = p[n + i], th = p[2 * n + i];
            const double sn = std::sin(th), cs = std::cos(th);
            const double xs = x + (cs * m[0] - sn * m[1]), ys = y + (sn * m[0] + cs * m[1]);
            CHECK(bits(s[2 * n + i]) == bits(th + m[2]));
            CHECK(std::fabs(s[i] - xs) <= bound(m, xs) && std::fabs(s[n + i] - ys) <= bound(m, ys));
            CHECK(std::fabs(b[i] - x) <= 2.0 * bound(m, x) && std::fabs(b[n + i] - y) <= 2.0 * bound(m, y));
            CHECK(std::fabs(b[2 * n + i] - th) <= std::ldexp(std::fabs(th) + std::fabs(m[2]), -52));
        }
        // one pose, in place of many
        double one[3] = {p[5], p[n + 5], p[2 * n + 5]}, out[3];
        CHECK(mcl_host_sensor_mount(m, one, 1, out) == MCL_OK && bits(out[0]) == bits(s[5]) && bits(out[2]) == bits(s[2 * n + 5]));
    }

    // the covariance map against a central-difference Jacobian of the map itself, both directions
    for (const auto &m : mounts) {
        for (int to_base = 0; to_base < 2; ++to_base) {
            const double pose[3] = {1.25, -0.75, 0.9};
            const double cov[9] = {0.04, 0.01, 0.002, 0.01, 0.09, -0.003, 0.002, -0.003, 0.01};
            double got[9];
            CHECK(mcl_host_sensor_mount_cov(m, pose, cov, to_base, got) == MCL_OK);
            double J[9];
            const double h = 1e-6;
            for (int k = 0; k < 3; ++k) {
                double lo[3] = {pose[0], pose[1], pose[2]}, hi[3] = {pose[0], pose[1], pose[2]}, flo[3], fhi[3];
                lo[k] -= h; hi[k] += h;
                CHECK((to_base ? mcl_host_sensor_unmount : mcl_host_sensor_mount)(m, lo, 1, flo) == MCL_OK);
                CHECK((to_base ? mcl_host_sensor_unmount : mcl_host_sensor_mount)(m, hi, 1, fhi) == MCL_OK);
                for (int r = 0; r < 3; ++r) J[r * 3 + k] = (fhi[r] - flo[r]) / (2.0 * h);
            }
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) {
                    double want = 0.0;
                    for (int a = 0; a < 3; ++a)
                        for (int c = 0; c < 3; ++c) want += J[r * 3 + a] * cov[a * 3 + c] * J[q * 3 + c];
                    // the difference quotient: h^2 truncation and 1e-16 / h of cancellation, on entries of order 0.1
                    CHECK(std::fabs(got[r * 3 + q] - want) <= 1e-8);
                    CHECK(bits(got[r * 3 + q]) == bits(got[q * 3 + r]) || std::fabs(got[r * 3 + q] - got[q * 3 + r]) <= 1e-17);
                }
        }
    }

    // refusals: SM1, null pointers, counts
    const double bad[6][3] = {{NAN, 0, 0}, {0, INFINITY, 0}, {0, 0, -INFINITY}, {0, 0, NAN}, {0, 0, std::nextafter(two_pi, 7.0)},
                              {0, 0, -std::nextafter(two_pi, 7.0)}};
    const double ok[3] = {0.1, 0.2, 0.5}, pose0[3] = {0.0, 0.0, 0.0}, eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    double o9[9];
    for (const auto &m : bad) {
        CHECK(mcl_host_sensor_mount(m, p.data(), n, s.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_sensor_unmount(m, p.data(), n, s.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_sensor_mount_cov(m, pose0, eye, 0, o9) == MCL_ERR_INVALID_ARG);
    }
    CHECK(mcl_host_sensor_mount(nullptr, p.data(), n, s.data()) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount(ok, nullptr, n, s.data()) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount(ok, p.data(), n, nullptr) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount(ok, p.data(), 0, s.data()) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_unmount(ok, p.data(), -1, s.data()) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount_cov(ok, nullptr, eye, 0, o9) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount_cov(ok, pose0, nullptr, 0, o9) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount_cov(ok, pose0, eye, 0, nullptr) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_sensor_mount_cov(ok, pose0, eye, 2, o9) == MCL_ERR_INVALID_ARG);
    const double nan_pose[3] = {0.0, NAN, 0.0};
    CHECK(mcl_host_sensor_mount_cov(ok, nan_pose, eye, 1, o9) == MCL_ERR_INVALID_ARG);
    // a non-finite pose is not refused by the transform: it gives what the operations give
    const double inf_pose[3] = {INFINITY, 1.0, NAN};
    double out[3];
    CHECK(mcl_host_sensor_mount(ok, inf_pose, 1, out) == MCL_OK && std::isnan(out[0]) && std::isnan(out[1]) && std::isnan(out[2]));
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
