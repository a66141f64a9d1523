// recovery_proposal_check.cpp -- mcl_host_recovery_proposal (rules P1 / P2) over its boundary and refusal cases,
// as a stand-alone host program for a sanitizer build: no device is opened.  Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/recovery_proposal_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o recovery_proposal_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static const uint64_t TWO53 = 1ull << 53;

// M components: means (c, -c, 0.1), covariances diag(0.25, 0.25, 0.01); exactly-sized vectors, so that one element too many is seen
struct Mix {
    std::vector<double> means, covs, w, fac;
    std::vector<uint64_t> thr;
    explicit Mix(int M) : means(3 * (size_t)M), covs(9 * (size_t)M, 0.0), w((size_t)M, 1.0), fac(9 * (size_t)M, -7.0), thr((size_t)M, 7u)
    {
        for (int c = 0; c < M; ++c) {
            means[3 * (size_t)c] = c; means[3 * (size_t)c + 1] = -c; means[3 * (size_t)c + 2] = 0.1;
            covs[9 * (size_t)c] = 0.25; covs[9 * (size_t)c + 4] = 0.25; covs[9 * (size_t)c + 8] = 0.01;
        }
    }
    int run(bool with_w = true) { return mcl_host_recovery_proposal((int32_t)thr.size(), means.data(), covs.data(), with_w ? w.data() : nullptr, thr.data(), fac.data()); }
    bool untouched() const
    {
        for (uint64_t t : thr) if (t != 7u) return false;
        for (double f : fac) if (f != -7.0) return false;
        return true;
    }
};

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // M = 1: one range, the whole of it
    {
        Mix m(1);
        CHECK(m.run() == MCL_OK && m.thr[0] == TWO53);
        CHECK(m.fac[0] == 0.0 && m.fac[2] == 0.1 && m.fac[3] == 0.5 && m.fac[4] == 0.0 && m.fac[5] == 0.5 && m.fac[8] == 0.1);
        m.w[0] = 1e-300;
        CHECK(m.run() == MCL_OK && m.thr[0] == TWO53);
        CHECK(mcl_host_recovery_proposal(1, m.means.data(), m.covs.data(), nullptr, nullptr, nullptr) == MCL_OK);
    }
    // M = 4096, the most: equal weights give t_k = (k + 1) 2^41; with and without a weight array
    {
        Mix m(4096);
        CHECK(m.run() == MCL_OK);
        bool ok = true;
        for (int k = 0; k < 4096; ++k) ok = ok && m.thr[(size_t)k] == (uint64_t)(k + 1) << 41;
        CHECK(ok);
        Mix n(4096);
        CHECK(n.run(false) == MCL_OK && n.thr == m.thr && n.fac == m.fac);
        CHECK(m.fac[9 * 4095] == 4095.0 && m.fac[9 * 4095 + 8] == 0.1);
        Mix big(4097);
        CHECK(big.run() == MCL_ERR_INVALID_ARG && big.untouched());
        CHECK(mcl_host_recovery_proposal(0, m.means.data(), m.covs.data(), nullptr, m.thr.data(), m.fac.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_recovery_proposal(-1, m.means.data(), m.covs.data(), nullptr, m.thr.data(), m.fac.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_recovery_proposal(0x7fffffff, m.means.data(), m.covs.data(), nullptr, nullptr, nullptr) == MCL_ERR_INVALID_ARG);
    }
    // leading and trailing zero weights: empty ranges, the last threshold still 2^53
    {
        Mix m(5);
        m.w = {0.0, 0.0, 1.0, 3.0, 0.0};
        CHECK(m.run() == MCL_OK);
        CHECK(m.thr[0] == 0 && m.thr[1] == 0 && m.thr[2] == TWO53 / 4 && m.thr[3] == TWO53 && m.thr[4] == TWO53);
        m.w = {0.0, 0.0, 0.0, 0.0, 5e-324};
        CHECK(m.run() == MCL_OK && m.thr[3] == 0 && m.thr[4] == TWO53);
        m.w = {5e-324, 0.0, 0.0, 0.0, 0.0};
        CHECK(m.run() == MCL_OK && m.thr[0] == TWO53 && m.thr[4] == TWO53);
        Mix z(3);
        z.w = {0.0, 0.0, 0.0};
        CHECK(z.run() == MCL_ERR_INVALID_ARG && z.untouched());
    }
    // weights whose sum overflows (each one finite), a weight that is not finite or negative
    {
        Mix m(3);
        m.w = {1.5e308, 1.5e308, 1.0};
        CHECK(m.run() == MCL_ERR_INVALID_ARG && m.untouched());
        m.w = {1.0e308, 7.0e307, 0.0};                       // 1.7e308: still finite
        CHECK(m.run() == MCL_OK && m.thr[1] == TWO53 && m.thr[2] == TWO53);
        const double bad[] = {-1.0, -5e-324, inf, -inf, nan};
        for (double b : bad)
            for (int at = 0; at < 3; ++at) {
                Mix q(3);
                q.w[(size_t)at] = b;
                CHECK(q.run() == MCL_ERR_INVALID_ARG && q.untouched());
            }
    }
    // covariances: singular ones are allowed (zero pivots), everything G1 refuses is refused
    {
        Mix m(3);
        for (int i = 0; i < 9; ++i) m.covs[(size_t)i] = 0.0;                                     // the zero matrix: a point
        m.covs[9 + 8] = 0.0;                                                                     // no heading uncertainty
        const double r1[9] = {1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.5};                      // rank 2 in x, y
        for (int i = 0; i < 9; ++i) m.covs[18 + (size_t)i] = r1[i];
        CHECK(m.run() == MCL_OK);
        bool zero = true;
        for (int i = 3; i < 9; ++i) zero = zero && m.fac[(size_t)i] == 0.0;
        CHECK(zero);
        CHECK(m.fac[9 + 3] == 0.5 && m.fac[9 + 5] == 0.5 && m.fac[9 + 8] == 0.0);
        CHECK(m.fac[18 + 3] == 1.0 && m.fac[18 + 4] == 1.0 && m.fac[18 + 5] == 0.0 && m.fac[18 + 8] == std::sqrt(0.5));
        for (int at = 0; at < 3; ++at) {
            Mix q(3);
            q.covs[9 * (size_t)at + 4] = -0.25;                                                  // negative pivot
            CHECK(q.run() == MCL_ERR_INVALID_ARG && q.untouched());
            Mix s(3);
            s.covs[9 * (size_t)at + 1] = 0.1;                                                    // not symmetric
            CHECK(s.run() == MCL_ERR_INVALID_ARG && s.untouched());
            Mix f(3);
            f.covs[9 * (size_t)at + 8] = nan;
            CHECK(f.run() == MCL_ERR_INVALID_ARG && f.untouched());
            Mix mu(3);
            mu.means[3 * (size_t)at + 2] = inf;
            CHECK(mu.run() == MCL_ERR_INVALID_ARG && mu.untouched());
        }
    }
    // null pointers
    {
        Mix m(2);
        CHECK(mcl_host_recovery_proposal(2, nullptr, m.covs.data(), nullptr, m.thr.data(), m.fac.data()) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_recovery_proposal(2, m.means.data(), nullptr, nullptr, m.thr.data(), m.fac.data()) == MCL_ERR_INVALID_ARG);
        CHECK(m.untouched());
        CHECK(mcl_host_recovery_proposal(2, m.means.data(), m.covs.data(), nullptr, m.thr.data(), nullptr) == MCL_OK && m.thr[0] == TWO53 / 2);
        CHECK(mcl_host_recovery_proposal(2, m.means.data(), m.covs.data(), nullptr, nullptr, m.fac.data()) == MCL_OK && m.fac[9] == 1.0);
    }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
