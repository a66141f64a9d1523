// beam_skip_check.cpp -- mcl_host_beam_skip_thresholds and mcl_host_beam_skip_plan (rules BS1 / BS3 / BS4) over
// their boundary cases and refusals, as a stand-alone host program for a sanitizer build: no device is opened.  Build it together
// with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/beam_skip_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o beam_skip_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// BS3 / BS4 by their definitions: the least integer that passes the float comparison
static int64_t min_count_ref(double t, int64_t n)
{
    for (int64_t c = 1; c <= n; ++c)
        if ((double)c / (double)n > t) return c;
    return n + 1;
}

static int32_t min_skipped_ref(double et, int32_t n_used)
{
    for (int32_t s = 0; s <= n_used; ++s)
        if ((double)s >= et * (double)n_used) return s;
    return n_used + 1;
}

int main()
{
    mcl_beam_skip_config_t c;
    mcl_default_beam_skip_config(&c);
    mcl_default_beam_skip_config(nullptr);
    CHECK(c.distance_m == 0.5 && c.threshold == 0.3 && c.error_threshold == 0.9 && c.reserved[0] == 0 && c.reserved[1] == 0);
    int32_t ka = -1, ms = -1;
    int64_t mc = -1;

    // Ka: K's expression, held at 65536; outputs may be NULL
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 2000, 1039, &ka, &mc, &ms) == MCL_OK);
    {
        const double q = 0.5 / (double)0.05f;
        CHECK(ka == (int32_t)std::ceil(q * q));
    }
    CHECK(mc == min_count_ref(0.3, 2000) && ms == min_skipped_ref(0.9, 1039));
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 2000, 1039, nullptr, nullptr, nullptr) == MCL_OK);
    c.distance_m = 1e9;
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 1, 0, &ka, &mc, &ms) == MCL_OK && ka == 65536);
    c.distance_m = 0.5;

    // min_count: n = 1, threshold 0 and 1, threshold * n an integer, thresholds one ulp either side of k / n
    const int64_t ns[] = {1, 2, 3, 10, 64, 2000, 8193};
    for (int64_t n : ns) {
        std::vector<double> ts = {0.0, 0.3, 1.0 / 3.0, 0.5, 1.0 - 1.0 / 9007199254740992.0, 1.0};
        for (int64_t k = 0; k <= n; k += (n > 64 ? n / 7 : 1)) {
            const double t = (double)k / (double)n;
            ts.push_back(t);
            ts.push_back(std::nextafter(t, 0.0));
            ts.push_back(std::nextafter(t, 2.0));
        }
        for (double t : ts) {
            if (!(t >= 0.0 && t <= 1.0)) continue;
            c.threshold = t;
            CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, n, 0, nullptr, &mc, nullptr) == MCL_OK && mc == min_count_ref(t, n));
        }
    }
    c.threshold = 1.0;
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 0x7fffffff, 0, nullptr, &mc, nullptr) == MCL_OK && mc == (int64_t)0x7fffffff + 1);
    c.threshold = 0.0;
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 0x7fffffff, 0, nullptr, &mc, nullptr) == MCL_OK && mc == 1);
    c.threshold = 0.3;

    // min_skipped: n_used = 0, error_threshold 0 and above 1, error_threshold * n_used an integer
    const int32_t nus[] = {0, 1, 2, 10, 59, 1039, 65536};
    const double ets[] = {0.0, 0.1, 0.5, 0.9, 1.0, std::nextafter(1.0, 2.0), 1.5, 2.0, 1e300};
    for (int32_t nu : nus)
        for (double et : ets) {
            c.error_threshold = et;
            CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 7, nu, nullptr, nullptr, &ms) == MCL_OK && ms == min_skipped_ref(et, nu));
            if (et == 0.0) CHECK(ms == 0);
            if (et > 1.0 && nu > 0) CHECK(ms == nu + 1);
        }
    c.error_threshold = 0.9;

    // the plan: counts at min_count - 1 and at min_count, the integrate_all flip at exactly min_skipped, all kept, all skipped
    {
        const int64_t n = 2000;
        const int32_t nu = 10;
        CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, n, nu, nullptr, &mc, &ms) == MCL_OK && ms == 9);
        std::vector<uint32_t> cnt(nu, (uint32_t)mc);
        std::vector<uint8_t> kept(nu, 7);
        int32_t sk = -1, all = -1;
        for (int32_t below = 0; below <= nu; ++below) {
            for (int32_t j = 0; j < nu; ++j) cnt[j] = (uint32_t)(j < below ? mc - 1 : mc);
            CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), nu, n, kept.data(), &sk, &all) == MCL_OK);
            CHECK(sk == below && all == (below >= ms));
            for (int32_t j = 0; j < nu; ++j) CHECK(kept[j] == ((all || j >= below) ? 1 : 2));
        }
        c.error_threshold = 2.0;                   // never integrates all: everything may be skipped
        for (int32_t j = 0; j < nu; ++j) cnt[j] = 0;
        CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), nu, n, kept.data(), &sk, &all) == MCL_OK && sk == nu && all == 0);
        for (int32_t j = 0; j < nu; ++j) CHECK(kept[j] == 2);
        c.error_threshold = 0.0;                   // always does
        for (int32_t j = 0; j < nu; ++j) cnt[j] = (uint32_t)n;
        CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), nu, n, kept.data(), &sk, &all) == MCL_OK && sk == 0 && all == 1);
        CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), nu, n, nullptr, nullptr, nullptr) == MCL_OK);
        c.error_threshold = 0.9;
        // no used beam: nothing to read, 0 >= 0 integrates all
        CHECK(mcl_host_beam_skip_plan(&c, nullptr, 0, n, nullptr, &sk, &all) == MCL_OK && sk == 0 && all == 1);
        CHECK(mcl_host_beam_skip_plan(&c, nullptr, 1, n, kept.data(), &sk, &all) == MCL_ERR_INVALID_ARG);
        // threshold 1 keeps nothing, threshold 0 keeps what any particle agrees with
        c.threshold = 1.0; c.error_threshold = 2.0;
        CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), nu, n, kept.data(), &sk, &all) == MCL_OK && sk == nu);
        c.threshold = 0.0;
        cnt[0] = 0; cnt[1] = 1;
        CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), nu, n, kept.data(), &sk, &all) == MCL_OK && sk == 1 && kept[0] == 2 && kept[1] == 1);
        // n = 1
        cnt[0] = 0; cnt[1] = 1;
        c.threshold = 0.3;
        CHECK(mcl_host_beam_skip_plan(&c, cnt.data(), 2, 1, kept.data(), &sk, &all) == MCL_OK && sk == 1 && kept[0] == 2 && kept[1] == 1);
    }

    // the refusals
    mcl_default_beam_skip_config(&c);
    const uint32_t one = 1;
    uint8_t k1 = 0;
    CHECK(mcl_host_beam_skip_thresholds(nullptr, 0.05f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_plan(nullptr, &one, 1, 10, &k1, nullptr, nullptr) == MCL_ERR_INVALID_ARG);
    const double bad_d[] = {0.0, -1.0, NAN, INFINITY}, bad_t[] = {-0.1, 1.1, NAN, INFINITY}, bad_e[] = {-0.1, NAN, INFINITY};
    for (double v : bad_d) {
        c.distance_m = v;
        CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_beam_skip_plan(&c, &one, 1, 10, &k1, nullptr, nullptr) == MCL_ERR_INVALID_ARG);
    }
    c.distance_m = 0.5;
    for (double v : bad_t) {
        c.threshold = v;
        CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    }
    c.threshold = 0.3;
    for (double v : bad_e) {
        c.error_threshold = v;
        CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    }
    c.error_threshold = 0.9;
    for (int i = 0; i < 2; ++i) {
        c.reserved[i] = 1;
        CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
        c.reserved[i] = 0;
    }
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.0f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, -0.05f, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, NAN, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, INFINITY, 10, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 0, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, -3, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, (int64_t)1 << 31, 1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, -1, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, 0x7fffffff, &ka, &mc, &ms) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_beam_skip_thresholds(&c, 0.05f, 10, 1, &ka, &mc, &ms) == MCL_OK);
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
