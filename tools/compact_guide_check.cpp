// compact_guide_check.cpp -- the guide of the compact parent list (csrc/mcl_compact_guide.h) through mcl_host_compact_guide and
// mcl_host_compact_search, over the lists of tests/test_compact_guide_host.py: sizes around the group of 64, equal, skewed and
// one-heavy weights, totals below 2^m, beside and at a power of two; every search result against a linear upper_bound, every
// guide word against its definition, from buffers of the exact size (bmax + 2 words) so that a sanitizer sees any word too many.
// A stand-alone host program for a sanitizer build: no device is opened.  Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/compact_guide_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o compact_guide_check
// It prints "ok" and returns 0, or says which case failed.
#include "../monte_carlo_localization_amd/csrc/mcl_host_math.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

static int failures = 0;
static long long cur_n = 0, cur_total = 0;
static int cur_m = 0;
#define CHECK(cond) do { if (!(cond)) { if (failures < 20) std::printf("FAILED line %d: %s (n %lld, total %lld, m %d)\n", __LINE__, #cond, cur_n, cur_total, cur_m); ++failures; } } while (0)

int main()
{
    std::mt19937_64 rng(12345);
    const int64_t sizes[] = {1, 2, 63, 64, 65, 127, 4097};
    const uint64_t totals[] = {70001ull, (1ull << 40) - 1, 1ull << 40, (1ull << 58) + 977};
    for (int m : {8, 17})
        for (int64_t n : sizes)
            for (uint64_t total : totals)
                for (int pattern = 0; pattern < 3; ++pattern) {
                    cur_n = n; cur_total = (long long)total; cur_m = m;
                    // weights >= 1 that add up to the total: equal shares, shares spread over twelve octaves, or one entry with all but n - 1
                    std::vector<uint64_t> q((size_t)n, 1ull);
                    uint64_t left = total - (uint64_t)n;
                    if (pattern < 2 && n > 1) {
                        std::vector<double> w((size_t)n);
                        double sum = 0.0;
                        for (auto &v : w) { v = pattern == 0 ? 1.0 : std::ldexp(1.0, (int)(rng() % 12)); sum += v; }
                        for (size_t i = 0; i < q.size(); ++i) { const uint64_t add = (uint64_t)((double)(total - (uint64_t)n) * 0.999 * (w[i] / sum)); q[i] += add; left -= add; }
                    }
                    q[(size_t)(rng() % (uint64_t)n)] += left;
                    std::vector<uint64_t> ccdf((size_t)n);
                    uint64_t c = 0;
                    for (size_t i = 0; i < q.size(); ++i) { c += q[i]; ccdf[i] = c; }
                    CHECK(c == total);
                    int32_t s = -1; uint32_t bmax = 0; int64_t written = -1;
                    CHECK(mcl_host_compact_guide(ccdf.data(), n, total, m, nullptr, 0, &s, &bmax, nullptr) == MCL_OK);
                    std::vector<uint32_t> guide((size_t)bmax + 2, 0xffffffffu);
                    CHECK(mcl_host_compact_guide(ccdf.data(), n, total, m, guide.data(), (size_t)bmax + 1, &s, &bmax, &written) == MCL_OK);
                    CHECK(written == (int64_t)bmax + 1 && guide[(size_t)bmax + 1] == 0xffffffffu && guide[0] == 0u);
                    for (uint32_t b = 0; b <= bmax; ++b) {
                        const uint64_t bound = (uint64_t)b << s;
                        const uint32_t want = (uint32_t)(std::lower_bound(ccdf.begin(), ccdf.end(), bound) - ccdf.begin());
                        if (guide[b] != want) { CHECK(guide[b] == want); break; }
                    }
                    std::vector<uint64_t> thr = {0ull, total - 1};
                    for (uint64_t v : ccdf) for (int d = -1; d <= 1; ++d) if (v + (uint64_t)d < total) thr.push_back(v + (uint64_t)d);
                    for (int k = 0; k < 20000; ++k) thr.push_back(rng() % total);
                    std::vector<int64_t> pos(thr.size(), -1);
                    CHECK(mcl_host_compact_search(ccdf.data(), n, guide.data(), guide.size(), s, bmax, thr.data(), (int64_t)thr.size(), pos.data()) == MCL_OK);
                    for (size_t i = 0; i < thr.size(); ++i) {
                        const int64_t want = std::min<int64_t>(std::upper_bound(ccdf.begin(), ccdf.end(), thr[i]) - ccdf.begin(), n - 1);
                        if (pos[i] != want) { CHECK(pos[i] == want); break; }
                    }
                    // a threshold at or beyond the total selects the last entry, as the two-level search does
                    const uint64_t far_thr[2] = {total, ~0ull};
                    int64_t far_pos[2] = {-1, -1};
                    CHECK(mcl_host_compact_search(ccdf.data(), n, guide.data(), guide.size(), s, bmax, far_thr, 2, far_pos) == MCL_OK);
                    CHECK(far_pos[0] == n - 1 && far_pos[1] == n - 1);
                }
    std::printf(failures ? "%d failures\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
