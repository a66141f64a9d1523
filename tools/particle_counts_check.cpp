// particle_counts_check.cpp -- the host functions whose arguments are particle counts, over the counts of tests/particle_sets.py:
// mcl_host_kld_target with round_to 1 and min_particles 1 (a KLD run may land on any size), pinned to one particle, and with the
// shrink rule at ragged current sizes; mcl_compact_chunk_bytes; and the chunk rule of the list exchange (compact_chunk_entries:
// the device group's and the communicator's).  A stand-alone host program for a sanitizer build: no device is opened.  Build it
// together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/particle_counts_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o particle_counts_check
// It prints "ok" and returns 0, or says which case failed.
#include "../monte_carlo_localization_amd/csrc/mcl_host_math.h"

#include <algorithm>
#include <cmath>
#include <cstdio>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s (n %lld, bins %lld)\n", __LINE__, #cond, (long long)cur_n, (long long)cur_bins); ++failures; } } while (0)
static int64_t cur_n = 0, cur_bins = 0;

// the family's counts, and the shard sizes and totals of its device groups
static const int64_t COUNTS[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4099, 8191, 8193, 12297, 16385};

// DESIGN.md §4.7 restated: (k - 1) / (2 err) * (1 - 2 / (9 (k - 1)) + sqrt(2 / (9 (k - 1))) z)^3, rounded up, from two bins on
static int64_t bound_ref(const mcl_kld_config_t &k, int64_t bins)
{
    if (bins <= 1) return k.max_particles;
    const double km1 = (double)(bins - 1), a = 2.0 / (9.0 * km1), b = 1.0 - a + std::sqrt(a) * k.z;
    const double n = std::ceil(km1 / (2.0 * k.err) * (b * b * b));
    if (!(n < (double)k.max_particles)) return k.max_particles;
    const int64_t r = k.round_to, up = ((int64_t)std::max(n, 0.0) + r - 1) / r * r;
    return std::min(std::max(up, k.min_particles), k.max_particles);
}

int main()
{
    // ---- targets at round_to 1, min_particles 1
    for (int64_t max_p : {(int64_t)8192, (int64_t)16385, (int64_t)1}) {
        mcl_kld_config_t k;
        mcl_default_kld_config(&k);
        k.min_particles = 1; k.max_particles = max_p; k.round_to = 1; k.shrink_permille = 1000;
        int64_t prev = 0, ragged = 0;
        for (int64_t bins = -1; bins <= 3000; ++bins) {
            cur_bins = bins;
            const int64_t want = bound_ref(k, bins);
            for (int64_t n : COUNTS) {
                cur_n = n;
                int64_t got = -1;
                CHECK(mcl_host_kld_target(&k, bins, n, &got) == MCL_OK);
                CHECK(got == want);                          // shrink_permille 1000: the target, whatever the current size
                CHECK(got >= 1 && got <= max_p);
            }
            if (bins >= 2) {
                CHECK(want >= prev);                         // more bins never ask for fewer particles
                ragged += (want < max_p && want % 16 != 0);
            }
            prev = bins >= 2 ? want : 0;
        }
        cur_bins = 2;
        int64_t two = -1;
        CHECK(mcl_host_kld_target(&k, 2, 4096, &two) == MCL_OK && two == std::min<int64_t>(max_p, bound_ref(k, 2)));
        if (max_p > 1) CHECK(ragged >= 100);                 // (round_to 1 does land on counts that are no multiple of a leader group)
        if (max_p == 1) CHECK(two == 1);
    }
    // ---- the shrink rule at ragged current sizes: keep n while target <= n and target * 1000 >= n * permille
    for (int permille : {0, 500, 800, 999, 1000}) {
        mcl_kld_config_t k;
        mcl_default_kld_config(&k);
        k.min_particles = 1; k.max_particles = 16385; k.round_to = 1; k.shrink_permille = permille;
        for (int64_t bins = 0; bins <= 600; ++bins) {
            cur_bins = bins;
            const int64_t target = bound_ref(k, bins);
            for (int64_t n : COUNTS) {
                cur_n = n;
                int64_t got = -1;
                CHECK(mcl_host_kld_target(&k, bins, n, &got) == MCL_OK);
                const bool keep = target <= n && target * 1000 >= n * (int64_t)permille;
                CHECK(got == (keep ? n : target));
            }
        }
    }
    // ---- refusals: codes, nothing written
    {
        mcl_kld_config_t k;
        mcl_default_kld_config(&k);
        k.min_particles = 1; k.max_particles = 1; k.round_to = 1;
        int64_t got = -7;
        cur_n = cur_bins = 0;
        CHECK(mcl_host_kld_target(&k, 5, -1, &got) == MCL_ERR_INVALID_ARG && got == -7);
        CHECK(mcl_host_kld_target(&k, 5, 1, nullptr) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_kld_target(nullptr, 5, 1, &got) == MCL_ERR_INVALID_ARG);
        k.min_particles = 0;
        CHECK(mcl_host_kld_target(&k, 5, 1, &got) == MCL_ERR_INVALID_ARG && got == -7);
        k.min_particles = 1; k.round_to = 0;
        CHECK(mcl_host_kld_target(&k, 5, 1, &got) == MCL_ERR_INVALID_ARG && got == -7);
        k.round_to = 1; k.min_particles = 2;                 // min above max
        CHECK(mcl_host_kld_target(&k, 5, 1, &got) == MCL_ERR_INVALID_ARG && got == -7);
    }
    // ---- the chunk of a list exchange and its bytes
    {
        const int64_t lens[] = {-1, 0, 1, 63, 64, 65, 127, 128, 129, 1025, 2049, 4095, 4096, 4097, 4099, 16385, 1048576, 1048577};
        for (int64_t longest : lens) {
            cur_n = longest; cur_bins = 0;
            const int64_t e = mcl_host::compact_chunk_entries(longest);
            CHECK(e >= 64 && e % 64 == 0 && e >= longest && (e == 64 || e < longest + 64));
            int64_t bytes = -1;
            CHECK(mcl_compact_chunk_bytes(e, &bytes) == MCL_OK && bytes == e * kCompactEntryBytes && bytes == e * (8 + 32 + 4));
        }
        CHECK(mcl_host::compact_chunk_entries(-1) == 64 && mcl_host::compact_chunk_entries(0) == 64 && mcl_host::compact_chunk_entries(64) == 64);
        CHECK(mcl_host::compact_chunk_entries(65) == 128 && mcl_host::compact_chunk_entries(4097) == 4160);
        int64_t bytes = -7;
        for (int64_t bad : {(int64_t)0, (int64_t)-64, (int64_t)1, (int64_t)63, (int64_t)65, (int64_t)4099}) {
            cur_n = bad;
            CHECK(mcl_compact_chunk_bytes(bad, &bytes) == MCL_ERR_INVALID_ARG && bytes == -7);
        }
        CHECK(mcl_compact_chunk_bytes(64, nullptr) == MCL_ERR_INVALID_ARG);
    }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
