// beam_grid_check.cpp -- mcl_host_search_beam_grid and the tile plan of mcl_global_search_beam (rules B1 / B5)
// over their refusal and boundary cases, as a stand-alone host program for a sanitizer build: no device is opened.  Build it
// together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/beam_grid_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o beam_grid_check
// It prints "ok" and returns 0, or says which case failed.
#include "../monte_carlo_localization_amd/csrc/mcl_host_math.h"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// B evenly spaced float angles from a0, as a driver forms them: a0 + i * inc in float
static std::vector<float> scan(int B, float a0, float inc)
{
    std::vector<float> a((size_t)B);
    for (int i = 0; i < B; ++i) a[(size_t)i] = a0 + (float)i * inc;
    return a;
}

static int grid(const std::vector<float> &a, int n_head, int32_t *M = nullptr, int32_t *s = nullptr, double *dev = nullptr,
                std::vector<double> *phi = nullptr)
{
    double delta = 0.0;
    return mcl_host_search_beam_grid(a.data(), (int32_t)a.size(), n_head, M, s, &delta, dev, phi ? phi->data() : nullptr, phi ? phi->size() : 0);
}

int main()
{
    const double kTwoPi = 6.283185307179586;
    const float a0 = (float)(-3.0 * M_PI / 4.0), inc = (float)((3.0 * M_PI / 2.0) / 1080.0);
    int32_t M = -1, s = -1;
    double dev = -1.0;

    // a Hokuyo's 1081 angles, every 20th of them, one of them
    const std::vector<float> full = scan(1081, a0, inc);
    CHECK(grid(full, 72, &M, &s, &dev) == MCL_OK && M == 1440 && s == 20 && dev > 0.0 && dev < 4e-7);
    std::vector<double> phi(1440);
    CHECK(grid(full, 72, nullptr, nullptr, nullptr, &phi) == MCL_OK);
    for (int m = 0; m < 1440; ++m) CHECK(phi[(size_t)m] == ((double)a0 - 3.141592653589793) + (double)m * (kTwoPi / 1440.0));
    phi.resize(1439);
    CHECK(grid(full, 72, nullptr, nullptr, nullptr, &phi) == MCL_ERR_INVALID_ARG);              // n_phi != M
    std::vector<float> sub;
    for (int i = 0; i < 1081; i += 20) sub.push_back(full[(size_t)i]);
    CHECK(grid(sub, 72, &M, &s, &dev) == MCL_OK && M == 72 && s == 1 && dev < 4e-7);
    CHECK(grid(sub, 8, &M, &s) == MCL_OK && M == 72 && s == 9);
    const std::vector<float> one(1, a0);
    CHECK(grid(one, 72, &M, &s, &dev) == MCL_OK && M == 72 && s == 1 && dev == 0.0);
    CHECK(grid(one, 1, &M, &s) == MCL_OK && M == 1 && s == 1);
    CHECK(grid(one, 16384, &M, &s) == MCL_OK && M == 16384);
    CHECK(grid(one, 16385) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_beam_grid(full.data(), 1081, 72, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == MCL_OK);   // no outputs
    // null, empty, bad counts
    CHECK(mcl_host_search_beam_grid(nullptr, 5, 72, &M, &s, nullptr, &dev, nullptr, 0) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_beam_grid(full.data(), 0, 72, &M, &s, nullptr, &dev, nullptr, 0) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_beam_grid(full.data(), -3, 72, &M, &s, nullptr, &dev, nullptr, 0) == MCL_ERR_INVALID_ARG);
    CHECK(grid(full, 0) == MCL_ERR_INVALID_ARG);
    CHECK(grid(full, -72) == MCL_ERR_INVALID_ARG);
    // n_headings must divide M
    CHECK(grid(full, 7) == MCL_ERR_INVALID_ARG);
    CHECK(grid(full, 1440, &M, &s) == MCL_OK && s == 1);
    CHECK(grid(full, 2880) == MCL_ERR_INVALID_ARG);
    // the deviation bound, either side
    std::vector<float> moved = full;
    moved[500] += 1e-4f;
    CHECK(grid(moved, 72, nullptr, nullptr, &dev) == MCL_ERR_INVALID_ARG && dev > 9e-5 && dev < 1.1e-4);
    moved = full;
    moved[500] += 2e-6f;
    CHECK(grid(moved, 72, nullptr, nullptr, &dev) == MCL_OK && dev <= 4e-6);
    // the increment: descending, zero, not a number, infinite
    std::vector<float> rev(full.rbegin(), full.rend());
    CHECK(grid(rev, 72) == MCL_ERR_INVALID_ARG);
    CHECK(grid(std::vector<float>(5, 0.25f), 72) == MCL_ERR_INVALID_ARG);
    moved = full;
    moved[1080] = NAN;
    CHECK(grid(moved, 72) == MCL_ERR_INVALID_ARG);
    moved[1080] = INFINITY;
    CHECK(grid(moved, 72) == MCL_ERR_INVALID_ARG);
    moved = full;
    moved[3] = NAN;
    CHECK(grid(moved, 72, nullptr, nullptr, &dev) == MCL_ERR_INVALID_ARG && dev != dev);
    moved = full;
    moved[0] = -INFINITY;
    CHECK(grid(moved, 72) == MCL_ERR_INVALID_ARG);
    CHECK(grid(std::vector<float>(1, NAN), 72) == MCL_ERR_INVALID_ARG);
    // B <= M <= 16384 at its edges
    CHECK(grid(scan(50, 0.0f, (float)(kTwoPi / 50.0)), 50, &M) == MCL_OK && M == 50);             // a full turn: B == M
    CHECK(grid(scan(51, 0.0f, (float)(kTwoPi / 50.0)), 50) == MCL_ERR_INVALID_ARG);               // B > M
    CHECK(grid(scan(3, 0.0f, (float)(kTwoPi / 16384.0)), 64, &M) == MCL_OK && M == 16384);
    CHECK(grid(scan(3, 0.0f, (float)(kTwoPi / 16386.0)), 64) == MCL_ERR_INVALID_ARG);
    CHECK(grid(scan(3, 0.0f, 1e-30f), 64) == MCL_ERR_INVALID_ARG);                                // 2 pi / inc beyond any integer
    CHECK(grid(scan(2, 0.0f, 13.0f), 1) == MCL_ERR_INVALID_ARG);                                  // M rounds to 0

    // B5: the tile plan
    mcl_host::SearchBeamTiles t;
    const uint64_t MiB = 1ull << 20;
    CHECK(mcl_host::search_beam_tiles(990000, 1440, 240, 0, t).empty() && t.entry_bytes == 1 && t.T == (int64_t)(256 * MiB / 1440 / 256 * 256) &&
          t.tiles == (990000 + t.T - 1) / t.T);
    CHECK(mcl_host::search_beam_tiles(990000, 1440, 255, 256 * MiB, t).empty() && t.entry_bytes == 1);
    CHECK(mcl_host::search_beam_tiles(990000, 1440, 256, 256 * MiB, t).empty() && t.entry_bytes == 2 &&
          t.T == (int64_t)(256 * MiB / 2880 / 256 * 256));
    // the budget at its edge
    CHECK(mcl_host::search_beam_tiles(1151, 72, 240, 256 * 72, t).empty() && t.T == 256 && t.tiles == 5);
    CHECK(!mcl_host::search_beam_tiles(1151, 72, 240, 256 * 72 - 1, t).empty());
    CHECK(!mcl_host::search_beam_tiles(1151, 72, 240, 1, t).empty());
    CHECK(mcl_host::search_beam_tiles(1151, 72, 480, 512 * 72, t).empty() && t.T == 256);
    CHECK(!mcl_host::search_beam_tiles(1151, 72, 480, 512 * 72 - 1, t).empty());
    CHECK(mcl_host::search_beam_tiles(1151, 72, 240, 512 * 72 - 1, t).empty() && t.T == 256);
    CHECK(mcl_host::search_beam_tiles(1151, 72, 240, 512 * 72, t).empty() && t.T == 512 && t.tiles == 3);
    // no larger than the lattice, and a tile's ray index below 2^31
    CHECK(mcl_host::search_beam_tiles(1151, 72, 240, ~0ull, t).empty() && t.T == 1280 && t.tiles == 1);
    CHECK(mcl_host::search_beam_tiles(1, 1, 1, 256, t).empty() && t.T == 256 && t.tiles == 1);
    CHECK(mcl_host::search_beam_tiles(((int64_t)1 << 27) - 1, 16384, 2047, ~0ull, t).empty() && t.T == 131072 &&
          (uint64_t)t.T * 16384 <= (1ull << 31) && t.tiles == 1024);
    CHECK(mcl_host::search_beam_tiles(((int64_t)1 << 27) - 1, 1, 240, ~0ull, t).empty() && t.T == (int64_t)1 << 27 && t.tiles == 1);
    // sizes no plan is made for
    CHECK(!mcl_host::search_beam_tiles(0, 72, 240, 0, t).empty());
    CHECK(!mcl_host::search_beam_tiles(-1, 72, 240, 0, t).empty());
    CHECK(!mcl_host::search_beam_tiles((int64_t)1 << 27, 72, 240, 0, t).empty());
    CHECK(!mcl_host::search_beam_tiles(1151, 0, 240, 0, t).empty());
    CHECK(!mcl_host::search_beam_tiles(1151, 16385, 240, 0, t).empty());
    CHECK(!mcl_host::search_beam_tiles(1151, 72, 0, 0, t).empty());
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
