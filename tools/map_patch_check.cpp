// map_patch_check.cpp -- mcl_host_map_patch_plan over its clipping, boundary and refusal cases, as a stand-alone
// host program for a sanitizer build: no device is opened.  Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/map_patch_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o map_patch_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <climits>
#include <cstdio>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool is(const int32_t got[4], int32_t a, int32_t b, int32_t c, int32_t d) { return got[0] == a && got[1] == b && got[2] == c && got[3] == d; }
static bool none(const int32_t w[4]) { return w[2] < w[0]; }

int main()
{
    const int R = 254;
    int32_t win[4], lf[4];
    // an interior cell: the padded cell (x + 1, y + 1) widened by the reach on every side; the field's window by its own reach
    { const int32_t b[4] = {300, 290, 300, 290};
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_OK && is(win, 301 - R, 291 - R, 301 + R, 291 + R) && is(lf, 260, 250, 340, 330));
      CHECK(mcl_host_map_patch_plan(600, 560, b, 0, win, lf) == MCL_OK && none(lf));
      CHECK(mcl_host_map_patch_plan(600, 560, b, -3, win, lf) == MCL_OK && none(lf)); }
    // grid row / column 0 feed padded row / column 0 as well
    { const int32_t b[4] = {0, 0, 0, 0};
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_OK && is(win, 0, 0, 1 + R, 1 + R) && is(lf, 0, 0, 40, 40)); }
    { const int32_t b[4] = {1, 1, 1, 1};
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_OK && is(win, 0, 0, 2 + R, 2 + R)); }
    { const int32_t b[4] = {R + 1, R + 1, R + 1, R + 1};                  // padded cell R + 2: the window starts at padded cell 2
      CHECK(mcl_host_map_patch_plan(2000, 2000, b, 40, win, lf) == MCL_OK && is(win, 2, 2, 2 * R + 2, 2 * R + 2)); }
    // the last cell, the whole map, a map smaller than the reach, a 1 x 1 map
    { const int32_t b[4] = {599, 559, 599, 559};
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_OK && is(win, 600 - R, 560 - R, 600, 560) && is(lf, 559, 519, 599, 559)); }
    { const int32_t b[4] = {0, 0, 3999, 3999};
      CHECK(mcl_host_map_patch_plan(4000, 4000, b, 40, win, lf) == MCL_OK && is(win, 0, 0, 4000, 4000) && is(lf, 0, 0, 3999, 3999)); }
    { const int32_t b[4] = {40, 30, 49, 32};
      CHECK(mcl_host_map_patch_plan(90, 70, b, 40, win, lf) == MCL_OK && is(win, 0, 0, 90, 70) && is(lf, 0, 0, 89, 69)); }
    { const int32_t b[4] = {0, 0, 0, 0};
      CHECK(mcl_host_map_patch_plan(1, 1, b, 1, win, lf) == MCL_OK && is(win, 0, 0, 1, 1) && is(lf, 0, 0, 0, 0)); }
    // clipping: a box that leaves the map on every side, extreme coordinates and reach
    { const int32_t b[4] = {-5, -7, 700, 800};
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_OK && is(win, 0, 0, 600, 560) && is(lf, 0, 0, 599, 559)); }
    { const int32_t b[4] = {INT_MIN, INT_MIN, INT_MAX, INT_MAX};
      CHECK(mcl_host_map_patch_plan(200000, 200000, b, INT_MAX, win, lf) == MCL_OK && is(win, 0, 0, 200000, 200000) && is(lf, 0, 0, 199999, 199999)); }
    { const int32_t b[4] = {590, 550, INT_MAX, INT_MAX};
      CHECK(mcl_host_map_patch_plan(600, 560, b, INT_MAX, win, lf) == MCL_OK && is(win, 591 - R, 551 - R, 600, 560) && is(lf, 0, 0, 599, 559)); }
    { const int32_t b[4] = {INT_MIN, 5, 0, 5};
      CHECK(mcl_host_map_patch_plan(600, 560, b, 2, win, lf) == MCL_OK && is(win, 0, 0, 1 + R, 6 + R) && is(lf, 0, 3, 2, 7)); }
    // refusals: outside the map, inverted, null pointers, map dimensions
    const int32_t outside[4][4] = {{600, 0, 610, 5}, {0, 560, 5, 570}, {-9, 3, -1, 4}, {3, INT_MIN, 4, -1}};
    for (const auto &b : outside) CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_ERR_INVALID_ARG);
    const int32_t inverted[3][4] = {{11, 20, 10, 20}, {10, 21, 10, 20}, {INT_MAX, 0, INT_MIN, 0}};
    for (const auto &b : inverted) CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, lf) == MCL_ERR_INVALID_ARG);
    { const int32_t b[4] = {1, 1, 2, 2};
      CHECK(mcl_host_map_patch_plan(600, 560, nullptr, 40, win, lf) == MCL_ERR_INVALID_ARG);
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, nullptr, lf) == MCL_ERR_INVALID_ARG);
      CHECK(mcl_host_map_patch_plan(600, 560, b, 40, win, nullptr) == MCL_ERR_INVALID_ARG);
      CHECK(mcl_host_map_patch_plan(0, 560, b, 40, win, lf) == MCL_ERR_INVALID_ARG);
      CHECK(mcl_host_map_patch_plan(600, 0, b, 40, win, lf) == MCL_ERR_INVALID_ARG);
      CHECK(mcl_host_map_patch_plan(200001, 560, b, 40, win, lf) == MCL_ERR_INVALID_ARG);
      CHECK(mcl_host_map_patch_plan(600, 0xFFFFFFFFu, b, 40, win, lf) == MCL_ERR_INVALID_ARG); }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
