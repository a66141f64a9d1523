// search_slabs_check.cpp -- mcl_host_search_slabs (rules ST4 / ST5) over its refusal and boundary cases, as a
// stand-alone host program for a sanitizer build: no device is opened.  Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/search_slabs_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o search_slabs_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <cstdio>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static uint64_t bytes_ref(uint64_t P, uint64_t G)
{
    return 8 * (G + 2) * P + 16 * G * P + 32 * (65536 + G * P) + 262144 + G * P / 16;
}

int main()
{
    mcl_search_config_t c;
    mcl_search_stream_config_t sc;
    mcl_default_search_config(&c);
    mcl_default_search_stream_config(&sc);
    mcl_default_search_stream_config(nullptr);
    CHECK(sc.budget_bytes == 0 && sc.slab_headings == 0);
    int32_t G = -1, slabs = -1;
    uint64_t bytes = 0;
    const int64_t P = 2611;

    // the defaults, with and without outputs and a stream config
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_OK && G == 72 && slabs == 1 && bytes == bytes_ref(P, 72));
    CHECK(mcl_host_search_slabs(&c, nullptr, P, 1, nullptr, nullptr, nullptr) == MCL_OK);
    CHECK(mcl_host_search_slabs(nullptr, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    // every G, and G above n
    for (int32_t g = 1; g <= 80; ++g) {
        sc.slab_headings = g;
        const int32_t want = g < 72 ? g : 72;
        CHECK(mcl_host_search_slabs(&c, &sc, P, 16, &G, &slabs, &bytes) == MCL_OK && G == want && slabs == (72 + want - 1) / want &&
              bytes == bytes_ref(P, want));
    }
    // the budget at its edge, for G = 1 and for an explicit G
    sc.slab_headings = 0;
    sc.budget_bytes = bytes_ref(P, 1);
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_OK && G == 1 && slabs == 72);
    sc.budget_bytes -= 1;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    sc.budget_bytes = 1;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    sc.budget_bytes = ~0ull;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_OK && G == 72);
    sc.slab_headings = 8;
    sc.budget_bytes = bytes_ref(P, 8) - 1;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    // ST4 at its edges: (G + 2) P < 2^27, P n < 2^40
    sc.budget_bytes = 1ull << 40;
    c.n_headings = 200;
    sc.slab_headings = 125;
    CHECK(mcl_host_search_slabs(&c, &sc, 1 << 20, 1, &G, &slabs, &bytes) == MCL_OK && G == 125 && slabs == 2);
    sc.slab_headings = 126;
    CHECK(mcl_host_search_slabs(&c, &sc, 1 << 20, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    sc.slab_headings = 0;
    CHECK(mcl_host_search_slabs(&c, &sc, 1 << 20, 1, &G, &slabs, &bytes) == MCL_OK && G == 125);
    c.n_headings = (1 << 20) - 1;
    CHECK(mcl_host_search_slabs(&c, &sc, 1 << 20, 1, &G, &slabs, &bytes) == MCL_OK && G == 125);
    c.n_headings = 1 << 20;
    CHECK(mcl_host_search_slabs(&c, &sc, 1 << 20, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    c.n_headings = 0x7fffffff;
    sc.slab_headings = 0x7fffffff;
    CHECK(mcl_host_search_slabs(&c, &sc, 1, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);       // (G + 2) P >= 2^27
    CHECK(mcl_host_search_slabs(&c, &sc, ((int64_t)1 << 27) - 1, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_slabs(&c, &sc, (int64_t)1 << 62, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    sc.slab_headings = 0;
    CHECK(mcl_host_search_slabs(&c, &sc, 1, 1, &G, &slabs, &bytes) == MCL_OK && G == (1 << 27) - 3);
    // the refused arguments
    mcl_default_search_config(&c);
    mcl_default_search_stream_config(&sc);
    sc.slab_headings = -1;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    sc.slab_headings = 0;
    for (int i = 0; i < 5; ++i) {
        sc.reserved[i] = 1;
        CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
        sc.reserved[i] = 0;
    }
    CHECK(mcl_host_search_slabs(&c, &sc, P, 0, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_slabs(&c, &sc, P, 17, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_slabs(&c, &sc, 0, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    CHECK(mcl_host_search_slabs(&c, &sc, -5, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    c.n_headings = 0;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    c.n_headings = 72;
    c.reserved[3] = 1;
    CHECK(mcl_host_search_slabs(&c, &sc, P, 1, &G, &slabs, &bytes) == MCL_ERR_INVALID_ARG);
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
