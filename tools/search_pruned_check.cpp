// search_pruned_check.cpp -- the host side of mcl_global_search_pruned (rules P1 / P2 / P4): the block plan, the
// pooled field's window and the round schedule over their boundary and refusal cases, and the one table the search over a scan
// sequence adds to them (mcl_global_search_sequence_pruned, §4.21: SQ1's offsets at every scan count), as a stand-alone host program
// for a sanitizer build: no device is opened.  Build it together with the host arithmetic unit, e.g.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         tools/search_pruned_check.cpp monte_carlo_localization_amd/csrc/mcl_host_math.hip -o search_pruned_check
// It prints "ok" and returns 0, or says which case failed.
#include "../include/mcl_hip_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// P2 by brute force
static std::vector<uint16_t> pool_ref(const std::vector<uint16_t> &D, int W, int H, int K, int w)
{
    const int Wp = W + w - 1, Hp = H + w - 1;
    std::vector<uint16_t> out((size_t)Wp * Hp);
    for (int ys = 0; ys < Hp; ++ys)
        for (int xs = 0; xs < Wp; ++xs) {
            int best = K;
            for (int y = ys - (w - 1); y <= ys; ++y)
                for (int x = xs - (w - 1); x <= xs; ++x)
                    if (x >= 0 && x < W && y >= 0 && y < H) best = std::min(best, (int)D[(size_t)y * W + x]);
            out[(size_t)ys * Wp + xs] = (uint16_t)best;
        }
    return out;
}

int main()
{
    mcl_search_config_t c;
    mcl_search_prune_config_t pc;
    mcl_default_search_config(&c);
    mcl_default_search_prune_config(&pc);
    mcl_default_search_prune_config(nullptr);
    CHECK(pc.block == 8 && pc.first_pairs == 0);

    // ---- P1: the block plan.  A 37 x 23 map at stride 2: the lattice is 18 x 11, so S = 8 gives 3 x 2 blocks, the last row and
    // column with fewer lattice cells; one free cell alone in its block; a map with no free cell
    {
        const int W = 37, H = 23;
        std::vector<int8_t> g((size_t)W * H, 0);
        int32_t n = -1, w = -1, nbx = -1, nby = -1;
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_OK);
        CHECK(n == 6 && w == 16 && nbx == 3 && nby == 2);
        std::vector<int32_t> blk((size_t)n * 3);
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, blk.data(), (size_t)n) == MCL_OK);
        CHECK(blk[0] == 0 && blk[1] == 0 && blk[2] == 64);
        CHECK(blk[6] == 2 && blk[7] == 0 && blk[8] == 16);                 // columns 16, 17 of the lattice: 2 x 8
        CHECK(blk[15] == 2 && blk[16] == 1 && blk[17] == 6);               // rows 8 .. 10: 2 x 3
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, blk.data(), (size_t)n + 1) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_blocks(&c, nullptr, g.data(), W, H, &n, nullptr, nullptr, nullptr, nullptr, 0) == MCL_OK && n == 6);
        std::fill(g.begin(), g.end(), (int8_t)100);
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_OK && n == 0);
        g[(size_t)21 * W + 35] = 0;                                        // lattice cell (17, 10): block (2, 1)
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, blk.data(), 1) == MCL_OK && n == 1);
        CHECK(blk[0] == 2 && blk[1] == 1 && blk[2] == 1);
        // every block side and stride: w, and a lattice smaller than one block
        for (int S : {2, 4, 8})
            for (int stride : {1, 2, 3, 7}) {
                pc.block = S; c.stride_cells = stride;
                CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_OK && w == (S - 1) * stride + 2);
            }
        c.stride_cells = 40;                                               // h0 = 20 < 37 and 23: one lattice cell
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_OK && nbx == 1 && nby == 1);
        // the refusals
        mcl_default_search_config(&c);
        for (int S : {-8, 0, 1, 3, 5, 16, 64}) {
            pc.block = S;
            CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
        }
        mcl_default_search_prune_config(&pc);
        pc.first_pairs = -1;
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
        pc.first_pairs = 0;
        for (int i = 0; i < 6; ++i) {
            pc.reserved[i] = 1;
            CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
            pc.reserved[i] = 0;
        }
        c.stride_cells = 9363;                                             // 7 * 9363 + 2 = 65543 > 65536
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
        c.stride_cells = 9362;                                             // 65536
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_OK && w == 65536);
        c.stride_cells = 0x7fffffff;
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
        mcl_default_search_config(&c);
        CHECK(mcl_host_search_blocks(nullptr, &pc, g.data(), W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_blocks(&c, &pc, nullptr, W, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_blocks(&c, &pc, g.data(), 0, H, &n, &w, &nbx, &nby, nullptr, 0) == MCL_ERR_INVALID_ARG);
    }

    // ---- P2: the window.  Every w from 1 to beyond both map sides, on a field with its minimum in a corner and on an edge
    {
        const int W = 7, H = 5, K = 50;
        std::vector<uint16_t> D((size_t)W * H);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) D[(size_t)y * W + x] = (uint16_t)std::min(K, 3 * x * x + y * y);
        D[(size_t)2 * W + 6] = 1;
        for (int w = 1; w <= 9; ++w) {
            const size_t n = (size_t)(W + w - 1) * (H + w - 1);
            std::vector<uint16_t> out(n);
            CHECK(mcl_host_lf_pool(D.data(), W, H, K, w, out.data(), n) == MCL_OK);
            CHECK(out == pool_ref(D, W, H, K, w));
            CHECK(out[0] == D[0] && out[n - 1] == D[(size_t)W * H - 1]);
            CHECK(mcl_host_lf_pool(D.data(), W, H, K, w, out.data(), n - 1) == MCL_ERR_INVALID_ARG);
        }
        std::vector<uint16_t> out(64);
        CHECK(mcl_host_lf_pool(D.data(), W, H, K, 0, out.data(), 24) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_lf_pool(D.data(), W, H, -1, 1, out.data(), 35) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_lf_pool(D.data(), W, H, 65536, 1, out.data(), 35) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_lf_pool(nullptr, W, H, K, 1, out.data(), 35) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_lf_pool(D.data(), W, H, K, 1, nullptr, 35) == MCL_ERR_INVALID_ARG);
        // one cell
        const uint16_t one = 7;
        CHECK(mcl_host_lf_pool(&one, 1, 1, 9, 3, out.data(), 9) == MCL_OK);
        for (int i = 0; i < 9; ++i) CHECK(out[(size_t)i] == 7);
    }

    // ---- P2: the bound table
    {
        const float ninf = -INFINITY;
        const float lf[6] = {-1.0f, ninf, -0.5f, -2.0f, ninf, -3.0f};
        float ub[6];
        CHECK(mcl_host_search_bound_table(lf, 5, ub) == MCL_OK);
        CHECK(ub[0] == -0.5f && ub[1] == -0.5f && ub[2] == -0.5f && ub[3] == -2.0f && ub[4] == -3.0f && ub[5] == -3.0f);
        CHECK(mcl_host_search_bound_table(&ninf, 0, ub) == MCL_OK && ub[0] == ninf);
        CHECK(mcl_host_search_bound_table(nullptr, 5, ub) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_bound_table(lf, -1, ub) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_bound_table(lf, 65536, ub) == MCL_ERR_INVALID_ARG);
    }

    // ---- P4: the round schedule
    {
        int64_t n = -1;
        mcl_default_search_prune_config(&pc);
        CHECK(mcl_host_search_prune_next(&pc, 1, 0, 0, &n) == MCL_OK && n == 1);
        CHECK(mcl_host_search_prune_next(&pc, 1023, 0, 0, &n) == MCL_OK && n == 1023);
        CHECK(mcl_host_search_prune_next(&pc, 65535, 0, 0, &n) == MCL_OK && n == 1024);
        CHECK(mcl_host_search_prune_next(&pc, 65536 + 64, 0, 0, &n) == MCL_OK && n == 1025);
        CHECK(mcl_host_search_prune_next(nullptr, 1 << 27, 0, 0, &n) == MCL_OK && n == 1 << 21);
        pc.first_pairs = 0x7fffffff;
        CHECK(mcl_host_search_prune_next(&pc, 5000, 0, 0, &n) == MCL_OK && n == 5000);
        pc.first_pairs = 3;
        CHECK(mcl_host_search_prune_next(&pc, 5000, 0, 0, &n) == MCL_OK && n == 3);
        CHECK(mcl_host_search_prune_next(&pc, 5000, 3, 0, &n) == MCL_OK && n == 6);
        CHECK(mcl_host_search_prune_next(&pc, 5000, 3, 7, &n) == MCL_OK && n == 7);
        CHECK(mcl_host_search_prune_next(&pc, 5000, 2500, 0, &n) == MCL_OK && n == 5000);
        CHECK(mcl_host_search_prune_next(&pc, 5000, 2501, 0, &n) == MCL_OK && n == 5000);
        CHECK(mcl_host_search_prune_next(&pc, 5001, 2500, 0, &n) == MCL_OK && n == 5000);
        CHECK(mcl_host_search_prune_next(&pc, 5000, 5000, 5000, &n) == MCL_OK && n == 5000);
        CHECK(mcl_host_search_prune_next(&pc, 5000, 10, 1ll << 62, &n) == MCL_OK && n == 5000);
        const int64_t big = 0x7fffffffffffffffll;
        CHECK(mcl_host_search_prune_next(&pc, big, big - 1, 0, &n) == MCL_OK && n == big);          // 2 n does not overflow
        CHECK(mcl_host_search_prune_next(&pc, big, big / 2 + 1, 0, &n) == MCL_OK && n == big);
        // every round of a schedule ends at `pairs`, growing strictly
        for (int64_t pairs : {1ll, 2ll, 1000ll, 1048577ll}) {
            int64_t at = 0, rounds = 0;
            while (at < pairs) {
                CHECK(mcl_host_search_prune_next(&pc, pairs, at, 0, &n) == MCL_OK && n > at && n <= pairs);
                at = n;
                ++rounds;
            }
            CHECK(rounds <= 64);
        }
        CHECK(mcl_host_search_prune_next(&pc, 0, 0, 0, &n) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_prune_next(&pc, 10, 11, 0, &n) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_prune_next(&pc, 10, -1, 0, &n) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_prune_next(&pc, 10, 1, -1, &n) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_prune_next(&pc, 10, 1, 0, nullptr) == MCL_ERR_INVALID_ARG);
        pc.first_pairs = -1;
        CHECK(mcl_host_search_prune_next(&pc, 10, 0, 0, &n) == MCL_ERR_INVALID_ARG);
    }

    // ---- §4.21 (PS2): what mcl_global_search_sequence_pruned uploads beside the single search's tables is SQ1's table, n x N
    // triples, formed by the one host function both sequence searches call.  Its size at every N the call accepts, its last triple
    // written and nothing behind it, the rows of a zero rel (PS5's identity rests on them), the refusals PS5 takes from SQ
    {
        mcl_default_search_config(&c);
        c.n_headings = 8;
        const double ang = 0.3, PI = 3.14159265358979323846;
        for (int N = 1; N <= MCL_SEARCH_MAX_SCANS; ++N) {
            std::vector<double> rel((size_t)N * 3);
            for (int s = 0; s < N; ++s) { rel[3 * s] = -0.5 * s; rel[3 * s + 1] = 0.13 * s; rel[3 * s + 2] = s == N - 1 ? 0.0 : ang; }
            const size_t n = (size_t)c.n_headings * (size_t)N * 3;
            std::vector<double> off(n + 1, 77.0);
            CHECK(mcl_host_search_sequence_offsets(&c, rel.data(), N, off.data(), n) == MCL_OK);
            CHECK(off[n] == 77.0);
            std::vector<double> theta((size_t)c.n_headings);
            CHECK(mcl_host_search_headings(&c, theta.data(), theta.size()) == MCL_OK);
            for (int k = 0; k < c.n_headings; ++k) {
                const double *last = &off[((size_t)k * N + (size_t)(N - 1)) * 3];
                CHECK(last[2] == theta[(size_t)k]);                                  // theta_k + 0.0 is theta_k
                if (N == 1) CHECK(last[0] == 0.0 && last[1] == 0.0);                 // a zero rel: no displacement (of either sign)
                if (N > 1) {
                    const double *first = &off[((size_t)k * N + 1) * 3];             // scan 1: dx = -0.5, dy = 0.13
                    const double dx = -0.5, dy = 0.13, ck = std::cos(theta[(size_t)k]), sk = std::sin(theta[(size_t)k]);
                    CHECK(first[0] == ck * dx - sk * dy && first[1] == sk * dx + ck * dy);
                    CHECK(std::fabs(std::hypot(first[0], first[1]) - std::hypot(dx, dy)) < 1e-12);
                }
                CHECK(theta[(size_t)k] >= -PI && theta[(size_t)k] < PI);
            }
            CHECK(mcl_host_search_sequence_offsets(&c, rel.data(), N, off.data(), n - 1) == MCL_ERR_INVALID_ARG);
        }
        double rel[3 * (MCL_SEARCH_MAX_SCANS + 1)] = {0.0}, out[8 * 3 * (MCL_SEARCH_MAX_SCANS + 1)];
        CHECK(mcl_host_search_sequence_offsets(&c, rel, 0, out, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_sequence_offsets(&c, rel, -1, out, 0) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_sequence_offsets(&c, rel, MCL_SEARCH_MAX_SCANS + 1, out, (size_t)8 * 3 * (MCL_SEARCH_MAX_SCANS + 1)) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_sequence_offsets(&c, nullptr, 1, out, 24) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_sequence_offsets(&c, rel, 1, nullptr, 24) == MCL_ERR_INVALID_ARG);
        CHECK(mcl_host_search_sequence_offsets(nullptr, rel, 1, out, 24) == MCL_ERR_INVALID_ARG);
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY})
            for (int i = 0; i < 6; ++i) {
                rel[i] = bad;
                CHECK(mcl_host_search_sequence_offsets(&c, rel, 2, out, 48) == MCL_ERR_INVALID_ARG);
                rel[i] = 0.0;
            }
        CHECK(mcl_host_search_sequence_offsets(&c, rel, 2, out, 48) == MCL_OK);
    }
    std::printf(failures ? "%d case(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
