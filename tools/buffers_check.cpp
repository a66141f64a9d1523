// buffers_check.cpp -- Buf (csrc/mcl_buffers.h), the owning buffer every device and pinned allocation of the library goes through,
// with a counting memory policy of its own: a stand-alone host program for a sanitizer build.  No GPU call is made, no device opened.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/buffers_check.cpp -o buffers_check
// It prints "ok" and returns 0, or says which case failed.
#include "../monte_carlo_localization_amd/csrc/mcl_buffers.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// (DeviceMem / PinnedMem report through it; this program never reaches them)
int mcl_host::fail(mcl_engine *, int code, const std::string &) { return code; }

// host memory, counted: the blocks alive, the allocations and releases so far, and a switch that makes the next alloc fail.
// A release of anything but a live block (a second release, a pointer that never was one) fails a check.
struct Counting {
    static std::set<void *> &alive() { static std::set<void *> s; return s; }
    static int &allocs() { static int n = 0; return n; }
    static int &releases() { static int n = 0; return n; }
    static bool &fail_next() { static bool f = false; return f; }
    static int alloc(mcl_engine *, void **p, size_t n)
    {
        if (fail_next()) { fail_next() = false; *p = (void *)16; return MCL_ERR_HIP; }   // (a failing call may scribble on *p)
        *p = std::malloc(n ? n : 1);
        alive().insert(*p);
        ++allocs();
        return MCL_OK;
    }
    static void release(void *p)
    {
        CHECK(alive().count(p) == 1);
        if (alive().erase(p)) std::free(p);
        ++releases();
    }
    static int live() { return (int)alive().size(); }
    static bool balanced() { return live() == 0 && allocs() == releases(); }
};
using CBuf = Buf<double, Counting>;

int main()
{
    size_t bytes = 0, last = 0;
    auto counter_grew = [&](size_t by) { const bool ok = bytes == last + by; last = bytes; return ok; };
    {
        CBuf b;
        CHECK(b.p == nullptr && b.cap == 0 && (double *)b == nullptr);
        CHECK(b.reserve(nullptr, 0, &bytes) == MCL_OK && b.p == nullptr && Counting::allocs() == 0 && counter_grew(0));
        CHECK(b.reserve(nullptr, 100, &bytes) == MCL_OK && b.p && b.cap == 100 && counter_grew(800));
        double *first = b.p;
        first[0] = 1.0; first[99] = 2.0;                                  // the whole block is ours (the sanitizer checks)
        CHECK(b.reserve(nullptr, 40, &bytes) == MCL_OK && b.p == first && b.cap == 100 && counter_grew(0));     // below cap
        CHECK(b.reserve(nullptr, 100, &bytes) == MCL_OK && b.p == first && Counting::allocs() == 1 && counter_grew(0));   // at cap
        CHECK(b.reserve(nullptr, 101, &bytes) == MCL_OK && b.cap == 101 && Counting::allocs() == 2 && counter_grew(808));   // above
        CHECK(Counting::releases() == 1 && Counting::alive().count(first) + Counting::alive().count(b.p) == 1 && Counting::live() == 1);
        b.p[100] = 3.0;
        // a failing alloc: the status comes back, the buffer is empty, the old block went exactly once, the counter stands
        Counting::fail_next() = true;
        CHECK(b.reserve(nullptr, 500, &bytes) == MCL_ERR_HIP && b.p == nullptr && b.cap == 0 && counter_grew(0));
        CHECK(Counting::releases() == 2 && Counting::live() == 0);
        CHECK(b.reserve(nullptr, 8) == MCL_OK && b.cap == 8 && counter_grew(0));       // and it can be used again; no counter given
        b.drop();
        CHECK(b.p == nullptr && b.cap == 0 && Counting::balanced());
        b.drop();                                                         // twice
        CHECK(b.p == nullptr && b.cap == 0 && Counting::balanced());
        CHECK(b.reserve(nullptr, 3, &bytes) == MCL_OK && Counting::live() == 1 && counter_grew(24));
    }                                                                     // the destructor releases the last block, once
    CHECK(Counting::balanced());
    {
        // moving: the source is left empty and nothing is released; the target's old block goes once
        CBuf a, b;
        CHECK(a.reserve(nullptr, 5, &bytes) == MCL_OK && b.reserve(nullptr, 6, &bytes) == MCL_OK && counter_grew(88));
        double *pa = a.p;
        const int live = Counting::live(), rel = Counting::releases();
        CBuf c(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && c.p == pa && c.cap == 5 && Counting::live() == live && Counting::releases() == rel);
        b = std::move(c);
        CHECK(c.p == nullptr && c.cap == 0 && b.p == pa && b.cap == 5 && Counting::releases() == rel + 1 && Counting::live() == live - 1);
        CBuf &self = b;
        b = std::move(self);
        CHECK(b.p == pa && b.cap == 5 && Counting::releases() == rel + 1);
        // a container of buffers, grown (its elements move) and destroyed: every block once
        std::vector<CBuf> v;
        for (int i = 0; i < 40; ++i) {
            v.emplace_back();
            CHECK(v.back().reserve(nullptr, (size_t)i + 1, &bytes) == MCL_OK && counter_grew(8 * ((size_t)i + 1)));
        }
        for (int i = 0; i < 40; ++i) CHECK(v[(size_t)i].cap == (size_t)i + 1);
        v.resize(64);
        v.resize(10);
        CHECK(Counting::live() == 1 + 10);
    }
    CHECK(Counting::balanced() && bytes == last);
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
