// The guide of the compact parent list (mcl::CompactOut, mcl_scan.h): a table over evenly spaced thresholds that tells the
// resampling search where in the list to look, written by the scan that writes the list.  Host and device: k_scan_final fills
// the table with guide_owner_range, resample_motion_body searches with compact_guide_search, and mcl_host_compact_guide /
// mcl_host_compact_search (mcl_host_math.hip) are the same functions run on the CPU.
//
//   s = guide_shift(q_total, m) = max(0, bit_width(q_total) - m);  the bucket of a threshold is thr >> s
//   bmax = q_total >> s: the largest b whose boundary b << s does not exceed q_total (bmax < 2^m when s > 0, bmax = q_total else)
//   guide[b], b = 0 .. bmax: the first list position p with ccdf[p] >= (b << s)                      (guide[0] = 0)
//   a reader takes guide[b + 1] as n_compact when b + 1 > bmax
// For thr in bucket b the first entry with ccdf > thr -- the upper_bound the search is after -- lies in [guide[b], guide[b + 1]]:
// it is not before guide[b] (ccdf[p] > thr >= b << s), and the first entry at or above the next boundary is above thr.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcl {

constexpr int kGuideLog2Min = 8, kGuideLog2Max = 20;
constexpr int kGuideLog2Default = 17;                        // 2^17 + 2 words: 512 KB, resident in L2 (profiles/resample_guide.md)

__host__ __device__ __forceinline__ int guide_bit_width(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 64 - __clzll((long long)v);
#else
    int w = 0;
    while (v) { ++w; v >>= 1; }
    return w;
#endif
}
__host__ __device__ __forceinline__ int guide_shift(uint64_t q_total, int m)
{
    const int s = guide_bit_width(q_total) - m;
    return s > 0 ? s : 0;
}
__host__ __device__ __forceinline__ uint32_t guide_bmax(uint64_t q_total, int s) { return (uint32_t)(q_total >> s); }
// words of a guide of 2^m buckets: 0 .. bmax <= 2^m (s == 0 with q_total < 2^m; else bmax < 2^m), and the one behind them that
// the search's pair fetch touches
__host__ __device__ __forceinline__ size_t guide_words(int m) { return ((size_t)1 << m) + 2; }

// The words entry `pos` of the list owns, [b0, b1): the boundaries b << s in (c - x, c], c its CDF value and x > 0 its weight
// (ccdf[pos - 1] = c - x lies below them, ccdf[pos] = c does not); entry 0 also owns word 0.  Every word 0 .. bmax then has
// exactly one owner: the intervals (c - x, c] tile (0, q_total].
__host__ __device__ __forceinline__ void guide_owner_range(uint64_t c, uint64_t x, int s, uint32_t pos, uint32_t &b0, uint32_t &b1)
{
    b0 = pos == 0 ? 0u : (uint32_t)((c - x) >> s) + 1u;
    b1 = (uint32_t)(c >> s) + 1u;
}

// Position of the first entry with ccdf > thr, clamped to n_compact - 1 (n_compact > 0): what the two-level search over
// ctop / ccdf returns.  A bucket beyond bmax (thr >= q_total: no entry is above it) is searched as bmax, which ends at
// n_compact and is clamped like the old search's "none found"; the two guide words are held to the list, so that no table can
// send a probe outside it.
__host__ __device__ __forceinline__ uint32_t compact_guide_search(const uint64_t *__restrict__ ccdf, uint32_t n_compact, const uint32_t *__restrict__ guide,
                                                                  int s, uint32_t bmax, uint64_t thr)
{
    const uint64_t bt = thr >> s;
    const uint32_t b = bt < (uint64_t)bmax ? (uint32_t)bt : bmax;
    uint32_t lo = guide[b];
    const uint32_t next = guide[b + 1u];            // (one fetch for the pair; word bmax + 1 exists, is never written and never used)
    uint32_t hi = b < bmax ? next : n_compact;
    hi = hi < n_compact ? hi : n_compact;
    lo = lo < hi ? lo : hi;
    uint32_t len = hi - lo;
    while (len > 0u) {
        const uint32_t half = len >> 1, mid = lo + half;
        if (!(ccdf[mid] > thr)) { lo = mid + 1u; len = len - half - 1u; }
        else len = half;
    }
    return lo >= n_compact ? n_compact - 1u : lo;
}

}  // namespace mcl
