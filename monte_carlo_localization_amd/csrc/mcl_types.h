// mcl_types.h -- the few plain types and constants that both the kernels (mcl_kernels.h) and the host-only translation units
// (mcl_comm.hip, mcl_group.hip, mcl_cluster.hip, through mcl_engine_internal.h) need.  The only device code is kld_bin, the
// pose-space bin rule that the KLD marking (mcl_resample.h), its host restatement and the pose clustering (mcl_cluster.hip) share.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace mcl {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems;
constexpr int kMaxShards = 16;
constexpr int kSwUnder = 127;            // table rows below "no hit": samples left in [-127, -1] after an over-long jump
// rows of the per-update fp64 table of k_rays_sweep (mcl_rays_sweep.h): row r = samples left + kSwUnder, plus one all-zero row
__host__ __device__ inline int sweep_table_rows(int P) { return P + kSwUnder + 2; }

// scratch the ray stage needs zeroed, cleared here instead of by one memset each (null = not used by this launch)
struct PrepClear {
    double *logw_acc;                  // n
    uint32_t *far_flags;               // n
    unsigned long long *fix_count;     // fix_words 64-bit words
    int fix_words;
    unsigned long long *fix_over;      // 2 words (overflow flag, work counter)
    unsigned long long *exact_count;   // 1 word
    unsigned long long *far_count;     // 1 word
    int *bbox;                         // 4: +big, +big, -big, -big; [4], [5]: k_tile_compact; [6] = bbox_play
    int bbox_play;                     // cells a ray window leaves for the particles of a work item (0: no windowed kernel): sort_layout
    uint32_t *hist;                    // hist_n bucket counters
    uint32_t hist_n;
};

// KLD-adaptive particle count: the pose-space bin of every child's parent pose (before the motion model) is
// marked in a bitmap of nx * ny * n_theta + 1 bits (the last one: "outside"), test-then-set, and the lane whose fetch-or found
// the bit clear owns the new bin: owners are summed per wave (one atomic per wave) and append their word index to a list, so
// that the count is exact and independent of the order, and the clearing kernel touches only those words.
struct KldArgs {
    uint32_t *bm;                     // bitmap (all zero on entry)
    uint32_t *list;                   // word index of every new bin, in the order the waves reserved them (*count entries)
    unsigned int *count;              // bins found by this update (zero on entry)
    unsigned int *count_next;         // the next update's counter: zeroed by the clearing kernel
    unsigned long long *result;       // where the clearing kernel leaves *count (a word of the result block)
    double ox, oy, inv_bx, inv_by;    // map origin, 1 / bin size (computed once in double on the host)
    double th_scale;                  // n_theta / (2 pi)
    double nx_d, ny_d;                // bins per axis (as doubles: the range test happens before any conversion)
    double nth_d, inv_nth;            // n_theta and its reciprocal
    uint32_t nx, ny, nth;
    uint32_t outside;                 // nx * ny * n_theta: the bin of every pose off the grid, non-finite or with |theta| >= 1e9
};

// bin of a pose: ix = floor((x - ox) * inv_bx), iy alike, it = floor((theta + pi) * th_scale) mod n_theta; each an add or
// subtract followed by a multiply (no form FMA contraction could fuse: the host restatement agrees bit for bit)
__host__ __device__ __forceinline__ uint32_t kld_bin(const KldArgs &k, double x, double y, double th)
{
    const double fx = floor((x - k.ox) * k.inv_bx), fy = floor((y - k.oy) * k.inv_by);
    if (!(fx >= 0.0 && fx < k.nx_d && fy >= 0.0 && fy < k.ny_d && fabs(th) < 1e9)) return k.outside;   // (NaN fails every test)
    // the heading bin: t mod n_theta of the integral t, in double (an emulated 64-bit remainder is a long sequence per child).
    // Below 2^52 the quotient from the reciprocal is off by at most one and q * n_theta, t - q * n_theta are exact integers,
    // so one correction gives the exact remainder; beyond (only with tens of millions of heading bins) the integer form.
    const double t = floor((th + 3.14159265358979323846) * k.th_scale);
    uint32_t it;
    if (fabs(t) < 4503599627370496.0) {
        double r = t - floor(t * k.inv_nth) * k.nth_d;
        if (r < 0.0) r += k.nth_d;
        else if (r >= k.nth_d) r -= k.nth_d;
        it = (uint32_t)r;
    } else {
        int64_t i = (int64_t)t % (int64_t)k.nth;
        if (i < 0) i += (int64_t)k.nth;
        it = (uint32_t)i;
    }
    // (every partial index is below nx * ny * n_theta <= 2^31)
    return (it * k.ny + (uint32_t)fy) * k.nx + (uint32_t)fx;
}

// mcl_group_update: the maximum over the shards' maxima, read where they live (peer pointers)
struct GroupMaxArgs { const double *src[kMaxShards]; int n; double *out; };

}  // namespace mcl
