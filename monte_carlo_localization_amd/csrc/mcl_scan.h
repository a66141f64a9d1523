// mcl_scan.h -- K5: the exact uint64 scan of the fixed-point weights (k_scan_*: the resampling CDF, its leaders and the compact
// list of the particles that carry weight), and the grid of the K4 / K7 reductions its spine finishes.
#pragma once

namespace mcl {

// K5: inclusive scan of uint64.  2048 items per 256-thread block (8 per thread), three launches:
// per-block totals -> single-block exclusive scan of the totals -> block-local scan + offset.
// Integer addition is associative, so the result does not depend on N, the block size or the
// number of GPUs the particle set is sharded over.
constexpr int kRedBlocks = 1024;              // K4 / K7 reductions (below): fixed grid, fixed-order final pass
constexpr int kRedThreads = 256;
__device__ __forceinline__ void final_sums_of(const double *__restrict__ part, int nb, double *__restrict__ scalars, double (*sm)[7]);

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        uint64_t t = (uint64_t)__shfl_up((long long)v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Order-preserving list of the particles with a non-zero fixed-point weight ("alive"), produced by the CDF scan itself.
// After an update with a thousand beams a few per cent of the particles carry all the weight (3.5 % at 4M x 1081 on
// Spielberg_map): the next update's resampling searches and gathers from this list -- 1 MB of CDF and 5 MB of records,
// cache-resident -- instead of the 33 MB CDF and the 134 MB of parent records, and a sharded set exchanges the lists
// instead of every weight.  A particle with q = 0 can never be selected (E6: the first i with
// C_i * lmul > rhs has q_i > 0), so the draw from the list equals the draw from the full CDF.
struct CompactOut {
    uint32_t *block_cnt;        // [tiles]: alive per scan tile -> exclusive prefix (k_scan_spine); null = no list wanted
    uint64_t *ccdf;             // CDF value at every alive particle (strictly increasing)
    uint32_t *cidx;             // its index
    double4 *crec;              // its record (x, y, theta, -)
    uint64_t *ctop;             // ccdf[64 g + 63] for every complete group of 64 entries: the search's first level
    const double *x, *y, *th;
    uint32_t cap;               // room in the arrays above
    unsigned long long *total;  // alive particles of this scan (may exceed cap: the list is then unusable)
    // the list's guide (mcl_compact_guide.h), or null: guide[b] = first entry at or above the boundary b << s, s from guide_m and
    // the grand total the spine left in *q_total before this kernel started
    uint32_t *guide;
    const uint64_t *q_total;
    int guide_m;
};
constexpr int kCompactGroupShift = 6;
constexpr uint32_t kGuideInline = 4;       // guide words an entry's thread writes alone; a longer range is filled by its wave

__global__ __launch_bounds__(kScanThreads) void k_scan_partials(const uint64_t *__restrict__ q, int64_t n,
                                                               uint64_t *__restrict__ block_tot, uint32_t *__restrict__ block_cnt)
{
    __shared__ uint64_t sm[kScanThreads / 64];
    __shared__ uint32_t smc[kScanThreads / 64];
    int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint64_t s = 0;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) { const uint64_t v = q[base + k]; s += v; c += v != 0ull; }
    s = wave_sum_u64(s);
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (block_cnt) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    }
    if (lane == 0) { sm[w] = s; smc[w] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        uint32_t tc = 0;
        for (int i = 0; i < kScanThreads / 64; ++i) { t += sm[i]; tc += smc[i]; }
        block_tot[blockIdx.x] = t;
        if (block_cnt) block_cnt[blockIdx.x] = tc;
    }
}

// exclusive scan of nb block totals in place (single block of 1024 threads), adds `offset`; the alive counts likewise.
// sum_part (optional): the per-workgroup partial sums k_weights has just left -> scalars[1..7], what a k_final_sums launch in
// between would do (this kernel is one workgroup anyway and runs after k_weights).
__global__ __launch_bounds__(1024) void k_scan_spine(uint64_t *__restrict__ block_tot, int nb, uint64_t offset,
                                                     uint64_t *__restrict__ grand_total, uint32_t *__restrict__ block_cnt,
                                                     unsigned long long *__restrict__ alive_total,
                                                     const double *__restrict__ sum_part = nullptr, int n_sum_part = 0, double *__restrict__ scalars = nullptr,
                                                     uint64_t *__restrict__ guide_total = nullptr)      // the grand total once more: CompactOut::q_total
{
    __shared__ uint64_t sm[16];
    if (sum_part) {
        __shared__ double sums_sm[kRedThreads / 64][7];
        final_sums_of(sum_part, n_sum_part, scalars, sums_sm);
    }
    __shared__ uint32_t smc[16];
    __shared__ uint64_t carry_s;
    __shared__ uint32_t carry_c;
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) { carry_s = offset; carry_c = 0u; }
    __syncthreads();
    for (int base = 0; base < nb; base += 1024) {
        int i = base + threadIdx.x;
        uint64_t v = (i < nb) ? block_tot[i] : 0;
        uint32_t vc = (block_cnt && i < nb) ? block_cnt[i] : 0u;
        uint64_t inc = wave_incl_scan_u64(v, lane);
        uint32_t incc = vc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incc, o, 64); if (lane >= o) incc += t; }
        if (lane == 63) { sm[w] = inc; smc[w] = incc; }
        __syncthreads();
        uint64_t woff = 0;
        uint32_t woffc = 0;
        for (int k = 0; k < w; ++k) { woff += sm[k]; woffc += smc[k]; }
        uint64_t carry = carry_s;
        uint32_t carryc = carry_c;
        if (i < nb) {
            block_tot[i] = carry + woff + inc - v;
            if (block_cnt) block_cnt[i] = carryc + woffc + incc - vc;
        }
        __syncthreads();
        if (threadIdx.x == 1023) { carry_s = carry + woff + inc; carry_c = carryc + woffc + incc; }
        __syncthreads();
    }
    if (threadIdx.x == 0 && grand_total) *grand_total = carry_s;
    if (threadIdx.x == 0 && guide_total) *guide_total = carry_s;
    if (threadIdx.x == 0 && alive_total) *alive_total = (unsigned long long)carry_c;
}

// `leaders` (optional) receives the last CDF entry of every 16-entry (128-byte) group: a 16x smaller copy the
// resampling search walks instead of the CDF itself, so that it fetches one CDF line per child, not seven
constexpr int kLeaderShift = 4;
__global__ __launch_bounds__(kScanThreads) void k_scan_final(const uint64_t *__restrict__ q, int64_t n,
                                                            const uint64_t *__restrict__ block_off,
                                                            uint64_t *__restrict__ cdf, uint64_t *__restrict__ leaders, CompactOut co)
{
    __shared__ uint64_t sm[kScanThreads / 64];
    __shared__ uint32_t smc[kScanThreads / 64];
    int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint64_t v[kScanItems];
    uint64_t s = 0;
    uint32_t alive = 0;                      // bit k: item k has a non-zero weight
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        uint64_t x = (base + k < n) ? q[base + k] : 0;
        s += x;
        v[k] = s;
        alive |= (x != 0ull ? 1u : 0u) << k;
    }
    int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = wave_incl_scan_u64(s, lane);
    const uint32_t cnt = (uint32_t)__popc(alive);
    uint32_t incc = cnt;
    if (co.block_cnt) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(incc, o, 64); if (lane >= o) incc += t; }
    }
    if (lane == 63) { sm[w] = inc; smc[w] = incc; }
    __syncthreads();
    uint64_t off = block_off[blockIdx.x] + inc - s;
    for (int k = 0; k < w; ++k) off += sm[k];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) cdf[base + k] = off + v[k];
    if (leaders) {
        static_assert(kScanItems == 8 && (1 << kLeaderShift) == 16, "a leader is the last item of every second thread");
        const int64_t last = base + kScanItems - 1;
        if ((last & 15) == 15 && last < n) leaders[last >> kLeaderShift] = off + v[kScanItems - 1];
        else if (base < n && n - 1 <= last && ((n - 1) & 15) != 15) leaders[(n - 1) >> kLeaderShift] = off + v[(n - 1) - base];   // ragged last group
    }
    uint32_t pos0 = 0;
    if (co.block_cnt) {
        pos0 = co.block_cnt[blockIdx.x] + incc - cnt;
        for (int k = 0; k < w; ++k) pos0 += smc[k];
    }
    if (co.block_cnt && alive) {
        uint32_t pos = pos0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k)
            if ((alive >> k) & 1u) {
                if (pos < co.cap) {
                    const int64_t i = base + k;
                    const uint64_t c = off + v[k];
                    co.ccdf[pos] = c;
                    co.cidx[pos] = (uint32_t)i;
                    co.crec[pos] = make_double4(co.x[i], co.y[i], co.th[i], 0.0);
                    if ((pos & ((1u << kCompactGroupShift) - 1u)) == (1u << kCompactGroupShift) - 1u) co.ctop[pos >> kCompactGroupShift] = c;
                }
                ++pos;
            }
    }
    if (co.block_cnt && co.guide) {
        // The guide words of this thread's entries (guide_owner_range: every word has one owner, so nothing is cleared first).
        // An entry that owns a few words writes them itself; a longer range -- one particle with all the weight owns every word --
        // is handed to the wave: ballot, broadcast, 64 words per store.  Every lane of the wave comes through here, whatever it holds.
        const int gs = guide_shift(*co.q_total, co.guide_m);
        uint32_t pos = pos0;
#pragma unroll
        for (int k = 0; k < kScanItems; ++k) {
            const bool mine = ((alive >> k) & 1u) && pos < co.cap;
            uint32_t b0 = 0u, b1 = 0u;
            if (mine) guide_owner_range(off + v[k], v[k] - (k ? v[k - 1] : 0ull), gs, pos, b0, b1);
            const uint32_t nb = b1 - b0;
            if (nb <= kGuideInline)
                for (uint32_t j = 0; j < nb; ++j) co.guide[b0 + j] = pos;
            for (unsigned long long wide = __ballot(nb > kGuideInline); wide; wide &= wide - 1ull) {
                const int l = __ffsll((long long)wide) - 1;
                const uint32_t wb0 = (uint32_t)__shfl((int)b0, l), wnb = (uint32_t)__shfl((int)nb, l), wpos = (uint32_t)__shfl((int)pos, l);
                for (uint32_t j = (uint32_t)lane; j < wnb; j += 64u) co.guide[wb0 + j] = wpos;
            }
            pos += (alive >> k) & 1u;
        }
    }
}

}  // namespace mcl
