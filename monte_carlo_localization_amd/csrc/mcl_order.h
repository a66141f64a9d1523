// mcl_order.h -- the ordering of the particles by (tile, cell, heading): bounding box and tiles, the counting sort over per-XCD
// histograms, the keys and the gather of the radix path, the slice means.
#pragma once

namespace mcl {

// ---- cell sort: particles ordered by (32x32 tile, cell in tile, heading) ---------------------------------
//
// k_rays_cell gives every LANE one particle and walks that particle's beams; the 64 lanes of a wave then trace
// near-parallel rays (same beam slot of the same direction range) and, once the particles are ordered by grid cell
// and heading, from almost the same origin: their trip counts are nearly equal and the wave no longer waits for
// its slowest lane.  The order is a counting sort: bucket = (tile-major cell id << theta_bits) | quantised
// heading over the bounding box of the particle set, as fine as fits kSortKeySpace.
//
// The histogram is kept once per XCD, hist[xcd][bucket]: a workgroup only touches the copy of the XCD it runs on,
// so its atomics can be workgroup-scope and execute in that XCD's L2 instead of at the memory side (device-scope
// atomics from eight XCDs on the same hot counters took 0.5 ms per update, these take 0.1).  The value an atomic
// returns is the particle's rank inside (bucket, xcd); the scan orders the counters bucket-major, xcd-minor.  The
// rank order varies from run to run — harmless: the order only decides which rays share a wave, every log-weight
// is an exact sum.
// (the key itself -- kSortKeySpace, SortLayout, sort_layout, sort_key, cell_of -- is in mcl_sort_key.h: host and device)
constexpr int kSortXcds = 8;                        // copies of the histogram (XCC_ID & 7)
constexpr uint32_t kSortBuckets = kSortKeySpace * kSortXcds;
constexpr int kHistTile = 4096;                     // entries per workgroup of the bucket scan

// bbox[0..3] = min cx, min cy, max cx, max cy over every `stride`-th particle (initialised to +big / -big by the
// host).  A sample is enough: sort_key clamps cells into the box, so a particle outside it merely lands in an
// edge bucket (the order is a performance matter only).
// bbox as PrepClear leaves it: empty box, no tiles numbered, [6] = the window play sort_layout works with
__global__ void k_bbox_init(int *__restrict__ bbox, int play)
{
    const int i = threadIdx.x;
    if (i < 7) bbox[i] = i < 2 ? 0x7fffffff : (i < 4 ? (int)0x80000000 : (i == 6 ? play : 0));
}

__global__ __launch_bounds__(256) void k_cell_bbox(const double4 *__restrict__ pc, int64_t n, int stride, int Wp, int Hp, int *__restrict__ bbox,
                                                  int *__restrict__ tilemark = nullptr, int ntx_abs = 0)
{
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = -1, y1 = -1;
    const int64_t ns = (n + stride - 1) / stride;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ns; k += (int64_t)gridDim.x * blockDim.x) {
        const double4 c = pc[k * stride];
        const int cx = cell_of(c.z * kSortSub, Wp * kSortSub - 1), cy = cell_of(c.w * kSortSub, Hp * kSortSub - 1);
        x0 = min(x0, cx); y0 = min(y0, cy); x1 = max(x1, cx); y1 = max(y1, cy);
        if (tilemark) tilemark[(cy >> 5) * ntx_abs + (cx >> 5)] = 1;      // occupied tiles of the map (k_tile_compact)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)); y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64)); y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    // one set of atomics per workgroup: same-address atomics serialise at ~12 ns each
    __shared__ int red[4][4];
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[w][0] = x0; red[w][1] = y0; red[w][2] = x1; red[w][3] = y1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { x0 = min(x0, red[k][0]); y0 = min(y0, red[k][1]); x1 = max(x1, red[k][2]); y1 = max(y1, red[k][3]); }
        if (x1 >= 0) { atomicMin(&bbox[0], x0); atomicMin(&bbox[1], y0); atomicMax(&bbox[2], x1); atomicMax(&bbox[3], y1); }
    }
}

// Occupied tiles.  The key of a particle starts with its 32 x 32-cell tile; numbering only the tiles that hold (sampled)
// particles instead of every tile of the bounding box gives the bits of the empty ones -- most of them when the set sits on
// a few far-apart clusters -- back to cells and heading.  bbox[4] = number of occupied tiles T, bbox[5] = 1 when the
// numbering is in use (a bounding box of at most kSortMaxTiles tiles); tilemap[t] = compact id, T for a tile no sampled
// particle fell into (its particles share one overflow tile: the order is a performance matter only).
constexpr int kSortMaxTiles = 8192;
// tilemark[t] (set by k_cell_bbox for the tiles of the MAP its sampled particles fall into) -> tilemap[t] = compact id,
// T for an unmarked tile; the marks are zeroed for the next update.  One workgroup, ntiles_abs <= kSortMaxTiles.
__global__ __launch_bounds__(1024) void k_tile_compact(int *__restrict__ bbox, int *__restrict__ tilemark, int *__restrict__ tilemap, int ntiles_abs)
{
    __shared__ int ws[16];
    __shared__ int carry_sh;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_sh = 0;
    __syncthreads();
    for (int t0 = 0; t0 < ntiles_abs; t0 += 1024) {
        const int t = t0 + (int)threadIdx.x;
        const int m = (t < ntiles_abs && tilemark[t] != 0) ? 1 : 0;
        int inc = m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
        if (lane == 63) ws[wv] = inc;
        __syncthreads();
        int id = carry_sh + inc - m;
        for (int k = 0; k < wv; ++k) id += ws[k];
        if (t < ntiles_abs) { tilemap[t] = m ? id : -1; tilemark[t] = 0; }
        __syncthreads();
        if (threadIdx.x == 1023) carry_sh = id + m;
        __syncthreads();
    }
    const int T = carry_sh;
    for (int t = threadIdx.x; t < ntiles_abs; t += 1024)
        if (tilemap[t] < 0) tilemap[t] = T;           // (written by this thread in the loop above: t = t0 + threadIdx.x)
    if (threadIdx.x == 0) { bbox[4] = T; bbox[5] = 1; }
}

__global__ __launch_bounds__(256) void k_sort_hist(const double4 *__restrict__ pc, const double *__restrict__ th, int64_t n, int Wp, int Hp,
                                                  const int *__restrict__ bbox, uint32_t *__restrict__ hist,
                                                  uint32_t *__restrict__ key_out, uint32_t *__restrict__ rank_out, uint32_t *__restrict__ tile_used,
                                                  const int *__restrict__ tilemap, int ntx_abs)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t xcd = (uint32_t)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) & (kSortXcds - 1);   // HW_REG_XCC_ID[3:0]
    const double4 c = pc[i];
    const uint32_t key = sort_key(bbox, tilemap, ntx_abs, cell_of(c.z * kSortSub, Wp * kSortSub - 1), cell_of(c.w * kSortSub, Hp * kSortSub - 1), th[i], n,
                                  c.z * kSortSub - floor(c.z * kSortSub), c.w * kSortSub - floor(c.w * kSortSub));
    key_out[i] = key;
    // this XCD's private copy: workgroup scope keeps the read-modify-write in the local L2
    const uint32_t r = __hip_atomic_fetch_add(&hist[(size_t)xcd * kSortKeySpace + key], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    rank_out[i] = (xcd << 28) | r;
    // the first arrival in a counter marks its tile of kHistTile buckets as used: the scan and the clearing of the
    // histogram then touch the used tiles only (a collapsed set uses a few dozen of the 1024)
    if (r == 0u) tile_used[key / kHistTile] = 1u;
}

// totals of kHistTile buckets (over all XCD copies) per workgroup: part[t], zero for a tile nobody fell into
__global__ __launch_bounds__(256) void k_hist_partials(const uint32_t *__restrict__ hist, uint32_t *__restrict__ part, const uint32_t *__restrict__ tile_used)
{
    __shared__ uint32_t ws[4];
    if (!tile_used[blockIdx.x]) {                 // wave-uniform
        if (threadIdx.x == 0) part[blockIdx.x] = 0u;
        return;
    }
    uint32_t s = 0;
    for (int x = 0; x < kSortXcds; ++x) {
        const uint4 *p = reinterpret_cast<const uint4 *>(hist + (size_t)x * kSortKeySpace + (size_t)blockIdx.x * kHistTile) + threadIdx.x * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) { uint4 v = p[k]; s += v.x + v.y + v.z + v.w; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// in place: counter (bucket b, xcd x) -> first slot of that group in the order bucket-major, xcd-minor
__global__ __launch_bounds__(256) void k_hist_final(uint32_t *__restrict__ hist, const uint32_t *__restrict__ part, const uint32_t *__restrict__ tile_used)
{
    __shared__ uint32_t ws[4], ps[4];
    if (!tile_used[blockIdx.x]) return;           // no particle in these buckets: nobody reads their offsets
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // slots in front of this tile: the totals of the tiles before it, summed here (at most 1023 words out of L2, by the used
    // tiles only) instead of scanned by a one-workgroup launch in between
    uint32_t pre = 0;
    for (int t = (int)threadIdx.x; t < (int)blockIdx.x; t += 256) pre += part[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o, 64);
    if (lane == 0) ps[w] = pre;
    const size_t b0 = (size_t)blockIdx.x * kHistTile + (size_t)threadIdx.x * 16;    // 16 consecutive buckets per thread
    uint4 v[kSortXcds][4];
    uint32_t s = 0;
#pragma unroll
    for (int x = 0; x < kSortXcds; ++x) {
        const uint4 *p = reinterpret_cast<const uint4 *>(hist + (size_t)x * kSortKeySpace + b0);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[x][k] = p[k]; s += v[x][k].x + v[x][k].y + v[x][k].z + v[x][k].w; }
    }
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { uint32_t t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) ws[w] = inc;
    __syncthreads();
    uint32_t run = ps[0] + ps[1] + ps[2] + ps[3] + inc - s;
    for (int k = 0; k < w; ++k) run += ws[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // bucket 4k..4k+3 of this thread: the xcd copies in turn
#pragma unroll
        for (int x = 0; x < kSortXcds; ++x) { uint32_t c = v[x][k].x; v[x][k].x = run; run += c; }
#pragma unroll
        for (int x = 0; x < kSortXcds; ++x) { uint32_t c = v[x][k].y; v[x][k].y = run; run += c; }
#pragma unroll
        for (int x = 0; x < kSortXcds; ++x) { uint32_t c = v[x][k].z; v[x][k].z = run; run += c; }
#pragma unroll
        for (int x = 0; x < kSortXcds; ++x) { uint32_t c = v[x][k].w; v[x][k].w = run; run += c; }
    }
#pragma unroll
    for (int x = 0; x < kSortXcds; ++x) {
        uint4 *p = reinterpret_cast<uint4 *>(hist + (size_t)x * kSortKeySpace + b0);
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = v[x][k];
    }
}

__global__ __launch_bounds__(256) void k_sort_scatter(const double4 *__restrict__ pc, const double *__restrict__ th, int64_t n,
                                                     const uint32_t *__restrict__ key, const uint32_t *__restrict__ rank,
                                                     const uint32_t *__restrict__ start, double4 *__restrict__ pcs,
                                                     double *__restrict__ ths, uint32_t *__restrict__ perm)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t rk = rank[i];
    const uint32_t slot = start[(size_t)(rk >> 28) * kSortKeySpace + key[i]] + (rk & 0x0FFFFFFFu);
    if (slot >= (uint64_t)n) return;                       // cannot happen (the counts sum to n); never write out of bounds
    pcs[slot] = pc[i];
    ths[slot] = th[i];
    perm[slot] = (uint32_t)i;
}

// ---- the same ordering through a radix sort of (key, index) pairs (MCL_SORT=radix): keys only, no atomics; the sort itself is
//      rocPRIM's (a plain library sort, like a library GEMM would be), the gather puts the records in sorted order ----
__global__ __launch_bounds__(256) void k_sort_keys(const double4 *__restrict__ pc, const double *__restrict__ th, int64_t n, int Wp, int Hp,
                                                  const int *__restrict__ bbox, uint32_t *__restrict__ key_out, uint32_t *__restrict__ val_out,
                                                  const int *__restrict__ tilemap, int ntx_abs, int fine)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double4 c = pc[i];
    key_out[i] = sort_key(bbox, tilemap, ntx_abs, cell_of(c.z * kSortSub, Wp * kSortSub - 1), cell_of(c.w * kSortSub, Hp * kSortSub - 1), th[i], n,
                          c.z * kSortSub - floor(c.z * kSortSub), c.w * kSortSub - floor(c.w * kSortSub), fine);
    val_out[i] = (uint32_t)i;
}
// cut_start[g] + 1 / cut_end[g]: first slot + 1 and end of bucket g in the sorted order (0 / anything: nobody there), written where
// the sorted keys change bucket -- what k_unit_table needs to cut a sparse set's units at bucket borders (it zeroes the
// entries it reads).  sorted_keys null: no borders wanted.  fine: the fine bits the keys were made with (dropped with the rest below a group).
__global__ __launch_bounds__(256) void k_sort_gather(const double4 *__restrict__ pc, const double *__restrict__ th, int64_t n,
                                                    const uint32_t *__restrict__ order, double4 *__restrict__ pcs, double *__restrict__ ths,
                                                    uint32_t *__restrict__ perm, const uint32_t *__restrict__ sorted_keys = nullptr,
                                                    const int *__restrict__ bbox = nullptr, uint32_t *__restrict__ cut_start = nullptr,
                                                    uint32_t *__restrict__ cut_end = nullptr, int fine = 0, int heading_form = 0)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const uint32_t i = order[s];
    // heading_form: pc holds (heading, 0, pixel x, pixel y) -- one scattered fetch per particle instead of two, and the sincos
    // of the constants is taken here, where the SIMDs wait for those fetches (same function, same argument: the same bits)
    const double4 rec = pc[i];
    if (heading_form) { pcs[s] = particle_constants_of(rec); ths[s] = rec.x; }
    else { pcs[s] = rec; ths[s] = th[i]; }
    perm[s] = i;
    if (sorted_keys) {
        const SortLayout L = sort_layout(bbox, n, fine);
        if (L.cuts()) {
            const int sh = L.cut_shift();
            const uint32_t g = sorted_keys[s] >> sh;
            const uint32_t gp = s > 0 ? sorted_keys[s - 1] >> sh : 0xFFFFFFFFu;
            if (g != gp && g < (uint32_t)kSwMaxCuts) {
                cut_start[g] = (uint32_t)s + 1u;
                if (s > 0 && gp < (uint32_t)kSwMaxCuts) cut_end[gp] = (uint32_t)s;
            }
            if (s == n - 1 && g < (uint32_t)kSwMaxCuts) cut_end[g] = (uint32_t)n;
        }
    }
}

// after the scatter: the used tiles of the histogram (all XCD copies) and their marks back to zero, so that the next
// update starts from an all-zero histogram without a pass over its 128 MB
__global__ __launch_bounds__(256) void k_hist_clear(uint32_t *__restrict__ hist, uint32_t *__restrict__ tile_used)
{
    if (!tile_used[blockIdx.x]) return;
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (int x = 0; x < kSortXcds; ++x) {
        uint4 *p = reinterpret_cast<uint4 *>(hist + (size_t)x * kSortKeySpace + (size_t)blockIdx.x * kHistTile) + threadIdx.x * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) p[k] = z;
    }
    __syncthreads();
    if (threadIdx.x == 0) tile_used[blockIdx.x] = 0u;
}

// mean pixel position of every slice of `per` sorted particles (non-finite positions excluded): k_rays_cell centres
// the sixteen wedge windows of a slice on it
__global__ __launch_bounds__(256) void k_slice_means(const double4 *__restrict__ pcs, int64_t n, int64_t per, double2 *__restrict__ out)
{
    __shared__ double sm[4][3];
    const int64_t p_begin = (int64_t)blockIdx.x * per;
    const int64_t p_end = (p_begin + per < n) ? p_begin + per : n;
    double sx = 0.0, sy = 0.0, cnt = 0.0;
    for (int64_t s = p_begin + threadIdx.x; s < p_end; s += blockDim.x) {
        const double4 c = pcs[s];
        if (c.z == c.z && c.w == c.w && fabs(c.z) < 1e9 && fabs(c.w) < 1e9) { sx += c.z; sy += c.w; cnt += 1.0; }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = sx; sm[threadIdx.x >> 6][1] = sy; sm[threadIdx.x >> 6][2] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sx = sm[0][0] + sm[1][0] + sm[2][0] + sm[3][0];
        sy = sm[0][1] + sm[1][1] + sm[2][1] + sm[3][1];
        cnt = sm[0][2] + sm[1][2] + sm[2][2] + sm[3][2];
        out[blockIdx.x] = cnt > 0.0 ? make_double2(sx / cnt, sy / cnt) : make_double2(0.0, 0.0);
    }
}

}  // namespace mcl
