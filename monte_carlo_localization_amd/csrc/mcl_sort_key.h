// The key the ray stage orders the particles by: how its bits are split for an update's set (sort_layout) and the key of one
// particle (sort_key).  Host and device: the ordering kernels of mcl_order.h and the resampling kernel make keys with these
// functions, mcl_host_sort_key (mcl_host_math.hip) is the same code run on the CPU.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace mcl {

#ifndef MCL_SORT_SUB
#define MCL_SORT_SUB 1
#endif
constexpr int kSortSub = MCL_SORT_SUB;               // sort cells per grid cell and axis (the ordering kernels)

// (22 key bits and half cells for the COARSE key: what units, cuts, windows and the counting sort's histogram see.  24 bits /
//  quarter cells and 26 bits / eighths were built and measured at the end of round 5: the ray kernel of the bench workload issues the
//  same number of instructions launch for launch with all three -- the density gate of sort_layout, not the key space, ends the
//  split there, so the order is the same -- and yet runs 1 % faster or slower: with where the buffers lie (the histogram allocation
//  is 128 MB / 512 MB / 2 GB), which is all that is left to differ: profiles/r05_experiments/sort_key_bits.txt.  Not taken.
//  Bits BELOW the coarse key are another matter -- they cost no histogram and no layout decision, only sort passes: the FINE bits
//  of the radix path, SortLayout::fine below, profiles/sort_fine.md.)
#ifndef MCL_SORT_KEY_LOG2
#define MCL_SORT_KEY_LOG2 22
#endif
constexpr int kSortKeyLog2 = MCL_SORT_KEY_LOG2;
constexpr uint32_t kSortKeySpace = 1u << kSortKeyLog2;
#ifndef MCL_SORT_MAX_SUB
#define MCL_SORT_MAX_SUB 1
#endif
constexpr int kSortMaxFine = 10;                    // fine bits a key may carry below the coarse ones (22 + 10 = 32)
static_assert(kSortKeyLog2 + kSortMaxFine <= 32, "a key is one 32-bit word");
// Fine bits the radix ordering path carries unless MCL_SORT_FINE says otherwise: two, both sub-cell bits -- one more bit of the
// position inside the cell per axis, i.e. quarter cells (24 key bits: still three 8-bit passes of the library sort).
// profiles/sort_fine.md has the measurement: further heading bits gain the ray kernel nothing, position bits do.
#ifndef MCL_SORT_FINE_DEFAULT
#define MCL_SORT_FINE_DEFAULT 2
#endif
#ifndef MCL_SORT_FINE_SUB_DEFAULT
#define MCL_SORT_FINE_SUB_DEFAULT 1
#endif
constexpr int kSortFineDefault = MCL_SORT_FINE_DEFAULT;
constexpr int kSortFineSubDefault = MCL_SORT_FINE_SUB_DEFAULT;      // sub-cell bits per axis among them (-1: the rule of SortLayout)

__host__ __device__ __forceinline__ int cell_of(double g, int hi)
{
    // padded cell coordinate of a pixel coordinate, clamped into the padded grid (NaN -> 0)
    int c = (g > -1.0) ? ((g < 1e9) ? (int)floor(g) + 1 : hi) : 0;
    return c < 0 ? 0 : (c > hi ? hi : c);
}

#ifndef MCL_SORT_SUB_GATE
#define MCL_SORT_SUB_GATE 32.0
#endif
constexpr double kSortSubGate = MCL_SORT_SUB_GATE;  // particles a bucket must hold (an eighth of its heading bins taken as occupied) to be split in four
constexpr int kSortMaxSub = MCL_SORT_MAX_SUB;        // sub-cell bits per axis a dense set may get (0: none)
// How the key bits are split for this update's set: a pure function of the bounding box / occupied-tile count and n, so that
// every particle -- and k_unit_table, which needs to know where a tile's keys start -- derives the same layout.
//   coarse = ((((tile << inner | iy) << inner | ix) << ss | sy) << ss | sx) << tb | heading bin
//   key    = coarse << fine | (((next fs bits of sy) << fs | next fs bits of sx) << ft | next ft bits of the heading)
// fine (0 .. kSortMaxFine) is handed in by the caller -- the engine's one setting on the radix ordering path, 0 on the counting-sort
// path and for k_unit_table -- and splits as fs = max(fine - 2, 0) / 4 sub-cell bits per axis and ft = fine - 2 fs heading bits:
// 2 -> two heading bits, 6 -> quarter cells and four heading bits, 10 -> eighths and six -- unless the caller names fs itself
// (sort_fine_code: the setting travels as ONE word, fine | (fs + 1) << 4; 2 with fs = 1 is quarter cells and no further heading
// bit, which is what the ray kernel gains from: profiles/sort_fine.md).  The fine bits only order the
// particles INSIDE a coarse bucket (which 64 of them share a wave): every reader of a key drops them first (tile_shift /
// cut_shift count them), so units, cuts, windows and the plan are what they are without them.
struct SortLayout {
    int cs, tb, inner, ss;
    int fine;                         // key bits below the coarse key
    int fsub;                         // fs: how many of them, per axis, are sub-cell bits
    uint32_t ntx;
    int tx0, ty0;
    bool compact;
    bool nocut;                       // bbox[6] < 0 (MCL_NO_BUCKET_CUTS): the plain grid of units, sparse sets by whole tiles
    bool sparse;                      // ordered by whole buckets of 2^cs x 2^cs cells (a spread cloud): units are cut at their borders
    uint64_t ntiles;
    __host__ __device__ __forceinline__ int fine_sub() const { return fsub; }                              // fs: sub-cell bits per axis among the fine bits
    __host__ __device__ __forceinline__ int fine_heading() const { return fine - 2 * fine_sub(); }         // ft: heading bits among them
    __host__ __device__ __forceinline__ int tile_shift() const { return 2 * inner + 2 * ss + tb + fine; }
    // Units are cut where the sorted order changes GROUP: a sparse set's bucket, a dense set's 32 x 32 tile (a set that sits on
    // a few far-apart clusters -- the steady state of a global re-localisation -- otherwise has units that end in one cluster
    // and begin in the next, whose minority side no window reaches: 0.85 ms of far pass per update at 4M on ~30 clusters).
    __host__ __device__ __forceinline__ int cut_shift() const { return sparse ? 2 * ss + tb + fine : tile_shift(); }          // key bits below the group
    __host__ __device__ __forceinline__ uint64_t cut_groups() const { return sparse ? ntiles << (2 * inner) : ntiles; }       // groups of the key space
    // (k_sort_gather notes the borders, k_unit_table uses them: one rule for both)
    __host__ __device__ __forceinline__ bool cuts() const;
};
// the fine setting as one word: the bits, and -- when the split is not the rule's -- the sub-cell bits per axis
__host__ __device__ __forceinline__ int sort_fine_code(int fine, int fs = -1) { return (fine & 15) | (fs >= 0 ? (fs + 1) << 4 : 0); }
__host__ __device__ __forceinline__ int sort_fine_bits(int code) { const int f = code & 15; return f > kSortMaxFine ? kSortMaxFine : f; }
constexpr int kSwMaxCuts = 65536;     // buckets up to which a sparse set's units are cut at bucket borders (k_unit_table)
__host__ __device__ __forceinline__ bool SortLayout::cuts() const
{
    return compact && !nocut && cut_groups() <= (uint64_t)kSwMaxCuts && (cut_groups() << (cut_shift() - fine)) <= kSortKeySpace;
}
__host__ __device__ __forceinline__ SortLayout sort_layout(const int *__restrict__ bbox, int64_t n, int fine = 0)      // fine: a sort_fine_code
{
    SortLayout L;
    L.fine = fine < 0 ? 0 : sort_fine_bits(fine);
    L.fsub = L.fine > 2 ? (L.fine - 2) / 4 : 0;
    if (fine > 0 && (fine >> 4) > 0) { L.fsub = (fine >> 4) - 1; if (2 * L.fsub > L.fine) L.fsub = L.fine / 2; }
    L.tx0 = bbox[0] >> 5; L.ty0 = bbox[1] >> 5;
    L.ntx = (uint32_t)((bbox[2] >> 5) - L.tx0 + 1);
    const uint32_t nty = (uint32_t)((bbox[3] >> 5) - L.ty0 + 1);
    L.compact = bbox[5] != 0;
    L.ntiles = L.compact ? (uint64_t)bbox[4] + 1u : (uint64_t)L.ntx * nty;       // + 1: the overflow tile
    // cells the set can be taken to live on: its bounding box, or its occupied tiles if that is less
    double cells_est = (double)(bbox[2] - bbox[0] + 1) * (double)(bbox[3] - bbox[1] + 1);
    if (L.compact && (double)bbox[4] * 1024.0 < cells_est) cells_est = (double)bbox[4] * 1024.0;
    // Heading first: the lanes of a wave must agree on which wedge their beams are in, so six heading bits (5.6 degrees)
    // are kept while the in-tile resolution is coarsened to make room (a particle set spread over a large bounding box
    // -- several far-apart clusters -- otherwise spends the whole key space on empty cells: 80 % slower ray stage);
    // only a bounding box of more than 2^14 tiles gives heading bits up.  What is left over goes to the heading.
    // A SPARSE set (fewer than 8 particles per cell of the bounding box: the uniform cloud of global localisation, or a
    // few far-apart clusters) is ordered by whole 32 x 32 tiles: 1024 consecutive particles cover hundreds of cells
    // whatever the bucket size, and with one bucket per tile the 64 particles of a wave are neighbours in heading
    // (first update of the global regime: ray kernel 13.8 -> 11.4 ms).  A dense set keeps single cells: there the
    // compactness of a unit is what the windows and the probe loop live on (coarser buckets cost 4-30 %).
    int cs = 0, tb = 6;
    L.nocut = bbox[6] < 0;
    L.sparse = cells_est > 0.0 && (double)n < 8.0 * cells_est;
    if (L.sparse) {
        cs = 5;
        // ... of the size the play of a ray window can hold: a unit is one bucket's particles, and a unit wider than the play
        // loses its particles to the far pass (the levine stand-in's 239-px range leaves 12 cells: whole tiles put 3.5M of the
        // 4M particles of a uniform cloud there, 35 ms).  Smaller buckets only while one still holds a couple of chunks.
        const int play = bbox[6];
        while (play > 0 && cs > 1 && (1 << cs) >= play - 2 && (double)n * (double)(1 << (2 * cs - 2)) >= 128.0 * cells_est) --cs;
    }
    while (cs < 5 && ((L.ntiles << (10 - 2 * cs + tb)) > kSortKeySpace)) ++cs;
    while (tb > 0 && ((L.ntiles << (10 - 2 * cs + tb)) > kSortKeySpace)) --tb;
    const int inner = 5 - cs;                             // log2 of the bucket grid inside one tile
    const uint64_t ncell = L.ntiles << (2 * inner);
    while (tb < 8 && (ncell << (tb + 1)) <= kSortKeySpace) ++tb;
    // Bits left over once the cells have their full resolution and the heading its eight bits go to the position inside
    // the cell (half cells, then quarter cells): a collapsed set is thousands of particles per cell, and rays that start
    // within half a cell of each other keep company longer (levine stand-in: ray kernel -10 %, Spielberg -3 %).
    int ss = 0;
    if (cs == 0 && tb == 8) {
        // ... as long as a bucket still holds a few waves' worth: particles per cell of the bounding box, an eighth of the
        // heading bins taken as occupied (262 144 particles on 25 cells are better off without: 43 per bucket)
        double per_bucket = cells_est > 0.0 ? (double)n / cells_est / 32.0 : 0.0;
        while (ss < kSortMaxSub && (ncell << (tb + 2 * (ss + 1))) <= kSortKeySpace && per_bucket >= kSortSubGate) { ++ss; per_bucket *= 0.25; }
    }
    L.cs = cs; L.tb = tb; L.inner = inner; L.ss = ss;
    return L;
}

// (cx, cy): sort cell of the particle (cell_of); (fx, fy): its position inside that cell; th: heading; fine: a sort_fine_code
__host__ __device__ __forceinline__ uint32_t sort_key(const int *__restrict__ bbox, const int *__restrict__ tilemap, int ntx_abs, int cx, int cy, double th,
                                                  int64_t n, double fx = 0.0, double fy = 0.0, int fine = 0)
{
    const bool in_box = cx >= bbox[0] && cx <= bbox[2] && cy >= bbox[1] && cy <= bbox[3];
    cx = cx < bbox[0] ? bbox[0] : (cx > bbox[2] ? bbox[2] : cx);
    cy = cy < bbox[1] ? bbox[1] : (cy > bbox[3] ? bbox[3] : cy);
    const SortLayout L = sort_layout(bbox, n, fine);
    const int cs = L.cs, tb = L.tb, inner = L.inner, ss = L.ss;
    uint32_t tile = (uint32_t)((cy >> 5) - L.ty0) * L.ntx + (uint32_t)((cx >> 5) - L.tx0);
    if (L.compact) tile = (uint32_t)tilemap[(cy >> 5) * ntx_abs + (cx >> 5)];
    const uint32_t ix = (uint32_t)(cx & 31) >> cs, iy = (uint32_t)(cy & 31) >> cs;
    uint64_t key = ((((uint64_t)tile << inner) | iy) << inner) | ix;
    if (ss > 0) {
        const uint32_t sx = (fx >= 0.0 && fx < 1.0) ? (uint32_t)(fx * (double)(1 << ss)) : 0u;
        const uint32_t sy = (fy >= 0.0 && fy < 1.0) ? (uint32_t)(fy * (double)(1 << ss)) : 0u;
        key = (((key << ss) | sy) << ss) | sx;
    }
    double f = th * 0.15915494309189533577;               // heading as a fraction of a turn
    f -= floor(f);
    uint32_t tq = (f >= 0.0 && f < 1.0) ? (uint32_t)(f * (double)(1u << tb)) : 0u;
    if (tq >> tb) tq = (1u << tb) - 1u;
    key = (key << tb) | tq;
    const uint32_t coarse = key < kSortKeySpace ? (uint32_t)key : kSortKeySpace - 1u;    // a bounding box beyond the key space: unsorted tail
    if (L.fine == 0) return coarse;
    // The fine bits: the same quantisations carried fs / ft bits further (a power of two times a double is exact, so the bits above
    // them are the coarse fields).  All zero unless every coarse field is the particle's own: its cell inside the box, its position
    // inside the cell, a finite heading below 2^32 rad (from there on the fraction of a turn has fewer good bits than tb + ft <= 18
    // may ask for), a coarse key inside the key space.
    const int fs = L.fine_sub(), ft = L.fine_heading();
    uint32_t low = 0u;
    if (in_box && key < kSortKeySpace && fx >= 0.0 && fx < 1.0 && fy >= 0.0 && fy < 1.0 && f >= 0.0 && f < 1.0 && fabs(th) < 4294967296.0) {
        const uint32_t qx = (uint32_t)(fx * (double)(1u << (ss + fs))) & ((1u << fs) - 1u);
        const uint32_t qy = (uint32_t)(fy * (double)(1u << (ss + fs))) & ((1u << fs) - 1u);
        const uint32_t qt = (uint32_t)(f * (double)(1u << (tb + ft))) & ((1u << ft) - 1u);
        low = (((qy << fs) | qx) << ft) | qt;
    }
    return (coarse << L.fine) | low;
}

}  // namespace mcl
