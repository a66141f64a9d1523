// mcl_resample.h -- K6 + K1 + K2: resample_motion_body and its twelve entry points (k_resample_motion* / k_resample_odo*),
// k_kld_clear, and the kernels of the sharded resampling: k_compact_merge, the k_bm_* bitmap of distinct parents, k_gather_records,
// k_pack_records.
#pragma once

namespace mcl {

// K6 + K1 + K2: one thread per child m (global child index child_first + m).
//   threshold:   multinomial  k53_m * Q   vs   C_i * 2^53      (k53 = floor(u*2^53), u Philox or injected)
//                systematic   (m*2^32 + k0) * Q   vs   C_i * (N_children * 2^32)
//   idx = first i with C_i*lmul > rhs  (C inclusive)  == upper_bound; Q == 0 -> idx = 0 (reference:
//   NaN CDF -> every draw returns 0).
//   then row gather (cpp:664) and the motion model (cpp:474-502) with the three normals.

__device__ __forceinline__ void prep_small_clear(const PrepClear &clr, int i, int nthreads)
{
    if (clr.fix_count) for (int k = i; k < clr.fix_words; k += nthreads) clr.fix_count[k] = 0ull;
    if (clr.fix_over && i < 2) clr.fix_over[i] = 0ull;
    if (clr.exact_count && i == 0) clr.exact_count[0] = 0ull;
    if (clr.far_count && i == 0) clr.far_count[0] = 0ull;
    if (clr.bbox && i < 7) clr.bbox[i] = i < 2 ? 0x7fffffff : (i < 4 ? (int)0x80000000 : (i == 6 ? clr.bbox_play : 0));
}

struct ResampleArgs {
    const double *px, *py, *pth;      // parents
    const uint64_t *cdf;              // inclusive CDF over parents
    const uint64_t *tile_excl;        // exclusive prefix before each kScanTile-sized tile of the CDF (the scan's spine)
    const uint64_t *leaders;          // last CDF entry of every 16-entry group (with tile_excl), or null
    const double4 *ppack;             // parents as (x, y, theta, -) records: one fetch per gathered parent, or null
    double4 *cpack;                   // children in the same form for the next update, or null
    int64_t n_parents;
    uint64_t q_total;
    double *cx, *cy, *cth;            // children out
    int32_t *idx_out;                 // may be null
    int64_t n_children;               // children handled by this launch
    int64_t child_first;              // global index of child 0 of this launch
    int64_t n_children_total;         // global number of children (systematic spacing)
    int mode;                         // 0 multinomial, 1 systematic
    const double *uniforms;           // injected uniforms (per local child) or null
    const double *normals;            // injected normals n x 3 row-major or null
    uint32_t seed_lo, seed_hi, update_idx, k0;
    double dt, v, w;                  // motion scalars (cpp:452-471, computed on the host)
    double disp_x, disp_y, disp_th;
    int do_resample;                  // 0: children = parents (identity): a kept update of adaptive resampling (E9), tests
    int64_t idx_out_base;             // ... whose parent index is reported as idx_out_base + own index (a shard's first global index)
    int do_motion;
    // sharded particle sets: parents of other shards are fetched on demand instead of being gathered
    const double4 *ppack_rank[kMaxShards];   // records of shard r (peer pointers within one process), or all null
    int64_t n_per_rank;               // parents per shard (global index = r * n_per_rank + local index)
    int self_rank;
    unsigned long long *remote_count; // += children whose parent lives in another shard (exchange accounting), or null
    const int32_t *idx_in;            // parent of every child decided earlier (index-only pass + exchange), or null
    int index_only;                   // 1: write idx_out and stop (the host fetches the selected parents, then calls again)
    // small updates (one launch less each): the per-particle constants k_particle_prep would compute, the CDF staged in
    // LDS (cdf_lds_entries = n_parents when the launch has n_parents * 8 bytes of dynamic LDS, else 0), counters to zero
    double4 *pc_out;                  // (cos, sin, pixel x, pixel y) per child, or null
    double *clr_logw_acc;             // with pc_out, for the windowed ray kernels: the per-particle scratch k_particle_prep
    uint32_t *clr_far_flags;          //   would zero (the launch then needs k_prep_small only), or null
    double ox, oy, res;
    int cdf_lds_entries;
    unsigned long long *clear_counters;   // 4 words zeroed by the first thread, or null
    // compact parent list (mcl::CompactOut: the particles with a non-zero fixed-point weight, in index order): the search
    // runs over ccdf / ctop, the parent's index and record come from the list.  Sharded sets gather the shards' lists as
    // chunks of cchunk_bytes ([ccdf | crec | cidx], ccap entries each; shard r's at cchunks + r * cchunk_bytes) and search
    // gcdf, the chunks' CDF columns made global (offsets added, padding turned into plateaus) by k_compact_merge.
    const uint64_t *ccdf;             // n_compact entries, non-decreasing, or null (dense search)
    const uint64_t *ctop;             // ccdf[64 g + 63], n_compact >> 6 entries
    int64_t n_compact;
    const uint32_t *cidx;             // single list: particle index of entry p ...
    const double4 *crec;              // ... and its record
    const unsigned char *cchunks;     // gathered lists (cidx / crec null): entry p lives in chunk p / ccap
    int64_t cchunk_bytes, ccap;
    // the single list's guide (mcl_compact_guide.h; the scan that wrote the list wrote it, and left its grand total in *cguide_q),
    // or null: a multinomial draw then takes two guide words and bisects the few entries between them instead of ctop and a group
    const uint32_t *cguide;
    const uint64_t *cguide_q;
    int cguide_m;
    // the ordering of the ray stage: (key, index) of every child from the layout (bounding box, occupied tiles) of the PREVIOUS update's
    // children -- the set moves by a cell or so per update, and a key only decides which rays share a wave -- so that the radix
    // sort can start right after this kernel (k_cell_bbox / k_tile_compact / k_sort_keys off the critical path)
    uint32_t *key_out, *val_out;      // null: keys are made by k_sort_keys / k_sort_hist
    const int *key_bbox, *key_tilemap;
    int key_ntx, key_Wp, key_Hp;
    int key_fine;                     // fine bits of those keys (SortLayout::fine: the engine's setting of the radix path)
    int pc_heading;                   // with key_out: pc_out gets the heading form (heading, 0, pixel x, pixel y) -- k_sort_gather, the one
                                      //   reader of such a record besides k_cell_bbox (.z / .w), takes the sincos (RayHandoff::heading)
    PrepClear prep;                   // prep_on: the first workgroup also clears the few words of the ray stage that are not per
    int prep_on;                      //   particle (what k_prep_small would do in a launch of its own)
    const float *obs_src;             // this update's ranges (pinned host memory, read once by the first workgroup), or null
    int32_t *obs_idx_out;             // their table rows (obs_index_of), for a ray kernel that reads the static table directly
    int obs_B, obs_P;
};

__device__ __forceinline__ int obs_index_of(float obs, double res, int P);

// (KldArgs and kld_bin, the KLD bin rule, are in mcl_types.h: mcl_cluster.hip bins with the same function)

// the words the update's owners listed back to zero, the next counter zeroed, the count into the result block; thread i of n
__device__ __forceinline__ void kld_clear_part(const KldArgs &k, int64_t i, int64_t nthreads)
{
    const unsigned int c = *k.count;
    for (int64_t j = i; j < (int64_t)c; j += nthreads) k.bm[k.list[j]] = 0u;
    if (i == 0) { *k.count_next = 0u; *k.result = c; }
}

__global__ __launch_bounds__(256) void k_kld_clear(KldArgs k)
{
    kld_clear_part(k, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// Recovery by random-particle injection (mcl_set_recovery): the _rec kernels are launched only for an update whose
// injection threshold thr = floor(p * 2^53) is > 0.  Child g is injected iff bits53 of Philox stream 8 is below thr; its pose is a
// free cell drawn as k_init_global draws one (stream 8's second half) and a heading from stream 9, it skips the parent search and the
// motion model and reports parent -1.  Every other child is the one the plain kernel would make.
struct RecArgs {
    uint64_t thr;                     // injection threshold, > 0
    const uint32_t *free_cells;       // the map's free cells (row * W + col), n_free > 0 of them
    uint64_t n_free;
    int W;
    double res, ox, oy;
    unsigned int *count;              // += injected children of this update
    unsigned int *count_next;         // the other counter, zeroed for the next injecting update
};

// The same injection from a pose mixture (mcl_set_recovery_proposal; the header's P2 / P3): the _mix kernels.  Which
// children are injected is the _rec kernels' rule (the same coin against the same threshold); an injected child's component is the
// first k with pick < thresholds[k], searched over [0, n_comp - 1] whatever the words hold, and its pose is G1's with the normals
// of streams 10 / 11.
struct MixArgs {
    uint64_t thr;                     // injection threshold, > 0
    const uint64_t *thresholds;       // n_comp words, non-decreasing, the last one 2^53
    const double *factors;            // 9 doubles per component: mean x, y, theta, L00 L10 L11 L20 L21 L22
    int n_comp;                       // >= 1
    unsigned int *count;              // += injected children of this update
    unsigned int *count_next;         // the other counter, zeroed for the next injecting update
};

// three standard normals of (g, counter): Box-Muller on Philox stream s_pair (n0, n1) and stream s_one (n2), as k_init_pose draws
__device__ __forceinline__ void normals3(uint64_t g, uint32_t counter, uint32_t s_pair, uint32_t s_one, uint32_t seed_lo, uint32_t seed_hi,
                                         double &n0, double &n1, double &n2)
{
    const double TWO_M53 = 1.0 / 9007199254740992.0;
    const double TWO_PI = 2.0 * 3.14159265358979323846;
    u32x4 o = philox4x32((uint32_t)g, counter, s_pair, (uint32_t)(g >> 32), seed_lo, seed_hi);
    double u1 = (double)(bits53(o.v[0], o.v[1]) + 1) * TWO_M53;
    double u2 = (double)bits53(o.v[2], o.v[3]) * TWO_M53;
    double rad = sqrt(-2.0 * log(u1));
    n0 = rad * cos(TWO_PI * u2);
    n1 = rad * sin(TWO_PI * u2);
    o = philox4x32((uint32_t)g, counter, s_one, (uint32_t)(g >> 32), seed_lo, seed_hi);
    u1 = (double)(bits53(o.v[0], o.v[1]) + 1) * TWO_M53;
    u2 = (double)bits53(o.v[2], o.v[3]) * TWO_M53;
    n2 = sqrt(-2.0 * log(u1)) * cos(TWO_PI * u2);
}

// REC: 0 no injection, kRecUniform from the free cells (RecArgs), kRecMixture from the pose mixture (MixArgs)
constexpr int kRecUniform = 1, kRecMixture = 2;

// ODO: the odometry motion models (mcl_set_motion_model): the child moves by odo_step (mcl_motion.h) with the same
// three normals instead of by the reference's arc and map-frame noise; everything else is the kernel without it.
template <bool KLD, int REC, bool ODO = false>
__device__ __forceinline__ void resample_motion_body(const ResampleArgs &a, const KldArgs &k, const RecArgs &r,
                                                     [[maybe_unused]] const OdoArgs &od = OdoArgs{},
                                                     [[maybe_unused]] const MixArgs &mx = MixArgs{})
{
    extern __shared__ __attribute__((aligned(16))) unsigned char resample_lds[];
    int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (a.clear_counters && m == 0) { a.clear_counters[0] = 0ull; a.clear_counters[1] = 0ull; a.clear_counters[2] = 0ull; a.clear_counters[3] = 0ull; }
    if (a.obs_src && blockIdx.x == 0)
        for (int j = threadIdx.x; j < a.obs_B; j += blockDim.x) a.obs_idx_out[j] = obs_index_of(a.obs_src[j], a.res, a.obs_P);
    if (a.prep_on && blockIdx.x == 0) prep_small_clear(a.prep, (int)threadIdx.x, (int)blockDim.x);
    const uint64_t *cdf = a.cdf;
    if (a.cdf_lds_entries > 0) {
        // a small CDF: one coalesced pass into LDS, then the bisection runs at LDS latency (11 dependent L2 round trips
        // were most of this kernel at the stock 2000 particles)
        uint64_t *c_sh = reinterpret_cast<uint64_t *>(resample_lds);
        for (int i = threadIdx.x; i < a.cdf_lds_entries; i += blockDim.x) c_sh[i] = a.cdf[i];
        __syncthreads();
        cdf = c_sh;
    }
    if constexpr (REC == kRecUniform) { if (m == 0) *r.count_next = 0u; }
    if constexpr (REC == kRecMixture) { if (m == 0) *mx.count_next = 0u; }
    if (m >= a.n_children) return;
    uint64_t g = (uint64_t)(a.child_first + m);
    [[maybe_unused]] bool inj = false;        // (REC: this child is a drawn free-space pose, or one drawn from the mixture)
    [[maybe_unused]] double ix = 0.0, iy = 0.0, ith = 0.0;
    if constexpr (REC == kRecMixture) {
        const u32x4 o = philox4x32((uint32_t)g, a.update_idx, 8u, (uint32_t)(g >> 32), a.seed_lo, a.seed_hi);
        inj = bits53(o.v[0], o.v[1]) < mx.thr;
        if (inj) {
            const uint64_t pick = bits53(o.v[2], o.v[3]);
            int lo = 0, len = mx.n_comp - 1;             // the first k in [0, M - 2] with pick < t_k, else M - 1: never outside [0, M - 1]
            while (len > 0) {
                const int half = len >> 1, mid = lo + half;
                if (!(pick < mx.thresholds[mid])) { lo = mid + 1; len = len - half - 1; }
                else len = half;
            }
            const double *f = mx.factors + 9 * (size_t)lo;
            double n0, n1, n2;
            normals3(g, a.update_idx, 10u, 11u, a.seed_lo, a.seed_hi, n0, n1, n2);
            ix = f[0] + f[3] * n0;                                       // G1
            iy = f[1] + (f[4] * n0 + f[5] * n1);
            ith = normalize_angle(f[2] + (f[6] * n0 + f[7] * n1 + f[8] * n2));
        }
    }
    if constexpr (REC == kRecUniform) {
        u32x4 o = philox4x32((uint32_t)g, a.update_idx, 8u, (uint32_t)(g >> 32), a.seed_lo, a.seed_hi);
        inj = bits53(o.v[0], o.v[1]) < r.thr;
        if (inj) {
            const uint64_t pick = __umul64hi(bits53(o.v[2], o.v[3]) << 11, r.n_free);     // floor(k/2^53 * n_free)
            const uint32_t cell = r.free_cells[pick];
            const int row = (int)(cell / (uint32_t)r.W), col = (int)(cell - (uint32_t)row * (uint32_t)r.W);
            ix = col * r.res + r.ox;                                 // the k_init_global rule (cpp:438-439)
            iy = row * r.res + r.oy;
            o = philox4x32((uint32_t)g, a.update_idx, 9u, (uint32_t)(g >> 32), a.seed_lo, a.seed_hi);
            ith = ((double)bits53(o.v[0], o.v[1]) * (1.0 / 9007199254740992.0) - 0.5) * (2.0 * 3.14159265358979323846);   // [-pi, pi)
        }
    }
    int64_t idx = m;
    int64_t cpos = -1;                        // position in the compact parent list, when that is what was searched
    if (REC && inj) {
        idx = -1;
    } else if (a.idx_in) {
        idx = a.idx_in[m];
    } else if (a.do_resample) {
        idx = 0;
        if (a.q_total != 0) {
            uint64_t lmul, r0, r1 = a.q_total;
            if (a.mode == 0) {
                uint64_t k53;
                if (a.uniforms) {
                    double u = a.uniforms[m];
                    u = (u >= 0.0) ? u : 0.0;
                    k53 = (uint64_t)(u * 9007199254740992.0);
                    if (k53 > 9007199254740991ull) k53 = 9007199254740991ull;
                } else {
                    u32x4 o = philox4x32((uint32_t)g, a.update_idx, 2u, (uint32_t)(g >> 32), a.seed_lo, a.seed_hi);
                    k53 = bits53(o.v[0], o.v[1]);
                }
                r0 = k53; lmul = 1ull << 53;
            } else {
                r0 = g * 4294967296ull + a.k0;
                lmul = (uint64_t)a.n_children_total * 4294967296ull;
            }
            // "entry c is above the threshold": c * lmul > r0 * r1 in exact 128-bit arithmetic.  With the multinomial draw's
            // lmul = 2^53 that is c > floor(r0 r1 / 2^53) for the integer c: one product per child instead of one per probe
            // (the search was a sixth of this kernel's instructions); the systematic comb keeps the product form.
            const bool by_thr = a.mode == 0;
            const uint64_t thr = (__umul64hi(r0, r1) << 11) | ((r0 * r1) >> 53);
            auto above = [&](uint64_t c) -> bool { return by_thr ? c > thr : mul_gt(c, lmul, r0, r1); };
            if (a.cguide && by_thr) {
                // compact list with its guide: the shift comes from the total the list was scanned to, so the table and the
                // search agree whatever the host holds; the result is the search's below, entry for entry
                const uint64_t gq = *a.cguide_q;
                const int gs = guide_shift(gq, a.cguide_m);
                cpos = (int64_t)compact_guide_search(a.ccdf, (uint32_t)a.n_compact, a.cguide, gs, guide_bmax(gq, gs), thr);
            } else if (a.ccdf) {
                // compact list: first group of 64 whose last entry exceeds the threshold (ctop: dense, a few KB), then
                // inside that group's 512 bytes
                const int64_t ng = a.n_compact >> kCompactGroupShift;
                int64_t glo = 0, glen = ng;
                while (glen > 0) {
                    int64_t half = glen >> 1, mid = glo + half;
                    if (!above(a.ctop[mid])) { glo = mid + 1; glen = glen - half - 1; }
                    else glen = half;
                }
                int64_t lo = glo << kCompactGroupShift;
                int64_t len = (lo + (1 << kCompactGroupShift) <= a.n_compact) ? (1 << kCompactGroupShift) : a.n_compact - lo;
                while (len > 0) {
                    int64_t half = len >> 1, mid = lo + half;
                    if (!above(a.ccdf[mid])) { lo = mid + 1; len = len - half - 1; }
                    else len = half;
                }
                cpos = (lo >= a.n_compact) ? a.n_compact - 1 : lo;
            } else {
            // two-level search: first the tile (its exclusive prefixes are a small, cache-resident array left by the
            // scan), then inside the tile's 16 KB of the CDF
            int64_t lo = 0, len = a.n_parents;
            if (a.tile_excl) {
                const int64_t ntiles = (a.n_parents + kScanTile - 1) / kScanTile;
                int64_t tlo = 0, tlen = ntiles;           // first tile whose exclusive prefix exceeds the threshold
                while (tlen > 0) {
                    int64_t half = tlen >> 1, mid = tlo + half;
                    if (!above(a.tile_excl[mid])) { tlo = mid + 1; tlen = tlen - half - 1; }
                    else tlen = half;
                }
                const int64_t t = tlo > 0 ? tlo - 1 : 0;
                lo = t * kScanTile;
                len = (lo + kScanTile <= a.n_parents) ? kScanTile : a.n_parents - lo;
                if (a.leaders) {
                    // first 16-entry group of the tile whose last entry exceeds the threshold, then only that group
                    const int64_t g0 = lo >> kLeaderShift, ng = (len + 15) >> kLeaderShift;
                    int64_t glo = g0, glen = ng;
                    while (glen > 0) {
                        int64_t half = glen >> 1, mid = glo + half;
                        if (!above(a.leaders[mid])) { glo = mid + 1; glen = glen - half - 1; }
                        else glen = half;
                    }
                    if (glo >= g0 + ng) glo = g0 + ng - 1;          // threshold beyond the tile (only at the very end)
                    const int64_t end = lo + len;
                    lo = glo << kLeaderShift;
                    len = (lo + 16 <= end) ? 16 : end - lo;
                }
            }
            while (len > 0) {
                int64_t half = len >> 1, mid = lo + half;
                if (!above(cdf[mid])) { lo = mid + 1; len = len - half - 1; }
                else len = half;
            }
            idx = (lo >= a.n_parents) ? a.n_parents - 1 : lo;
            }
        }
    }
    double x, y, th;
    bool have_rec = false;
    if (cpos >= 0) {
        // index and record of the selected entry of the compact list
        if (a.cchunks) {
            const int64_t r = cpos / a.ccap, e = cpos - r * a.ccap;
            const unsigned char *chunk = a.cchunks + (size_t)r * (size_t)a.cchunk_bytes;
            const double4 pr = reinterpret_cast<const double4 *>(chunk + (size_t)a.ccap * 8)[e];
            idx = r * a.n_per_rank + (int64_t)reinterpret_cast<const uint32_t *>(chunk + (size_t)a.ccap * 40)[e];
            x = pr.x; y = pr.y; th = pr.z;
            if (a.remote_count) {
                const unsigned long long rem = __ballot(r != a.self_rank);
                if ((threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1 && rem) atomicAdd(a.remote_count, (unsigned long long)__popcll(rem));
            }
        } else {
            const double4 pr = a.crec[cpos];
            idx = (int64_t)a.cidx[cpos];
            x = pr.x; y = pr.y; th = pr.z;
        }
        have_rec = true;
    }
    if (a.idx_out) a.idx_out[m] = (int32_t)((a.do_resample || a.idx_in) ? idx : idx + a.idx_out_base);
    if (a.index_only) return;
    if (have_rec) {
    } else if (REC && inj) {
        x = ix; y = iy; th = ith;
    } else if (a.n_per_rank > 0) {
        // the parent's record straight from the shard that owns it (this GPU or a peer over xGMI): only selected
        // parents ever cross a link, and a parent many children share is served from this GPU's L2 after the first fetch
        const int r = (int)(idx / a.n_per_rank);
        const double4 pr = a.ppack_rank[r][idx - (int64_t)r * a.n_per_rank];
        x = pr.x; y = pr.y; th = pr.z;
        if (a.remote_count) {
            const unsigned long long rem = __ballot(r != a.self_rank);
            if ((threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1 && rem) atomicAdd(a.remote_count, (unsigned long long)__popcll(rem));
        }
    } else if (a.ppack) { const double4 pr = a.ppack[idx]; x = pr.x; y = pr.y; th = pr.z; }
    else { x = a.px[idx]; y = a.py[idx]; th = a.pth[idx]; }
    [[maybe_unused]] const double kx = x, ky = y, kth = th;     // (KLD: the parent's pose, marked at the end of the kernel; REC: the injected pose)
    if (a.do_motion && !(REC && inj)) {
        double n0, n1, n2;
        if (a.normals) {
            n0 = a.normals[3 * m + 0]; n1 = a.normals[3 * m + 1]; n2 = a.normals[3 * m + 2];
        } else {
            const double TWO_M53 = 1.0 / 9007199254740992.0;
            const double TWO_PI = 2.0 * 3.14159265358979323846;
            u32x4 o = philox4x32((uint32_t)g, a.update_idx, 0u, (uint32_t)(g >> 32), a.seed_lo, a.seed_hi);
            double u1 = (double)(bits53(o.v[0], o.v[1]) + 1) * TWO_M53;
            double u2 = (double)bits53(o.v[2], o.v[3]) * TWO_M53;
            double rad = sqrt(-2.0 * log(u1));
            double sn, cs;
            sincos(TWO_PI * u2, &sn, &cs);            // one argument reduction for the pair; the values are those of sin() and cos()
            n0 = rad * cs;
            n1 = rad * sn;
            o = philox4x32((uint32_t)g, a.update_idx, 1u, (uint32_t)(g >> 32), a.seed_lo, a.seed_hi);
            u1 = (double)(bits53(o.v[0], o.v[1]) + 1) * TWO_M53;
            u2 = (double)bits53(o.v[2], o.v[3]) * TWO_M53;
            rad = sqrt(-2.0 * log(u1));
            n2 = rad * cos(TWO_PI * u2);
        }
        double nx, ny, nth;
        if constexpr (ODO) {
            nx = x; ny = y; nth = th;
            odo_step(od, nx, ny, nth, n0, n1, n2);
        } else {
        if (fabs(a.w) < 1e-6) {                       // cpp:480-484
            double sn, cs;
            sincos(th, &sn, &cs);
            nx = x + a.v * a.dt * cs;
            ny = y + a.v * a.dt * sn;
            nth = th;
        } else {                                      // cpp:485-493
            double radius = a.v / a.w;
            double dth = a.w * a.dt;
            double s0, c0, s1, c1;
            sincos(th, &s0, &c0);
            sincos(th + dth, &s1, &c1);
            nx = x + radius * (s1 - s0);
            ny = y - radius * (c1 - c0);
            nth = th + dth;
        }
        nx += n0 * a.disp_x;                          // cpp:496-498
        ny += n1 * a.disp_y;
        nth += n2 * a.disp_th;
        }
        nth = normalize_angle(nth);                   // cpp:501
        x = nx; y = ny; th = nth;
    }
    a.cx[m] = x; a.cy[m] = y; a.cth[m] = th;
    if (a.cpack) a.cpack[m] = make_double4(x, y, th, 0.0);
    if (a.pc_out) {
        const double4 c = a.pc_heading ? particle_heading_record(x, y, th, a.ox, a.oy, a.res) : particle_constants(x, y, th, a.ox, a.oy, a.res);
        a.pc_out[m] = c;
        if (a.key_out) {
            // the same key k_sort_keys would make (same function, same arguments), from the layout handed in
            a.key_out[m] = sort_key(a.key_bbox, a.key_tilemap, a.key_ntx, cell_of(c.z * kSortSub, a.key_Wp * kSortSub - 1),
                                    cell_of(c.w * kSortSub, a.key_Hp * kSortSub - 1), th, a.n_children, c.z * kSortSub - floor(c.z * kSortSub),
                                    c.w * kSortSub - floor(c.w * kSortSub), a.key_fine);
            a.val_out[m] = (uint32_t)m;
        }
    }
    if (a.clr_logw_acc) a.clr_logw_acc[m] = 0.0;
    if (a.clr_far_flags) a.clr_far_flags[m] = 0u;
    if constexpr (REC != 0) {
        // the injected children of the wave: one atomic
        const unsigned long long injm = __ballot(inj);
        unsigned int *const count = REC == kRecMixture ? mx.count : r.count;
        if (injm && (threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) atomicAdd(count, (unsigned int)__popcll(injm));
    }
    if constexpr (KLD) {
        // the parent's pose (a kept update: the particle's own), after the child's stores (the marking's dependent loads and
        // atomics then wait behind them, not in front of them): plain load first, the atomic only for a bit not seen set, and
        // only by one lane per distinct bin of the wave (the children of a parent are neighbours, a tracking set has a few tens
        // of bins: one fetch-or per lane would pile thousands of waves' atomics onto the same few words)
        const uint32_t b = kld_bin(k, kx, ky, kth);
        const uint32_t wi = b >> 5, bit = 1u << (b & 31u);
        const int lane = (int)(threadIdx.x & 63);
        const bool need = !(k.bm[wi] & bit);
        bool owner = false;
        for (unsigned long long pending = __ballot(need); pending;) {
            const int l = __ffsll((long long)pending) - 1;
            const uint32_t bl = (uint32_t)__shfl((int)b, l);
            pending &= ~__ballot(need && b == bl);
            if (lane == l) owner = !(__hip_atomic_fetch_or(&k.bm[wi], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit);
        }
        const unsigned long long own = __ballot(owner);
        if (own) {
            const int first = __ffsll((long long)own) - 1;
            unsigned int base = 0;
            if (lane == first) base = atomicAdd(k.count, (unsigned int)__popcll(own));
            base = (unsigned int)__shfl((int)base, first);
            if (owner) k.list[base + (unsigned int)__popcll(own & ((1ull << lane) - 1ull))] = wi;
        }
    }
}

__global__ __launch_bounds__(256) void k_resample_motion(ResampleArgs a) { resample_motion_body<false, 0>(a, KldArgs{}, RecArgs{}); }
// the same with the KLD bin marking (a separate instantiation: the kernel without it is the one above, unchanged)
__global__ __launch_bounds__(256) void k_resample_motion_kld(ResampleArgs a, KldArgs k) { resample_motion_body<true, 0>(a, k, RecArgs{}); }
// the two with recovery injection (launched only for an update whose threshold is > 0)
__global__ __launch_bounds__(256) void k_resample_motion_rec(ResampleArgs a, RecArgs r) { resample_motion_body<false, kRecUniform>(a, KldArgs{}, r); }
__global__ __launch_bounds__(256) void k_resample_motion_kld_rec(ResampleArgs a, KldArgs k, RecArgs r) { resample_motion_body<true, kRecUniform>(a, k, r); }
// the four with an odometry motion model (DIFF / OMNI: one instantiation each, the model is a wave-uniform branch in odo_step)
__global__ __launch_bounds__(256) void k_resample_odo(ResampleArgs a, OdoArgs o) { resample_motion_body<false, 0, true>(a, KldArgs{}, RecArgs{}, o); }
__global__ __launch_bounds__(256) void k_resample_odo_kld(ResampleArgs a, KldArgs k, OdoArgs o) { resample_motion_body<true, 0, true>(a, k, RecArgs{}, o); }
__global__ __launch_bounds__(256) void k_resample_odo_rec(ResampleArgs a, RecArgs r, OdoArgs o) { resample_motion_body<false, kRecUniform, true>(a, KldArgs{}, r, o); }
__global__ __launch_bounds__(256) void k_resample_odo_kld_rec(ResampleArgs a, KldArgs k, RecArgs r, OdoArgs o) { resample_motion_body<true, kRecUniform, true>(a, k, r, o); }
// the four that inject from the pose mixture (launched only for an injecting update with a proposal in place)
__global__ __launch_bounds__(256) void k_resample_motion_mix(ResampleArgs a, MixArgs x) { resample_motion_body<false, kRecMixture>(a, KldArgs{}, RecArgs{}, OdoArgs{}, x); }
__global__ __launch_bounds__(256) void k_resample_motion_kld_mix(ResampleArgs a, KldArgs k, MixArgs x) { resample_motion_body<true, kRecMixture>(a, k, RecArgs{}, OdoArgs{}, x); }
__global__ __launch_bounds__(256) void k_resample_odo_mix(ResampleArgs a, MixArgs x, OdoArgs o) { resample_motion_body<false, kRecMixture, true>(a, KldArgs{}, RecArgs{}, o, x); }
__global__ __launch_bounds__(256) void k_resample_odo_kld_mix(ResampleArgs a, KldArgs k, MixArgs x, OdoArgs o) { resample_motion_body<true, kRecMixture, true>(a, k, RecArgs{}, o, x); }

// The shards' compact lists, gathered as chunks ([ccdf | crec | cidx], ccap entries each), become ONE searchable CDF: chunk r's
// column plus the fixed-point total of the shards before it, its unused tail turned into a plateau at the shard's end value
// (a plateau entry is never the first one above a threshold, so it is never selected), and the first search level beside it.
struct MergeArgs {
    const unsigned char *chunks;
    int64_t chunk_bytes, ccap;
    int n_shards;
    uint32_t count[kMaxShards];
    uint64_t off[kMaxShards], tot[kMaxShards];
    uint64_t *gcdf, *gtop;
};
__global__ __launch_bounds__(256) void k_compact_merge(MergeArgs a)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)a.n_shards * a.ccap) return;
    const int r = (int)(p / a.ccap);
    const int64_t e = p - (int64_t)r * a.ccap;
    const uint64_t *col = reinterpret_cast<const uint64_t *>(a.chunks + (size_t)r * (size_t)a.chunk_bytes);
    const uint64_t v = a.off[r] + (e < (int64_t)a.count[r] ? col[e] : a.tot[r]);
    a.gcdf[p] = v;
    if ((p & ((1 << kCompactGroupShift) - 1)) == (1 << kCompactGroupShift) - 1) a.gtop[p >> kCompactGroupShift] = v;
}

// ---- distinct parents of a shard's children (sharded resampling): a bitmap over the GLOBAL particle indices, its popcount
//      prefix and two expansions.  Every pass but the marking is over n_total / 32 words. ----
__global__ void k_bm_mark(const int32_t *__restrict__ parent, int64_t n, int64_t n_total, uint32_t *__restrict__ bm)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = (uint32_t)parent[i];
    if ((int64_t)p < n_total) atomicOr(&bm[p >> 5], 1u << (p & 31u));
}
__global__ void k_bm_pop(const uint32_t *__restrict__ bm, int64_t nwords, uint64_t *__restrict__ pop)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w < nwords) pop[w] = (uint64_t)__popc(bm[w]);
}
// pref = inclusive prefix of pop: the set bits of word w are distinct parents pref[w] - popc(word) ... pref[w] - 1
__global__ void k_bm_expand(const uint32_t *__restrict__ bm, const uint64_t *__restrict__ pref, int64_t nwords, int64_t *__restrict__ distinct)
{
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    uint32_t word = bm[w];
    int64_t at = (int64_t)pref[w] - __popc(word);
    while (word) {
        const int b = __ffs((int)word) - 1;
        distinct[at++] = w * 32 + b;
        word &= word - 1u;
    }
}
__global__ void k_bm_slot(const int32_t *__restrict__ parent, int64_t n, int64_t n_total, const uint32_t *__restrict__ bm,
                          const uint64_t *__restrict__ pref, int32_t *__restrict__ slot)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = (uint32_t)parent[i];
    if ((int64_t)p >= n_total) { slot[i] = 0; return; }
    const uint32_t word = bm[p >> 5];
    slot[i] = (int32_t)((int64_t)pref[p >> 5] - __popc(word) + __popc(word & ((1u << (p & 31u)) - 1u)));
}
// records of the listed particles (indices into the packed records of one shard)
__global__ void k_gather_records(const double4 *__restrict__ rec, const int64_t *__restrict__ index, int64_t count, int64_t n,
                                 double4 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t k = index[i];
    out[i] = (k >= 0 && k < n) ? rec[k] : make_double4(0.0, 0.0, 0.0, 0.0);
}

// (x, y, theta) columns -> packed records (the form k_resample_motion gathers parents from)
__global__ void k_pack_records(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ th, int64_t n,
                               double4 *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_double4(x[i], y[i], th[i], 0.0);
}

}  // namespace mcl
