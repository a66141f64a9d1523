// mcl_rays_lists.h -- what the kernels with work lists share: first_beam_in_wedge, the legacy kernels under their build flag, the
// fix-up pass (k_rays_fix, k_rays_exact, k_gather_logw, k_fix_overflow), the far pass (k_far_*, k_rays_far), k_product_weights.
#pragma once

namespace mcl {

// first beam j with beam_wedge(th, angle[j]) >= m (beam angles increase, so the wedge index is monotone in j).
// For the usual evenly spaced scan the answer is within a beam or two of (m * 2pi/K - th - a0) / increment: the
// bisection starts from a five-beam bracket around that guess when the bracket holds and from [0, B] otherwise.
// GRID: the scan is evenly spaced to within 2e-6 rad (mcl_set_beam_angles: the REC condition, a0 / inv_inc the grid through the
// first and the last beam).  The guess is then the answer unless x lies within 4e-6 rad (twice the bound on a beam's offset; ten
// orders above the rounding of this arithmetic) of a whole beam -- no load, no second evaluation of beam_wedge in all but one
// visit in a thousand at a quarter of a degree per beam.
template <bool GRID = false>
__device__ __forceinline__ int first_beam_in_wedge(double th, const float *__restrict__ angle, int B, int m, double a0, double inv_inc)
{
    int lo = 0, hi = B;
    const double x = ((double)m * (6.283185307179586476925286766559 / kWedges) - th - a0) * inv_inc;
    if (x > -4.0 && x < (double)B + 4.0) {
        const int jg = min(max((int)ceil(x), 0), B);
        if (GRID && fabs(x - rint(x)) > 4e-6 * inv_inc + 1e-6) return jg;
        const bool below = jg == 0 || beam_wedge(th, angle[jg - 1]) < m;      // beam jg-1 is still before wedge m
        const bool at = jg == B || beam_wedge(th, angle[jg]) >= m;           // beam jg is in wedge m or later
        if (below && at) return jg;                                           // the usual case: two loads
        // off by a beam or two (float rounding of the angles): a five-beam bracket when it holds, else [0, B]
        const int l = max(jg - 2, 0), h = min(jg + 2, B);
        if ((l == 0 || beam_wedge(th, angle[l - 1]) < m) && (h == B || beam_wedge(th, angle[h]) >= m)) { lo = l; hi = h; }
    }
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (beam_wedge(th, angle[mid]) >= m) hi = mid; else lo = mid + 1;
    }
    return lo;
}

#ifdef MCL_LEGACY_RAY_KERNELS
}  // namespace mcl
#include "mcl_rays_legacy.h"        // k_rays_quad, k_rays_cell: the predecessors of k_rays_sweep (a build flag: AUTO never picks them)
namespace mcl {
#endif

// Levels 2 and 3 for the rays the ray kernel could not decide (k_rays_fix): fp64 positions on the global byte field (padded
// global coordinates shifted by 2^18), then the literal march if still ambiguous.  profiles/fix_pass.md has the measurements
// behind the two things below: the flat deal, one add per slot and wave.
constexpr int kFixSegMax = 1024;      // segments whose prefix a workgroup keeps in LDS (the persistent grid has 2 per CU)
constexpr int kFixWgPerCu = 6;        // workgroups of k_rays_fix per CU: what 73 .. 80 VGPRs keep resident (6 waves per SIMD)

// One add per run of equal slots in a wave: consecutive list entries are the ~68 beams one walk handed over, so the 64 lanes
// of a wave mostly hold ONE slot, and 64 fp64 atomics to one address are served one after the other.  Segmented reduction
// over the runs of equal `p` among the lanes that `add`, then one atomicAdd by the run's first lane.  The sums are fp64 sums
// of fp32 table entries, exact in any order (E4), and a -inf term gives -inf in any order: the accumulators keep their bits.
// All 64 lanes must be here.
__device__ __forceinline__ void wave_run_add(double *__restrict__ acc, int64_t p, bool add, double v, int lane)
{
    const long long key = add ? (long long)p : -1ll;
    const long long prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || !add || prev != key;               // a lane with nothing to add is a run of its own
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int next = above ? lane + __ffsll((long long)above) : 64;   // first lane of the next run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_down(v, d, 64);
        if (lane + d < next) v += o;                                  // v: the sum of lanes lane .. min(lane + 2d, next) - 1
    }
    if (head && add) atomicAdd(&acc[p], v);
}

// One listed ray of a lane, all 64 lanes of the wave together.  e: the entry; an entry that is not `valid` (the ragged end of
// the deal) repeats a valid one so that the lane stays with its wave, is not traced and adds nothing.  The ray itself is what
// it always was: the wedge field, or the isotropic one for a non-finite heading, !sane, the hand-over to the exact list and
// the inline march when that list is full, store_step, the counters.
template <bool COUNT>
__device__ __forceinline__ void fix_ray(const RayArgs &a, unsigned long long e, bool valid, int lane, unsigned long long &cnt_exact,
                                        unsigned long long &cnt_probe)
{
    const int64_t p = (int64_t)(e >> 16);                     // particle index, or sorted slot (slot_space)
    const int j = (int)(e & 0xFFFF);
    bool add = valid;
    int r = a.P;
    unsigned np = 0;
    if (valid) {
        const double4 pci = a.slot_space ? a.pcs[p] : a.pc[p];
        // k_rays_sweep's rays are re-traced on the field of their own wedge (half the probes of the isotropic field)
        const uint8_t *wfield = nullptr;
        if (a.slot_space && a.distw) {
            const double hth = a.ths[p];
            if (hth == hth && fabs(hth) < 1e6) wfield = a.distw + (size_t)(beam_wedge(hth, a.beam_angle[j]) & (kWedges - 1)) * a.distw_stride;
        }
        const double2 cs = a.beam_cs[j];
        const double ux = pci.x * cs.x - pci.y * cs.y, uy = pci.y * cs.x + pci.x * cs.y;
        const RayOrigin o = ray_origin(a, pci.z, pci.w);
        uint32_t amb = o.amb0;
        if (o.sane)
            r = trace_fp64<false, COUNT>(a, nullptr, 0, kOriginBase, o.p0x, o.p0y, ux, uy, first_skip(a, o, wfield ? wfield : a.dist, wfield != nullptr),
                                         amb, np, wfield, wfield != nullptr);
        if (takes_literal_march(a, o.sane, amb)) {
            // level 3, the literal march: 207 dependent steps in one thread would set the duration of this kernel, so the
            // (few) rays that need it go to k_rays_exact, which gives each of them a whole wave
            bool handed = false;
            if (a.exact_list) {
                const unsigned long long slot = atomicAdd(a.exact_count, 1ull);
                if (slot < a.exact_cap) { atomicExch(&a.exact_list[slot], e); handed = true; }
            }
            if (!handed) {
                const int64_t i = a.slot_space ? (int64_t)a.perm[p] : p;
                r = march_exact(a, a.x[i], a.y[i], a.th[i] + (double)a.beam_angle[j]);
                ++cnt_exact;
            }
            add = !handed;
        }
    }
    const double v = add ? (double)a.Lt[(size_t)r * a.bpad + j] : 0.0;
    wave_run_add(a.logw, p, add, v, lane);
    if (add) {
        if (a.steps || a.steps16) store_step(a, a.slot_space ? (int64_t)a.perm[p] : p, j, r);
        if (COUNT) cnt_probe += np;
    }
}

// The deal.  flat: every workgroup forms the exclusive prefix of the segments' usable counts in LDS (512 strided 8-byte reads
// out of L2 and one scan: the whole grid is resident, so this is paid once, side by side) and a grid-stride loop maps a global
// ray index to (segment, k) by bisection: no lane waits for the fullest segment (the sweep's workgroups flag ~23 walks each,
// Poisson-distributed), and there is no load by thread 0 with two barriers per segment.  A wave reads 64 consecutive entries,
// which mostly share a slot (wave_run_add).  !flat (more segments than the LDS table holds): `split` workgroups share a
// segment, as before.  The counts and entries of the legacy kernels (slot_space == 0) were written by memory-side atomics and
// are read the same way.  Every loop is bounded by a count clipped to fix_cap; nothing waits for another workgroup.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_rays_fix(RayArgs a, int flat)
{
    __shared__ uint32_t pre[kFixSegMax + 1];
    __shared__ uint32_t wsum[4];
    __shared__ unsigned long long n_sh;
    unsigned long long cnt_exact = 0, cnt_probe = 0, cnt_l2 = 0;
    const int lane = threadIdx.x & 63;
    if (flat) {
        const int nseg = a.fix_segments;                             // <= kFixSegMax, nseg * fix_cap < 2^32 (the host checked)
        uint32_t c[4], t = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int seg = (int)threadIdx.x * 4 + i;
            unsigned long long n = 0;
            if (seg < nseg) n = a.slot_space ? a.fix_count[(size_t)seg * 8] : atomicAdd(&a.fix_count[(size_t)seg * 8], 0ull);
            if (n > a.fix_cap) n = 0;                                // overflow (or a ray kernel that stood down): the host re-runs the stage with
            c[i] = (uint32_t)n;                                      // k_rays_skip and discards this one, so nothing of the segment is traced
            t += c[i];
        }
        uint32_t inc = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wsum[threadIdx.x >> 6] = inc;
        __syncthreads();
        uint32_t run = inc - t;
        for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) run += wsum[w];
        if (threadIdx.x == 0) pre[0] = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int seg = (int)threadIdx.x * 4 + i;
            run += c[i];
            if (seg < nseg) pre[seg + 1] = run;
        }
        __syncthreads();
        const unsigned long long total = pre[nseg];
        if (blockIdx.x == 0 && threadIdx.x == 0) cnt_l2 = total;     // level2_rays: once per launch
        for (unsigned long long base = (unsigned long long)blockIdx.x * 256; base < total; base += (unsigned long long)gridDim.x * 256) {
            const unsigned long long idx = base + threadIdx.x;
            const bool valid = idx < total;
            const uint32_t ic = (uint32_t)(valid ? idx : total - 1);
            int lo = 0, hi = nseg - 1;                               // the segment with pre[seg] <= ic < pre[seg + 1]
            for (int it = 0; it < 11 && lo < hi; ++it) {             // (11 halvings empty any range of kFixSegMax)
                const int mid = (lo + hi) >> 1;
                if (pre[mid + 1] <= ic) lo = mid + 1; else hi = mid;
            }
            const unsigned long long *src = a.fix_list + (size_t)lo * a.fix_cap + (ic - pre[lo]);
            const unsigned long long e = a.slot_space ? *src : atomicAdd(const_cast<unsigned long long *>(src), 0ull);
            fix_ray<COUNT>(a, e, valid, lane, cnt_exact, cnt_probe);
        }
    } else {
        // gridDim.x = split * fix_segments: `split` workgroups share one segment
        const int split = max(1, (int)gridDim.x / a.fix_segments);
        const int part = blockIdx.x % split;
        for (int seg = blockIdx.x / split; seg < a.fix_segments; seg += gridDim.x / split) {
            if (threadIdx.x == 0) n_sh = a.slot_space ? a.fix_count[(size_t)seg * 8] : atomicAdd(&a.fix_count[(size_t)seg * 8], 0ull);
            __syncthreads();
            unsigned long long n = n_sh;
            __syncthreads();
            if (n > a.fix_cap) n = 0;
            cnt_l2 += (threadIdx.x == 0 && part == 0) ? n : 0;
            const unsigned long long *list = a.fix_list + (size_t)seg * a.fix_cap;
            for (unsigned long long base = (unsigned long long)part * 256; base < n; base += (unsigned long long)split * 256) {
                const unsigned long long idx = base + threadIdx.x;
                const bool valid = idx < n;
                const unsigned long long ic = valid ? idx : n - 1;
                const unsigned long long e = a.slot_space ? list[ic] : atomicAdd(const_cast<unsigned long long *>(&list[ic]), 0ull);
                fix_ray<COUNT>(a, e, valid, lane, cnt_exact, cnt_probe);
            }
        }
    }
    if (a.counters) {
        if (cnt_exact) atomicAdd(&a.counters[0], cnt_exact);
        if (COUNT && cnt_probe) atomicAdd(&a.counters[2], cnt_probe);
        if (cnt_l2) atomicAdd(&a.counters[3], cnt_l2);
    }
}

// Level 3 for the rays k_rays_fix handed over: the literal march of cast_ray (cpp:611-650), one WAVE per ray (wave_march_exact_dir).
template <bool COUNT>
__global__ __launch_bounds__(256) void k_rays_exact(RayArgs a)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long wave_id = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned long long nwaves = ((unsigned long long)gridDim.x * blockDim.x) >> 6;
    unsigned long long n = 0;
    if (lane == 0) n = atomicAdd(a.exact_count, 0ull);
    n = (unsigned long long)__shfl((long long)n, 0, 64);
    if (n > a.exact_cap) n = a.exact_cap;
    unsigned long long done = 0;
    for (unsigned long long k = wave_id; k < n; k += nwaves) {
        unsigned long long e = 0;
        if (lane == 0) e = atomicAdd(&a.exact_list[k], 0ull);
        e = (unsigned long long)__shfl((long long)e, 0, 64);
        const int64_t p = (int64_t)(e >> 16);
        const int64_t i = a.slot_space ? (int64_t)a.perm[p] : p;
        const int j = (int)(e & 0xFFFF);
        const double angle = a.th[i] + (double)a.beam_angle[j];
        const double dx = cos(angle) * a.res, dy = sin(angle) * a.res;
        const int r = wave_march_exact_dir(a, a.x[i], a.y[i], dx, dy, lane);
        if (lane == 0) {
            atomicAdd(&a.logw[p], (double)a.Lt[(size_t)r * a.bpad + j]);
            if (a.steps || a.steps16) store_step(a, i, j, r);
            ++done;
        }
    }
    if (a.counters && lane == 0 && done) atomicAdd(&a.counters[0], done);
}

// acc (fp64 atomics of the ray kernels of this launch sequence) -> plain array for the rest of the pipeline.  Plain loads
// in a LATER kernel see the result of memory-side atomics (tools/ubench/coherence.hip, profiles/r02_coherence.txt: 0 stale
// entries in 8 x 84M reads, whether the zeroing was a plain or a write-through store); round 1 read these back with atomics
// because of wrong sums that went away with the stream fix of the same day (memsets on the null stream racing the engine's
// stream), not because of the cache hierarchy.
__global__ void k_gather_logw(const double *__restrict__ acc, int64_t n, double *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = acc[i];
}

// overflow flag of the fix-up list: *over = number of segments whose append count exceeded the capacity
__global__ void k_fix_overflow(const unsigned long long *__restrict__ counts, int nseg, unsigned long long cap, unsigned long long *over)
{
    __shared__ unsigned int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    unsigned int c = 0;
    for (int k = threadIdx.x; k < nseg; k += blockDim.x)
        c += atomicAdd(const_cast<unsigned long long *>(&counts[(size_t)k * 8]), 0ull) > cap ? 1u : 0u;
    if (c) atomicAdd(&s, c);
    __syncthreads();
    if (threadIdx.x == 0) *over = s;
}

// The flagged slots in ascending order (k_rays_sweep appends them in arrival order): count per 2048 slots, exclusive scan of the
// counts by one workgroup, scatter.  All three stand down below kFarWindowedMin flagged slots (k_rays_far handles those).
constexpr int kFarTile = 2048;
__global__ __launch_bounds__(256) void k_far_count(const uint32_t *__restrict__ flags32, int64_t n, const unsigned long long *__restrict__ far_count,
                                                  uint32_t *__restrict__ cnt)
{
    if (*far_count < kFarWindowedMin) return;
    __shared__ uint32_t ws[4];
    const int64_t base = (int64_t)blockIdx.x * kFarTile + (int64_t)threadIdx.x * 8;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) c += (base + k < n && flags32[base + k] != 0u) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(1024) void k_far_spine(uint32_t *__restrict__ cnt, int nb, const unsigned long long *__restrict__ far_count)
{
    if (*far_count < kFarWindowedMin) return;
    __shared__ uint32_t ws[16];
    __shared__ uint32_t carry_sh;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_sh = 0u;
    __syncthreads();
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + (int)threadIdx.x;
        const uint32_t v = i < nb ? cnt[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
        if (lane == 63) ws[wv] = inc;
        __syncthreads();
        uint32_t at = carry_sh + inc - v;
        for (int k = 0; k < wv; ++k) at += ws[k];
        if (i < nb) cnt[i] = at;
        __syncthreads();
        if (threadIdx.x == 1023) carry_sh = at + v;
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_far_scatter(const uint32_t *__restrict__ flags32, int64_t n, const unsigned long long *__restrict__ far_count,
                                                    const uint32_t *__restrict__ cnt_excl, uint32_t *__restrict__ out)
{
    if (*far_count < kFarWindowedMin) return;
    __shared__ uint32_t ws[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kFarTile + (int64_t)threadIdx.x * 8;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m |= ((base + k < n && flags32[base + k] != 0u) ? 1u : 0u) << k;
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    uint32_t at = cnt_excl[blockIdx.x] + inc - c;
    for (int k = 0; k < wv; ++k) at += ws[k];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((m >> k) & 1u) out[at++] = (uint32_t)(base + k);
}

// (particle, quadrant) pairs outside their quadrant window: the global-field path, one wave per particle.
template <bool COUNT>
__global__ __launch_bounds__(kRayThreads, 8) void k_rays_far(RayArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t p_end = a.n;
    unsigned long long cnt_exact = 0, cnt_off = 0, cnt_probe = 0;
    const uint32_t *flags32 = reinterpret_cast<const uint32_t *>(a.far_flags);
    if (a.far_windowed && a.far_count && *a.far_count >= kFarWindowedMin) return;     // k_rays_skip<.., FAR> takes this launch
    // each wave scans 64 particles' flags with one coalesced load and visits only the flagged ones.  The 64-particle
    // chunks are dealt round-robin over ALL waves of the grid: in sorted-slot order (k_rays_sweep) the flagged particles
    // sit in a few long runs, which a contiguous range per workgroup would hand to a few workgroups
    // With a list of the flagged slots (k_rays_sweep appends a slot when it sets its first flag) every wave takes list entries
    // round-robin: in sorted-slot order the flagged particles sit in a few long runs, which any partition of the slot range
    // would hand to a few waves.  Without a list the 64-particle chunks of the flag array are dealt round-robin.
    const int64_t n_list = a.far_list ? (int64_t)min((unsigned long long)a.n, *a.far_count) : 0;
    const int64_t wave_global = (int64_t)wave * gridDim.x + blockIdx.x, waves_total = (int64_t)kRayWaves * gridDim.x;
    for (int64_t i0 = a.far_list ? wave_global : wave_global * 64; i0 < (a.far_list ? n_list : p_end); i0 += a.far_list ? waves_total : waves_total * 64) {
      uint32_t myfl;
      unsigned long long todo;
      int64_t listed = 0;
      if (a.far_list) {
          listed = (int64_t)a.far_list[i0];
          myfl = flags32[listed];
          todo = 1ull;
      } else {
          myfl = (i0 + lane < p_end) ? flags32[i0 + lane] : 0u;
          todo = __ballot(myfl != 0u);
      }
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t p = a.far_list ? listed : i0 + src;           // particle index, or sorted slot (slot_space)
        const int64_t i = a.slot_space ? (int64_t)a.perm[p] : p;
        const uint32_t fl = a.far_list ? myfl : (uint32_t)__shfl((int)myfl, src, 64);
        if (lane == 0) ++cnt_off;
        const double4 pci = a.slot_space ? a.pcs[p] : a.pc[p];
        const double cth = pci.x, sth = pci.y, gpx = pci.z, gpy = pci.w;
        // (ray_origin of mcl_ray_core.h written out, and the bits must match it: through the helper this kernel spills more VGPRs)
        const bool sane = (gpx > -200000.0) && (gpx < 200000.0) && (gpy > -200000.0) && (gpy < 200000.0);
        const double p0x = (gpx + 1.0 + 262144.0) + kMagic, p0y = (gpy + 1.0 + 262144.0) + kMagic;
        const int base = kOriginBase;
        uint32_t amb0 = 0;
        int cx0 = 0, cy0 = 0;
        bool in0 = false;
        if (sane) {
            uint32_t lox = (uint32_t)__double2loint(p0x), loy = (uint32_t)__double2loint(p0y);
            cx0 = (__double2hiint(p0x) & 0xFFFFF) - base; cy0 = (__double2hiint(p0y) & 0xFFFFF) - base;
            amb0 = lox < loy ? lox : loy;
            in0 = (unsigned)cx0 < (unsigned)a.Wp && (unsigned)cy0 < (unsigned)a.Hp;
        }
        // k_rays_cell does not materialise the ranges: recompute them for the (few) flagged particles
        short4 qr;
        if (a.qr) qr = a.qr[i];
        else { const double t = a.th[i]; qr = quadrant_ranges_of(t, t == t && fabs(t) < 1e6, a.beam_angle, a.B); }
        double acc = 0.0;
        for (int q = 0; q < 4; ++q) {
            if (((fl >> (8 * q)) & 0xFFu) == 0) continue;
            const uint8_t *field = a.distq[q];               // directional field of this quadrant
            const int d0 = in0 ? field[(size_t)cy0 * a.Wps + cx0] : 0;
            const int s0 = d0 > 1 ? d0 : 1;
            int ja, jb, ja2;
            quad_ranges(qr, q, a.B, ja, jb, ja2);
            for (int seg = 0; seg < 2; ++seg)
            for (int j0 = seg ? ja2 : ja, je = seg ? a.B : jb; j0 < je; j0 += 64) {
                int j = j0 + lane;
                if (j < je) {
                    int r = a.P;
                    unsigned np = 0;
                    uint32_t amb = amb0;
                    if (sane) {
                        double2 cs = a.beam_cs[j];
                        double ux = cth * cs.x - sth * cs.y;
                        double uy = sth * cs.x + cth * cs.y;
                        r = trace_fp64<false, COUNT>(a, nullptr, 0, base, p0x, p0y, ux, uy, s0, amb, np, field);
                    }
                    if (takes_literal_march(a, sane, amb)) {
                        r = march_exact(a, a.x[i], a.y[i], a.th[i] + (double)a.beam_angle[j]);
                        ++cnt_exact;
                    }
                    acc += (double)a.Lt[(size_t)r * a.bpad + j];
                    if (a.steps || a.steps16) store_step(a, i, j, r);
                    if (COUNT) cnt_probe += np;
                }
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) atomicAdd(&a.logw[p], acc);
      }
    }
    if (a.counters) {
        cnt_exact = wave_sum_u64(cnt_exact);
        cnt_off = wave_sum_u64(cnt_off);
        cnt_probe = wave_sum_u64(cnt_probe);
        if (lane == 0) {
            if (cnt_exact) atomicAdd(&a.counters[0], cnt_exact);
            if (cnt_off) atomicAdd(&a.counters[1], cnt_off);
            if (COUNT && cnt_probe) atomicAdd(&a.counters[2], cnt_probe);
        }
    }
}

// product-as-reference weights (cpp:566-578) from materialised steps: one thread per particle,
// sequential double product in beam order, then pow(.,inv_squash).
__global__ void k_product_weights(const uint8_t *__restrict__ steps, const uint16_t *__restrict__ steps16, const int32_t *__restrict__ obs_idx, int64_t n, int B,
                                  const double *__restrict__ table /* col-major (P+1)^2 */, int tw, double inv_squash,
                                  double *__restrict__ w_out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double w = 1.0;
    for (int j = 0; j < B; ++j) w *= table[(size_t)(steps16 ? (int)steps16[(size_t)i * B + j] : (int)steps[(size_t)i * B + j]) * tw + obs_idx[j]];
    w_out[i] = pow(w, inv_squash);
}

}  // namespace mcl
