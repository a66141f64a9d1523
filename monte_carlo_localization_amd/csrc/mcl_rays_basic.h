// mcl_rays_basic.h -- K3: the per-particle constants (k_particle_prep, k_prep_small), the literal march (K3a, k_rays_march) and the
// self-contained skipping kernel (K3b, k_rays_skip, also the windowed far pass); the raw LDS offset and the quadrant ranges the
// windowed kernels share.
#pragma once

namespace mcl {

// step index of ray (i, j) to whichever output the launch has
__device__ __forceinline__ void store_step(const RayArgs &a, int64_t i, int j, int r)
{
    if (a.steps16) a.steps16[(size_t)i * a.B + j] = (uint16_t)r;
    else if (a.steps) a.steps[(size_t)i * a.B + j] = (uint8_t)r;
}

constexpr int kRayThreads = 1024;
constexpr int kRayWaves = kRayThreads / 64;

// per-particle constants of the skipping march, computed once by one lane instead of by all 64 lanes
// of the wave that owns the particle
// k_rays_quad assigns a ray to the quadrant floor((theta + a_j) / (pi/2)) of its direction.  Beam angles
// increase monotonically over less than a full turn (checked at mcl_set_beam_angles), so the beams of one
// particle fall into at most five contiguous index ranges with quadrants q0, q0+1, ..., q0+4 (mod 4).
// qr = (start of ranges 1..4, B when absent); q0 is packed into the top two bits of .x.
// direction bin (wedge, unwrapped) of beam `angle` for heading th; the quadrant index is derived from it so that
// every kernel classifies a ray the same way
__device__ __forceinline__ int beam_wedge(double th, float angle) { return (int)floor((th + (double)angle) * (kWedges * 0.15915494309189533577)); }
__device__ __forceinline__ int beam_wedge_d(double th, double angle) { return (int)floor((th + angle) * (kWedges * 0.15915494309189533577)); }   // angle = (double) of the float
__device__ __forceinline__ int beam_turns(double th, float angle) { return beam_wedge(th, angle) >> kWedgeShift; }

// quadrant ranges of one particle's beams (see above); a garbage heading gets one range in quadrant 0
__device__ __forceinline__ short4 quadrant_ranges_of(double t, bool heading_ok, const float *__restrict__ beam_angle, int B)
{
    short st[4];
    int q0 = 0;
    if (heading_ok) {
        const int k0 = beam_turns(t, beam_angle[0]);
        q0 = k0 & 3;
        for (int k = 1; k <= 4; ++k) {
            int lo = 0, hi = B;              // first j with turns(j) - turns(0) >= k
            while (lo < hi) {
                int mid = (lo + hi) >> 1;
                if (beam_turns(t, beam_angle[mid]) - k0 >= k) hi = mid; else lo = mid + 1;
            }
            st[k - 1] = (short)lo;
        }
    } else {
        st[0] = st[1] = st[2] = st[3] = (short)B;   // garbage heading: one range, marched literally by k_rays_far
    }
    return make_short4((short)(st[0] | (q0 << 14)), st[1], st[2], st[3]);
}

__global__ __launch_bounds__(256) void k_particle_prep(const double *__restrict__ x, const double *__restrict__ y,
                                                      const double *__restrict__ th, int64_t n, double ox, double oy, double res,
                                                      double4 *__restrict__ pc, const float *__restrict__ beam_angle, int B,
                                                      short4 *__restrict__ qr, PrepClear clr)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (clr.logw_acc) clr.logw_acc[i] = 0.0;
    if (clr.far_flags) clr.far_flags[i] = 0u;
    if (clr.fix_count) for (int64_t k = i; k < clr.fix_words; k += n) clr.fix_count[k] = 0ull;
    if (clr.fix_over) for (int64_t k = i; k < 2; k += n) clr.fix_over[k] = 0ull;
    if (clr.exact_count && i == 0) clr.exact_count[0] = 0ull;
    if (clr.far_count && i == 0) clr.far_count[0] = 0ull;
    if (clr.bbox) for (int64_t k = i; k < 7; k += n) clr.bbox[k] = k < 2 ? 0x7fffffff : (k < 4 ? (int)0x80000000 : (k == 6 ? clr.bbox_play : 0));
    if (clr.hist) for (int64_t k = i; k < clr.hist_n; k += n) clr.hist[k] = 0u;
    const double t = th[i];
    pc[i] = particle_constants(x[i], y[i], t, ox, oy, res);
    if (qr) qr[i] = quadrant_ranges_of(t, t == t && fabs(t) < 1e6, beam_angle, B);
}

// the few words of k_particle_prep's clearing that are not per particle: what is left to do when the resampling kernel has
// already written the constants and zeroed the per-particle scratch
__global__ __launch_bounds__(256) void k_prep_small(PrepClear clr)
{
    prep_small_clear(clr, (int)threadIdx.x, 256);
}

// D = a*b + c on the low 24 bits of a and b (v_mad_i32_i24): the level-1 position update
__device__ __forceinline__ uint32_t mad_i24(int a, int b, uint32_t c)
{
    uint32_t d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// D = a*b + c on the low 24 bits (unsigned): LDS byte offset = row * stride + column byte
__device__ __forceinline__ uint32_t mad_u24(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
__device__ __forceinline__ uint32_t mad_u24_s(uint32_t a, uint32_t b_uniform, uint32_t c)
{
    uint32_t d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "s"(b_uniform), "v"(c));
    return d;
}
// the same with a wave-uniform first factor kept in a scalar register
__device__ __forceinline__ uint32_t mad_i24_s(int a, int b, uint32_t c)
{
    uint32_t d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=&v"(d) : "s"(a), "v"(b), "v"(c));
    return d;
}
// round-to-nearest-even double -> int32 through the 1.5*2^52 magic add (|x| < 2^31)
__device__ __forceinline__ int rint_i32(double x) { return __double2loint(x + 6755399441055744.0); }

// ---- K3a: literal march for every ray (MCL_RAYS_MARCH): the on-device ground truth -------------
template <bool COUNT>
__global__ __launch_bounds__(kRayThreads) void k_rays_march(RayArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t per = (a.n + gridDim.x - 1) / gridDim.x;
    const int64_t p_begin = (int64_t)blockIdx.x * per;
    const int64_t p_end = (p_begin + per < a.n) ? p_begin + per : a.n;
    unsigned long long cnt_probe = 0;
    for (int64_t i = p_begin + wave; i < p_end; i += kRayWaves) {
        const double x = a.x[i], y = a.y[i], th = a.th[i];
        double acc = 0.0;
        for (int j0 = 0; j0 < a.B; j0 += 64) {
            int j = j0 + lane;
            if (j < a.B) {
                int r = march_exact(a, x, y, th + (double)a.beam_angle[j]);   // cpp:533
                acc += (double)a.Lt[(size_t)r * a.bpad + j];
                store_step(a, i, j, r);
                if (COUNT) cnt_probe += (r < a.P) ? (r + 1) : a.P;
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) a.logw[i] = acc;
    }
    if (COUNT && a.counters) {
        cnt_probe = wave_sum_u64(cnt_probe);
        if (lane == 0 && cnt_probe) atomicAdd(&a.counters[2], cnt_probe);
    }
}

// ---- K3b: empty-space skipping on the same sample lattice (MCL_RAYS_SKIP) ----------------------
//
// A ray's k-th sample is p0 + k*u (pixel units).  D(c) = Chebyshev distance from cell c to the
// nearest "stop" cell (occupied or outside the map).  Successive samples are at most one cell apart
// in either axis, so if sample k lies in cell c the samples k+1 .. k+D(c)-1 cannot be stops: the
// march may jump from k to k+max(D(c),1) and still returns exactly the first stop sample of the
// fixed-step march (cpp:622-647).  Three precision levels keep that claim bit-exact:
//   level 1  32-bit fixed point (22 fractional bits) on the LDS window: T = P0 + s*U with
//            P0 = rint(p0*2^22), U = rint(u*2^22)  =>  |T - exact| <= (1+s)/2 <= 128 units (s <= 255);
//            a sample with fraction in [kG1, 2^22-kG1) units is in the cell the reference computes;
//   level 2  rays with any level-1 sample closer than that to a cell boundary are re-run with fp64
//            positions (error ~1 unit of 2^-32 px, guard 2^-30 px);
//   level 3  what is still ambiguous, and every ray of a particle whose own cell is ambiguous,
//            is re-run by march_exact (the literal restatement).
// The reference's own accumulated rounding (207 sequential fp64 adds at |x| ~ 85 m) stays below
// 3e-11 px, far inside the level-2 guard, which is what makes the equality with cpp:611-650 hold.
constexpr int kFx = 22;
constexpr uint32_t kG1 = 132u;

// R = rays per lane per pass (independent dependency chains that hide the LDS round trip).
// FAR: the windowed pass over the (particle, quadrant) pairs k_rays_sweep could not fit into its 256-cell windows -- the
// uniform cloud of a global re-localisation, where 1024 consecutive sorted particles cover more cells than a window leaves
// room for.  The flagged slots arrive in ascending (= tile-sorted) order; persistent workgroups take slices of kFarSlice
// of them, centre this kernel's 568-cell nibble window on each slice (a 32 x 32-cell tile or two fit its play at any
// supported range) and trace only the beams of the flagged quadrants; the sums are added to the slot's accumulator.
constexpr int kFarSlice = 256;
constexpr unsigned long long kFarWindowedMin = 2048;     // fewer flagged slots than this: k_rays_far (no window loads)
template <int R, bool COUNT, bool FAR = false>
__global__ __launch_bounds__(kRayThreads) void k_rays_skip(RayArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    unsigned long long cnt_exact = 0, cnt_off = 0, cnt_probe = 0, cnt_l2 = 0;
    const int64_t n_items = FAR ? (int64_t)min((unsigned long long)a.n, *a.far_count) : a.n;
    if (FAR && (unsigned long long)n_items < kFarWindowedMin) return;
    const uint32_t *flags32 = reinterpret_cast<const uint32_t *>(a.far_flags);
    for (int64_t slice = blockIdx.x; FAR ? slice * kFarSlice < n_items : slice == (int64_t)blockIdx.x; slice += gridDim.x) {
    if (FAR && slice != (int64_t)blockIdx.x) __syncthreads();          // every wave is done with the previous slice's window
    const int64_t per = FAR ? kFarSlice : (a.n + gridDim.x - 1) / gridDim.x;
    const int64_t p_begin = (FAR ? slice : (int64_t)blockIdx.x) * per;
    const int64_t p_end = (p_begin + per < n_items) ? p_begin + per : n_items;

    const int TW = a.tw_cells;
    const int strideB = TW >> 1;
    const int wpr = TW >> 3;                 // 32-bit words (8 cells) per window row
    // requested before the window is loaded, needed after: this wave's first particle and the lane's first beam direction
    // (a small update is one particle per wave: these two round trips would otherwise follow the fill)
    const int64_t i_first = p_begin + wave;
    double4 pci_first = make_double4(0.0, 0.0, 0.0, 0.0);
    if (!FAR && i_first < p_end) pci_first = a.pc[i_first];
    const double2 cs_first = a.beam_cs[lane];          // beam_cs is padded to a multiple of 64 * R entries
    const int tw = a.P + 1;
    int wx0, wy0;
    {
        // ---- window placement: centred on the mean padded-pixel position of this slice (FAR: on the centre of its bounding
        //      box -- a slice that straddles two neighbouring tiles, 64 x 32 cells, then fits the play as a whole) ----
        double *red = reinterpret_cast<double *>(lds_raw);   // scratch, overwritten by the window below
        double sx = 0.0, sy = 0.0, bx0 = INFINITY, bx1 = -INFINITY, by0 = INFINITY, by1 = -INFINITY;
        for (int64_t i = p_begin + threadIdx.x; i < p_end; i += kRayThreads) {
            double4 c = FAR ? a.pcs[a.far_sorted[i]] : a.pc[i];
            double gx = c.z, gy = c.w;
            if (gx == gx && gy == gy && fabs(gx) < 1e9 && fabs(gy) < 1e9) {
                sx += gx; sy += gy;
                if (FAR) { bx0 = fmin(bx0, gx); bx1 = fmax(bx1, gx); by0 = fmin(by0, gy); by1 = fmax(by1, gy); }
            }
        }
        double mx = 0.0, my = 0.0;
        if (FAR) {
            bx0 = -wave_max(-bx0); bx1 = wave_max(bx1); by0 = -wave_max(-by0); by1 = wave_max(by1);
            if (lane == 0) { red[4 * wave] = bx0; red[4 * wave + 1] = bx1; red[4 * wave + 2] = by0; red[4 * wave + 3] = by1; }
            __syncthreads();
            for (int k = 0; k < kRayWaves; ++k) { bx0 = fmin(bx0, red[4 * k]); bx1 = fmax(bx1, red[4 * k + 1]); by0 = fmin(by0, red[4 * k + 2]); by1 = fmax(by1, red[4 * k + 3]); }
            if (bx1 >= bx0) { mx = 0.5 * (bx0 + bx1); my = 0.5 * (by0 + by1); }
        } else {
            sx = wave_sum(sx); sy = wave_sum(sy);
            if (lane == 0) { red[2 * wave] = sx; red[2 * wave + 1] = sy; }
            __syncthreads();
            for (int k = 0; k < kRayWaves; ++k) { mx += red[2 * k]; my += red[2 * k + 1]; }
            int64_t cntp = p_end - p_begin;
            if (cntp > 0) { mx /= (double)cntp; my /= (double)cntp; }
        }
        wx0 = (((int)floor(mx) + 1 - TW / 2)) & ~7;      // padded coordinate = global + 1
        wy0 = (int)floor(my) + 1 - TW / 2;
        __syncthreads();
        // ---- load the window: a straight copy of the nibble field, 8 cells per 32-bit word, twenty independent loads in
        //      flight per thread (at the stock 2000 x 61 the fill is a third of the kernel: dependent round trips to L2) ----
        uint32_t *win = reinterpret_cast<uint32_t *>(lds_raw);
        const uint32_t *src4 = reinterpret_cast<const uint32_t *>(a.dist4);
        const int nwords = wpr * TW, spw = a.Wps >> 3, gxw0 = wx0 >> 3;        // wx0 is a multiple of 8 (possibly negative)
        constexpr int kBatch = 20;
        for (int wi0 = threadIdx.x; wi0 < nwords; wi0 += kRayThreads * kBatch) {
            uint32_t v[kBatch];
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int wi = wi0 + k * kRayThreads;
                const int row = wi / wpr, cw = wi - row * wpr;
                const int gy = wy0 + row, gxw = gxw0 + cw;
                v[k] = 0u;
                if (wi < nwords && gy >= 0 && gy < a.Hp && gxw >= 0 && gxw < spw) v[k] = src4[(size_t)gy * spw + gxw];
            }
#pragma unroll
            for (int k = 0; k < kBatch; ++k) {
                const int wi = wi0 + k * kRayThreads;
                if (wi < nwords) win[wi] = v[k];
            }
        }
        __syncthreads();
    }
    const unsigned char *ldsb = lds_raw;
    const int ngroups = (a.B + 64 * R - 1) / (64 * R);
    // the level-1 loop addresses the window with raw LDS offsets: the dynamic segment must start at 0, i.e. the kernel has no
    // static LDS -- checked on the host at mcl_create (hipFuncGetAttributes), which keeps the engine off this kernel otherwise
    // level-1 error bound: (1 + s) / 2 units for s <= P samples (+ 4 of slack); kG1 covers the byte ranges
    const uint32_t g1 = (uint32_t)a.P > 255u ? (uint32_t)(a.P + 2) / 2u + 4u : kG1;
    uint32_t strideB_v = (uint32_t)strideB, gbias_v = g1 << (32 - kFx);
    asm volatile("" : "+v"(strideB_v), "+v"(gbias_v));   // keep both in VGPRs across the loop

    for (int64_t ii = p_begin + wave; ii < p_end; ii += kRayWaves) {
        // FAR: list entry ii is a sorted slot; its constants, heading and flags live in slot space, its particle index is perm[slot]
        const int64_t slot = FAR ? (int64_t)a.far_sorted[ii] : ii;
        const int64_t i = FAR ? (int64_t)a.perm[slot] : ii;
        const double4 pci = FAR ? a.pcs[slot] : ((ii == i_first) ? pci_first : a.pc[ii]);
        const uint32_t farfl = FAR ? flags32[slot] : 0u;
        const double hth = FAR ? a.ths[slot] : 0.0;
        const bool hth_ok = hth == hth && fabs(hth) < 1e6;
        double acc = 0.0;
        const double cth = pci.x, sth = pci.y;
        const double gpx = pci.z;                     // global pixel coordinate of the particle
        const double gpy = pci.w;
        const double wpx = gpx - (double)(wx0 - 1);   // window-relative padded coordinate
        const double wpy = gpy - (double)(wy0 - 1);
        const double reach = (double)(a.P + 2);
        const bool inwin = (wpx - reach >= 0.0) && (wpx + reach < (double)TW) && (wpy - reach >= 0.0) && (wpy + reach < (double)TW);
        // outside the window the same algorithm runs on the global byte field, in padded global
        // coordinates shifted by 2^18 so that the magic add sees positive values
        const bool sane = (gpx > -200000.0) && (gpx < 200000.0) && (gpy > -200000.0) && (gpy < 200000.0);
        const double p0x = inwin ? (wpx + kMagic) : ((gpx + 1.0 + 262144.0) + kMagic);
        const double p0y = inwin ? (wpy + kMagic) : ((gpy + 1.0 + 262144.0) + kMagic);
        const int base = inwin ? kCellBase : (kCellBase + 262144);
        if ((FAR || !inwin) && lane == 0) ++cnt_off;      // FAR: every pair here is one k_rays_sweep's windows did not fit
        // the particle's own cell gives a first skip shared by all its beams
        uint32_t amb0 = 0;
        int s0 = 1;
        if (inwin || sane) {
            uint32_t lox = (uint32_t)__double2loint(p0x), loy = (uint32_t)__double2loint(p0y);
            int cx = (__double2hiint(p0x) & 0xFFFFF) - base;
            int cy = (__double2hiint(p0y) & 0xFFFFF) - base;
            amb0 = lox < loy ? lox : loy;
            int d;
            if (inwin) {
                uint32_t byte = ldsb[cy * strideB + (cx >> 1)];
                d = (byte >> ((cx & 1) * 4)) & 15;
            } else {
                d = ((unsigned)cx < (unsigned)a.Wp && (unsigned)cy < (unsigned)a.Hp) ? a.dist[(size_t)cy * a.Wps + cx] : 0;
            }
            s0 = d > 1 ? d : 1;
        }

        if (inwin) {
            const uint32_t P0x = (uint32_t)rint_i32(wpx * 4194304.0 - 2147483648.0) + 0x80000000u;   // rint(wpx*2^22) mod 2^32
            const uint32_t P0y = (uint32_t)rint_i32(wpy * 4194304.0 - 2147483648.0) + 0x80000000u;
            const uint32_t g0 = (amb0 < kGuard) ? 0u : 0xFFFFFFFFu;
            const int rem_start = s0 <= a.P ? a.P - s0 : 0;
            const double ncth22 = -cth * 4194304.0, sth22 = sth * 4194304.0;
            for (int grp = 0; grp < ngroups; ++grp) {
                int NUx[R], NUy[R], rem[R], n[R];
                uint32_t Pex[R], Pey[R], g[R];
                bool want[R];
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    int j = (grp * R + k) * 64 + lane;        // beam_cs is padded: no clamp needed
                    double2 cs = (grp == 0 && k == 0) ? cs_first : a.beam_cs[j];
                    // -U = -rint(2^22 * (cos, sin)(theta + a_j)); T(s) = P0 + s*U = Pe - rem*U with rem = P - s
                    NUx[k] = rint_i32(__builtin_fma(ncth22, cs.x, sth22 * cs.y));
                    NUy[k] = rint_i32(__builtin_fma(ncth22, cs.y, -(sth22 * cs.x)));
                    Pex[k] = mad_i24(-a.P, NUx[k], P0x);
                    Pey[k] = mad_i24(-a.P, NUy[k], P0y);
                    rem[k] = (j < a.B) ? rem_start : 0;       // a padding slot probes its end sample once
                    if (FAR) {
                        // only the beams of a flagged quadrant (the others were traced by k_rays_sweep); the quadrant of a
                        // beam is derived as everywhere else (beam_turns), a garbage heading has all its beams in quadrant 0
                        const int qj = (j < a.B) ? (hth_ok ? (beam_turns(hth, a.beam_angle[j]) & 3) : 0) : 0;
                        want[k] = j < a.B && ((farfl >> (8 * qj)) & 0xFFu) != 0u;
                        if (!want[k]) rem[k] = 0;
                    }
                    g[k] = g0;
                    n[k] = 0;
                }
                // ---- level 1: all R rays of the lane advance together; a finished ray keeps
                //      re-probing its last sample (same state every trip) until the wave is done ----
                bool any;
                do {
                    any = false;
#pragma unroll
                    for (int k = 0; k < R; ++k) {
                        // One hand-scheduled block per probe (13 VALU + 1 LDS read): position update, LDS byte
                        // address = row * stride + (cx >> 1) (the window starts at LDS offset 0), boundary guard
                        // and nibble select overlapped with the LDS round trip.
                        uint32_t Tx, Ty, t0, t1, addr, byte;
                        asm volatile(
                            "v_mad_i32_i24 %[tx], %[rem], %[nux], %[pex]\n\t"     // Tx = rem*NUx + Pex
                            "v_mad_i32_i24 %[ty], %[rem], %[nuy], %[pey]\n\t"     // Ty = rem*NUy + Pey
                            "v_lshrrev_b32 %[t0], 23, %[tx]\n\t"                  // cx >> 1
                            "v_lshrrev_b32 %[t1], 22, %[ty]\n\t"                  // cy
                            "v_mad_u32_u24 %[ad], %[t1], %[str], %[t0]\n\t"       // byte address
                            "ds_read_u8 %[by], %[ad]\n\t"
                            "v_lshl_add_u32 %[t0], %[tx], 10, %[gb]\n\t"          // biased fraction of x in the top 22 bits
                            "v_lshl_add_u32 %[t1], %[ty], 10, %[gb]\n\t"
                            "v_min3_u32 %[g], %[g], %[t0], %[t1]\n\t"             // closest approach to a cell boundary so far
                            "v_lshrrev_b32 %[t0], 20, %[tx]\n\t"
                            "v_and_b32 %[t0], 4, %[t0]\n\t"                       // nibble select: (cx & 1) * 4
                            "s_waitcnt lgkmcnt(0)\n\t"
                            "v_bfe_u32 %[by], %[by], %[t0], 4"                     // skip distance, 0 on a stop
                            : [tx] "=&v"(Tx), [ty] "=&v"(Ty), [t0] "=&v"(t0), [t1] "=&v"(t1), [ad] "=&v"(addr), [by] "=&v"(byte),
                              [g] "+v"(g[k])
                            : [rem] "v"(rem[k]), [nux] "v"(NUx[k]), [nuy] "v"(NUy[k]), [pex] "v"(Pex[k]), [pey] "v"(Pey[k]),
                              [str] "v"(strideB_v), [gb] "v"(gbias_v)
                            : "memory");
                        n[k] = (int)byte;
                        uint32_t nr;
                        bool over = __builtin_usub_overflow((uint32_t)rem[k], (uint32_t)n[k], &nr);   // skip > samples left
                        bool go = !over && n[k] != 0;
                        if (R == 1) {
                            rem[k] = (int)nr;                                                    // unchanged on a stop
                        } else {
                            rem[k] = go ? (int)nr : rem[k];
                        }
                        any |= go;
                        if (COUNT) cnt_probe += go ? 1 : 0;
                    }
                } while (any);
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    int j = (grp * R + k) * 64 + lane;
                    if (j < a.B && (!FAR || want[k])) {
                        // R == 1: rem was decremented once more after an overshoot; only the stop case reads it
                        int r = (n[k] == 0) ? a.P - rem[k] - 1 : a.P;
                        if (COUNT) ++cnt_probe;
                        if (g[k] < ((2u * g1) << (32 - kFx)) || a.force_exact) {
                            // ---- level 2 (and 3): rare, everything recomputed from scratch ----
                            double2 cs = a.beam_cs[j];
                            double ux = cth * cs.x - sth * cs.y;
                            double uy = sth * cs.x + cth * cs.y;
                            uint32_t amb = amb0;
                            unsigned np = 0;
                            r = trace_fp64<true, COUNT>(a, ldsb, strideB, kCellBase, p0x, p0y, ux, uy, s0, amb, np);
                            ++cnt_l2;
                            if (COUNT) cnt_probe += np;
                            if (amb < kGuard || a.force_exact == 1) {
                                r = march_exact(a, a.x[i], a.y[i], a.th[i] + (double)a.beam_angle[j]);
                                ++cnt_exact;
                            }
                        }
                        acc += a.Ldirect ? (double)a.Ldirect[(size_t)a.obs_idx[j] * tw + r] : (double)a.Lt[(size_t)r * a.bpad + j];
                        store_step(a, i, j, r);
                    }
                }
            }
        } else {
            for (int j0 = 0; j0 < a.B; j0 += 64) {
                int j = j0 + lane;
                bool mine = j < a.B;
                if (FAR && mine) {
                    const int qj = hth_ok ? (beam_turns(hth, a.beam_angle[j]) & 3) : 0;
                    mine = ((farfl >> (8 * qj)) & 0xFFu) != 0u;
                }
                if (mine) {
                    int r = a.P;
                    unsigned np = 0;
                    uint32_t amb = amb0;
                    if (sane) {
                        double2 cs = a.beam_cs[j];
                        double ux = cth * cs.x - sth * cs.y;
                        double uy = sth * cs.x + cth * cs.y;
                        r = trace_fp64<false, COUNT>(a, ldsb, strideB, base, p0x, p0y, ux, uy, s0, amb, np);
                    }
                    if (!sane || amb < kGuard || a.force_exact == 1) {
                        r = march_exact(a, a.x[i], a.y[i], a.th[i] + (double)a.beam_angle[j]);
                        ++cnt_exact;
                    }
                    acc += a.Ldirect ? (double)a.Ldirect[(size_t)a.obs_idx[j] * tw + r] : (double)a.Lt[(size_t)r * a.bpad + j];
                    store_step(a, i, j, r);
                    if (COUNT) cnt_probe += np;
                }
            }
        }
        acc = wave_sum(acc);          // exact: fp32 table entries, |sum| < 2^13
        if (lane == 0) {
            if (FAR) atomicAdd(&a.logw[slot], acc);      // beside what k_rays_sweep / k_rays_fix leave for this slot
            else a.logw[i] = acc;
        }
    }
    }   // slices
    if (a.counters) {
        cnt_exact = wave_sum_u64(cnt_exact);
        cnt_off = wave_sum_u64(cnt_off);
        cnt_probe = wave_sum_u64(cnt_probe);
        cnt_l2 = wave_sum_u64(cnt_l2);
        if (lane == 0) {
            if (cnt_exact) atomicAdd(&a.counters[0], cnt_exact);
            if (cnt_off) atomicAdd(&a.counters[1], cnt_off);
            if (cnt_probe) atomicAdd(&a.counters[2], cnt_probe);
            if (cnt_l2) atomicAdd(&a.counters[3], cnt_l2);
        }
    }
}

// raw LDS offset of the windows of k_rays_sweep (and of the legacy k_rays_quad / k_rays_cell): they follow 16 bytes of static LDS
constexpr int kQLdsBase = 16;            // the window follows 16 bytes of static LDS (the work-item slot)

// beams of particle i in quadrant q: range [ja, jb) and, when the first quadrant is visited twice, [ja2, B)
__device__ __forceinline__ void quad_ranges(short4 qr, int q, int B, int &ja, int &jb, int &ja2)
{
    const int st1 = qr.x & 0x3FFF, st2 = qr.y, st3 = qr.z, st4 = qr.w, q0 = ((int)qr.x >> 14) & 3;
    const int r_idx = (q - q0) & 3;
    ja = r_idx == 0 ? 0 : (r_idx == 1 ? st1 : (r_idx == 2 ? st2 : st3));
    jb = r_idx == 0 ? st1 : (r_idx == 1 ? st2 : (r_idx == 2 ? st3 : st4));
    ja2 = r_idx == 0 ? st4 : B;
}

}  // namespace mcl
