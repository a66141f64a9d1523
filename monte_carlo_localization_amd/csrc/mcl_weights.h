// mcl_weights.h -- K4 / K7: the reductions, k_weights (max-subtracted weights, fixed-point weights, pose sums), k_final_sums, the
// tail of a tiny update (k_tiny_tail), carry, normalise, column sums, k_sample, and the small kernels of the sharded hosts.
#pragma once

namespace mcl {

// K4 / K7: reductions.  Fixed grid (kRedBlocks x 256) with grid-stride loops and a fixed-order
// final pass: deterministic for a given N.
__global__ __launch_bounds__(kRedThreads) void k_reduce_max(const double *__restrict__ v, int64_t n, double *__restrict__ part)
{
    __shared__ double sm[kRedThreads / 64];
    double m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRedThreads)
        m = fmax(m, v[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kRedThreads / 64; ++k) m = fmax(m, sm[k]);
        part[blockIdx.x] = m;
    }
}
// (out2: a second place for the same value -- the caller's exchange buffer in the device-ordered staged flow -- or null)
__global__ __launch_bounds__(kRedThreads) void k_final_max(const double *__restrict__ part, int nb, double *__restrict__ out,
                                                           double *__restrict__ out2)
{
    __shared__ double sm[kRedThreads / 64];
    double m = -INFINITY;
    for (int i = threadIdx.x; i < nb; i += kRedThreads) m = fmax(m, part[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kRedThreads / 64; ++k) m = fmax(m, sm[k]);
        out[0] = m;
        if (out2) out2[0] = m;
    }
}

__global__ void k_copy_double(const double *__restrict__ src, double *__restrict__ dst) { dst[0] = src[0]; }
__global__ void k_set_double(double *__restrict__ dst, double v) { dst[0] = v; }
// keeps a stream busy for `ms` milliseconds (at most two seconds): the test switch of the sharded update's bounded wait
__global__ void k_spin_ms(double ms)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();           // 100 MHz
    const unsigned long long ticks = (unsigned long long)((ms < 2000.0 ? ms : 2000.0) * 1e5);
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

// mcl_group_update: the maximum over the shards' maxima, read where they live (peer pointers)
__global__ void k_group_max(GroupMaxArgs a)
{
    double m = -INFINITY;
    for (int i = 0; i < a.n; ++i) m = fmax(m, a.src[i][0]);
    a.out[0] = m;
}

// Device-ordered staged flow (mcl_stage_weights_async): this shard's contribution to the one SUM exchange of an update, written
// where the collective reads it.  vec = [sum w, sum w x, sum w y, sum w sin, sum w cos | per shard: list length + 1 (0: no list),
// low and high half of the fixed-point weight total | 1 when the ray stage's fix-up lists overflowed | sum w^2]; every other shard's
// slots are zeroed here, so that the SUM over the shards fills them in.  res = the engine's result block.
__global__ void k_stage_pack(const unsigned long long *__restrict__ res, double *__restrict__ vec, int n_shards, int self, int listed,
                             unsigned long long list_cap)
{
    const int len = 5 + 3 * n_shards + 2;
    const double *sc = reinterpret_cast<const double *>(res);
    for (int i = threadIdx.x; i < len; i += blockDim.x) {
        double v = 0.0;
        if (i == 0) v = sc[1];
        else if (i < 5) v = sc[2 + i];
        else if (i == 5 + 3 * self) v = (listed && res[16] <= list_cap) ? (double)(res[16] + 1ull) : 0.0;
        else if (i == 6 + 3 * self) v = (double)(res[2] & 0xFFFFFFFFull);
        else if (i == 7 + 3 * self) v = (double)(res[2] >> 32);
        else if (i == len - 2) v = res[12] != 0ull ? 1.0 : 0.0;
        else if (i == len - 1) v = sc[7];                       // sum w^2 (adaptive resampling: the effective sample size of the whole set)
        vec[i] = v;
    }
}

// from_log: w = det_exp(logw - *maxp) (max element -> exactly 1), and w = 0 where logw = -inf (E5: also when the maximum is
// -inf, where logw - max would be NaN); else w given, scaled by 1/ *maxp
// for the fixed-point value only.  Writes w, q and per-block partials
// [sum w, sum q (bits), sum w x, sum w y, sum w sin, sum w cos].
__global__ __launch_bounds__(kRedThreads) void k_weights(const double *__restrict__ logw_or_w, int from_log,
                                                        const double *__restrict__ maxp, const double *__restrict__ x,
                                                        const double *__restrict__ y, const double *__restrict__ th, int64_t n,
                                                        double *__restrict__ w_out, uint64_t *__restrict__ q_out,
                                                        double *__restrict__ part /* gridDim.x * 8 */,
                                                        double *__restrict__ carry_out /* logw - max, or null */,
                                                        const double *__restrict__ max_parts = nullptr, int n_max_parts = 0)
{
    __shared__ double sm[kRedThreads / 64][7];
    // max_parts: the maximum is still in pieces (per-workgroup maxima of an earlier kernel; a separate array from `part`): every
    // workgroup reduces the few KB itself -- a maximum does not depend on the order -- instead of a one-workgroup launch in
    // between, and the first leaves it in *maxp for the host
    double mx;
    if (max_parts) {
        __shared__ double mxs[kRedThreads / 64];
        double m = -INFINITY;
        for (int i = threadIdx.x; i < n_max_parts; i += kRedThreads) m = fmax(m, max_parts[i]);
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0) mxs[threadIdx.x >> 6] = m;
        __syncthreads();
        mx = mxs[0];
        for (int k = 1; k < kRedThreads / 64; ++k) mx = fmax(mx, mxs[k]);
        if (blockIdx.x == 0 && threadIdx.x == 0) const_cast<double *>(maxp)[0] = mx;
    } else {
        mx = *maxp;
    }
    double sw = 0, swx = 0, swy = 0, sws = 0, swc = 0, sww = 0;
    uint64_t sq = 0;
    for (int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRedThreads) {
        double w, wq;
        if (from_log) {
            const double lw = logw_or_w[i];
            const double d = lw == -INFINITY ? -INFINITY : lw - mx;
            w = det_exp(d); wq = w; if (carry_out) carry_out[i] = d;
        }
        else {
            w = logw_or_w[i];
            wq = (mx > 0.0 && w > 0.0) ? (w / mx) : 0.0;
        }
        uint64_t q = (uint64_t)(wq * kWeightScale);
        w_out[i] = w;
        q_out[i] = q;
        double s, c;
        sincos(th[i], &s, &c);
        sw += w; sq += q; swx += w * x[i]; swy += w * y[i]; sws += w * s; swc += w * c; sww += w * w;
    }
    sw = wave_sum(sw); swx = wave_sum(swx); swy = wave_sum(swy); sws = wave_sum(sws); swc = wave_sum(swc); sww = wave_sum(sww);
    sq = wave_sum_u64(sq);
    int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sm[wv][0] = sw; sm[wv][1] = __longlong_as_double((long long)sq); sm[wv][2] = swx; sm[wv][3] = swy; sm[wv][4] = sws; sm[wv][5] = swc; sm[wv][6] = sww;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t tq = 0;
        double t[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < kRedThreads / 64; ++k) {
            t[0] += sm[k][0]; tq += (uint64_t)__double_as_longlong(sm[k][1]);
            t[2] += sm[k][2]; t[3] += sm[k][3]; t[4] += sm[k][4]; t[5] += sm[k][5]; t[6] += sm[k][6];
        }
        double *p = part + (size_t)blockIdx.x * 8;
        p[0] = t[0]; p[1] = __longlong_as_double((long long)tq); p[2] = t[2]; p[3] = t[3]; p[4] = t[4]; p[5] = t[5]; p[6] = t[6];
    }
}
// scalars[1..6] = fixed-order sums of the partials (scalars[0] = max stays): the first kRedThreads threads of the workgroup,
// thread t over partials t, t + kRedThreads, ..., wave butterflies, waves in order.  sm: [kRedThreads / 64][7] doubles of LDS.
// Every thread of the workgroup must call it (one barrier inside).
__device__ __forceinline__ void final_sums_of(const double *__restrict__ part, int nb, double *__restrict__ scalars, double (*sm)[7])
{
    const bool mine = threadIdx.x < kRedThreads;
    double t[7] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t tq = 0;
    if (mine)
        for (int i = threadIdx.x; i < nb; i += kRedThreads) {
            const double *p = part + (size_t)i * 8;
            t[0] += p[0]; tq += (uint64_t)__double_as_longlong(p[1]); t[2] += p[2]; t[3] += p[3]; t[4] += p[4]; t[5] += p[5]; t[6] += p[6];
        }
    t[0] = wave_sum(t[0]); t[2] = wave_sum(t[2]); t[3] = wave_sum(t[3]); t[4] = wave_sum(t[4]); t[5] = wave_sum(t[5]); t[6] = wave_sum(t[6]);
    tq = wave_sum_u64(tq);
    int wv = threadIdx.x >> 6;
    if (mine && (threadIdx.x & 63) == 0) {
        sm[wv][0] = t[0]; sm[wv][1] = __longlong_as_double((long long)tq); sm[wv][2] = t[2]; sm[wv][3] = t[3]; sm[wv][4] = t[4]; sm[wv][5] = t[5]; sm[wv][6] = t[6];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[7] = {0, 0, 0, 0, 0, 0, 0};
        uint64_t rq = 0;
        for (int k = 0; k < kRedThreads / 64; ++k) {
            r[0] += sm[k][0]; rq += (uint64_t)__double_as_longlong(sm[k][1]);
            r[2] += sm[k][2]; r[3] += sm[k][3]; r[4] += sm[k][4]; r[5] += sm[k][5]; r[6] += sm[k][6];
        }
        scalars[1] = r[0]; scalars[2] = __longlong_as_double((long long)rq);
        scalars[3] = r[2]; scalars[4] = r[3]; scalars[5] = r[4]; scalars[6] = r[5];
        scalars[7] = r[6];                      // sum w^2: effective sample size = (sum w)^2 / sum w^2
    }
}
__global__ __launch_bounds__(kRedThreads) void k_final_sums(const double *__restrict__ part, int nb, double *__restrict__ scalars)
{
    __shared__ double sm[kRedThreads / 64][7];
    final_sums_of(part, nb, scalars, sm);
}

// The whole tail of a SMALL update (N <= kTinyTailMax) by ONE workgroup: maximum, max-subtracted weights, fixed-point
// weights, the seven sums and the inclusive CDF -- seven launches of ~4 us each otherwise, and no cross-workgroup
// reduction is needed at this size.  Same formulas as k_reduce_max / k_weights / k_scan_*.  The per-particle work (the
// deterministic exp, the weighted sums) is dealt thread-strided so that all 1024 threads work at the stock 2000-4000
// particles; the fixed-point weights wait in LDS for the scan, which needs consecutive runs per thread.  The sums are
// reduced in this kernel's own fixed order (thread-strided, wave butterflies, waves in order): deterministic for a given N.
// pc: (cos, sin, ., .) of every heading as k_particle_prep left them (the same sincos call), or null.
// KLD: the one workgroup also clears the bitmap words the resampling kernel listed (<= n) and reports the bin count (word 17).
constexpr int64_t kTinyTailMax = 8192;
template <bool KLD>
__global__ __launch_bounds__(1024) void k_tiny_tail(const double *__restrict__ logw, const double *__restrict__ x, const double *__restrict__ y,
                                                   const double *__restrict__ th, const double4 *__restrict__ pc, int64_t n,
                                                   double *__restrict__ w_out, uint64_t *__restrict__ q_out, uint64_t *__restrict__ cdf_out,
                                                   double *__restrict__ scalars, unsigned long long *__restrict__ host_out,
                                                   unsigned long long host_seq, KldArgs kld)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char tail_lds[];
    if constexpr (KLD) kld_clear_part(kld, threadIdx.x, 1024);
    uint64_t *q_sh = reinterpret_cast<uint64_t *>(tail_lds);       // n entries
    __shared__ double sm[16][7];
    __shared__ uint64_t wave_tot[16];
    __shared__ double mx_sh;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += 1024) m = fmax(m, logw[i]);
    m = wave_max(m);
    if (lane == 0) sm[wv][0] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sm[0][0];
        for (int k = 1; k < 16; ++k) t = fmax(t, sm[k][0]);
        mx_sh = t;
    }
    __syncthreads();
    const double mx = mx_sh;
    double sw = 0, swx = 0, swy = 0, sws = 0, swc = 0, sww = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const double lw = logw[i];
        const double w = det_exp(lw == -INFINITY ? -INFINITY : lw - mx);      // E5: logw = -inf -> w = 0, even when mx = -inf
        const uint64_t q = (uint64_t)(w * kWeightScale);
        w_out[i] = w;
        q_out[i] = q;
        q_sh[i] = q;
        double s, c;
        if (pc) { const double4 r = pc[i]; c = r.x; s = r.y; }
        else sincos(th[i], &s, &c);
        sw += w; swx += w * x[i]; swy += w * y[i]; sws += w * s; swc += w * c; sww += w * w;
    }
    sw = wave_sum(sw); swx = wave_sum(swx); swy = wave_sum(swy); sws = wave_sum(sws); swc = wave_sum(swc); sww = wave_sum(sww);
    __syncthreads();                            // every q_sh entry written; sm[.][0] (the maxima) read by everyone
    if (lane == 0) { sm[wv][0] = sw; sm[wv][2] = swx; sm[wv][3] = swy; sm[wv][4] = sws; sm[wv][5] = swc; sm[wv][6] = sww; }
    // inclusive scan: thread t owns the `per` consecutive entries from t * per
    const int per = (int)((n + 1023) / 1024);
    const int64_t c0 = (int64_t)threadIdx.x * per;
    uint64_t tot = 0;
    for (int k = 0; k < per; ++k) tot += (c0 + k < n) ? q_sh[c0 + k] : 0ull;
    const uint64_t inc = wave_incl_scan_u64(tot, lane);
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    uint64_t run = inc - tot;
    for (int k = 0; k < wv; ++k) run += wave_tot[k];
    for (int k = 0; k < per; ++k)
        if (c0 + k < n) { run += q_sh[c0 + k]; cdf_out[c0 + k] = run; }
    if (host_out) __syncthreads();              // every store of this kernel is out before the host is told it may look
    if (threadIdx.x == 0) {
        double r[7] = {0, 0, 0, 0, 0, 0, 0};
        uint64_t rq = 0;
        for (int k = 0; k < 16; ++k) { r[0] += sm[k][0]; r[2] += sm[k][2]; r[3] += sm[k][3]; r[4] += sm[k][4]; r[5] += sm[k][5]; r[6] += sm[k][6]; rq += wave_tot[k]; }
        scalars[0] = mx;
        scalars[1] = r[0]; scalars[2] = __longlong_as_double((long long)rq);
        scalars[3] = r[2]; scalars[4] = r[3]; scalars[5] = r[4]; scalars[6] = r[5];
        scalars[7] = r[6];
        if (host_out) {
            // the result block (8 scalars, then the counters and flags the ray kernels left behind them in the same
            // allocation) straight into pinned host memory: no copy node, no hand-over to a DMA engine
            const unsigned long long *blk = reinterpret_cast<const unsigned long long *>(scalars);
            for (int k = 0; k < 8; ++k) host_out[k] = (unsigned long long)__double_as_longlong(scalars[k]);
            for (int k = 8; k < 14; ++k) host_out[k] = blk[k];
            if constexpr (KLD) host_out[17] = *kld.count;
            // the host may be polling word 32 (kResultStamp) instead of waiting for the stream's completion signal
            __threadfence_system();
            __hip_atomic_store(&host_out[32], host_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// out[i] = w[i] / sum (sum > 0) else w[i]   (cpp:680-686)
// log-weights of an update that kept its particles (no resampling): add what they carried
__global__ void k_add_carry(double *__restrict__ logw, const double *__restrict__ carry, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) logw[i] += carry[i];
}

__global__ void k_normalized(const double *__restrict__ w, int64_t n, double sum, double *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (sum > 0.0) ? (w[i] / sum) : w[i];
}

// column sums for particles_.colwise().mean() (cpp:904); part = gridDim.x * 4 doubles
__global__ __launch_bounds__(kRedThreads) void k_colsum(const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ th, int64_t n, double *__restrict__ part)
{
    __shared__ double sm[kRedThreads / 64][3];
    double a = 0, b = 0, c = 0;
    for (int64_t i = (int64_t)blockIdx.x * kRedThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kRedThreads) {
        a += x[i]; b += y[i]; c += th[i];
    }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wv][0] = a; sm[wv][1] = b; sm[wv][2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0, t1 = 0, t2 = 0;
        for (int k = 0; k < kRedThreads / 64; ++k) { t0 += sm[k][0]; t1 += sm[k][1]; t2 += sm[k][2]; }
        part[blockIdx.x * 4 + 0] = t0; part[blockIdx.x * 4 + 1] = t1; part[blockIdx.x * 4 + 2] = t2;
    }
}

// k draws from the current CDF (visualize, cpp:949-956): out k x 3 column-major
__global__ void k_sample(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ th,
                         const uint64_t *__restrict__ cdf, int64_t n, uint64_t q_total, const double *__restrict__ uniforms,
                         uint32_t seed_lo, uint32_t seed_hi, uint32_t ctr, int k, double *__restrict__ out)
{
    int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= k) return;
    uint64_t k53;
    if (uniforms) {
        double u = uniforms[m];
        u = (u >= 0.0) ? u : 0.0;
        k53 = (uint64_t)(u * 9007199254740992.0);
        if (k53 > 9007199254740991ull) k53 = 9007199254740991ull;
    } else {
        u32x4 o = philox4x32((uint32_t)m, ctr, 4u, 0u, seed_lo, seed_hi);
        k53 = bits53(o.v[0], o.v[1]);
    }
    int64_t idx = 0;
    if (q_total) {
        int64_t lo = 0, len = n;
        while (len > 0) {
            int64_t half = len >> 1, mid = lo + half;
            if (!mul_gt(cdf[mid], 1ull << 53, k53, q_total)) { lo = mid + 1; len = len - half - 1; }
            else len = half;
        }
        idx = lo >= n ? n - 1 : lo;
    }
    out[m] = x[idx]; out[k + m] = y[idx]; out[2 * k + m] = th[idx];
}

}  // namespace mcl
