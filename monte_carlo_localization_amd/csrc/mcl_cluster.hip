// mcl_cluster.hip -- mcl_pose_clusters / mcl_get_cluster_labels: the pose hypotheses of the particle set, as
// connected components of occupied pose-space bins with their weights, means and covariances.  Called outside the update: it
// reads the current particles and their fixed-point weights and writes only buffers of its own (struct mcl_cluster).
//
// The pipeline, on the engine's stream (grid sizes from host-known bounds; counts the device found are read on the device):
//   k_clu_bin      bin of every particle (kld_bin), test-then-set in the bitmap, the totals Q / outside
//   (scan)         exclusive scan of the bitmap words' popcounts -> node id of an occupied bin = its rank in bin order
//   k_clu_nodes    the bin of every node, parent = self
//   k_clu_union    every node unites with its 13 forward neighbours (heading wraps): union-find, roots = smallest node
//   k_clu_compress parent = root; root flags; exclusive scan -> cluster index (clusters in first_bin order)
//   k_clu_key      (cluster, index) of every particle; k_clu_nbins: bins per cluster, first_bin; radix sort by cluster
//   k_clu_seg      each cluster's run of the sorted order; units of kChunk particles; exclusive scan of the unit counts
//   k_clu_pass1    per unit, one wave: sum q, q x, q y, q sin, q cos in a fixed order; k_clu_comb1 per cluster: mean
//   radix sort of (~weight_q, cluster): the ranks (stable: ties keep first_bin order); k_clu_rank, k_clu_label
//   k_clu_pass2    per unit of a reported cluster: the six second moments about its mean; k_clu_out: the records
// Every fp64 sum has a fixed shape (a unit's lanes add their particles in order, then a fixed butterfly; a cluster's lanes add
// its units in order, then the same butterfly), so the same state gives the same bits; the integer sums are exact.
#include "mcl_cluster.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

using namespace mcl_clu;

namespace mcl_clu {     // (named: the kernels keep readable symbols)

constexpr int kThreads = 256;

// the flat loops run over waves: every lane of a wave takes the same number of trips (the ballots stay whole)
__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ int64_t gthreads() { return (int64_t)gridDim.x * blockDim.x; }
__device__ __forceinline__ int64_t gwave() { return gtid() >> 6; }
__device__ __forceinline__ int64_t gwaves() { return gthreads() >> 6; }

__global__ __launch_bounds__(kThreads) void k_clu_bin(Args a)
{
    const int64_t i = gtid();
    const int lane = (int)(threadIdx.x & 63);
    uint32_t b = kNone;
    unsigned long long qi = 0, qo = 0, no = 0;
    if (i < a.n) {
        qi = a.q[i];
        const uint32_t bb = mcl::kld_bin(a.kb, a.x[i], a.y[i], a.th[i]);
        if (bb == a.kb.outside) { qo = qi; no = 1; }
        else if (qi != 0) b = bb;
        a.pbin[i] = b;
    }
    // test-then-set, one fetch-or per distinct new bin of the wave (the KLD marking's scheme, mcl_resample.h)
    const uint32_t wi = b >> 5, bit = 1u << (b & 31u);
    const bool need = b != kNone && !(a.bm[wi] & bit);
    for (unsigned long long pending = __ballot(need); pending;) {
        const int l = __ffsll((long long)pending) - 1;
        const uint32_t bl = (uint32_t)__shfl((int)b, l);
        pending &= ~__ballot(need && b == bl);
        if (lane == l) __hip_atomic_fetch_or(&a.bm[wi], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // the totals: wave sums, then one atomic per wave (integers: any order gives the same sum)
    qi = wave_sum(qi); qo = wave_sum(qo); no = wave_sum(no);
    if (lane == 0) {
        if (qi) atomicAdd(&a.hdr->q_total, qi);
        if (no) { atomicAdd(&a.hdr->q_outside, qo); atomicAdd(&a.hdr->n_outside, no); }
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_nodes(Args a)
{
    for (int64_t w = gtid(); w < a.nwords; w += gthreads()) {
        uint32_t bits = a.bm[w];
        const uint32_t base = a.wpref[w];
        if (w == a.nwords - 1) a.hdr->n_nodes = base + (uint32_t)__popc(bits);
        for (uint32_t j = 0; bits; ++j, bits &= bits - 1u) {
            const uint32_t node = base + j;
            a.node_bin[node] = (uint32_t)(w * 32) + (uint32_t)(__ffs(bits) - 1);
            a.parent[node] = node;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_union(Args a)
{
    const int64_t nn = (int64_t)a.hdr->n_nodes;
    const uint32_t nx = a.kb.nx, ny = a.kb.ny, nth = a.kb.nth;
    for (int64_t v = gtid(); v < nn; v += gthreads()) {
        const uint32_t b = a.node_bin[v];
        const int64_t ix = b % nx, r = b / nx, iy = r % ny, it = r / ny;
        // the 13 offsets (dt, dy, dx) after (0, 0, 0) in lexicographic order: with their negatives they are all 26, so every
        // pair of touching bins is tested by one of its two nodes
        for (int o = 14; o < 27; ++o) {
            const int dt = o / 9 - 1, dy = (o / 3) % 3 - 1, dx = o % 3 - 1;
            const int64_t jx = ix + dx, jy = iy + dy;
            if (jx < 0 || jx >= (int64_t)nx || jy < 0 || jy >= (int64_t)ny) continue;
            int64_t jt = it + dt;
            if (jt < 0) jt += nth;
            else if (jt >= (int64_t)nth) jt -= nth;
            const uint32_t nb = (uint32_t)((jt * ny + jy) * nx + jx);
            if (nb == b || !((a.bm[nb >> 5] >> (nb & 31u)) & 1u)) continue;
            uf_unite(a.parent, (uint32_t)v, node_of(a, nb));
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_compress(Args a)
{
    const int64_t nn = (int64_t)a.hdr->n_nodes;
    for (int64_t v = gtid(); v < (int64_t)a.max_nodes; v += gthreads()) {
        uint32_t flag = 0;
        if (v < nn) {
            uint32_t r = (uint32_t)v, p;
            while ((p = uf_load(a.parent + r)) != r) r = p;
            uf_store(a.parent + v, r);
            flag = r == (uint32_t)v;
        }
        a.rflag[v] = flag;
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_key(Args a)
{
    const int64_t nn = (int64_t)a.hdr->n_nodes;
    if (gtid() == 0) a.hdr->n_comp = nn ? a.cid[nn - 1] + a.rflag[nn - 1] : 0;
    for (int64_t i = gtid(); i < a.n; i += gthreads()) {
        const uint32_t b = a.pbin[i];
        a.key[i] = b == kNone ? a.max_nodes : a.cid[a.parent[node_of(a, b)]];
        a.val[i] = (uint32_t)i;
    }
}

// bins per cluster: one atomic per distinct cluster of a wave (the nodes of a wave are neighbours in bin order)
__global__ __launch_bounds__(kThreads) void k_clu_nbins(Args a)
{
    const int64_t nn = (int64_t)a.hdr->n_nodes;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t base = gwave() * 64; base < nn; base += gwaves() * 64) {
        const int64_t v = base + lane;
        const bool valid = v < nn;
        uint32_t c = 0;
        if (valid) {
            const uint32_t r = a.parent[v];
            c = a.cid[r];
            if (r == (uint32_t)v) a.first_bin[c] = a.node_bin[v];
        }
        for (unsigned long long pending = __ballot(valid); pending;) {
            const int l = __ffsll((long long)pending) - 1;
            const uint32_t cl = (uint32_t)__shfl((int)c, l);
            const unsigned long long m = __ballot(valid && c == cl);
            pending &= ~m;
            if (lane == l) atomicAdd(&a.nbins[cl], (uint32_t)__popcll(m));
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_seg(Args a)
{
    for (int64_t p = gtid(); p < a.n; p += gthreads()) {
        const uint32_t k = a.key2[p];
        if (k == a.max_nodes) continue;
        if (p == 0 || a.key2[p - 1] != k) a.seg_start[k] = (uint32_t)p;
        if (p == a.n - 1 || a.key2[p + 1] != k) a.seg_end[k] = (uint32_t)(p + 1);
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_ucnt(Args a)
{
    const int64_t nc = (int64_t)a.hdr->n_comp;
    for (int64_t c = gtid(); c < (int64_t)a.max_nodes; c += gthreads())
        a.ucnt[c] = c < nc ? (a.seg_end[c] - a.seg_start[c] + (uint32_t)kChunk - 1u) / (uint32_t)kChunk : 0u;
}

// the cluster of unit u: the last c with ubase[c] <= u (every cluster has at least one unit: ubase rises strictly)
__device__ __forceinline__ uint32_t unit_owner(const Args &a, int64_t nc, int64_t u)
{
    int64_t lo = 0, hi = nc;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)a.ubase[mid] <= u) lo = mid;
        else hi = mid;
    }
    return (uint32_t)lo;
}

__device__ __forceinline__ int64_t n_units(const Args &a, int64_t nc) { return nc ? (int64_t)a.ubase[nc - 1] + a.ucnt[nc - 1] : 0; }

__global__ __launch_bounds__(kThreads) void k_clu_pass1(Args a)
{
    const int64_t nc = (int64_t)a.hdr->n_comp, nu = n_units(a, nc);
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t u = gwave(); u < nu; u += gwaves()) {
        const uint32_t c = unit_owner(a, nc, u);
        const int64_t s = (int64_t)a.seg_start[c] + (u - a.ubase[c]) * kChunk, e = std::min<int64_t>(s + kChunk, a.seg_end[c]);
        unsigned long long wq = 0;
        double sx = 0.0, sy = 0.0, ss = 0.0, sc = 0.0;
        for (int64_t p = s + lane; p < e; p += 64) {
            const uint32_t i = a.val2[p];
            const uint64_t qi = a.q[i];
            const double qd = (double)qi, t = a.th[i];
            wq += qi;
            sx += qd * a.x[i];
            sy += qd * a.y[i];
            ss += qd * sin(t);
            sc += qd * cos(t);
        }
        wq = wave_sum(wq); sx = wave_sum(sx); sy = wave_sum(sy); ss = wave_sum(ss); sc = wave_sum(sc);
        if (lane == 0) {
            a.upart[u] = wq;
            double *o = a.part + u * 6;
            o[0] = sx; o[1] = sy; o[2] = ss; o[3] = sc;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_comb1(Args a)
{
    const int64_t nc = (int64_t)a.hdr->n_comp;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t c = gwave(); c < nc; c += gwaves()) {
        const int64_t u0 = a.ubase[c], u1 = u0 + a.ucnt[c];
        unsigned long long wq = 0;
        double sx = 0.0, sy = 0.0, ss = 0.0, sc = 0.0;
        for (int64_t u = u0 + lane; u < u1; u += 64) {
            const double *p = a.part + u * 6;
            wq += a.upart[u];
            sx += p[0]; sy += p[1]; ss += p[2]; sc += p[3];
        }
        wq = wave_sum(wq); sx = wave_sum(sx); sy = wave_sum(sy); ss = wave_sum(ss); sc = wave_sum(sc);
        if (lane == 0) {
            const double W = (double)wq;
            a.wq[c] = wq;
            a.mean[c * 3 + 0] = sx / W;
            a.mean[c * 3 + 1] = sy / W;
            a.mean[c * 3 + 2] = atan2(ss, sc);
            a.ckey[c] = ~(uint64_t)wq;
            a.cval[c] = (uint32_t)c;
        }
    }
    // the rest of the ranking's input sorts after every cluster (a cluster's weight_q is at least 1)
    for (int64_t c = nc + gtid(); c < (int64_t)a.max_nodes; c += gthreads()) {
        a.ckey[c] = ~0ull;
        a.cval[c] = (uint32_t)c;
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_rank(Args a)
{
    const int64_t nc = (int64_t)a.hdr->n_comp;
    for (int64_t k = gtid(); k < nc; k += gthreads()) a.rank_of[a.cval2[k]] = (uint32_t)k;
}

__global__ __launch_bounds__(kThreads) void k_clu_label(Args a)
{
    for (int64_t p = gtid(); p < a.n; p += gthreads()) {
        const uint32_t k = a.key2[p];
        a.label[a.val2[p]] = k == a.max_nodes ? -1 : (int32_t)a.rank_of[k];
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_pass2(Args a)
{
    const int64_t nc = (int64_t)a.hdr->n_comp, nu = n_units(a, nc);
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t u = gwave(); u < nu; u += gwaves()) {
        const uint32_t c = unit_owner(a, nc, u);
        if (a.rank_of[c] >= (uint32_t)a.max_clusters) continue;
        const int64_t s = (int64_t)a.seg_start[c] + (u - a.ubase[c]) * kChunk, e = std::min<int64_t>(s + kChunk, a.seg_end[c]);
        const double mx = a.mean[c * 3 + 0], my = a.mean[c * 3 + 1], mt = a.mean[c * 3 + 2];
        double sxx = 0.0, sxy = 0.0, sxt = 0.0, syy = 0.0, syt = 0.0, stt = 0.0;
        for (int64_t p = s + lane; p < e; p += 64) {
            const uint32_t i = a.val2[p];
            const double qd = (double)a.q[i];
            const double dx = a.x[i] - mx, dy = a.y[i] - my, dt = remainder(a.th[i] - mt, 2.0 * 3.14159265358979323846);
            const double qx = qd * dx, qy = qd * dy, qt = qd * dt;
            sxx += qx * dx; sxy += qx * dy; sxt += qx * dt;
            syy += qy * dy; syt += qy * dt; stt += qt * dt;
        }
        sxx = wave_sum(sxx); sxy = wave_sum(sxy); sxt = wave_sum(sxt); syy = wave_sum(syy); syt = wave_sum(syt); stt = wave_sum(stt);
        if (lane == 0) {
            double *o = a.part + u * 6;
            o[0] = sxx; o[1] = sxy; o[2] = sxt; o[3] = syy; o[4] = syt; o[5] = stt;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_clu_out(Args a)
{
    const int64_t nc = (int64_t)a.hdr->n_comp, nk = std::min<int64_t>(nc, a.max_clusters);
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t k = gwave(); k < nk; k += gwaves()) {
        const uint32_t c = a.cval2[k];
        const int64_t u0 = a.ubase[c], u1 = u0 + a.ucnt[c];
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t u = u0 + lane; u < u1; u += 64)
            for (int j = 0; j < 6; ++j) s[j] += a.part[u * 6 + j];
        for (int j = 0; j < 6; ++j) s[j] = wave_sum(s[j]);
        if (lane == 0) {
            mcl_cluster_t r;
            const uint64_t wq = a.wq[c];
            const double W = (double)wq;
            r.weight_q = wq;
            r.weight = W / (double)a.hdr->q_total;
            r.n_particles = (int64_t)(a.seg_end[c] - a.seg_start[c]);
            r.n_bins = a.nbins[c];
            r.first_bin = a.first_bin[c];
            for (int j = 0; j < 3; ++j) r.mean[j] = a.mean[c * 3 + j];
            r.cov[0] = s[0] / W; r.cov[1] = s[1] / W; r.cov[2] = s[2] / W;
            r.cov[3] = r.cov[1]; r.cov[4] = s[3] / W; r.cov[5] = s[4] / W;
            r.cov[6] = r.cov[2]; r.cov[7] = r.cov[5]; r.cov[8] = s[5] / W;
            a.out[k] = r;
        }
    }
}

struct Popc {
    __host__ __device__ uint32_t operator()(uint32_t w) const { return (uint32_t)__builtin_popcount(w); }
};

inline int bit_width(uint64_t v)
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

}  // namespace mcl_clu

// the buffers of the clustering, kept between calls and grown when the grid, N or max_clusters grows (the fields of Args they fill)
struct mcl_cluster {
    DevBuf<uint32_t> bm, wpref, pbin, node_bin, parent, rflag, cid, nbins, first_bin, key, val, key2, val2, seg_start, seg_end, ucnt, ubase;
    DevBuf<uint64_t> wq, ckey, ckey2;
    DevBuf<double> mean, part;
    DevBuf<uint32_t> cval, cval2, rank_of;
    DevBuf<unsigned long long> upart;
    DevBuf<int32_t> label;
    DevBuf<mcl_cluster_t> out;
    DevBuf<Header> hdr;
    DevBuf<unsigned char> tmp;               // rocPRIM's scratch, in bytes
    HostBuf<Header> h_hdr;
    HostBuf<mcl_cluster_t> h_out;
    bool labels_valid = false;
    unsigned long long labels_epoch = 0;
    int64_t labels_n = 0;
};

void cluster_free(struct mcl_cluster *c) { delete c; }

namespace {

using mcl_host::fail;

// buffers for n particles, max_nodes nodes, nwords bitmap words, K reported clusters (none of them empty); a: the kernels' view
int cluster_alloc(mcl_engine *h, mcl_cluster *c, int64_t n, int64_t max_nodes, int64_t nwords, int64_t K, Args &a)
{
    const size_t sn = (size_t)std::max<int64_t>(n, 1), sm = (size_t)std::max<int64_t>(max_nodes, 1), sw = (size_t)std::max<int64_t>(nwords, 1);
    const size_t su = (size_t)std::max<int64_t>((n + kChunk - 1) / kChunk + max_nodes, 1), sk = (size_t)std::max<int64_t>(K, 1);
#define CLU_BUF(field, want) do { MCL_TRY(c->field.reserve(h, want)); a.field = c->field; } while (0)
    CLU_BUF(bm, sw); CLU_BUF(wpref, sw);
    CLU_BUF(pbin, sn); CLU_BUF(key, sn); CLU_BUF(val, sn); CLU_BUF(key2, sn); CLU_BUF(val2, sn); CLU_BUF(label, sn);
    CLU_BUF(node_bin, sm); CLU_BUF(parent, sm); CLU_BUF(rflag, sm); CLU_BUF(cid, sm); CLU_BUF(nbins, sm); CLU_BUF(first_bin, sm);
    CLU_BUF(seg_start, sm); CLU_BUF(seg_end, sm); CLU_BUF(ucnt, sm); CLU_BUF(ubase, sm); CLU_BUF(wq, sm); CLU_BUF(mean, sm * 3);
    CLU_BUF(ckey, sm); CLU_BUF(ckey2, sm); CLU_BUF(cval, sm); CLU_BUF(cval2, sm); CLU_BUF(rank_of, sm);
    CLU_BUF(part, su * 6); CLU_BUF(upart, su);
    CLU_BUF(out, sk); CLU_BUF(hdr, 1);
#undef CLU_BUF
    MCL_TRY(c->h_out.reserve(h, sk));
    MCL_TRY(c->h_hdr.reserve(h, 1));
    // rocPRIM's scratch: the largest of the two scans and the two sorts at these sizes
    size_t need = 0, b = 0;
    HIPCHK(h, rocprim::exclusive_scan(nullptr, b, rocprim::make_transform_iterator(a.bm, Popc{}), a.wpref, 0u, (size_t)nwords,
                                      rocprim::plus<uint32_t>(), h->stream));
    need = std::max(need, b);
    HIPCHK(h, rocprim::exclusive_scan(nullptr, b, a.rflag, a.cid, 0u, (size_t)max_nodes, rocprim::plus<uint32_t>(), h->stream));
    need = std::max(need, b);
    HIPCHK(h, rocprim::radix_sort_pairs(nullptr, b, a.key, a.key2, a.val, a.val2, (size_t)n, 0, 32, h->stream));
    need = std::max(need, b);
    HIPCHK(h, rocprim::radix_sort_pairs(nullptr, b, a.ckey, a.ckey2, a.cval, a.cval2, (size_t)max_nodes, 0, 64, h->stream));
    need = std::max(need, b);
    return c->tmp.reserve(h, std::max<size_t>(need, 16));
}

unsigned grid_of(const mcl_engine *h, int64_t threads)
{
    const int64_t blocks = (threads + kThreads - 1) / kThreads;
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, (int64_t)h->num_cu * 8));
}

const char *config_invalid(const mcl_cluster_config_t *c)
{
    if (!(std::isfinite(c->bin_x_m) && c->bin_x_m > 0.0 && std::isfinite(c->bin_y_m) && c->bin_y_m > 0.0))
        return "clusters: bin sizes must be finite and positive";
    if (c->n_theta_bins < 1) return "clusters: n_theta_bins must be >= 1";
    if (c->reserved != 0) return "clusters: reserved must be 0";
    return nullptr;
}

#define CLU_LAUNCH(kernel, grid)                                                                  \
    do {                                                                                          \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kThreads), 0, h->stream, a);                  \
        HIPCHK(h, hipGetLastError());                                                             \
    } while (0)

}  // namespace

extern "C" {

void mcl_default_cluster_config(mcl_cluster_config_t *c)
{
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->bin_x_m = 0.5; c->bin_y_m = 0.5;
    c->n_theta_bins = 36;
}

int mcl_pose_clusters(mcl_engine_t *h, const mcl_cluster_config_t *cfg, int32_t max_clusters, mcl_cluster_t *out, int64_t *n_clusters,
                      uint64_t totals[3])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!cfg) return fail(h, MCL_ERR_INVALID_ARG, "clusters: null config");
    if (const char *why = config_invalid(cfg)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (max_clusters < 0 || max_clusters > kMaxClusters) return fail(h, MCL_ERR_INVALID_ARG, "clusters: max_clusters must be in [0, 65536]");
    if (max_clusters > 0 && !out) return fail(h, MCL_ERR_INVALID_ARG, "clusters: out is null");
    if (h->comm || h->in_group)
        return fail(h, MCL_ERR_UNSUPPORTED, "clusters: single engine only (this engine has a communicator or belongs to a device group)");
    if (!h->have_map || !h->have_particles || h->N <= 0) return fail(h, MCL_ERR_NOT_READY, "clusters: map and particles must be set first");
    mcl_kld_config_t kc{};
    kc.bin_x_m = cfg->bin_x_m; kc.bin_y_m = cfg->bin_y_m; kc.n_theta_bins = cfg->n_theta_bins;
    int64_t nx = 0, ny = 0;
    uint64_t bits = 0;
    if (!mcl_host::kld_grid(&kc, (uint32_t)h->W, (uint32_t)h->H, (float)h->res, nx, ny, bits))
        return fail(h, MCL_ERR_INVALID_ARG, "clusters: the bin grid over this map exceeds 2^31 bits");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->clu) h->clu = new mcl_cluster();
    mcl_cluster *c = h->clu;
    c->labels_valid = false;
    const int64_t n = h->N, grid_bins = (int64_t)bits - 1;       // (the outside bin has no bit)
    const int64_t max_nodes = std::min<int64_t>(n, grid_bins), nwords = (grid_bins + 31) / 32;
    Args a{};
    int rc = cluster_alloc(h, c, n, max_nodes, nwords, max_clusters, a);
    if (rc) return rc;

    const int cur = h->cur;
    a.x = h->d_x[cur]; a.y = h->d_y[cur]; a.th = h->d_th[cur]; a.q = h->d_q; a.n = n;
    a.kb = mcl_host::kld_args_of(&kc, nx, ny, h->ox, h->oy);
    a.nwords = nwords;
    a.max_nodes = (uint32_t)max_nodes;
    a.max_clusters = max_clusters;
    HIPCHK(h, hipMemsetAsync(a.bm, 0, (size_t)nwords * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(a.nbins, 0, (size_t)max_nodes * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(a.hdr, 0, sizeof(Header), h->stream));

    size_t tb = c->tmp.cap;
    CLU_LAUNCH(k_clu_bin, (unsigned)((n + kThreads - 1) / kThreads));
    HIPCHK(h, rocprim::exclusive_scan(c->tmp.p, tb, rocprim::make_transform_iterator(a.bm, Popc{}), a.wpref, 0u, (size_t)nwords,
                                      rocprim::plus<uint32_t>(), h->stream));
    CLU_LAUNCH(k_clu_nodes, grid_of(h, nwords));
    CLU_LAUNCH(k_clu_union, grid_of(h, max_nodes));
    CLU_LAUNCH(k_clu_compress, grid_of(h, max_nodes));
    tb = c->tmp.cap;
    HIPCHK(h, rocprim::exclusive_scan(c->tmp.p, tb, a.rflag, a.cid, 0u, (size_t)max_nodes, rocprim::plus<uint32_t>(), h->stream));
    CLU_LAUNCH(k_clu_key, grid_of(h, n));
    CLU_LAUNCH(k_clu_nbins, grid_of(h, max_nodes));
    tb = c->tmp.cap;
    HIPCHK(h, rocprim::radix_sort_pairs(c->tmp.p, tb, a.key, a.key2, a.val, a.val2, (size_t)n, 0, bit_width((uint64_t)max_nodes), h->stream));
    CLU_LAUNCH(k_clu_seg, grid_of(h, n));
    CLU_LAUNCH(k_clu_ucnt, grid_of(h, max_nodes));
    tb = c->tmp.cap;
    HIPCHK(h, rocprim::exclusive_scan(c->tmp.p, tb, a.ucnt, a.ubase, 0u, (size_t)max_nodes, rocprim::plus<uint32_t>(), h->stream));
    const int64_t units = (n + kChunk - 1) / kChunk + max_nodes;
    CLU_LAUNCH(k_clu_pass1, grid_of(h, units * 64));
    CLU_LAUNCH(k_clu_comb1, grid_of(h, max_nodes * 64));
    tb = c->tmp.cap;
    HIPCHK(h, rocprim::radix_sort_pairs(c->tmp.p, tb, a.ckey, a.ckey2, a.cval, a.cval2, (size_t)max_nodes, 0, 64, h->stream));
    CLU_LAUNCH(k_clu_rank, grid_of(h, max_nodes));
    CLU_LAUNCH(k_clu_label, grid_of(h, n));
    if (max_clusters > 0) {
        CLU_LAUNCH(k_clu_pass2, grid_of(h, units * 64));
        CLU_LAUNCH(k_clu_out, grid_of(h, (int64_t)max_clusters * 64));
        HIPCHK(h, hipMemcpyAsync(c->h_out, a.out, (size_t)max_clusters * sizeof(mcl_cluster_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(c->h_hdr, a.hdr, sizeof(Header), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait

    const Header &hd = *c->h_hdr;
    const int64_t nk = std::min<int64_t>((int64_t)hd.n_comp, max_clusters);
    if (nk > 0) std::memcpy(out, c->h_out, (size_t)nk * sizeof(mcl_cluster_t));
    if (max_clusters > nk) std::memset(out + nk, 0, (size_t)(max_clusters - nk) * sizeof(mcl_cluster_t));
    if (n_clusters) *n_clusters = (int64_t)hd.n_comp;
    if (totals) { totals[0] = hd.q_total; totals[1] = hd.q_outside; totals[2] = hd.n_outside; }
    c->labels_valid = true;
    c->labels_epoch = h->set_epoch;
    c->labels_n = n;
    return MCL_OK;
}

int mcl_get_cluster_labels(mcl_engine_t *h, int32_t *labels, int64_t n)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    mcl_cluster *c = h->clu;
    if (!c || !c->labels_valid || !h->have_particles || c->labels_epoch != h->set_epoch || c->labels_n != h->N)
        return fail(h, MCL_ERR_NOT_READY, "clusters: no clustering of the current particle set (call mcl_pose_clusters first)");
    if (!labels || n != h->N) return fail(h, MCL_ERR_INVALID_ARG, "clusters: labels must hold N entries");
    return read_back(h, {{labels, c->label, (size_t)n * sizeof(int32_t)}});
}

}  // extern "C"
