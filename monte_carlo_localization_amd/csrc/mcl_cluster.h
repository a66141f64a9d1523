// mcl_cluster.h -- pose clustering (mcl_pose_clusters): the arguments of its kernels and the device helpers
// they share.  Only mcl_cluster.hip includes it; the engine reaches it through cluster_free (mcl_engine_internal.h).
#pragma once
#include "mcl_engine_internal.h"

namespace mcl_clu {

constexpr uint32_t kNone = 0xFFFFFFFFu;      // a particle in no cluster (q = 0 or the outside bin)
constexpr int kChunk = 512;                  // sorted particles per unit of a moment pass: 8 per lane of one wave
constexpr int32_t kMaxClusters = 65536;

// what the kernels count on the device; copied to the host once, at the end of the call
struct Header {
    unsigned long long q_total, q_outside, n_outside;   // sum q over every particle; q and particles of the outside bin
    unsigned long long n_nodes, n_comp;                  // occupied bins, clusters
};

// every buffer of the pipeline (mcl_cluster.hip allocates them); n particles, max_nodes = min(n, bins of the grid)
struct Args {
    const double *x, *y, *th;
    const uint64_t *q;
    int64_t n;
    mcl::KldArgs kb;                         // the bin rule (its bitmap / list / counter fields are not used)
    uint32_t *bm;                            // one bit per bin of the grid (the outside bin excluded)
    uint32_t *wpref;                         // exclusive prefix of the words' popcounts: node id = rank among occupied bins
    int64_t nwords;
    uint32_t max_nodes;                      // the sentinel key of a particle in no cluster, and the size of every per-node array
    uint32_t *pbin;                          // n: bin of each particle, or kNone
    uint32_t *node_bin, *parent, *rflag, *cid;   // per node: its bin, union-find parent, root flag, exclusive prefix of the flags
    uint32_t *nbins, *first_bin;             // per cluster (in first_bin order)
    uint32_t *key, *val, *key2, *val2;       // n: (cluster, particle index), and sorted by cluster (stable: indices ascending)
    uint32_t *seg_start, *seg_end;           // per cluster: its run of the sorted order
    uint32_t *ucnt, *ubase;                  // per cluster: moment units (kChunk particles each), their exclusive prefix
    uint64_t *wq;                            // per cluster: sum q
    double *mean;                            // per cluster: 3
    uint64_t *ckey, *ckey2;                  // per cluster: ~wq (the sort key of the ranking), sorted
    uint32_t *cval, *cval2, *rank_of;        // cluster index, sorted (rank -> cluster), and its inverse
    double *part;                            // per unit: 6 partial sums (pass 1 uses 4)
    unsigned long long *upart;               // per unit: partial sum of q
    int32_t *label;                          // n: rank of the particle's cluster, or -1
    mcl_cluster_t *out;                      // the max_clusters heaviest
    int32_t max_clusters;
    Header *hdr;
};

// rank of bin b among the occupied bins (its node id); b must be occupied
__device__ __forceinline__ uint32_t node_of(const Args &a, uint32_t b)
{
    const uint32_t w = b >> 5;
    return a.wpref[w] + (uint32_t)__popc(a.bm[w] & ((1u << (b & 31u)) - 1u));
}

__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Union-find with every link pointing to a smaller id (parent[v] <= v): find halves the path it walks; unite hooks the larger
// root under the smaller one by CAS and climbs again when another lane got there first.  The smallest node of a component is
// never hooked, so once every edge is united it is the root of the whole component.
__device__ __forceinline__ uint32_t uf_find(uint32_t *par, uint32_t v)
{
    uint32_t p = uf_load(par + v);
    if (p != v) {
        uint32_t prev = v, next;
        while (p > (next = uf_load(par + p))) {
            uf_store(par + prev, next);
            prev = p;
            p = next;
        }
    }
    return p;
}

__device__ __forceinline__ void uf_unite(uint32_t *par, uint32_t a, uint32_t b)
{
    uint32_t ra = uf_find(par, a), rb = uf_find(par, b);
    while (ra != rb) {
        if (ra < rb) { const uint32_t t = ra; ra = rb; rb = t; }
        uint32_t expected = ra;
        if (__hip_atomic_compare_exchange_strong(par + ra, &expected, rb, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        ra = uf_find(par, expected);
        rb = uf_find(par, rb);
    }
}

// sum over the 64 lanes of a wave in a fixed pattern (every lane ends with the same bits)
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

}  // namespace mcl_clu
