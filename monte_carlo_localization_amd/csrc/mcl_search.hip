// mcl_search.hip -- mcl_global_search: the likelihood-field score of every pose of a regular lattice over the
// map's free cells against one scan, and the best-fitting poses.  Called outside the update: it reads the map's cells, the beams,
// the likelihood field and its table, writes only buffers of its own (struct mcl_search) and leaves every engine state as it was.
//
// A call, on the engine's stream:
//   (upload)         the lattice (positions, their lattice coordinates, the dense position map) and the headings, when they
//                    differ from the last search's; the used beams of the scan from pinned staging
//   k_search_score   one lane per pose, a workgroup = 256 consecutive positions at one heading: the score volume
//   k_search_mark    one lane per pose: candidate or not (S5), every pose's sort key and index, the candidate count
//   radix sort       (key, index) pairs, ascending and stable: the candidates first, best first, ties by index
//   (copy)           the count and the first max_hits pairs; one host wait
// mcl_global_search_sequence (§4.15) is the same call with S scans: the S used-beam lists one after the other, the table of SQ1
// from the host, k_search_score_seq in k_search_score's place, and everything after it unchanged.
// mcl_global_search_streamed (§4.16) walks the same volume in slabs of G headings and never holds more than a slab:
//   per slab:  k_search_score(_seq)  the headings the ring lacks (Args.head0 / ring)
//              k_search_mark_slab    candidate or not, the key, the flag of a candidate worth merging, the candidate count
//              exclusive scan        of the flags
//              k_search_compact      (key, 64-bit index) of the flagged, in index order, behind the running list
//              segmented radix sort  one segment, its end on the device: the list and the slab's candidates, stable
//   (copy)     the counts and the first max_hits pairs of the list; one host wait
#include "mcl_search.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mcl_srch;

constexpr int32_t kMaxHits = 65536;
constexpr size_t kSlabStateBytes = 64;           // 2 SlabState and the 2 bounds of the sort's segment: the end of the streamed search's scratch
static_assert(2 * sizeof(SlabState) + 2 * sizeof(unsigned long long) <= kSlabStateBytes, "the slab states and the segment's bounds");

// the buffers of the search, kept between calls and grown with the lattice
struct mcl_search {
    // the lattice on the device and what it was made from
    unsigned long long lattice_epoch = 0;       // map_epoch of the lattice (0: none)
    int32_t lattice_stride = 0;
    int64_t n_pos = 0;
    int nx = 0, ny = 0;
    std::vector<double> xy;                     // 2 n_pos: the table the device holds
    int64_t cap_pos = 0, cap_map = 0;
    double2 *d_xy = nullptr;
    int2 *d_lat = nullptr;
    int32_t *d_pmap = nullptr;
    std::vector<double> theta;                  // the headings the device holds
    int64_t cap_head = 0;
    double *d_theta = nullptr;
    // the scan
    int64_t cap_b = 0;
    double2 *d_beams = nullptr, *h_beams = nullptr;
    float *h_obs = nullptr;
    // the scan sequence: the table of SQ1 and where each scan's beams begin (pinned staging beside each)
    int64_t cap_off = 0;
    double *d_off = nullptr, *h_off = nullptr;
    int32_t *d_begin = nullptr, *h_begin = nullptr;
    // the volume and the hits
    int64_t cap_poses = 0;
    double *d_score = nullptr;
    uint64_t *d_key = nullptr, *d_key2 = nullptr;
    uint32_t *d_val = nullptr, *d_val2 = nullptr;
    void *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    unsigned long long *d_count = nullptr, *h_count = nullptr;
    uint64_t *h_key = nullptr;                  // kMaxHits each, pinned
    uint32_t *h_val = nullptr;
    // the volume d_score holds: of which map, how many poses (0: none)
    unsigned long long volume_epoch = 0;
    int64_t volume_n = 0;
    size_t device_bytes = 0;
    // the streamed search (§4.16): the ring, a slab's flags / scan / keys, the list with the slab's candidates behind it (twice),
    // the scratch of the scan and the sort; sized by the plan (ST5), reused while a plan fits them
    uint64_t cap_ring = 0, cap_slab = 0;        // bytes of the ring; poses of a slab
    double *d_ring = nullptr;
    uint32_t *d_flag = nullptr, *d_pos = nullptr;
    uint64_t *d_skey = nullptr;
    uint64_t *d_ckey[2] = {nullptr, nullptr}, *d_cidx[2] = {nullptr, nullptr};
    void *d_stmp = nullptr;
    size_t stmp_bytes = 0;
    mcl_srch::SlabState *d_state = nullptr, *h_state = nullptr;     // 2 on the device (inside d_stmp); the last one, pinned
    unsigned long long *d_seg = nullptr;                            // 2 (inside d_stmp)
    uint64_t *h_idx = nullptr;                                      // kMaxHits, pinned
};

namespace {

using mcl_host::dfree;
using mcl_host::fail;

template <class T>
void hfree(T *&p)
{
    if (p) (void)hipHostFree(p);
    p = nullptr;
}

template <class T>
int grow_dev(mcl_engine *h, mcl_search *s, T *&p, size_t want)
{
    dfree(p);
    HIPCHK(h, hipMalloc(&p, want * sizeof(T)));
    s->device_bytes += want * sizeof(T);
    return MCL_OK;
}

template <class T>
int grow_host(mcl_engine *h, T *&p, size_t want)
{
    hfree(p);
    HIPCHK(h, hipHostMalloc((void **)&p, want * sizeof(T)));
    return MCL_OK;
}

#define SRCH_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// the lattice of this map at this stride on the device (formed and uploaded when either changed)
int search_lattice_upload(mcl_engine *h, mcl_search *s, int stride)
{
    if (s->lattice_epoch == h->map_epoch && s->lattice_stride == stride) return MCL_OK;
    s->lattice_epoch = 0;
    std::vector<int32_t> lat, pmap;
    s->xy.clear();
    s->n_pos = mcl_host::search_lattice(stride, h->grid_host.data(), h->W, h->H, h->res, h->ox, h->oy, nullptr, &s->xy, &lat, &pmap, s->nx,
                                        s->ny);
    if (s->n_pos > 0) {
        if (s->n_pos > s->cap_pos) {
            s->cap_pos = 0;
            SRCH_TRY(grow_dev(h, s, s->d_xy, (size_t)s->n_pos));
            SRCH_TRY(grow_dev(h, s, s->d_lat, (size_t)s->n_pos));
            s->cap_pos = s->n_pos;
        }
        if ((int64_t)pmap.size() > s->cap_map) {
            s->cap_map = 0;
            SRCH_TRY(grow_dev(h, s, s->d_pmap, pmap.size()));
            s->cap_map = (int64_t)pmap.size();
        }
        HIPCHK(h, hipMemcpy(s->d_xy, s->xy.data(), (size_t)s->n_pos * sizeof(double2), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(s->d_lat, lat.data(), (size_t)s->n_pos * sizeof(int2), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(s->d_pmap, pmap.data(), pmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    s->lattice_epoch = h->map_epoch;
    s->lattice_stride = stride;
    return MCL_OK;
}

int search_headings_upload(mcl_engine *h, mcl_search *s, int n_head)
{
    if ((int64_t)s->theta.size() == n_head) return MCL_OK;
    s->theta.clear();
    std::vector<double> t((size_t)n_head);
    mcl_host::search_headings(n_head, t.data());
    if (n_head > s->cap_head) {
        s->cap_head = 0;
        SRCH_TRY(grow_dev(h, s, s->d_theta, (size_t)n_head));
        s->cap_head = n_head;
    }
    HIPCHK(h, hipMemcpy(s->d_theta, t.data(), (size_t)n_head * sizeof(double), hipMemcpyHostToDevice));
    s->theta.swap(t);
    return MCL_OK;
}

// room for the counts and the hits on the host, and for a scan of B beams
int search_alloc_scan(mcl_engine *h, mcl_search *s, int B)
{
    if (!s->d_count) {
        SRCH_TRY(grow_dev(h, s, s->d_count, 1));
        SRCH_TRY(grow_host(h, s->h_count, 1));
        SRCH_TRY(grow_host(h, s->h_key, (size_t)kMaxHits));
        SRCH_TRY(grow_host(h, s->h_val, (size_t)kMaxHits));
    }
    if (B > s->cap_b) {
        s->cap_b = 0;
        SRCH_TRY(grow_dev(h, s, s->d_beams, (size_t)B));
        SRCH_TRY(grow_host(h, s->h_beams, (size_t)B));
        SRCH_TRY(grow_host(h, s->h_obs, (size_t)B));
        s->cap_b = B;
    }
    return MCL_OK;
}

// room for a volume of n_poses, its sort and a scan of B beams
int search_alloc(mcl_engine *h, mcl_search *s, int64_t n_poses, int B)
{
    SRCH_TRY(search_alloc_scan(h, s, B));
    if (n_poses > s->cap_poses) {
        s->cap_poses = 0;
        s->volume_n = 0;
        SRCH_TRY(grow_dev(h, s, s->d_score, (size_t)n_poses));
        SRCH_TRY(grow_dev(h, s, s->d_key, (size_t)n_poses));
        SRCH_TRY(grow_dev(h, s, s->d_key2, (size_t)n_poses));
        SRCH_TRY(grow_dev(h, s, s->d_val, (size_t)n_poses));
        SRCH_TRY(grow_dev(h, s, s->d_val2, (size_t)n_poses));
        size_t tb = 0;
        HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, s->d_key, s->d_key2, s->d_val, s->d_val2, (size_t)n_poses, 0, 64, h->stream));
        dfree(s->d_tmp);
        s->tmp_bytes = std::max<size_t>(tb, 16);
        HIPCHK(h, hipMalloc(&s->d_tmp, s->tmp_bytes));
        s->device_bytes += s->tmp_bytes;
        s->cap_poses = n_poses;
    }
    return MCL_OK;
}

// the score a sort key stands for (score_key's inverse)
double key_score(uint64_t key)
{
    const uint64_t asc = ~key;
    const uint64_t b = (asc >> 63) ? (asc & 0x7fffffffffffffffull) : ~asc;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

// What every search checks before it touches the device: the arguments and the readiness (S8).  c receives the config in force.
int search_check(mcl_engine *h, const mcl_search_config_t *cfg, const void *obs, int32_t n_beams, int32_t max_hits,
                 const mcl_search_hit_t *hits, const int64_t *n_hits, mcl_search_config_t &c)
{
    if (cfg) c = *cfg; else mcl_default_search_config(&c);
    if (const char *why = mcl_host::search_invalid(&c)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!obs || !n_hits) return fail(h, MCL_ERR_INVALID_ARG, "global search: obs / n_hits is null");
    if (max_hits < 0 || max_hits > kMaxHits) return fail(h, MCL_ERR_INVALID_ARG, "global search: max_hits must be in [0, 65536]");
    if (max_hits > 0 && !hits) return fail(h, MCL_ERR_INVALID_ARG, "global search: hits is null");
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "global search: no map is set");
    if (h->B <= 0 || h->beam_cs_host.empty()) return fail(h, MCL_ERR_NOT_READY, "global search: no beam angles are set");
    if (!h->lf_on || h->lf_K < 0 || !h->d_lf_D)
        return fail(h, MCL_ERR_NOT_READY, "global search: the likelihood-field model is off (mcl_set_likelihood_field; the search reads its field and table)");
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "global search: n_beams does not match the beam angles");
    return MCL_OK;
}

// What both unstreamed searches do before they score: search_check, the lattice and the headings on the device, room for the
// volume and for n_scans scans.  n_poses receives the size of the volume.
int search_prepare(mcl_engine *h, const mcl_search_config_t *cfg, const void *obs, int n_scans, int32_t n_beams, int32_t max_hits,
                   const mcl_search_hit_t *hits, const int64_t *n_hits, mcl_search_config_t &c, int64_t &n_poses)
{
    SRCH_TRY(search_check(h, cfg, obs, n_beams, max_hits, hits, n_hits, c));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->srch) h->srch = new mcl_search();
    mcl_search *s = h->srch;
    SRCH_TRY(search_lattice_upload(h, s, c.stride_cells));
    if (s->n_pos == 0) return fail(h, MCL_ERR_NOT_READY, "global search: the lattice has no free position on this map");
    n_poses = s->n_pos * (int64_t)c.n_headings;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "global search: n_positions * n_headings must stay below 2^27 (a larger stride_cells or fewer headings)");
    SRCH_TRY(search_headings_upload(h, s, c.n_headings));
    SRCH_TRY(search_alloc(h, s, n_poses, n_scans * h->B));
    s->volume_n = 0;                                             // until this volume is whole
    return MCL_OK;
}

// S3: the used beams of one scan at `out`, through the update's own rule -- the readings of the candidate beams, the others NaN
// (no contribution).  Returns their number.
int search_used_beams(mcl_engine *h, mcl_search *s, int beam_stride, const float *obs, double2 *out)
{
    for (int j = 0; j < h->B; ++j) s->h_obs[j] = (j % beam_stride == 0) ? obs[j] : NAN;
    return mcl_host::lf_used_beams(h, s->h_obs, 1, out);
}

// everything of the kernels' arguments but the beams
Args search_args(const mcl_engine *h, const mcl_search *s, const mcl_search_config_t &c)
{
    Args a{};
    a.xy = s->d_xy; a.lat = s->d_lat; a.pmap = s->d_pmap; a.theta = s->d_theta;
    a.n_pos = (int32_t)s->n_pos; a.n_head = c.n_headings; a.nx = s->nx; a.ny = s->ny;
    a.blocks_per_heading = (uint32_t)((s->n_pos + kThreads - 1) / kThreads);
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.score = s->d_score;
    a.nms = c.nms;
    a.key = s->d_key; a.val = s->d_val; a.count = s->d_count;
    return a;
}

// SQ3 and SQ1 on their way to the device: every scan's used beams, one list after the other (nb: their number), where each list
// begins, and the table of offsets
int search_stage_sequence(mcl_engine *h, mcl_search *s, const mcl_search_config_t &c, const float *scans, const double *rel, int S, int &nb)
{
    const int B = h->B;
    const int64_t n_off = (int64_t)c.n_headings * S * 3;
    if (!s->d_begin) {
        SRCH_TRY(grow_dev(h, s, s->d_begin, (size_t)MCL_SEARCH_MAX_SCANS + 1));
        SRCH_TRY(grow_host(h, s->h_begin, (size_t)MCL_SEARCH_MAX_SCANS + 1));
    }
    if (n_off > s->cap_off) {
        s->cap_off = 0;
        SRCH_TRY(grow_dev(h, s, s->d_off, (size_t)n_off));
        SRCH_TRY(grow_host(h, s->h_off, (size_t)n_off));
        s->cap_off = n_off;
    }

    // SQ3: every scan's used beams, one list after the other; SQ1: the table
    nb = 0;
    for (int sc = 0; sc < S; ++sc) {
        s->h_begin[sc] = nb;
        nb += search_used_beams(h, s, c.beam_stride, scans + (size_t)sc * (size_t)B, s->h_beams + nb);
    }
    s->h_begin[S] = nb;
    mcl_host::search_sequence_offsets(c.n_headings, s->theta.data(), rel, S, s->h_off);
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(s->d_beams, s->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_begin, s->h_begin, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_off, s->h_off, (size_t)n_off * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return MCL_OK;
}

// What both searches do with the volume in d_score (S5): the marking, the sort, the copies, the one host wait, the hits.
int search_finish(mcl_engine *h, mcl_search *s, const Args &a, int64_t n_poses, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits)
{
    hipLaunchKernelGGL(k_search_mark, dim3((unsigned)((n_poses + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    const int64_t top = std::min<int64_t>(max_hits, n_poses);
    if (top > 0) {
        size_t tb = s->tmp_bytes;
        HIPCHK(h, rocprim::radix_sort_pairs(s->d_tmp, tb, s->d_key, s->d_key2, s->d_val, s->d_val2, (size_t)n_poses, 0, 64, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_key, s->d_key2, (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_val, s->d_val2, (size_t)top * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(s->h_count, s->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait
    s->volume_epoch = h->map_epoch;
    s->volume_n = n_poses;

    const int64_t found = (int64_t)*s->h_count;
    *n_hits = found;
    const int64_t m = std::min<int64_t>(top, found);
    for (int64_t r = 0; r < m; ++r) {
        const int64_t idx = (int64_t)s->h_val[r];
        const int64_t k = idx / s->n_pos, p = idx - k * s->n_pos;
        hits[r].pose[0] = s->xy[(size_t)2 * p];
        hits[r].pose[1] = s->xy[(size_t)2 * p + 1];
        hits[r].pose[2] = s->theta[(size_t)k];
        hits[r].log_likelihood = key_score(s->h_key[r]);
        hits[r].index = idx;
    }
    return MCL_OK;
}

// room for the buffers of a plan (ST5): exactly the plan's bytes, when an earlier plan's buffers do not hold it
int search_alloc_slabs(mcl_engine *h, mcl_search *s, const mcl_host::SearchSlabPlan &p)
{
    if (!s->h_state) {
        SRCH_TRY(grow_host(h, s->h_state, 1));
        SRCH_TRY(grow_host(h, s->h_idx, (size_t)kMaxHits));
    }
    if (p.ring_bytes <= s->cap_ring && p.slab_poses <= s->cap_slab) return MCL_OK;
    s->cap_ring = s->cap_slab = 0;
    const mcl_host::SearchSlabPlan &q = p;
    SRCH_TRY(grow_dev(h, s, s->d_ring, (size_t)(q.ring_bytes / sizeof(double))));
    SRCH_TRY(grow_dev(h, s, s->d_flag, (size_t)q.slab_poses));
    SRCH_TRY(grow_dev(h, s, s->d_pos, (size_t)q.slab_poses));
    SRCH_TRY(grow_dev(h, s, s->d_skey, (size_t)q.slab_poses));
    for (int i = 0; i < 2; ++i) {
        SRCH_TRY(grow_dev(h, s, s->d_ckey[i], (size_t)q.list_entries));
        SRCH_TRY(grow_dev(h, s, s->d_cidx[i], (size_t)q.list_entries));
    }
    // the scratch: what the scan and the sort may use, and at its end, 64-byte aligned, the two slab states and the segment's bounds
    dfree(s->d_stmp);
    s->d_state = nullptr; s->d_seg = nullptr;
    HIPCHK(h, hipMalloc(&s->d_stmp, (size_t)q.scratch_bytes));
    s->device_bytes += (size_t)q.scratch_bytes;
    s->stmp_bytes = ((size_t)q.scratch_bytes - kSlabStateBytes) & ~(size_t)63;
    s->d_state = reinterpret_cast<SlabState *>(static_cast<char *>(s->d_stmp) + s->stmp_bytes);
    s->d_seg = reinterpret_cast<unsigned long long *>(s->d_state + 2);
    s->cap_ring = q.ring_bytes;
    s->cap_slab = q.slab_poses;
    return MCL_OK;
}

}  // namespace

extern "C" int mcl_global_search_streamed(mcl_engine_t *h, const mcl_search_config_t *cfg, const mcl_search_stream_config_t *scfg,
                                          const float *scans, const double *rel, int32_t n_scans, int32_t n_beams, int32_t max_hits,
                                          mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[8])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    static const double kZeroRel[3] = {0.0, 0.0, 0.0};
    const bool single = n_scans == 1 && !rel;                       // mcl_global_search's kernel; a zero rel gives the same bits (SQ7)
    if (const char *why = mcl_host::search_sequence_invalid(single ? kZeroRel : rel, n_scans)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!scans) return fail(h, MCL_ERR_INVALID_ARG, "global search: scans is null");
    mcl_search_config_t c;
    SRCH_TRY(search_check(h, cfg, scans, n_beams, max_hits, hits, n_hits, c));
    mcl_search_stream_config_t sc;
    if (scfg) sc = *scfg; else mcl_default_search_stream_config(&sc);

    // the plan, before anything is allocated or uploaded (ST5): the position count of this lattice, on the host
    mcl_search *s = h->srch;
    int64_t n_pos;
    if (s && s->lattice_epoch == h->map_epoch && s->lattice_stride == c.stride_cells) {
        n_pos = s->n_pos;
    } else {
        int nx, ny;
        n_pos = mcl_host::search_lattice(c.stride_cells, h->grid_host.data(), h->W, h->H, h->res, h->ox, h->oy, nullptr, nullptr, nullptr,
                                         nullptr, nx, ny);
    }
    if (n_pos == 0) return fail(h, MCL_ERR_NOT_READY, "global search: the lattice has no free position on this map");
    mcl_host::SearchSlabPlan plan;
    const std::string why = mcl_host::search_slabs(&c, &sc, n_pos, n_scans, plan);
    if (!why.empty()) return fail(h, MCL_ERR_INVALID_ARG, why);

    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!s) s = h->srch = new mcl_search();
    SRCH_TRY(search_lattice_upload(h, s, c.stride_cells));
    SRCH_TRY(search_headings_upload(h, s, c.n_headings));
    SRCH_TRY(search_alloc_scan(h, s, n_scans * h->B));
    SRCH_TRY(search_alloc_slabs(h, s, plan));
    s->volume_n = 0;                                                // ST6: no volume is kept
    const int n = c.n_headings, G = plan.G;
    const int64_t n_poses = s->n_pos * (int64_t)n;
    const uint64_t slab_cap = (uint64_t)G * (uint64_t)s->n_pos, list_cap = mcl_host::kSearchListHits + slab_cap;

    // what the scan and the sort ask for must be within the plan's scratch
    rocprim::double_buffer<uint64_t> keys(s->d_ckey[0], s->d_ckey[1]), vals(s->d_cidx[0], s->d_cidx[1]);
    if (max_hits > 0) {
        size_t scan_b = 0, sort_b = 0;
        HIPCHK(h, rocprim::exclusive_scan(nullptr, scan_b, s->d_flag, s->d_pos, 0u, (size_t)slab_cap, rocprim::plus<uint32_t>(), h->stream));
        HIPCHK(h, rocprim::segmented_radix_sort_pairs(nullptr, sort_b, keys, vals, (unsigned)list_cap, 1u, s->d_seg, s->d_seg + 1, 0, 64,
                                                      h->stream));
        if (std::max(scan_b, sort_b) > s->stmp_bytes)
            return fail(h, MCL_ERR_UNSUPPORTED, "streamed search: the scan or the sort asks for " + std::to_string(std::max(scan_b, sort_b)) +
                                                    " bytes of scratch, the plan has " + std::to_string(s->stmp_bytes));
    }

    // the scans
    int nb = 0;
    if (single) {
        nb = search_used_beams(h, s, c.beam_stride, scans, s->h_beams);
        if (nb > 0) HIPCHK(h, hipMemcpyAsync(s->d_beams, s->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    } else {
        SRCH_TRY(search_stage_sequence(h, s, c, scans, rel, n_scans, nb));
    }
    HIPCHK(h, hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(s->d_state, 0, 2 * sizeof(SlabState), h->stream));
    HIPCHK(h, hipMemsetAsync(s->d_seg, 0, 2 * sizeof(unsigned long long), h->stream));

    SeqArgs q{};
    q.a = search_args(h, s, c);
    q.a.beams = s->d_beams; q.a.nb = nb;
    q.a.score = s->d_ring; q.a.key = s->d_skey; q.a.val = nullptr;
    q.off = s->d_off; q.beam_begin = s->d_begin; q.S = n_scans;
    const bool one_slab = plan.n_slabs == 1;
    const int ring = one_slab ? 0 : G + 2;
    const size_t lds = h->lf_K < mcl::kLfLdsEntries ? (size_t)(h->lf_K + 1) * sizeof(float) : 0;
    // the linear headings [first, last] into the ring ((G + 2) * n_positions < 2^27, so the grid stays far below 2^31 workgroups)
    const auto score = [&](int first, int last) -> int {
        q.a.head0 = first; q.a.ring = ring;
        const dim3 grid((unsigned)((uint64_t)q.a.blocks_per_heading * (uint64_t)(last - first + 1)));
        if (single) {
            if (lds) hipLaunchKernelGGL(k_search_score<true>, grid, dim3(kThreads), lds, h->stream, q.a);
            else hipLaunchKernelGGL(k_search_score<false>, grid, dim3(kThreads), 0, h->stream, q.a);
        } else {
            if (lds) hipLaunchKernelGGL(k_search_score_seq<true>, grid, dim3(kThreads), lds, h->stream, q);
            else hipLaunchKernelGGL(k_search_score_seq<false>, grid, dim3(kThreads), 0, h->stream, q);
        }
        HIPCHK(h, hipGetLastError());
        return MCL_OK;
    };

    int64_t scored = 0;
    int next = one_slab ? 0 : -1;                                   // the next linear heading the ring lacks
    for (int t = 0; t < plan.n_slabs; ++t) {
        const int lo = t * G, g = std::min(G, n - lo);
        const int last = one_slab ? n - 1 : std::min(lo + G, n);    // the slab's headings and one beyond; n stands for heading 0
        if (next <= last) {
            SRCH_TRY(score(next, last));
            scored += last - next + 1;
            next = last + 1;
        }
        SlabArgs m{};
        m.a = q.a;
        m.a.ring = ring;
        m.head_lo = lo; m.g = g; m.wrap = one_slab ? 1 : 0;
        m.max_hits = (uint64_t)max_hits;
        m.in = s->d_state + (t & 1); m.out = s->d_state + ((t + 1) & 1);
        m.flag = s->d_flag; m.pos = s->d_pos;
        m.ckey = keys.current(); m.cidx = vals.current();
        m.seg = s->d_seg;
        const uint64_t n_slab = (uint64_t)g * (uint64_t)s->n_pos;
        const dim3 grid((unsigned)((n_slab + kThreads - 1) / kThreads));
        hipLaunchKernelGGL(k_search_mark_slab, grid, dim3(kThreads), 0, h->stream, m);
        HIPCHK(h, hipGetLastError());
        if (max_hits == 0) continue;
        size_t tb = s->stmp_bytes;
        HIPCHK(h, rocprim::exclusive_scan(s->d_stmp, tb, s->d_flag, s->d_pos, 0u, (size_t)n_slab, rocprim::plus<uint32_t>(), h->stream));
        hipLaunchKernelGGL(k_search_compact, grid, dim3(kThreads), 0, h->stream, m);
        HIPCHK(h, hipGetLastError());
        tb = s->stmp_bytes;
        HIPCHK(h, rocprim::segmented_radix_sort_pairs(s->d_stmp, tb, keys, vals, (unsigned)list_cap, 1u, s->d_seg, s->d_seg + 1, 0, 64,
                                                      h->stream));
    }

    const int64_t top = std::min<int64_t>(max_hits, n_poses);
    if (top > 0) {
        HIPCHK(h, hipMemcpyAsync(s->h_key, keys.current(), (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_idx, vals.current(), (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(s->h_count, s->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->h_state, s->d_state + (plan.n_slabs & 1), sizeof(SlabState), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait

    const int64_t found = (int64_t)*s->h_count;
    *n_hits = found;
    const int64_t m = std::min<int64_t>(top, found);
    for (int64_t r = 0; r < m; ++r) {
        const int64_t idx = (int64_t)s->h_idx[r];
        const int64_t k = idx / s->n_pos, p = idx - k * s->n_pos;
        hits[r].pose[0] = s->xy[(size_t)2 * p];
        hits[r].pose[1] = s->xy[(size_t)2 * p + 1];
        hits[r].pose[2] = s->theta[(size_t)k];
        hits[r].log_likelihood = key_score(s->h_key[r]);
        hits[r].index = idx;
    }
    if (stats) {
        stats[0] = (uint64_t)s->n_pos; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)s->device_bytes;
        stats[4] = (uint64_t)G; stats[5] = (uint64_t)plan.n_slabs; stats[6] = (uint64_t)scored; stats[7] = (uint64_t)s->h_state->compacted;
    }
    return MCL_OK;
}

void search_free(struct mcl_search *s)
{
    if (!s) return;
    dfree(s->d_xy); dfree(s->d_lat); dfree(s->d_pmap); dfree(s->d_theta); dfree(s->d_beams); dfree(s->d_score); dfree(s->d_key); dfree(s->d_key2);
    dfree(s->d_val); dfree(s->d_val2); dfree(s->d_tmp); dfree(s->d_count); dfree(s->d_off); dfree(s->d_begin);
    dfree(s->d_ring); dfree(s->d_flag); dfree(s->d_pos); dfree(s->d_skey); dfree(s->d_ckey[0]); dfree(s->d_ckey[1]); dfree(s->d_cidx[0]);
    dfree(s->d_cidx[1]); dfree(s->d_stmp);
    hfree(s->h_beams); hfree(s->h_obs); hfree(s->h_count); hfree(s->h_key); hfree(s->h_val); hfree(s->h_off); hfree(s->h_begin);
    hfree(s->h_state); hfree(s->h_idx);
    delete s;
}

extern "C" {

int mcl_global_search(mcl_engine_t *h, const mcl_search_config_t *cfg, const float *obs, int32_t n_beams, int32_t max_hits,
                      mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[4])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    mcl_search_config_t c;
    int64_t n_poses = 0;
    SRCH_TRY(search_prepare(h, cfg, obs, 1, n_beams, max_hits, hits, n_hits, c, n_poses));
    mcl_search *s = h->srch;
    const int nb = search_used_beams(h, s, c.beam_stride, obs, s->h_beams);
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(s->d_beams, s->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), h->stream));

    Args a = search_args(h, s, c);
    a.beams = s->d_beams; a.nb = nb;
    // (n_poses < 2^27, so both grids stay far below 2^31 workgroups)
    const dim3 grid_score((unsigned)((uint64_t)a.blocks_per_heading * (uint64_t)c.n_headings));
    if (h->lf_K < mcl::kLfLdsEntries)
        hipLaunchKernelGGL(k_search_score<true>, grid_score, dim3(kThreads), (size_t)(h->lf_K + 1) * sizeof(float), h->stream, a);
    else
        hipLaunchKernelGGL(k_search_score<false>, grid_score, dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    SRCH_TRY(search_finish(h, s, a, n_poses, max_hits, hits, n_hits));
    if (stats) {
        stats[0] = (uint64_t)s->n_pos; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)s->device_bytes;
    }
    return MCL_OK;
}

int mcl_global_search_sequence(mcl_engine_t *h, const mcl_search_config_t *cfg, const float *scans, const double *rel, int32_t n_scans,
                               int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[5])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    // the sequence's own arguments, then everything the single search checks
    if (const char *why = mcl_host::search_sequence_invalid(rel, n_scans)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!scans) return fail(h, MCL_ERR_INVALID_ARG, "global search: scans is null");
    mcl_search_config_t c;
    int64_t n_poses = 0;
    SRCH_TRY(search_prepare(h, cfg, scans, n_scans, n_beams, max_hits, hits, n_hits, c, n_poses));
    mcl_search *s = h->srch;
    const int S = n_scans;
    int nb = 0;
    SRCH_TRY(search_stage_sequence(h, s, c, scans, rel, S, nb));
    HIPCHK(h, hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), h->stream));

    SeqArgs q{};
    q.a = search_args(h, s, c);
    q.a.beams = s->d_beams; q.a.nb = nb;
    q.off = s->d_off; q.beam_begin = s->d_begin; q.S = S;
    const dim3 grid_score((unsigned)((uint64_t)q.a.blocks_per_heading * (uint64_t)c.n_headings));
    if (h->lf_K < mcl::kLfLdsEntries)
        hipLaunchKernelGGL(k_search_score_seq<true>, grid_score, dim3(kThreads), (size_t)(h->lf_K + 1) * sizeof(float), h->stream, q);
    else
        hipLaunchKernelGGL(k_search_score_seq<false>, grid_score, dim3(kThreads), 0, h->stream, q);
    HIPCHK(h, hipGetLastError());
    SRCH_TRY(search_finish(h, s, q.a, n_poses, max_hits, hits, n_hits));
    if (stats) {
        stats[0] = (uint64_t)s->n_pos; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)s->device_bytes;
        stats[4] = (uint64_t)S;
    }
    return MCL_OK;
}

int mcl_get_search_scores(mcl_engine_t *h, double *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    const mcl_search *s = h->srch;
    if (!s || s->volume_n == 0 || s->volume_epoch != h->map_epoch || !h->have_map)
        return fail(h, MCL_ERR_NOT_READY, "no score volume: no global search has run on this map");
    if (n != (size_t)s->volume_n) return fail(h, MCL_ERR_INVALID_ARG, "the volume has n_headings x n_positions entries");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemcpyAsync(out, s->d_score, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_get_search_bytes(const mcl_engine_t *h, uint64_t *bytes)
{
    if (!h || !bytes) return MCL_ERR_INVALID_ARG;
    *bytes = h->srch ? (uint64_t)h->srch->device_bytes : 0;
    return MCL_OK;
}

}  // extern "C"
