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
// mcl_global_search_beam (§4.17) fills the same volume under the beam model, from a per-position ray table made in tiles:
//   k_beam_rows          once: the table rows of the scan's used beams
//   per tile:  k_beam_table        one lane per (position, grid angle): E3's step, flagged rays listed
//              k_beam_table_exact  one wave per listed ray: the literal march
//              k_beam_score        one lane per pose: the in-order sum of the rows' entries at the tile's steps
//   then k_search_mark, the sort and the copies as above (search_finish)
// mcl_global_search_pruned (§4.20) reports mcl_global_search's hits from the blocks of poses a bound cannot rule out:
//   (once per map, field, w)   k_lf_pool_rows, k_lf_pool_cols: the pooled field Dp
//   k_search_bound        one lane per (block, heading) pair: U
//   radix sort            the pairs, U descending, ties by pair; k_search_rank: the slot map
//   per round: k_search_score_block  one wave per pair of the round's ranks: its S x S scores into the store
//              k_search_mark_block   S5 over the scored pairs, an unscored neighbour counting as worse
//              two radix sorts       the store's entries by index, then stably by key: the candidates, best first
//              k_search_decide       c, stop or not, the first rank below c
//              (copy)                the round's state and the first max_hits entries; the round's one host wait
// mcl_global_search_sequence_pruned (§4.21) is the same call with S scans: the staging of mcl_global_search_sequence,
// k_search_bound_seq and k_search_score_block_seq in the places of k_search_bound and k_search_score_block (PruneKernels), and
// everything else unchanged.
#include "mcl_search.h"
#include "mcl_search_beam.h"
#include "mcl_search_pruned.h"
#include "mcl_side_buffers.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

using namespace mcl_srch;
using namespace mcl_side;
using mcl_host::fail;

constexpr int32_t kMaxHits = 65536;
constexpr size_t kSlabStateBytes = 64;           // 2 SlabState and the 2 bounds of the sort's segment: the end of the streamed search's scratch
static_assert(2 * sizeof(SlabState) + 2 * sizeof(unsigned long long) <= kSlabStateBytes, "the slab states and the segment's bounds");

// the buffers of a streamed search's plan (§4.16, ST5): made together with exactly the plan's bytes, reused while a plan fits
// them, dropped together when one does not
struct SlabBufs {
    DevBuf<double> ring;
    DevBuf<uint32_t> flag, pos;                  // a slab's flags and their exclusive scan
    DevBuf<uint64_t> skey;                       // a slab's keys
    DevBuf<uint64_t> ckey[2], cidx[2];           // the list with the slab's candidates behind it, twice
    DevBuf<char> tmp;                            // the scratch of the scan and the sort: tmp_bytes of it, then, 64-byte aligned,
    size_t tmp_bytes = 0;                        // the two slab states and the segment's bounds
    SlabState *state = nullptr;                  // 2 (inside tmp)
    unsigned long long *seg = nullptr;           // 2 (inside tmp); set last: null until every buffer is there
};

// the ray table a beam search left on the device (B5): of which map, its shape, which positions (n = 0: none)
struct BeamTable {
    unsigned long long epoch = 0;
    int32_t M = 0, entry_bytes = 0;
    int64_t T = 0, first = 0, n = 0;
};

// the buffers of a pruned search (§4.20), kept between calls: the pooled field of one (map, field, w), the block tables of one
// (lattice, S), the bounds of the last call, the store of scores and its sort buffers (grown by rounds, never beyond the volume)
struct PruneBufs {
    size_t bytes = 0;                            // what these buffers have asked of the device so far
    unsigned long long pool_map = 0, pool_lf = 0;
    int pool_w = 0;                              // 0: no pooled field
    DevBuf<uint16_t> d_R, d_Dp;                  // the row pass's output, Dp
    DevBuf<float> d_ub;
    unsigned long long blk_epoch = 0;            // lattice_epoch of the block tables (0: none)
    int blk_stride = 0, blk_S = 0;
    mcl_host::SearchBlocks plan;
    DevBuf<double4> d_corner;
    DevBuf<int2> d_blk;
    DevBuf<int32_t> d_bmap;
    DevBuf<double> d_U;
    DevBuf<uint64_t> d_ukey[2];
    DevBuf<uint32_t> d_upair[2], d_rank;
    Volume bounds;                               // what d_U holds: of which map, how many pairs
    DevBuf<double> store;
    DevBuf<uint64_t> ckey[2];
    DevBuf<uint32_t> cval[2];
    DevBuf<char> tmp;                            // the sorts' scratch
    DevBuf<unsigned long long> d_guard;
    HostBuf<unsigned long long> h_guard;
    DevBuf<mcl_prune::Round> d_round;
    HostBuf<mcl_prune::Round> h_round;
};

// the buffers of the search, kept between calls and grown with the lattice
struct mcl_search {
    // the lattice on the device and what it was made from
    unsigned long long lattice_epoch = 0;       // map_epoch of the lattice (0: none)
    int32_t lattice_stride = 0;
    int64_t n_pos = 0;
    int nx = 0, ny = 0;
    std::vector<double> xy;                     // 2 n_pos: the table the device holds
    DevBuf<double2> d_xy;
    DevBuf<int2> d_lat;
    DevBuf<int32_t> d_pmap;
    std::vector<double> theta;                  // the headings the device holds
    DevBuf<double> d_theta;
    // the scan
    DevBuf<double2> d_beams;
    HostBuf<double2> h_beams;
    HostBuf<float> h_obs;
    // the scan sequence: the table of SQ1 and where each scan's beams begin (pinned staging beside each)
    DevBuf<double> d_off;
    HostBuf<double> h_off;
    DevBuf<int32_t> d_begin;
    HostBuf<int32_t> h_begin;
    // the volume (d_score: what `volume` says) and the hits
    DevBuf<double> d_score;
    DevBuf<uint64_t> d_key, d_key2;
    DevBuf<uint32_t> d_val, d_val2;
    DevBuf<char> d_tmp;                         // the sort's scratch
    Volume volume;
    DevBuf<unsigned long long> d_count;
    HostBuf<unsigned long long> h_count;
    HostBuf<uint64_t> h_key;                    // kMaxHits each
    HostBuf<uint32_t> h_val;
    size_t device_bytes = 0;
    // the streamed search (§4.16): the plan's buffers; the last slab state and the hits' 64-bit indices on the host
    std::unique_ptr<SlabBufs> slab;
    HostBuf<SlabState> h_state;
    HostBuf<uint64_t> h_idx;                    // kMaxHits
    // the search under the beam model (§4.17): the grid's directions, a tile's ray table and its level-3 list, the scan and its rows
    std::vector<double> bphi;                   // the grid angles the device's directions were made from
    DevBuf<double2> d_bdir;
    HostBuf<double2> h_bdir;
    DevBuf<uint8_t> d_btab;                     // T x M entries of 1 or 2 bytes
    DevBuf<uint32_t> d_blist;
    DevBuf<mcl_sbeam::Header> d_bhdr;
    HostBuf<mcl_sbeam::Header> h_bhdr;
    DevBuf<float> d_bobs, d_lobs;
    BeamTable btab;                             // what d_btab holds: the last tile of the last beam search
    // the search with exact pruning (§4.20)
    std::unique_ptr<PruneBufs> prune;
};

namespace {

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
        SIDE_TRY(s->d_xy.reserve(h, (size_t)s->n_pos, &s->device_bytes));
        SIDE_TRY(s->d_lat.reserve(h, (size_t)s->n_pos, &s->device_bytes));
        SIDE_TRY(s->d_pmap.reserve(h, pmap.size(), &s->device_bytes));
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
    SIDE_TRY(s->d_theta.reserve(h, (size_t)n_head, &s->device_bytes));
    HIPCHK(h, hipMemcpy(s->d_theta, t.data(), (size_t)n_head * sizeof(double), hipMemcpyHostToDevice));
    s->theta.swap(t);
    return MCL_OK;
}

// room for the counts and the hits on the host, and for a scan of B beams
int search_alloc_scan(mcl_engine *h, mcl_search *s, size_t B)
{
    SIDE_TRY(s->d_count.reserve(h, 1, &s->device_bytes));
    SIDE_TRY(s->h_count.reserve(h, 1));
    SIDE_TRY(s->h_key.reserve(h, (size_t)kMaxHits));
    SIDE_TRY(s->h_val.reserve(h, (size_t)kMaxHits));
    SIDE_TRY(s->d_beams.reserve(h, B, &s->device_bytes));
    SIDE_TRY(s->h_beams.reserve(h, B));
    SIDE_TRY(s->h_obs.reserve(h, B));
    return MCL_OK;
}

// room for a volume of n_poses, its sort and a scan of B beams
int search_alloc(mcl_engine *h, mcl_search *s, size_t n_poses, size_t B)
{
    SIDE_TRY(search_alloc_scan(h, s, B));
    if (n_poses > s->d_val2.cap) {               // (d_val2: the last of the five to grow)
        s->volume.n = 0;
        s->d_tmp.drop();                         // the sort's scratch is made again with every volume that grows
    }
    SIDE_TRY(s->d_score.reserve(h, n_poses, &s->device_bytes));
    SIDE_TRY(s->d_key.reserve(h, n_poses, &s->device_bytes));
    SIDE_TRY(s->d_key2.reserve(h, n_poses, &s->device_bytes));
    SIDE_TRY(s->d_val.reserve(h, n_poses, &s->device_bytes));
    SIDE_TRY(s->d_val2.reserve(h, n_poses, &s->device_bytes));
    if (!s->d_tmp.cap) {
        size_t tb = 0;
        HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, s->d_key.p, s->d_key2.p, s->d_val.p, s->d_val2.p, s->d_val2.cap, 0, 64, h->stream));
        SIDE_TRY(s->d_tmp.reserve(h, std::max<size_t>(tb, 16), &s->device_bytes));
    }
    return MCL_OK;
}

// room for the buffers of a plan (ST5): exactly the plan's bytes, when an earlier plan's buffers do not hold it
int search_alloc_slabs(mcl_engine *h, mcl_search *s, const mcl_host::SearchSlabPlan &p)
{
    SIDE_TRY(s->h_state.reserve(h, 1));
    SIDE_TRY(s->h_idx.reserve(h, (size_t)kMaxHits));
    if (s->slab && s->slab->seg && p.ring_bytes <= s->slab->ring.cap * sizeof(double) && p.slab_poses <= s->slab->flag.cap) return MCL_OK;
    s->slab.reset(new SlabBufs());
    SlabBufs &b = *s->slab;
    SIDE_TRY(b.ring.reserve(h, (size_t)(p.ring_bytes / sizeof(double)), &s->device_bytes));
    SIDE_TRY(b.flag.reserve(h, (size_t)p.slab_poses, &s->device_bytes));
    SIDE_TRY(b.pos.reserve(h, (size_t)p.slab_poses, &s->device_bytes));
    SIDE_TRY(b.skey.reserve(h, (size_t)p.slab_poses, &s->device_bytes));
    for (int i = 0; i < 2; ++i) {
        SIDE_TRY(b.ckey[i].reserve(h, (size_t)p.list_entries, &s->device_bytes));
        SIDE_TRY(b.cidx[i].reserve(h, (size_t)p.list_entries, &s->device_bytes));
    }
    SIDE_TRY(b.tmp.reserve(h, (size_t)p.scratch_bytes, &s->device_bytes));
    b.tmp_bytes = ((size_t)p.scratch_bytes - kSlabStateBytes) & ~(size_t)63;
    b.state = reinterpret_cast<SlabState *>(b.tmp.p + b.tmp_bytes);
    b.seg = reinterpret_cast<unsigned long long *>(b.state + 2);
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

// What every search checks before it touches the device: the arguments and the readiness (S8; beam_model: B6, which asks for no
// field).  c receives the config in force.
int search_check(mcl_engine *h, const mcl_search_config_t *cfg, const void *obs, int32_t n_beams, int32_t max_hits,
                 const mcl_search_hit_t *hits, const int64_t *n_hits, mcl_search_config_t &c, bool beam_model = false)
{
    if (cfg) c = *cfg; else mcl_default_search_config(&c);
    if (const char *why = mcl_host::search_invalid(&c)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!obs || !n_hits) return fail(h, MCL_ERR_INVALID_ARG, "global search: obs / n_hits is null");
    if (max_hits < 0 || max_hits > kMaxHits) return fail(h, MCL_ERR_INVALID_ARG, "global search: max_hits must be in [0, 65536]");
    if (max_hits > 0 && !hits) return fail(h, MCL_ERR_INVALID_ARG, "global search: hits is null");
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "global search: no map is set");
    if (h->B <= 0 || h->beam_cs_host.empty()) return fail(h, MCL_ERR_NOT_READY, "global search: no beam angles are set");
    if (!beam_model && (!h->lf_on || h->lf_K < 0 || !h->d_lf_D))
        return fail(h, MCL_ERR_NOT_READY, "global search: the likelihood-field model is off (mcl_set_likelihood_field; the search reads its field and table)");
    if (n_beams != h->B) return fail(h, MCL_ERR_INVALID_ARG, "global search: n_beams does not match the beam angles");
    return MCL_OK;
}

// What the unstreamed searches do before they score: search_check, the lattice and the headings on the device, room for the
// volume and for n_scans scans.  n_poses receives the size of the volume.
int search_prepare(mcl_engine *h, const mcl_search_config_t *cfg, const void *obs, int n_scans, int32_t n_beams, int32_t max_hits,
                   const mcl_search_hit_t *hits, const int64_t *n_hits, mcl_search_config_t &c, int64_t &n_poses)
{
    SIDE_TRY(search_check(h, cfg, obs, n_beams, max_hits, hits, n_hits, c));
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->srch) h->srch = new mcl_search();
    mcl_search *s = h->srch;
    SIDE_TRY(search_lattice_upload(h, s, c.stride_cells));
    if (s->n_pos == 0) return fail(h, MCL_ERR_NOT_READY, "global search: the lattice has no free position on this map");
    n_poses = s->n_pos * (int64_t)c.n_headings;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "global search: n_positions * n_headings must stay below 2^27 (a larger stride_cells or fewer headings)");
    SIDE_TRY(search_headings_upload(h, s, c.n_headings));
    SIDE_TRY(search_alloc(h, s, (size_t)n_poses, (size_t)n_scans * (size_t)h->B));
    s->volume.n = 0;                                             // until this volume is whole
    return MCL_OK;
}

// ---- the streamed search, like search_prepare before anything goes to the stream: what the steps of one call share, its plan,
// its buffers
struct Stream {
    mcl_search_config_t c;
    mcl_host::SearchSlabPlan plan;
    bool single;                                        // mcl_global_search's kernel; a zero rel gives the same bits (SQ7)
    int32_t max_hits;
    SeqArgs q;                                          // a.score: the ring, a.key: the slab's keys
    rocprim::double_buffer<uint64_t> keys, vals;        // the list, twice: the sort flips them
    unsigned list_cap;                                  // entries the sort's one segment may have
    int next;                                           // the next linear heading the ring lacks
    int64_t scored;                                     // headings scored so far
};

// The plan, before anything is allocated or uploaded (ST5): the position count of this lattice, on the host.
int stream_plan(mcl_engine *h, const mcl_search_stream_config_t *scfg, int32_t n_scans, Stream &st)
{
    mcl_search_stream_config_t sc;
    if (scfg) sc = *scfg; else mcl_default_search_stream_config(&sc);
    const mcl_search *s = h->srch;
    int64_t n_pos;
    if (s && s->lattice_epoch == h->map_epoch && s->lattice_stride == st.c.stride_cells) {
        n_pos = s->n_pos;
    } else {
        int nx, ny;
        n_pos = mcl_host::search_lattice(st.c.stride_cells, h->grid_host.data(), h->W, h->H, h->res, h->ox, h->oy, nullptr, nullptr, nullptr,
                                         nullptr, nx, ny);
    }
    if (n_pos == 0) return fail(h, MCL_ERR_NOT_READY, "global search: the lattice has no free position on this map");
    const std::string why = mcl_host::search_slabs(&st.c, &sc, n_pos, n_scans, st.plan);
    if (!why.empty()) return fail(h, MCL_ERR_INVALID_ARG, why);
    return MCL_OK;
}

// The lattice and the headings on the device, room for the scans and the plan's buffers; what the scan and the sort ask for must
// be within the plan's scratch.
int stream_ensure(mcl_engine *h, int32_t n_scans, Stream &st)
{
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->srch) h->srch = new mcl_search();
    mcl_search *s = h->srch;
    SIDE_TRY(search_lattice_upload(h, s, st.c.stride_cells));
    SIDE_TRY(search_headings_upload(h, s, st.c.n_headings));
    SIDE_TRY(search_alloc_scan(h, s, (size_t)n_scans * (size_t)h->B));
    SIDE_TRY(search_alloc_slabs(h, s, st.plan));
    s->volume.n = 0;                                                // ST6: no volume is kept
    const SlabBufs &b = *s->slab;
    const uint64_t slab_cap = (uint64_t)st.plan.G * (uint64_t)s->n_pos;
    st.list_cap = (unsigned)(mcl_host::kSearchListHits + slab_cap);
    st.keys = rocprim::double_buffer<uint64_t>(b.ckey[0], b.ckey[1]);
    st.vals = rocprim::double_buffer<uint64_t>(b.cidx[0], b.cidx[1]);
    if (st.max_hits > 0) {
        size_t scan_b = 0, sort_b = 0;
        HIPCHK(h, rocprim::exclusive_scan(nullptr, scan_b, b.flag.p, b.pos.p, 0u, (size_t)slab_cap, rocprim::plus<uint32_t>(), h->stream));
        HIPCHK(h, rocprim::segmented_radix_sort_pairs(nullptr, sort_b, st.keys, st.vals, st.list_cap, 1u, b.seg, b.seg + 1, 0, 64, h->stream));
        if (std::max(scan_b, sort_b) > b.tmp_bytes)
            return fail(h, MCL_ERR_UNSUPPORTED, "streamed search: the scan or the sort asks for " + std::to_string(std::max(scan_b, sort_b)) +
                                                    " bytes of scratch, the plan has " + std::to_string(b.tmp_bytes));
    }
    return MCL_OK;
}

// SQ3 and SQ1 on their way to the device: every scan's used beams, one list after the other (nb: their number), where each list
// begins, and the table of offsets
int search_stage_sequence(mcl_engine *h, mcl_search *s, const mcl_search_config_t &c, const float *scans, const double *rel, int S, int &nb)
{
    const int B = h->B;
    const size_t n_off = (size_t)c.n_headings * (size_t)S * 3;
    SIDE_TRY(s->d_begin.reserve(h, (size_t)MCL_SEARCH_MAX_SCANS + 1, &s->device_bytes));
    SIDE_TRY(s->h_begin.reserve(h, (size_t)MCL_SEARCH_MAX_SCANS + 1));
    SIDE_TRY(s->d_off.reserve(h, n_off, &s->device_bytes));
    SIDE_TRY(s->h_off.reserve(h, n_off));

    // SQ3: every scan's used beams, one list after the other; SQ1: the table
    nb = 0;
    for (int sc = 0; sc < S; ++sc) {
        s->h_begin[sc] = nb;
        nb += stage_used_beams(h, c.beam_stride, scans + (size_t)sc * (size_t)B, s->h_obs, s->h_beams + nb);
    }
    s->h_begin[S] = nb;
    mcl_host::search_sequence_offsets(c.n_headings, s->theta.data(), rel, S, s->h_off);
    if (nb > 0) HIPCHK(h, hipMemcpyAsync(s->d_beams, s->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_begin, s->h_begin, (size_t)(S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->d_off, s->h_off, n_off * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return MCL_OK;
}

// The scans on their way to the device (nb: the used beams of all of them) and the candidate count reset: the one scan's used
// beams (S3), or search_stage_sequence.
int stage_scans(mcl_engine *h, mcl_search *s, const mcl_search_config_t &c, const float *scans, const double *rel, int S, bool single, int &nb)
{
    if (single) {
        nb = stage_used_beams(h, c.beam_stride, scans, s->h_obs, s->h_beams);
        if (nb > 0) HIPCHK(h, hipMemcpyAsync(s->d_beams, s->h_beams, (size_t)nb * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    } else {
        SIDE_TRY(search_stage_sequence(h, s, c, scans, rel, S, nb));
    }
    HIPCHK(h, hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), h->stream));
    return MCL_OK;
}

// the kernels' arguments of an unstreamed search over the S scans staged by stage_scans: the whole volume in d_score
SeqArgs search_args(const mcl_engine *h, const mcl_search *s, const mcl_search_config_t &c, int nb, int S)
{
    SeqArgs q{};
    Args &a = q.a;
    a.xy = s->d_xy; a.lat = s->d_lat; a.pmap = s->d_pmap; a.theta = s->d_theta;
    a.n_pos = (int32_t)s->n_pos; a.n_head = c.n_headings; a.nx = s->nx; a.ny = s->ny;
    a.blocks_per_heading = (uint32_t)((s->n_pos + kThreads - 1) / kThreads);
    a.beams = s->d_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.K = h->lf_K;
    a.score = s->d_score;
    a.nms = c.nms;
    a.key = s->d_key; a.val = s->d_val; a.count = s->d_count;
    q.off = s->d_off; q.beam_begin = s->d_begin; q.S = S;
    return q;
}

// The only place the score kernels are launched: the `count` linear headings from `first` on, into the planes q.a.ring says.
// single: mcl_global_search's kernel on q.a.  (A launch scores fewer than 2^27 poses, so the grid stays far below 2^31 workgroups.)
int launch_score(mcl_engine *h, SeqArgs &q, bool single, int first, int count)
{
    q.a.head0 = first;
    const dim3 grid((unsigned)((uint64_t)q.a.blocks_per_heading * (uint64_t)count));
    const size_t lds = lf_lds_bytes(h);
    if (single) {
        if (lds) hipLaunchKernelGGL(k_search_score<true>, grid, dim3(kThreads), lds, h->stream, q.a);
        else hipLaunchKernelGGL(k_search_score<false>, grid, dim3(kThreads), 0, h->stream, q.a);
    } else {
        if (lds) hipLaunchKernelGGL(k_search_score_seq<true>, grid, dim3(kThreads), lds, h->stream, q);
        else hipLaunchKernelGGL(k_search_score_seq<false>, grid, dim3(kThreads), 0, h->stream, q);
    }
    HIPCHK(h, hipGetLastError());
    return MCL_OK;
}

// After the host wait: the candidate count and the hits of the first `top` entries of a sorted list (keys in h_key, indices in idx).
template <class Index>
void decode_hits(const mcl_search *s, const Index *idx, int64_t top, mcl_search_hit_t *hits, int64_t *n_hits)
{
    const int64_t found = (int64_t)*s->h_count;
    *n_hits = found;
    const int64_t m = std::min<int64_t>(top, found);
    for (int64_t r = 0; r < m; ++r) {
        const int64_t i = (int64_t)idx[r];
        const int64_t k = i / s->n_pos, p = i - k * s->n_pos;
        hits[r].pose[0] = s->xy[(size_t)2 * p];
        hits[r].pose[1] = s->xy[(size_t)2 * p + 1];
        hits[r].pose[2] = s->theta[(size_t)k];
        hits[r].log_likelihood = key_score(s->h_key[r]);
        hits[r].index = i;
    }
}

// stats[0..3] of every search
void search_stats(uint64_t *stats, const mcl_search *s, int64_t n_poses, int nb)
{
    stats[0] = (uint64_t)s->n_pos; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)s->device_bytes;
}

// What the unstreamed searches do with the volume in d_score (S5): the marking, the sort, the copies, the one host wait, the hits.
int search_finish(mcl_engine *h, mcl_search *s, const Args &a, int64_t n_poses, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits)
{
    hipLaunchKernelGGL(k_search_mark, dim3((unsigned)((n_poses + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    const int64_t top = std::min<int64_t>(max_hits, n_poses);
    if (top > 0) {
        size_t tb = s->d_tmp.cap;
        HIPCHK(h, rocprim::radix_sort_pairs(s->d_tmp.p, tb, s->d_key.p, s->d_key2.p, s->d_val.p, s->d_val2.p, (size_t)n_poses, 0, 64, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_key, s->d_key2, (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_val, s->d_val2, (size_t)top * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(s->h_count, s->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait
    s->volume = {h->map_epoch, n_poses};
    decode_hits(s, s->h_val.p, top, hits, n_hits);
    return MCL_OK;
}

// mcl_global_search (single: its kernel, rel unused) and mcl_global_search_sequence behind their own argument checks
int search_unstreamed(mcl_engine *h, const mcl_search_config_t *cfg, const float *scans, const double *rel, int S, bool single,
                      int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t *stats)
{
    mcl_search_config_t c;
    int64_t n_poses = 0;
    SIDE_TRY(search_prepare(h, cfg, scans, S, n_beams, max_hits, hits, n_hits, c, n_poses));
    mcl_search *s = h->srch;
    int nb = 0;
    SIDE_TRY(stage_scans(h, s, c, scans, rel, S, single, nb));
    SeqArgs q = search_args(h, s, c, nb, S);
    SIDE_TRY(launch_score(h, q, single, 0, c.n_headings));
    SIDE_TRY(search_finish(h, s, q.a, n_poses, max_hits, hits, n_hits));
    if (stats) search_stats(stats, s, n_poses, nb);
    return MCL_OK;
}

// ---- the streamed search on the stream, after stream_plan and stream_ensure
// The slab states and the segment's bounds reset; the kernels' arguments: the search's, with the ring and a slab's keys in the
// volume's place.
int stream_begin(mcl_engine *h, const mcl_search *s, int nb, int32_t n_scans, Stream &st)
{
    const SlabBufs &b = *s->slab;
    HIPCHK(h, hipMemsetAsync(b.state, 0, 2 * sizeof(SlabState), h->stream));
    HIPCHK(h, hipMemsetAsync(b.seg, 0, 2 * sizeof(unsigned long long), h->stream));
    const bool one_slab = st.plan.n_slabs == 1;
    st.q = search_args(h, s, st.c, nb, n_scans);
    st.q.a.score = b.ring; st.q.a.key = b.skey; st.q.a.val = nullptr;
    st.q.a.ring = one_slab ? 0 : st.plan.G + 2;
    st.next = one_slab ? 0 : -1;
    st.scored = 0;
    return MCL_OK;
}

// Slab t, as the header of this file lists it.
int stream_slab(mcl_engine *h, const mcl_search *s, Stream &st, int t)
{
    const SlabBufs &b = *s->slab;
    const int n = st.c.n_headings, G = st.plan.G;
    const bool one_slab = st.plan.n_slabs == 1;
    const int lo = t * G, g = std::min(G, n - lo);
    // k_search_score(_seq): the headings the ring lacks, up to the slab's last and one beyond (n stands for heading 0)
    const int last = one_slab ? n - 1 : std::min(lo + G, n);
    if (st.next <= last) {
        SIDE_TRY(launch_score(h, st.q, st.single, st.next, last - st.next + 1));
        st.scored += last - st.next + 1;
        st.next = last + 1;
    }
    // k_search_mark_slab
    SlabArgs m{};
    m.a = st.q.a;
    m.head_lo = lo; m.g = g; m.wrap = one_slab ? 1 : 0;
    m.max_hits = (uint64_t)st.max_hits;
    m.in = b.state + (t & 1); m.out = b.state + ((t + 1) & 1);
    m.flag = b.flag; m.pos = b.pos;
    m.ckey = st.keys.current(); m.cidx = st.vals.current();
    m.seg = b.seg;
    const uint64_t n_slab = (uint64_t)g * (uint64_t)s->n_pos;
    const dim3 grid((unsigned)((n_slab + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(k_search_mark_slab, grid, dim3(kThreads), 0, h->stream, m);
    HIPCHK(h, hipGetLastError());
    if (st.max_hits == 0) return MCL_OK;
    // exclusive scan of the flags
    size_t tb = b.tmp_bytes;
    HIPCHK(h, rocprim::exclusive_scan(b.tmp.p, tb, b.flag.p, b.pos.p, 0u, (size_t)n_slab, rocprim::plus<uint32_t>(), h->stream));
    // k_search_compact
    hipLaunchKernelGGL(k_search_compact, grid, dim3(kThreads), 0, h->stream, m);
    HIPCHK(h, hipGetLastError());
    // segmented radix sort: the list and the slab's candidates
    tb = b.tmp_bytes;
    HIPCHK(h, rocprim::segmented_radix_sort_pairs(b.tmp.p, tb, st.keys, st.vals, st.list_cap, 1u, b.seg, b.seg + 1, 0, 64, h->stream));
    return MCL_OK;
}

// The counts and the first max_hits pairs of the list; the one host wait; the hits and the stats.
int stream_finish(mcl_engine *h, mcl_search *s, const Stream &st, int nb, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t *stats)
{
    const SlabBufs &b = *s->slab;
    const int64_t n_poses = s->n_pos * (int64_t)st.c.n_headings;
    const int64_t top = std::min<int64_t>(st.max_hits, n_poses);
    if (top > 0) {
        HIPCHK(h, hipMemcpyAsync(s->h_key, st.keys.current(), (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_idx, st.vals.current(), (size_t)top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(s->h_count, s->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(s->h_state, b.state + (st.plan.n_slabs & 1), sizeof(SlabState), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));                   // the one host wait
    decode_hits(s, s->h_idx.p, top, hits, n_hits);
    if (stats) {
        search_stats(stats, s, n_poses, nb);
        stats[4] = (uint64_t)st.plan.G; stats[5] = (uint64_t)st.plan.n_slabs; stats[6] = (uint64_t)st.scored;
        stats[7] = (uint64_t)s->h_state->compacted;
    }
    return MCL_OK;
}

// ---- the search under the beam model (§4.17)
// the directions of the grid angles on the device (formed and uploaded when the grid changed): the host's cos / sin, in double (B2)
int beam_directions_upload(mcl_engine *h, mcl_search *s, const mcl_host::SearchBeamGrid &g)
{
    std::vector<double> phi((size_t)g.M);
    mcl_host::search_beam_angles(g, phi.data());
    if (phi == s->bphi) return MCL_OK;
    s->bphi.clear();
    SIDE_TRY(s->d_bdir.reserve(h, (size_t)g.M, &s->device_bytes));
    SIDE_TRY(s->h_bdir.reserve(h, (size_t)g.M));
    for (int32_t m = 0; m < g.M; ++m) s->h_bdir[m] = make_double2(std::cos(phi[(size_t)m]), std::sin(phi[(size_t)m]));
    // on the engine's stream, from pinned staging: no host wait of its own (the staging is rewritten only by a later call,
    // and every call ends in a host wait)
    HIPCHK(h, hipMemcpyAsync(s->d_bdir, s->h_bdir, (size_t)g.M * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    s->bphi.swap(phi);
    return MCL_OK;
}

// entries of a tile's level-3 list (B2): the share of rays that run along cell edges is near 1 in 180 on a Hokuyo's grid; room
// for 1 in 64, at least 4096, and never more than the tile has rays
size_t beam_list_entries(uint64_t tile_rays)
{
    return (size_t)std::min<uint64_t>(tile_rays, std::max<uint64_t>(4096, tile_rays / 64));
}

template <class E>
int beam_tiles_run(mcl_engine *h, mcl_search *s, mcl_sbeam::Args &a, const mcl_host::SearchBeamTiles &tp)
{
    using namespace mcl_sbeam;
    for (int64_t tile = 0; tile < tp.tiles; ++tile) {
        a.pos0 = (int32_t)(tile * tp.T);
        a.count = (int32_t)std::min<int64_t>(tp.T, s->n_pos - (int64_t)a.pos0);
        a.blocks_per_row = (uint32_t)((a.count + mcl_sbeam::kThreads - 1) / mcl_sbeam::kThreads);
        HIPCHK(h, hipMemsetAsync(&s->d_bhdr.p->listed, 0, sizeof(unsigned long long), h->stream));
        hipLaunchKernelGGL(k_beam_table<E>, dim3((unsigned)((uint64_t)a.blocks_per_row * (uint64_t)a.M)), dim3(mcl_sbeam::kThreads), 0,
                           h->stream, a);
        HIPCHK(h, hipGetLastError());
        // one wave per listed ray, as many as the list can hold
        const unsigned grid_exact = level3_grid(h, (int64_t)std::min<unsigned long long>((unsigned long long)a.count * (unsigned long long)a.M, a.list_cap));
        hipLaunchKernelGGL(k_beam_table_exact<E>, dim3(grid_exact), dim3(mcl_sbeam::kThreads), 0, h->stream, a);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL(k_beam_score<E>, dim3((unsigned)((uint64_t)a.blocks_per_row * (uint64_t)a.n_head)), dim3(mcl_sbeam::kThreads), 0,
                           h->stream, a);
        HIPCHK(h, hipGetLastError());
    }
    return MCL_OK;
}

int search_beam(mcl_engine *h, const mcl_search_config_t *cfg, const float *obs, int32_t n_beams, uint64_t budget, int32_t max_hits,
                mcl_search_hit_t *hits, int64_t *n_hits, uint64_t *stats)
{
    // B6 / B1 / B5: everything that can refuse the call, before anything is allocated for it
    mcl_search_config_t c;
    SIDE_TRY(search_check(h, cfg, obs, n_beams, max_hits, hits, n_hits, c, true));
    SIDE_TRY(beam_model_check(h, "beam search", false));        // (search_check has asked for the map and the beam angles)
    mcl_host::SearchBeamGrid g;
    const std::string why_grid = mcl_host::search_beam_grid(h->angles.data(), h->B, c.n_headings, g);
    if (!why_grid.empty()) return fail(h, MCL_ERR_INVALID_ARG, why_grid);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->srch) h->srch = new mcl_search();
    mcl_search *s = h->srch;
    SIDE_TRY(search_lattice_upload(h, s, c.stride_cells));
    if (s->n_pos == 0) return fail(h, MCL_ERR_NOT_READY, "global search: the lattice has no free position on this map");
    const int64_t n_poses = s->n_pos * (int64_t)c.n_headings;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "global search: n_positions * n_headings must stay below 2^27 (a larger stride_cells or fewer headings)");
    mcl_host::SearchBeamTiles tp;
    const std::string why_tiles = mcl_host::search_beam_tiles(s->n_pos, g.M, h->P, budget, tp);
    if (!why_tiles.empty()) return fail(h, MCL_ERR_INVALID_ARG, why_tiles);

    // the buffers: the volume and its sort as every unstreamed search, then the beam search's own
    const int B = h->B, tw = h->P + 1;
    const int nb = (B + c.beam_stride - 1) / c.beam_stride;
    SIDE_TRY(search_headings_upload(h, s, c.n_headings));
    SIDE_TRY(search_alloc(h, s, (size_t)n_poses, (size_t)B));
    s->volume.n = 0;                                             // until this volume is whole
    s->btab.n = 0;
    SIDE_TRY(beam_directions_upload(h, s, g));
    const uint64_t tile_rays = (uint64_t)tp.T * (uint64_t)g.M;
    SIDE_TRY(s->d_btab.reserve(h, (size_t)(tile_rays * (uint64_t)tp.entry_bytes), &s->device_bytes));
    SIDE_TRY(s->d_blist.reserve(h, beam_list_entries(tile_rays), &s->device_bytes));
    SIDE_TRY(s->d_bhdr.reserve(h, 1, &s->device_bytes));
    SIDE_TRY(s->h_bhdr.reserve(h, 1));
    SIDE_TRY(s->d_bobs.reserve(h, (size_t)B, &s->device_bytes));
    SIDE_TRY(s->d_lobs.reserve(h, (size_t)nb * (size_t)tw, &s->device_bytes));

    // the scan, the counters, the rows
    std::memcpy(s->h_obs, obs, (size_t)B * sizeof(float));
    HIPCHK(h, hipMemcpyAsync(s->d_bobs, s->h_obs, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(s->d_bhdr, 0, sizeof(mcl_sbeam::Header), h->stream));
    mcl_sbeam::Args a{};
    fill_ray_args(h, a.ray);
    a.xy = s->d_xy; a.dir = s->d_bdir;
    a.M = g.M; a.T = (int32_t)tp.T;
    a.tab = s->d_btab;
    a.list = s->d_blist; a.list_cap = (unsigned long long)beam_list_entries(tile_rays);
    a.hdr = s->d_bhdr;
    a.obs = s->d_bobs; a.B = B; a.beam_stride = c.beam_stride; a.nb = nb;
    a.L = h->d_L; a.lobs = s->d_lobs;
    a.n_pos = (int32_t)s->n_pos; a.n_head = c.n_headings; a.heading_step = g.heading_step;
    a.score = s->d_score;
    hipLaunchKernelGGL(mcl_sbeam::k_beam_rows, dim3((unsigned)(((uint64_t)nb * (uint64_t)tw + mcl_sbeam::kThreads - 1) / mcl_sbeam::kThreads)),
                       dim3(mcl_sbeam::kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    if (tp.entry_bytes == 1) SIDE_TRY(beam_tiles_run<uint8_t>(h, s, a, tp));
    else SIDE_TRY(beam_tiles_run<uint16_t>(h, s, a, tp));
    HIPCHK(h, hipMemcpyAsync(s->h_bhdr, s->d_bhdr, sizeof(mcl_sbeam::Header), hipMemcpyDeviceToHost, h->stream));
    const SeqArgs q = search_args(h, s, c, nb, 1);
    SIDE_TRY(search_finish(h, s, q.a, n_poses, max_hits, hits, n_hits));      // (the one host wait)
    s->btab = {h->map_epoch, g.M, tp.entry_bytes, tp.T, (tp.tiles - 1) * tp.T, s->n_pos - (tp.tiles - 1) * tp.T};
    if (stats) {
        search_stats(stats, s, n_poses, nb);
        stats[4] = (uint64_t)g.M; stats[5] = (uint64_t)tp.T; stats[6] = (uint64_t)tp.tiles; stats[7] = (uint64_t)s->h_bhdr->level3;
    }
    return MCL_OK;
}


// ---- the search with exact pruning (§4.20)
// P1 on the device: the block tables of this lattice at this S (formed and uploaded when either changed).  A block's corners are
// S1's cell centres of its first and last lattice column and row, the expressions of search_lattice.
int prune_blocks_upload(mcl_engine *h, mcl_search *s, PruneBufs &pb, int stride, int S)
{
    if (pb.blk_epoch == s->lattice_epoch && pb.blk_stride == stride && pb.blk_S == S) return MCL_OK;
    pb.blk_epoch = 0;
    std::vector<int32_t> pmap((size_t)s->nx * (size_t)s->ny);
    HIPCHK(h, hipMemcpy(pmap.data(), s->d_pmap, pmap.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    mcl_host::search_blocks(S, stride, pmap.data(), s->nx, s->ny, pb.plan);
    const mcl_host::SearchBlocks &b = pb.plan;
    const size_t n = (size_t)b.n_blocks;
    std::vector<double4> corner(n);
    std::vector<int2> blk(n);
    const int64_t h0 = stride / 2;
    for (size_t i = 0; i < n; ++i) {
        const int bx = b.blk[3 * i], by = b.blk[3 * i + 1];
        const int64_t c0 = h0 + (int64_t)bx * S * stride, c1 = h0 + (int64_t)std::min(bx * S + S - 1, s->nx - 1) * stride;
        const int64_t r0 = h0 + (int64_t)by * S * stride, r1 = h0 + (int64_t)std::min(by * S + S - 1, s->ny - 1) * stride;
        corner[i] = make_double4(h->ox + ((double)c0 + 0.5) * h->res, h->oy + ((double)r0 + 0.5) * h->res,
                                 h->ox + ((double)c1 + 0.5) * h->res, h->oy + ((double)r1 + 0.5) * h->res);
        blk[i] = make_int2(bx, by);
    }
    SIDE_TRY(pb.d_corner.reserve(h, n, &pb.bytes));
    SIDE_TRY(pb.d_blk.reserve(h, n, &pb.bytes));
    SIDE_TRY(pb.d_bmap.reserve(h, b.bmap.size(), &pb.bytes));
    HIPCHK(h, hipMemcpy(pb.d_corner, corner.data(), n * sizeof(double4), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(pb.d_blk, blk.data(), n * sizeof(int2), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(pb.d_bmap, b.bmap.data(), b.bmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    pb.blk_epoch = s->lattice_epoch;
    pb.blk_stride = stride;
    pb.blk_S = S;
    return MCL_OK;
}

// P2 on the device: Ub and the pooled field of this map's field at this w (made when any of the three changed)
int prune_pool(mcl_engine *h, PruneBufs &pb, int w)
{
    if (pb.pool_w == w && pb.pool_map == h->map_epoch && pb.pool_lf == h->lf_epoch) return MCL_OK;
    pb.pool_w = 0;
    const int K = h->lf_K;
    std::vector<float> ub((size_t)K + 1);
    mcl_host::search_bound_table(h->lf_tab.data(), K, ub.data());
    const size_t Wp = (size_t)h->W + (size_t)w - 1, Hp = (size_t)h->H + (size_t)w - 1;
    SIDE_TRY(pb.d_ub.reserve(h, ub.size(), &pb.bytes));
    SIDE_TRY(pb.d_R.reserve(h, Wp * (size_t)h->H, &pb.bytes));
    SIDE_TRY(pb.d_Dp.reserve(h, Wp * Hp, &pb.bytes));
    HIPCHK(h, hipMemcpy(pb.d_ub, ub.data(), ub.size() * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(mcl_prune::k_lf_pool_rows, dim3((unsigned)((Wp * (size_t)h->H + 255) / 256)), dim3(256), 0, h->stream, h->d_lf_D.p, h->W,
                       h->H, K, w, pb.d_R.p);
    hipLaunchKernelGGL(mcl_prune::k_lf_pool_cols, dim3((unsigned)((Wp * Hp + 255) / 256)), dim3(256), 0, h->stream, pb.d_R.p, h->W, h->H, K, w,
                       pb.d_Dp.p);
    HIPCHK(h, hipGetLastError());
    pb.pool_map = h->map_epoch;
    pb.pool_lf = h->lf_epoch;
    pb.pool_w = w;
    return MCL_OK;
}

// room in the store and its sort buffers for `want` entries, the first `keep` entries of the store kept
int prune_grow(mcl_engine *h, PruneBufs &pb, size_t keep, size_t want)
{
    if (want > pb.store.cap) {
        DevBuf<double> bigger;
        SIDE_TRY(bigger.reserve(h, want, &pb.bytes));
        if (keep) HIPCHK(h, hipMemcpyAsync(bigger, pb.store, keep * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));                 // before the old store goes
        pb.store = std::move(bigger);
    }
    for (int i = 0; i < 2; ++i) {
        SIDE_TRY(pb.ckey[i].reserve(h, want, &pb.bytes));
        SIDE_TRY(pb.cval[i].reserve(h, want, &pb.bytes));
    }
    return MCL_OK;
}

// adds what a call's own buffers have asked for to the search's byte count, however the call ends
struct PruneBytes {
    mcl_search *s;
    PruneBufs &pb;
    size_t before;
    ~PruneBytes() { s->device_bytes += pb.bytes - before; }
};

// What differs between the pruned searches: how the scans reach the device (stage_scans' `single`) and the two kernels that read
// them.  Everything else -- the checks, the buffers, the order of the bounds, the rounds, the result -- is search_pruned.
struct PruneKernels {
    bool single;                                 // mcl_global_search_pruned: one scan, its kernels read q.a alone
    void (*bound)(mcl_engine *h, const mcl_prune::SeqArgs &q, dim3 grid, size_t lds);
    void (*score)(mcl_engine *h, const mcl_prune::SeqArgs &q, dim3 grid, size_t lds);
};

template <class Kernel, class KernelArgs>
void prune_launch(mcl_engine *h, Kernel with_lds, Kernel without, dim3 grid, size_t lds, const KernelArgs &a)
{
    if (lds) hipLaunchKernelGGL(with_lds, grid, dim3(kThreads), lds, h->stream, a);
    else hipLaunchKernelGGL(without, grid, dim3(kThreads), 0, h->stream, a);
}

const PruneKernels kPruneSingle = {
    true,
    [](mcl_engine *h, const mcl_prune::SeqArgs &q, dim3 grid, size_t lds) {
        prune_launch(h, mcl_prune::k_search_bound<true>, mcl_prune::k_search_bound<false>, grid, lds, q.a);
    },
    [](mcl_engine *h, const mcl_prune::SeqArgs &q, dim3 grid, size_t lds) {
        prune_launch(h, mcl_prune::k_search_score_block<true>, mcl_prune::k_search_score_block<false>, grid, lds, q.a);
    }};
const PruneKernels kPruneSequence = {
    false,
    [](mcl_engine *h, const mcl_prune::SeqArgs &q, dim3 grid, size_t lds) {
        prune_launch(h, mcl_prune::k_search_bound_seq<true>, mcl_prune::k_search_bound_seq<false>, grid, lds, q);
    },
    [](mcl_engine *h, const mcl_prune::SeqArgs &q, dim3 grid, size_t lds) {
        prune_launch(h, mcl_prune::k_search_score_block_seq<true>, mcl_prune::k_search_score_block_seq<false>, grid, lds, q);
    }};

// mcl_global_search_pruned (kPruneSingle: one scan, rel unused) and mcl_global_search_sequence_pruned (kPruneSequence) behind
// their own argument checks
int search_pruned(mcl_engine *h, const PruneKernels &kern, const mcl_search_config_t *cfg, const mcl_search_prune_config_t *pcfg,
                  const float *scans, const double *rel, int n_scans, int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits,
                  int64_t *n_hits, uint64_t *stats)
{
    // P6: everything that can refuse the call, before anything is allocated for it
    mcl_search_config_t c;
    SIDE_TRY(search_check(h, cfg, scans, n_beams, max_hits, hits, n_hits, c));
    if (max_hits == 0) return fail(h, MCL_ERR_INVALID_ARG, "pruned search: max_hits must be >= 1 (with no hit to report the call has nothing to do)");
    mcl_search_prune_config_t pc;
    if (pcfg) pc = *pcfg; else mcl_default_search_prune_config(&pc);
    if (const char *why = mcl_host::search_prune_invalid(&c, &pc)) return fail(h, MCL_ERR_INVALID_ARG, why);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->srch) h->srch = new mcl_search();
    mcl_search *s = h->srch;
    SIDE_TRY(search_lattice_upload(h, s, c.stride_cells));
    if (s->n_pos == 0) return fail(h, MCL_ERR_NOT_READY, "global search: the lattice has no free position on this map");
    const int64_t n_poses = s->n_pos * (int64_t)c.n_headings;
    if (n_poses >= MCL_MAX_TOTAL_PARTICLES)
        return fail(h, MCL_ERR_INVALID_ARG, "global search: n_positions * n_headings must stay below 2^27 (a larger stride_cells or fewer headings)");
    SIDE_TRY(search_headings_upload(h, s, c.n_headings));
    SIDE_TRY(search_alloc_scan(h, s, (size_t)n_scans * (size_t)h->B));
    if (!s->prune) s->prune.reset(new PruneBufs());
    PruneBufs &pb = *s->prune;
    const PruneBytes count_bytes{s, pb, pb.bytes};
    pb.bounds.n = 0;                                             // until this call's bounds are whole
    const int S = pc.block;
    const uint64_t SS = (uint64_t)(S * S);
    SIDE_TRY(prune_blocks_upload(h, s, pb, c.stride_cells, S));
    const int64_t n_pairs = (int64_t)pb.plan.n_blocks * (int64_t)c.n_headings;
    if ((uint64_t)n_pairs * SS >= (1ull << 31))
        return fail(h, MCL_ERR_INVALID_ARG, "pruned search: pairs * block * block must stay below 2^31 (a smaller block, a larger stride_cells or fewer headings)");
    SIDE_TRY(prune_pool(h, pb, pb.plan.w));
    SIDE_TRY(pb.d_U.reserve(h, (size_t)n_pairs, &pb.bytes));
    for (int i = 0; i < 2; ++i) {
        SIDE_TRY(pb.d_ukey[i].reserve(h, (size_t)n_pairs, &pb.bytes));
        SIDE_TRY(pb.d_upair[i].reserve(h, (size_t)n_pairs, &pb.bytes));
    }
    SIDE_TRY(pb.d_rank.reserve(h, (size_t)n_pairs, &pb.bytes));
    SIDE_TRY(pb.d_guard.reserve(h, 1, &pb.bytes));
    SIDE_TRY(pb.h_guard.reserve(h, 1));
    SIDE_TRY(pb.d_round.reserve(h, 1, &pb.bytes));
    SIDE_TRY(pb.h_round.reserve(h, 1));

    // the scans; the bounds, their order, the slot map
    int nb = 0;
    SIDE_TRY(stage_scans(h, s, c, scans, rel, n_scans, kern.single, nb));
    HIPCHK(h, hipMemsetAsync(pb.d_guard, 0, sizeof(unsigned long long), h->stream));
    mcl_prune::SeqArgs q{};
    q.off = s->d_off; q.beam_begin = s->d_begin; q.n_scans = n_scans;
    mcl_prune::Args &a = q.a;
    a.xy = s->d_xy; a.pmap = s->d_pmap; a.theta = s->d_theta;
    a.n_pos = (int32_t)s->n_pos; a.n_head = c.n_headings; a.nx = s->nx; a.ny = s->ny;
    a.S = S; a.n_blocks = pb.plan.n_blocks; a.nbx = pb.plan.nbx;
    a.n_pairs = (uint32_t)n_pairs;
    a.groups_per_heading = (uint32_t)((pb.plan.n_blocks + kThreads - 1) / kThreads);
    a.corner = pb.d_corner; a.blk = pb.d_blk; a.bmap = pb.d_bmap;
    a.beams = s->d_beams; a.nb = nb;
    a.D = h->d_lf_D; a.W = h->W; a.H = h->H;
    a.ox = h->ox; a.oy = h->oy; a.inv_res = 1.0 / h->res;
    a.lf = h->d_lf_tab; a.ub = pb.d_ub; a.K = h->lf_K;
    a.Dp = pb.d_Dp; a.w = pb.plan.w;
    a.U = pb.d_U; a.ukey = pb.d_ukey[0]; a.upair = pb.d_upair[0];
    a.ukey_sorted = pb.d_ukey[1]; a.pair_sorted = pb.d_upair[1]; a.rank = pb.d_rank;
    a.guard = pb.d_guard;
    a.nms = c.nms;
    a.count = s->d_count;
    a.max_hits = (uint32_t)max_hits;
    a.round = pb.d_round;
    const size_t lds = lf_lds_bytes(h);
    const dim3 grid_bound((unsigned)((uint64_t)a.groups_per_heading * (uint64_t)c.n_headings));
    kern.bound(h, q, grid_bound, lds);
    HIPCHK(h, hipGetLastError());
    size_t tb = 0;
    HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb, pb.d_ukey[0].p, pb.d_ukey[1].p, pb.d_upair[0].p, pb.d_upair[1].p, (size_t)n_pairs, 0, 64, h->stream));
    SIDE_TRY(pb.tmp.reserve(h, std::max<size_t>(tb, 16), &pb.bytes));
    tb = pb.tmp.cap;
    HIPCHK(h, rocprim::radix_sort_pairs(pb.tmp.p, tb, pb.d_ukey[0].p, pb.d_ukey[1].p, pb.d_upair[0].p, pb.d_upair[1].p, (size_t)n_pairs, 0, 64, h->stream));
    hipLaunchKernelGGL(mcl_prune::k_search_rank, dim3((unsigned)((n_pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(pb.h_guard, pb.d_guard, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));

    // P4: the rounds
    unsigned index_bits = 1;
    while (((int64_t)1 << index_bits) < n_poses) ++index_bits;
    int64_t n_scored = 0, next = mcl_host::search_prune_next(pc, n_pairs, 0, 0), rounds = 0;
    size_t top = 0;
    for (;;) {
        const size_t entries = (size_t)((uint64_t)next * SS);
        SIDE_TRY(prune_grow(h, pb, (size_t)((uint64_t)n_scored * SS), entries));
        size_t tb1 = 0, tb2 = 0;
        HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb1, pb.cval[0].p, pb.cval[1].p, pb.ckey[0].p, pb.ckey[1].p, entries, 0, index_bits, h->stream));
        HIPCHK(h, rocprim::radix_sort_pairs(nullptr, tb2, pb.ckey[1].p, pb.ckey[0].p, pb.cval[1].p, pb.cval[0].p, entries, 0, 64, h->stream));
        SIDE_TRY(pb.tmp.reserve(h, std::max(tb1, tb2), &pb.bytes));
        a.store = pb.store; a.ckey = pb.ckey[0]; a.cval = pb.cval[0];
        a.r0 = (uint32_t)n_scored; a.r1 = (uint32_t)next; a.n_scored = (uint32_t)next;
        const dim3 grid_score((unsigned)((next - n_scored + kThreads / 64 - 1) / (kThreads / 64)));
        kern.score(h, q, grid_score, lds);
        HIPCHK(h, hipGetLastError());
        n_scored = next;
        ++rounds;
        HIPCHK(h, hipMemsetAsync(s->d_count, 0, sizeof(unsigned long long), h->stream));
        hipLaunchKernelGGL(mcl_prune::k_search_mark_block, dim3((unsigned)((entries + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, a);
        HIPCHK(h, hipGetLastError());
        // the entries by index, then stably by key: the candidates first, best first, ties by index (S5)
        tb = pb.tmp.cap;
        HIPCHK(h, rocprim::radix_sort_pairs(pb.tmp.p, tb, pb.cval[0].p, pb.cval[1].p, pb.ckey[0].p, pb.ckey[1].p, entries, 0, index_bits, h->stream));
        tb = pb.tmp.cap;
        HIPCHK(h, rocprim::radix_sort_pairs(pb.tmp.p, tb, pb.ckey[1].p, pb.ckey[0].p, pb.cval[1].p, pb.cval[0].p, entries, 0, 64, h->stream));
        hipLaunchKernelGGL(mcl_prune::k_search_decide, dim3(1), dim3(64), 0, h->stream, a);
        HIPCHK(h, hipGetLastError());
        top = std::min<size_t>((size_t)max_hits, entries);
        HIPCHK(h, hipMemcpyAsync(s->h_key, pb.ckey[0], top * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_val, pb.cval[0], top * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(s->h_count, s->d_count, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(pb.h_round, pb.d_round, sizeof(mcl_prune::Round), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));               // the round's one host wait
        if (pb.h_round->stop) break;
        next = mcl_host::search_prune_next(pc, n_pairs, n_scored, (int64_t)pb.h_round->next);
    }
    pb.bounds = {h->map_epoch, n_pairs};
    // P5: the first min(max_hits, candidates) entries; a stop with pairs left unscored has at least max_hits of them
    const int64_t m = std::min<int64_t>((int64_t)top, (int64_t)*s->h_count);
    for (int64_t r = 0; r < m; ++r) {
        const int64_t i = (int64_t)s->h_val[r];
        const int64_t k = i / s->n_pos, p = i - k * s->n_pos;
        hits[r].pose[0] = s->xy[(size_t)2 * p];
        hits[r].pose[1] = s->xy[(size_t)2 * p + 1];
        hits[r].pose[2] = s->theta[(size_t)k];
        hits[r].log_likelihood = key_score(s->h_key[r]);
        hits[r].index = i;
    }
    *n_hits = m;
    if (stats) {
        stats[0] = (uint64_t)s->n_pos; stats[1] = (uint64_t)n_poses; stats[2] = (uint64_t)nb; stats[3] = (uint64_t)pb.bytes;
        stats[4] = (uint64_t)n_pairs; stats[5] = (uint64_t)n_scored; stats[6] = (uint64_t)rounds; stats[7] = (uint64_t)*pb.h_guard;
    }
    return MCL_OK;
}

}  // namespace

void search_free(struct mcl_search *s) { delete s; }

extern "C" {

int mcl_global_search(mcl_engine_t *h, const mcl_search_config_t *cfg, const float *obs, int32_t n_beams, int32_t max_hits,
                      mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[4])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    return search_unstreamed(h, cfg, obs, nullptr, 1, true, n_beams, max_hits, hits, n_hits, stats);
}

int mcl_global_search_sequence(mcl_engine_t *h, const mcl_search_config_t *cfg, const float *scans, const double *rel, int32_t n_scans,
                               int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[5])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    // the sequence's own arguments, then everything the single search checks
    if (const char *why = mcl_host::search_sequence_invalid(rel, n_scans)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!scans) return fail(h, MCL_ERR_INVALID_ARG, "global search: scans is null");
    SIDE_TRY(search_unstreamed(h, cfg, scans, rel, n_scans, false, n_beams, max_hits, hits, n_hits, stats));
    if (stats) stats[4] = (uint64_t)n_scans;
    return MCL_OK;
}

int mcl_global_search_streamed(mcl_engine_t *h, const mcl_search_config_t *cfg, const mcl_search_stream_config_t *scfg, const float *scans,
                               const double *rel, int32_t n_scans, int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits,
                               int64_t *n_hits, uint64_t stats[8])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    static const double kZeroRel[3] = {0.0, 0.0, 0.0};
    Stream st{};
    st.single = n_scans == 1 && !rel;
    st.max_hits = max_hits;
    if (const char *why = mcl_host::search_sequence_invalid(st.single ? kZeroRel : rel, n_scans)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!scans) return fail(h, MCL_ERR_INVALID_ARG, "global search: scans is null");
    SIDE_TRY(search_check(h, cfg, scans, n_beams, max_hits, hits, n_hits, st.c));
    SIDE_TRY(stream_plan(h, scfg, n_scans, st));
    SIDE_TRY(stream_ensure(h, n_scans, st));
    mcl_search *s = h->srch;
    int nb = 0;
    SIDE_TRY(stage_scans(h, s, st.c, scans, rel, n_scans, st.single, nb));
    SIDE_TRY(stream_begin(h, s, nb, n_scans, st));
    for (int t = 0; t < st.plan.n_slabs; ++t) SIDE_TRY(stream_slab(h, s, st, t));
    return stream_finish(h, s, st, nb, hits, n_hits, stats);
}

int mcl_global_search_beam(mcl_engine_t *h, const mcl_search_config_t *cfg, const float *obs, int32_t n_beams, uint64_t table_budget_bytes,
                           int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[8])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    return search_beam(h, cfg, obs, n_beams, table_budget_bytes, max_hits, hits, n_hits, stats);
}

int mcl_get_search_beam_table(mcl_engine_t *h, uint16_t *out, size_t n, int64_t *first_position, int64_t *n_positions)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    const mcl_search *s = h->srch;
    if (!s || s->btab.n == 0 || s->btab.epoch != h->map_epoch || !h->have_map)
        return fail(h, MCL_ERR_NOT_READY, "no ray table: no beam search has run on this map");
    const BeamTable &b = s->btab;
    if (first_position) *first_position = b.first;
    if (n_positions) *n_positions = b.n;
    if (!out && n == 0) return MCL_OK;                                  // the shape alone
    if (!out || n != (size_t)b.n * (size_t)b.M) return fail(h, MCL_ERR_INVALID_ARG, "the last tile's table has n_positions x M entries");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // the tile's first b.n columns of every angle's row, then position-major and widened on the host
    const size_t e = (size_t)b.entry_bytes, row = (size_t)b.n * e;
    std::vector<uint8_t> raw(row * (size_t)b.M);
    HIPCHK(h, hipMemcpy2DAsync(raw.data(), row, s->d_btab.p, (size_t)b.T * e, row, (size_t)b.M, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int64_t t = 0; t < b.n; ++t)
        for (int32_t m = 0; m < b.M; ++m) {
            const size_t i = (size_t)m * (size_t)b.n + (size_t)t;
            uint16_t v;
            if (e == 1) v = raw[i];
            else std::memcpy(&v, &raw[2 * i], sizeof v);
            out[(size_t)t * (size_t)b.M + (size_t)m] = v;
        }
    return MCL_OK;
}

int mcl_global_search_pruned(mcl_engine_t *h, const mcl_search_config_t *cfg, const mcl_search_prune_config_t *pcfg, const float *obs,
                             int32_t n_beams, int32_t max_hits, mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[8])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    return search_pruned(h, kPruneSingle, cfg, pcfg, obs, nullptr, 1, n_beams, max_hits, hits, n_hits, stats);
}

int mcl_global_search_sequence_pruned(mcl_engine_t *h, const mcl_search_config_t *cfg, const mcl_search_prune_config_t *pcfg,
                                      const float *scans, const double *rel, int32_t n_scans, int32_t n_beams, int32_t max_hits,
                                      mcl_search_hit_t *hits, int64_t *n_hits, uint64_t stats[9])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    // the sequence's own arguments, where the call works (PS5), then everything the pruned search checks
    if (const char *why = mcl_host::search_sequence_invalid(rel, n_scans)) return fail(h, MCL_ERR_INVALID_ARG, why);
    if (!scans) return fail(h, MCL_ERR_INVALID_ARG, "global search: scans is null");
    if (h->comm || h->in_group)
        return fail(h, MCL_ERR_UNSUPPORTED, "pruned sequence search: single-engine only: this engine has a communicator or belongs to a device group");
    SIDE_TRY(search_pruned(h, kPruneSequence, cfg, pcfg, scans, rel, n_scans, n_beams, max_hits, hits, n_hits, stats));
    if (stats) stats[8] = (uint64_t)n_scans;
    return MCL_OK;
}

int mcl_get_search_bounds(mcl_engine_t *h, double *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    const PruneBufs *pb = h->srch ? h->srch->prune.get() : nullptr;
    return read_volume(h, pb ? &pb->bounds : nullptr, pb ? pb->d_U.p : nullptr, out, n, "no bounds: no pruned search has run on this map",
                       "the bounds have n_headings x n_blocks entries");
}

int mcl_get_search_scores(mcl_engine_t *h, double *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    const mcl_search *s = h->srch;
    return read_volume(h, s ? &s->volume : nullptr, s ? s->d_score.p : nullptr, out, n, "no score volume: no global search has run on this map",
                       "the volume has n_headings x n_positions entries");
}

int mcl_get_search_bytes(const mcl_engine_t *h, uint64_t *bytes)
{
    if (!h || !bytes) return MCL_ERR_INVALID_ARG;
    *bytes = h->srch ? (uint64_t)h->srch->device_bytes : 0;
    return MCL_OK;
}

}  // extern "C"
