// mcl_host_math.h -- the host arithmetic of the engine (mcl_host_math.hip): plain functions that neither call HIP nor touch a mcl_engine.
// It builds the tables, fields and per-update scalars; the ABI's mcl_host_* entry points (same unit) expose them to the tests bit for bit.
#pragma once
#include "../../include/mcl_hip_engine.h"
#include <cstdint>
#include <string>
#include <vector>
#include "mcl_types.h"

// An entry of a compact list as the shards exchange it (mcl_export_compact): [ccdf: 8 | crec: 32 | cidx: 4] bytes,
// stored column by column in a chunk of chunk_entries entries (the ccdf column, then the crec column, then the cidx column)
constexpr int kCompactEntryBytes = 44;

namespace mcl_host {
const char *bad_sensor_fields(const mcl_config_t &c);
void build_sensor_table(const mcl_config_t &c, int P, std::vector<double> &t);
void build_distance_field(const int8_t *grid, int W, int H, int Wp, int Hp, int Wps, std::vector<uint8_t> &dist);
void build_directional_field(const int8_t *grid, int W, int H, int Wp, int Hp, int Wps, int sx, int sy, std::vector<uint8_t> &dist);
// The windows of a map patch (mcl_update_map_region), inclusive, x1 < x0: none.  From the box of the grid cells
// whose stop bit changed: `win` the isotropic field's (padded cells; the union of the others), quad[q] the window of quadrant field
// q and of the wedge fields of that quadrant, lf the likelihood field's (grid cells; lf_reach <= 0: none).  The box is clipped to
// the map; false when it is inverted or has no cell inside.
constexpr int kMapPatchReach = 254;      // a stop cell further away than this, per axis, changes no skip value (the cap is 255)
struct MapPatchPlan { int32_t win[4], quad[4][4], lf[4]; };
bool map_patch_plan(int W, int H, const int32_t stop_bbox[4], int lf_reach, MapPatchPlan &p);
void motion_scalars(const double action[3], double &dt, double &v, double &w);
uint32_t systematic_offset(uint32_t seed_lo, uint32_t seed_hi, uint32_t update_idx);
const char *kld_invalid(const mcl_kld_config_t *k, int64_t cap);
bool kld_grid(const mcl_kld_config_t *k, uint32_t W, uint32_t H, float res, int64_t &nx, int64_t &ny, uint64_t &bits);
mcl::KldArgs kld_args_of(const mcl_kld_config_t *k, int64_t nx, int64_t ny, double ox, double oy);
int64_t kld_target(const mcl_kld_config_t *k, int64_t bins, int64_t n_current);
// the chunk of a list exchange (device group, communicator): room for the longest list in whole groups of 64 entries, at least one
int64_t compact_chunk_entries(int64_t longest);
const char *recov_invalid(const mcl_recovery_config_t *c);
double recov_likelihood(const mcl_recovery_config_t &c, double max_logw, double sum_w, double denom, int n_beams);
void recov_fold(const mcl_recovery_config_t &c, double &S, double &F, double l);
double recov_p(double S, double F);
uint64_t recov_threshold(double p);
// the proposal of an injecting update (P1 / P2): thresholds (M words) and factors (9 doubles per component), either may be null;
// empty when the arguments are fine, else why not (the component named)
constexpr int32_t kRecovProposalMax = 4096;
std::string recov_proposal(int32_t M, const double *means, const double *covs, const double *weights, uint64_t *thresholds, double *factors);
const char *lf_invalid(const mcl_likelihood_field_config_t *c);
int lf_cap(const mcl_likelihood_field_config_t *c, float resolution);
void lf_table(const mcl_config_t &cfg, const mcl_likelihood_field_config_t &c, double res, int K, std::vector<float> &t);
// beam skipping: BS1's Ka (held at 65536), BS3's min_count, BS4's min_skipped
const char *bs_invalid(const mcl_beam_skip_config_t *c);
int bs_ka(const mcl_beam_skip_config_t *c, float resolution);
int64_t bs_min_count(double threshold, int64_t n);
int32_t bs_min_skipped(double error_threshold, int32_t n_used);
// sensor mount: SM1's validity -- every component finite, |mtheta| <= 2 pi
bool mount_valid(const double mount[3]);
// per-beam sensor offsets.  DS1: a'_j = (float)((double)a_j + dtheta_j) and its direction pair, formed of that
// float as mcl_set_beam_angles forms a beam's.  DS5: the likelihood field's pair of a used beam of range r.  The device block of a
// table of B beams, in doubles: [B pairs | 3 B table | B float angles].
void deskew_table(const float *angles, const double *offsets_colmajor, int32_t n_beams, float *effective_angles, double2 *cs);
inline double2 deskew_pair(double r, double ox, double oy, double2 cs, double inv_res) { return make_double2((ox + r * cs.x) * inv_res, (oy + r * cs.y) * inv_res); }
inline size_t deskew_block_words(size_t B) { return 5 * B + (B + 1) / 2; }
const char *motion_invalid(const mcl_motion_config_t *c);
const char *gaussian_factor(const double cov[9], double L[6]);
const char *search_invalid(const mcl_search_config_t *c);
// the lattice of a global search over a map (S1): positions in row-major order of (iy, ix).  Any output may be null: cells (the
// position's linear map cell), xy (2 per position), lat (ix, iy per position), pmap (ny x nx: position or -1).  Returns the count.
int64_t search_lattice(int stride, const int8_t *data, int W, int H, double res, double ox, double oy, std::vector<uint32_t> *cells,
                       std::vector<double> *xy, std::vector<int32_t> *lat, std::vector<int32_t> *pmap, int &nx, int &ny);
void search_headings(int n_headings, double *theta);
// SQ1: the table of a sequence search, off[(k * S + s) * 3 + {0, 1, 2}] = {ax_ks, ay_ks, theta_ks}; null when rel is fine, else why not
const char *search_sequence_invalid(const double *rel, int n_scans);
void search_sequence_offsets(int n_headings, const double *theta, const double *rel, int n_scans, double *out);
// The plan of a streamed search (ST2 / ST4 / ST5): the bytes of every buffer whose size depends on G, part by part, and the plan
// itself.  search_slabs returns an empty string and fills `plan`, or says why the call is refused.
struct SearchSlabPlan {
    int32_t G = 0, n_slabs = 0;
    uint64_t slab_poses = 0;            // G * n_positions
    uint64_t ring_bytes = 0, flag_bytes = 0, pos_bytes = 0, key_bytes = 0, list_entries = 0, list_bytes = 0, scratch_bytes = 0, bytes = 0;
};
constexpr uint64_t kSearchStreamDefaultBudget = 1ull << 30;
constexpr uint64_t kSearchListHits = 65536;             // the running list is sized for the largest max_hits
SearchSlabPlan search_slab_bytes(int64_t n_positions, int32_t G);
std::string search_slabs(const mcl_search_config_t *c, const mcl_search_stream_config_t *sc, int64_t n_positions, int32_t n_scans,
                         SearchSlabPlan &plan);
// The search under the beam model (mcl_global_search_beam).  B1: the angle grid of a scan and a heading count
// (phi_m = phi0 + m delta); search_beam_grid returns an empty string and fills `g`, or says which condition failed (max_dev is
// filled whenever M could be formed).  B5: the tiles of a table of n_positions x M entries in a budget (0: the default).
struct SearchBeamGrid {
    int32_t M = 0, heading_step = 0;
    double delta = 0.0, max_dev = 0.0, phi0 = 0.0;
};
std::string search_beam_grid(const float *angles, int n_beams, int n_headings, SearchBeamGrid &g);
void search_beam_angles(const SearchBeamGrid &g, double *phi);          // g.M entries
struct SearchBeamTiles {
    int64_t T = 0, tiles = 0;               // positions per tile (a multiple of 256), tiles
    int32_t entry_bytes = 0;                // 1: MAX_RANGE_PX <= 255, else 2
};
constexpr uint64_t kSearchBeamDefaultBudget = 256ull << 20;
std::string search_beam_tiles(int64_t n_positions, int32_t M, int32_t max_range_px, uint64_t budget_bytes, SearchBeamTiles &t);
// The search with exact pruning (mcl_global_search_pruned).  P1: the live blocks of a lattice (its pmap, ny x nx)
// in row-major order of (by, bx); P2: w, the pooled field and the bound table; P4: the round schedule.
struct SearchBlocks {
    int32_t S = 0, w = 0, nbx = 0, nby = 0, n_blocks = 0;
    std::vector<int32_t> blk;               // 3 per live block: bx, by, positions in it
    std::vector<int32_t> bmap;              // nby x nbx: (by, bx) -> live block, -1: none
};
const char *search_prune_invalid(const mcl_search_config_t *c, const mcl_search_prune_config_t *pc);
void search_blocks(int S, int stride, const int32_t *pmap, int nx, int ny, SearchBlocks &out);
void lf_pool(const uint16_t *D, int W, int H, int K, int w, uint16_t *out);             // (H + w - 1) x (W + w - 1)
void search_bound_table(const float *lf, int K, float *ub);                             // K + 1 entries
int64_t search_prune_next(const mcl_search_prune_config_t &pc, int64_t pairs, int64_t n_scored, int64_t first_below_c);
const char *refine_invalid(const mcl_refine_config_t *c);
// The refinement over a scan sequence (mcl_refine_poses_sequence).  What RS7 refuses of rel and of the table's
// size (M seeds x nt window headings x S scans rows against MCL_REFINE_SEQ_MAX_ROWS): null / empty when fine, else why not.
// RS1: the table off[((m * nt + it) * S + s) * 3 + {0, 1, 2}] = {ax, ay, theta_s} of M column-major seeds.
const char *refine_sequence_invalid(const double *rel, int n_scans);
std::string refine_sequence_rows_refused(int64_t M, int64_t nt, int64_t S);
void refine_sequence_offsets(int32_t half_theta, double step_theta, const double *seeds_colmajor, int32_t M, const double *rel, int n_scans,
                             double *out);
}  // namespace mcl_host
