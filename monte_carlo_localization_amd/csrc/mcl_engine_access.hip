// mcl_engine_access.hip -- the engine's entry points that launch no kernel and plan no launch: the getters that copy device state back
// (read_back, mcl_engine_internal.h) or report host state, the setters that only validate, allocate, clear or store an option.  No
// header with a non-static __global__ is included.  What launches, asks choose_ray_mode or belongs to the staged flow: mcl_engine.hip.
#include "mcl_engine_internal.h"
#include "mcl_wedge.h"
#include "mcl_compact_guide.h"
#include <cstring>

using namespace mcl_host;

int mcl_get_max_range_px(const mcl_engine_t *h, int32_t *out)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (!h->have_map) return MCL_ERR_NOT_READY;
    *out = h->P;
    return MCL_OK;
}

int mcl_get_sensor_table(const mcl_engine_t *h, double *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (!h->have_map) return MCL_ERR_NOT_READY;
    if (n != h->table.size()) return MCL_ERR_INVALID_ARG;
    std::memcpy(out, h->table.data(), n * sizeof(double));
    return MCL_OK;
}

int mcl_get_particles(mcl_engine_t *h, double *xyz, int64_t n)
{
    if (!h || !xyz) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    if (n != h->N) return fail(h, MCL_ERR_INVALID_ARG, "n != active particle count");
    const size_t nb = (size_t)n * sizeof(double);
    return read_back(h, {{xyz, h->d_x[h->cur], nb}, {xyz + n, h->d_y[h->cur], nb}, {xyz + 2 * n, h->d_th[h->cur], nb}});
}

int mcl_expected_pose(mcl_engine_t *h, double out[3])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    const double s = h->global_sums[0];
    // cpp:704-713 sums w_i*x_i with normalised w_i; here the division by sum(w) comes last
    double k = (s > 0.0) ? 1.0 / s : 1.0;
    out[0] = h->global_sums[1] * k;
    out[1] = h->global_sums[2] * k;
    out[2] = std::atan2(h->global_sums[3] * k, h->global_sums[4] * k);
    return MCL_OK;
}

int mcl_get_stage_timings(const mcl_engine_t *h, double ms[6])
{
    if (!h || !ms) return MCL_ERR_INVALID_ARG;
    std::memcpy(ms, h->timings, sizeof(h->timings));
    return MCL_OK;
}

int mcl_get_resample_indices(mcl_engine_t *h, int32_t *idx, int64_t n)
{
    if (!h || !idx) return MCL_ERR_INVALID_ARG;
    if (!h->have_idx) return MCL_ERR_NOT_READY;
    if (n != h->N) return MCL_ERR_INVALID_ARG;
    return read_back(h, {{idx, h->d_idx, (size_t)n * 4}});
}

static int lf_refuse_rays(const mcl_engine_t *h)
{
    if (!h->last_lf) return MCL_OK;
    return fail(const_cast<mcl_engine_t *>(h), MCL_ERR_UNSUPPORTED, "the last update used the likelihood field (mcl_set_likelihood_field): it cast no rays");
}

int mcl_get_ray_steps(mcl_engine_t *h, uint8_t *steps, size_t n)
{
    if (!h || !steps) return MCL_ERR_INVALID_ARG;
    if (const int rc = lf_refuse_rays(h)) return rc;
    if (!h->cfg.keep_ray_steps) return fail(h, MCL_ERR_UNSUPPORTED, "engine created without keep_ray_steps");
    if (h->P > 255) return fail(h, MCL_ERR_UNSUPPORTED, "MAX_RANGE_PX > 255: step indices do not fit bytes, use mcl_get_ray_steps16");
    if (!h->have_steps) return MCL_ERR_NOT_READY;
    if (n != (size_t)h->N * h->B) return MCL_ERR_INVALID_ARG;
    return read_back(h, {{steps, h->d_steps, n}});
}

int mcl_get_ray_steps16(mcl_engine_t *h, uint16_t *steps, size_t n)
{
    if (!h || !steps) return MCL_ERR_INVALID_ARG;
    if (const int rc = lf_refuse_rays(h)) return rc;
    if (!h->cfg.keep_ray_steps) return fail(h, MCL_ERR_UNSUPPORTED, "engine created without keep_ray_steps");
    if (!h->have_steps) return MCL_ERR_NOT_READY;
    if (n != (size_t)h->N * h->B) return MCL_ERR_INVALID_ARG;
    if (h->P > 255) return read_back(h, {{steps, h->d_steps, n * 2}});
    std::vector<uint8_t> b(n);
    MCL_TRY(read_back(h, {{b.data(), h->d_steps, n}}));
    for (size_t k = 0; k < n; ++k) steps[k] = b[k];
    return MCL_OK;
}

int mcl_get_log_weights(mcl_engine_t *h, double *logw, int64_t n)
{
    if (!h || !logw) return MCL_ERR_INVALID_ARG;
    if (!h->have_logw) return MCL_ERR_NOT_READY;
    if (n != h->N) return MCL_ERR_INVALID_ARG;
    return read_back(h, {{logw, h->d_logw, (size_t)n * 8}});
}

int mcl_get_counters(mcl_engine_t *h, uint64_t out[4])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = h->h_counters[i];
    return MCL_OK;
}

int mcl_get_compact_list(const mcl_engine_t *h, int64_t *n_entries, int32_t *used_by_last_update)
{
    if (!h || !n_entries || !used_by_last_update) return MCL_ERR_INVALID_ARG;
    *n_entries = h->compact_n;
    *used_by_last_update = h->compact_used ? 1 : 0;
    return MCL_OK;
}

int mcl_set_debug_count_probes(mcl_engine_t *h, int32_t on)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    graph_reset(h);                        // a captured tail holds the non-counting kernel
    h->cfg.debug_count_probes = on ? 1 : 0;
    return MCL_OK;
}

int mcl_set_debug_force_exact(mcl_engine_t *h, int32_t level)
{
    if (!h || level < 0 || level > 2) return MCL_ERR_INVALID_ARG;
    graph_reset(h);                        // (RayArgs::force_exact is an argument of the captured kernels)
    h->cfg.debug_force_exact = level;
    return MCL_OK;
}

int mcl_get_ray_kernel_ms(const mcl_engine_t *h, double *ms)
{
    if (!h || !ms) return MCL_ERR_INVALID_ARG;
    *ms = h->ray_ms;
    return MCL_OK;
}

int mcl_get_ray_kernel_id(const mcl_engine_t *h, int32_t *kernel)
{
    if (!h || !kernel) return MCL_ERR_INVALID_ARG;
    if (const int rc = lf_refuse_rays(h)) return rc;
    *kernel = h->last_mode;
    return MCL_OK;
}

int mcl_get_ray_kernel_variant(const mcl_engine_t *h, int32_t out[3])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (const int rc = lf_refuse_rays(h)) return rc;
    out[0] = h->last_sweep_global; out[1] = h->last_sweep_rec; out[2] = h->last_sweep_pairs;
    return MCL_OK;
}

int mcl_get_effective_sample_size(const mcl_engine_t *h, double *n_eff, int32_t *resampled_last_update)
{
    if (!h || !n_eff || !resampled_last_update) return MCL_ERR_INVALID_ARG;
    if (!h->have_particles) return MCL_ERR_NOT_READY;
    const double sw = h->h_scalars[1], sww = h->h_scalars[7];
    *n_eff = sww > 0.0 ? sw * sw / sww : 0.0;
    *resampled_last_update = h->resampled_last ? 1 : 0;
    return MCL_OK;
}

int mcl_set_kld(mcl_engine_t *h, const mcl_kld_config_t *k)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!k) {
        h->kld_on = false;
        kld_reset(h);
        return MCL_OK;
    }
    MCL_TRY(refuse_shared(h, "KLD sampling"));
    if (const char *why = kld_invalid(k, h->cap)) return fail(h, MCL_ERR_INVALID_ARG, why);
    int64_t nx = 0, ny = 0;
    uint64_t bits = 0;
    if (h->have_map && !kld_grid(k, (uint32_t)h->W, (uint32_t)h->H, (float)h->res, nx, ny, bits))
        return fail(h, MCL_ERR_INVALID_ARG, "KLD: the bin grid over this map exceeds 2^31 bits");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->kld = *k; h->kld_nx = nx; h->kld_ny = ny; h->kld_bits = bits;
    h->kld_on = true;
    const int rc = kld_alloc(h);
    if (rc) { h->kld_on = false; return rc; }
    kld_reset(h);
    return MCL_OK;
}

int mcl_get_particle_count(const mcl_engine_t *h, int64_t *n)
{
    if (!h || !n) return MCL_ERR_INVALID_ARG;
    *n = h->have_particles ? h->N : 0;
    return MCL_OK;
}

int mcl_get_kld_state(const mcl_engine_t *h, int64_t *bins_last, int64_t *n_next)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (bins_last) *bins_last = h->kld_on ? h->kld_bins_last : -1;
    if (n_next) *n_next = h->kld_on ? h->kld_n_next : (h->have_particles ? h->N : 0);
    return MCL_OK;
}

int mcl_set_motion_model(mcl_engine_t *h, const mcl_motion_config_t *c)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!c) { h->motion = mcl_motion_config_t{}; return MCL_OK; }
    if (const char *why = motion_invalid(c)) return fail(h, MCL_ERR_INVALID_ARG, why);
    h->motion = *c;
    return MCL_OK;
}

int mcl_get_motion_model(const mcl_engine_t *h, mcl_motion_config_t *out)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    *out = h->motion;
    return MCL_OK;
}

int mcl_set_recovery(mcl_engine_t *h, const mcl_recovery_config_t *c)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!c) {
        h->recov_on = false;
        recov_unset(h);
        h->recov_cnt_slot = -1; h->recov_injected = 0;
        return MCL_OK;
    }
    MCL_TRY(refuse_shared(h, "recovery"));
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_UNSUPPORTED, "recovery needs weight_mode LOG");
    if (const char *why = recov_invalid(c)) return fail(h, MCL_ERR_INVALID_ARG, why);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!h->d_recov_cnt) {
        MCL_TRY(h->d_recov_cnt.reserve(h, 2));
        HIPCHK(h, hipMemsetAsync(h->d_recov_cnt, 0, 2 * sizeof(unsigned int), h->stream));
    }
    h->recov = *c;
    h->recov_on = true;
    recov_unset(h);
    h->recov_cnt_slot = -1; h->recov_injected = 0;
    return MCL_OK;
}

int mcl_get_recovery_state(mcl_engine_t *h, double state[3], int64_t *injected_last)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (state) {
        state[0] = h->recov_S; state[1] = h->recov_F;
        state[2] = h->recov_on ? recov_p(h->recov_S, h->recov_F) : 0.0;
    }
    if (injected_last) {
        if (h->recov_cnt_slot >= 0 && h->recov_injected < 0) {
            // the count of the last injecting update, read once (the update has synchronised with its kernels already)
            unsigned int c = 0;
            MCL_TRY(read_back(h, {{&c, h->d_recov_cnt + h->recov_cnt_slot, sizeof(c)}}));
            h->recov_injected = (int64_t)c;
        }
        *injected_last = h->recov_cnt_slot >= 0 ? h->recov_injected : 0;
    }
    return MCL_OK;
}

int mcl_set_recovery_state(mcl_engine_t *h, const double state[2])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!state || state[0] == INFINITY || state[1] == INFINITY) return fail(h, MCL_ERR_INVALID_ARG, "recovery: S and F must be NaN or below +inf");
    if (!h->recov_on) return fail(h, MCL_ERR_NOT_READY, "recovery is off (mcl_set_recovery)");
    h->recov_S = state[0]; h->recov_F = state[1];
    return MCL_OK;
}

// ---- the proposal of the next injecting update (the header's P1-P7)
int mcl_set_recovery_proposal(mcl_engine_t *h, int32_t n_components, const double *means, const double *covs, const double *weights)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (n_components == 0) { h->mix_n = 0; return MCL_OK; }
    MCL_TRY(refuse_shared(h, "recovery"));
    if (h->cfg.weight_mode != MCL_WEIGHT_LOG) return fail(h, MCL_ERR_UNSUPPORTED, "recovery needs weight_mode LOG");
    if (n_components < 0 || n_components > kRecovProposalMax)
        return fail(h, MCL_ERR_INVALID_ARG, "recovery proposal: n_components must be in [0, 4096]");
    const size_t M = (size_t)n_components;
    std::vector<uint64_t> thr(M);
    std::vector<double> fac(9 * M);
    const std::string why = recov_proposal(n_components, means, covs, weights, thr.data(), fac.data());
    if (!why.empty()) return fail(h, MCL_ERR_INVALID_ARG, why);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // behind whatever the stream still runs (an update's kernel may be reading the previous proposal); the buffers only ever grow
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->mix_n = 0;
    MCL_TRY(h->d_mix_thr.reserve(h, M));
    MCL_TRY(h->d_mix_fac.reserve(h, 9 * M));
    HIPCHK(h, hipMemcpy(h->d_mix_thr, thr.data(), M * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->d_mix_fac, fac.data(), 9 * M * sizeof(double), hipMemcpyHostToDevice));
    h->mix_thr.swap(thr); h->mix_fac.swap(fac);
    h->mix_n = n_components;
    return MCL_OK;
}

int mcl_get_recovery_proposal(const mcl_engine_t *h, int32_t *n_components, uint64_t *thresholds, double *factors)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (n_components) *n_components = h->mix_n;
    const size_t M = (size_t)h->mix_n;
    if (thresholds && M) std::memcpy(thresholds, h->mix_thr.data(), M * sizeof(uint64_t));
    if (factors && M) std::memcpy(factors, h->mix_fac.data(), 9 * M * sizeof(double));
    return MCL_OK;
}

int mcl_set_beam_skip(mcl_engine_t *h, const mcl_beam_skip_config_t *c)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (c) {
        if (!h->lf_on) return fail(h, MCL_ERR_NOT_READY, "beam skipping needs the likelihood field (mcl_set_likelihood_field) switched on first");
        if (const char *why = bs_invalid(c)) return fail(h, MCL_ERR_INVALID_ARG, why);
        h->bs = *c;
    }
    h->bs_on = c != nullptr;
    h->bs_have = false;
    return MCL_OK;
}

int mcl_get_beam_skip_state(mcl_engine_t *h, uint32_t *counts, uint8_t *kept, size_t n, mcl_beam_skip_state_t *st)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->bs_on || !h->bs_have) return fail(h, MCL_ERR_NOT_READY, "beam skipping is off or no update has run with it");
    if (n != (size_t)h->bs_B) return fail(h, MCL_ERR_INVALID_ARG, "counts and kept have one entry per beam of the scan");
    const size_t nb = h->bs_idx.size();
    std::vector<uint32_t> cnt(nb);
    std::vector<uint8_t> kp(nb);
    mcl_beam_skip_state_t rec{};
    MCL_TRY(read_back(h, {{nb && counts ? cnt.data() : nullptr, h->d_bs_cnt, nb * sizeof(uint32_t)}, {nb && kept ? kp.data() : nullptr, h->d_bs_kept, nb},
                          {st ? &rec : nullptr, h->d_bs_state, sizeof rec}}));
    if (counts) std::memset(counts, 0, n * sizeof(uint32_t));
    if (kept) std::memset(kept, 0, n);
    for (size_t k = 0; k < nb; ++k) {
        const size_t j = (size_t)h->bs_idx[k];
        if (counts) counts[j] = cnt[k];
        if (kept) kept[j] = kp[k];
    }
    if (st) *st = rec;
    return MCL_OK;
}

int mcl_get_likelihood_field(mcl_engine_t *h, uint16_t *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (!h->lf_on || !h->have_map || h->lf_K < 0) return fail(h, MCL_ERR_NOT_READY, "the likelihood field is off or no map is set");
    if (n != (size_t)h->W * h->H) return fail(h, MCL_ERR_INVALID_ARG, "the field has width x height entries");
    return read_back(h, {{out, h->d_lf_D, n * sizeof(uint16_t)}});
}

int mcl_get_likelihood_table(mcl_engine_t *h, float *out, size_t n, int32_t *K)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->lf_on || !h->have_map || h->lf_K < 0) return fail(h, MCL_ERR_NOT_READY, "the likelihood field is off or no map is set");
    if (K) *K = h->lf_K;
    if (!out) return MCL_OK;
    if (n != (size_t)h->lf_K + 1) return fail(h, MCL_ERR_INVALID_ARG, "the table has K + 1 entries");
    return read_back(h, {{out, h->d_lf_tab, n * sizeof(float)}});
}

// ---- the tables under the ray stage, read back as stored (test infrastructure: copies only, no launch, no state changed)
int mcl_get_wedge_fields(mcl_engine_t *h, uint8_t *out, size_t n, int32_t dims[3])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->have_map || !h->d_distw) return fail(h, MCL_ERR_NOT_READY, "no map is set or this map has no wedge fields");
    if (dims) { dims[0] = h->Hp; dims[1] = h->Wp; dims[2] = h->Wps; }
    if (!out) return MCL_OK;
    if (n != (size_t)mcl::kWedges * h->Hp * h->Wps) return fail(h, MCL_ERR_INVALID_ARG, "the wedge fields have MCL_WEDGES x Hp x Wps bytes");
    return read_back(h, {{out, h->d_distw, n}});
}

int mcl_get_sort_order(mcl_engine_t *h, uint32_t *keys, uint32_t *perm, size_t n, int32_t bbox[7], int32_t *tilemap, size_t n_tiles,
                       int64_t *n_out, int32_t *fine)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    const OrderLast &o = h->order_last;
    if (!o.bbox || o.n <= 0) return fail(h, MCL_ERR_NOT_READY, "the last ray stage did not order its particles through the radix sort");
    if (n_out) *n_out = o.n;
    if (fine) *fine = o.fine;                 // (a sort_fine_code)
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (keys || perm) {
        if (n != (size_t)o.n) return fail(h, MCL_ERR_INVALID_ARG, "keys and perm have one entry per particle of the last update");
        if (keys) HIPCHK(h, hipMemcpyAsync(keys, h->d_skey2, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        if (perm) HIPCHK(h, hipMemcpyAsync(perm, h->d_perm, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    if (bbox) HIPCHK(h, hipMemcpyAsync(bbox, o.bbox, 7 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (tilemap) {
        const auto [ntx_abs, nty_abs, tiles_ok] = sort_tiles(h);
        if (n_tiles != (size_t)ntx_abs * nty_abs || !tiles_ok) return fail(h, MCL_ERR_INVALID_ARG, "the tile map has one entry per 32 x 32-cell tile of the padded map (at most 8192)");
        HIPCHK(h, hipMemcpyAsync(tilemap, o.tilemap, n_tiles * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return MCL_OK;
}

int mcl_get_compact_guide(mcl_engine_t *h, uint32_t *guide, size_t n_guide, uint64_t *ccdf, size_t n_ccdf, int64_t info[6])
{
    if (!h || !info) return MCL_ERR_INVALID_ARG;
    info[0] = -1; info[1] = -1; info[2] = h->compact_n; info[3] = 0; info[4] = h->d_cguide ? h->guide_m : 0; info[5] = h->guide_used ? 1 : 0;
    if (!h->guide_valid || h->compact_n <= 0) {
        if (!guide && !ccdf) return MCL_OK;               // (what the host knows without a list: its length, m, the last draw's path)
        return fail(h, MCL_ERR_NOT_READY, "no compact list with a guide describes the current particles");
    }
    uint64_t q = 0;
    MCL_TRY(read_back(h, {{&q, h->d_result.p + kResultGuideTotal, sizeof(q)}}));
    const int s = mcl::guide_shift(q, h->guide_m);
    const uint32_t bmax = mcl::guide_bmax(q, s);
    info[0] = s; info[1] = (int64_t)bmax; info[2] = h->compact_n; info[3] = (int64_t)q; info[4] = h->guide_m; info[5] = h->guide_used ? 1 : 0;
    if (guide) {
        if (n_guide != (size_t)bmax + 1) return fail(h, MCL_ERR_INVALID_ARG, "the guide has bmax + 1 words");
        MCL_TRY(read_back(h, {{guide, h->d_cguide, n_guide * sizeof(uint32_t)}}));
    }
    if (ccdf) {
        if (n_ccdf != (size_t)h->compact_n) return fail(h, MCL_ERR_INVALID_ARG, "the list has n_compact entries");
        MCL_TRY(read_back(h, {{ccdf, h->d_ccdf, n_ccdf * sizeof(uint64_t)}}));
    }
    return MCL_OK;
}

int mcl_get_sort_record_form(mcl_engine_t *h, int32_t *heading_form)
{
    if (!h || !heading_form) return MCL_ERR_INVALID_ARG;
    const OrderLast &o = h->order_last;
    if (!o.bbox || o.n <= 0) return fail(h, MCL_ERR_NOT_READY, "the last ray stage did not order its particles through the radix sort");
    *heading_form = o.heading ? 1 : 0;
    return MCL_OK;
}

int mcl_get_ring_fields(mcl_engine_t *h, uint8_t *out, size_t n)
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    if (!h->have_map || !h->d_distg) return fail(h, MCL_ERR_NOT_READY, "no map is set or the engine holds no ringed copies of the wedge fields");
    if (n != h->distg_stride * (size_t)mcl::kWedges) return fail(h, MCL_ERR_INVALID_ARG, "the ringed fields have the bytes of mcl_host_sweep_global_layout's allocation");
    return read_back(h, {{out, h->d_distg, n}});
}

int mcl_get_sweep_table(mcl_engine_t *h, double *out, size_t n, int32_t dims[3])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->have_map || h->B <= 0 || !h->d_Ltd || !h->ltd_ready)
        return fail(h, MCL_ERR_NOT_READY, "no sweep ray stage has built its table for the current scan");
    const int rows = mcl::sweep_table_rows(h->P);
    if (dims) { dims[0] = rows; dims[1] = h->ltd_cols; dims[2] = h->beam_margin; }
    if (!out) return MCL_OK;
    if (n != (size_t)rows * h->ltd_cols) return fail(h, MCL_ERR_INVALID_ARG, "the table has rows x cols entries");
    return read_back(h, {{out, h->d_Ltd, n * sizeof(double)}});
}

int mcl_get_scalars(mcl_engine_t *h, double out[8])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    return read_back(h, {{out, h->d_scalars, 8 * sizeof(double)}});
}

int mcl_get_host_scalars(const mcl_engine_t *h, double out[8])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    std::memcpy(out, h->h_scalars, 8 * sizeof(double));
    return MCL_OK;
}

int mcl_set_reserved_cus(mcl_engine_t *h, int32_t n_cus)
{
    if (!h || n_cus < 0 || n_cus >= h->num_cu) return MCL_ERR_INVALID_ARG;
    h->reserved_cus = n_cus;
    return MCL_OK;
}

int mcl_set_sensor_mount(mcl_engine_t *h, const double mount[3])
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!mount || !mount_valid(mount))
        return fail(h, MCL_ERR_INVALID_ARG, "sensor mount: three finite numbers (mx, my, mtheta) with |mtheta| <= 2 pi");
    // graph_reset-class state, like the beam angles: a captured tail holds the mount as a kernel argument, the cleared-word cache
    // and the pending layout belong to the poses the last stage worked on.  Particles, weights and every option stay.
    graph_reset(h);
    for (int k = 0; k < 3; ++k) h->mount[k] = mount[k];
    h->mounted = !(mount[0] == 0.0 && mount[1] == 0.0 && mount[2] == 0.0);         // (either sign of zero)
    return MCL_OK;
}

int mcl_get_sensor_mount(const mcl_engine_t *h, double out[3])
{
    if (!h || !out) return MCL_ERR_INVALID_ARG;
    for (int k = 0; k < 3; ++k) out[k] = h->mounted ? h->mount[k] : 0.0;
    return MCL_OK;
}

int mcl_get_sensor_poses(mcl_engine_t *h, double *out_colmajor, int64_t n)
{
    if (!h || !out_colmajor) return MCL_ERR_INVALID_ARG;
    if (!h->sp_valid || !h->d_sth)
        return fail(h, MCL_ERR_NOT_READY, "sensor poses: no sensor stage has run with a mount on the current particles");
    if (n != h->sp_n) return fail(h, MCL_ERR_INVALID_ARG, "sensor poses: n is not the particle count of that stage");
    const size_t nb = (size_t)n * sizeof(double);
    return read_back(h, {{out_colmajor, h->d_sx, nb}, {out_colmajor + n, h->d_sy, nb}, {out_colmajor + 2 * n, h->d_sth, nb}});
}
