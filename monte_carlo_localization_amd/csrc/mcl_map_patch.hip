// mcl_map_patch.hip -- mcl_update_map_region: a changed rectangle of the map into every map-derived table, so
// that the engine equals, byte for byte, one given the edited grid by mcl_set_map; and mcl_get_map_table, which reads such a table
// back.  The host touches the rectangle (the comparison with grid_host, the copy) and the rows of the free-cell list the rectangle
// crosses; every field is rebuilt on the device inside the windows of mcl_host::map_patch_plan by the kernels of mcl_map_patch.h
// (launched from mcl_engine.hip, which holds the kernels: launch_patch_*).  No header with a __global__ is included here.
#include "mcl_engine_internal.h"

#include <chrono>
#include <cstring>

using namespace mcl_host;

namespace {

struct PatchDiff {
    int32_t changed = 0, changed_stop = 0;
    bool free_changed = false;                  // some cell became or ceased to be a free cell (value == 0)
    int32_t stop_box[4] = {0, 0, -1, -1};       // the cells whose stop bit changed, grid cells, inclusive
};

PatchDiff patch_diff(const mcl_engine *h, const int8_t *cells, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t row_stride)
{
    PatchDiff d;
    int bx0 = 1 << 30, by0 = 1 << 30, bx1 = -1, by1 = -1;
    for (uint32_t j = 0; j < height; ++j) {
        const int8_t *nw = cells + (size_t)j * row_stride, *old = h->grid_host.data() + (size_t)(y0 + j) * h->W + x0;
        if (std::memcmp(nw, old, width) == 0) continue;
        for (uint32_t i = 0; i < width; ++i) {
            if (nw[i] == old[i]) continue;
            ++d.changed;
            if ((nw[i] == 0) != (old[i] == 0)) d.free_changed = true;
            if ((nw[i] > 50) != (old[i] > 50)) {
                ++d.changed_stop;
                const int x = (int)(x0 + i), y = (int)(y0 + j);
                bx0 = std::min(bx0, x); bx1 = std::max(bx1, x); by0 = std::min(by0, y); by1 = std::max(by1, y);
            }
        }
    }
    if (d.changed_stop) { d.stop_box[0] = bx0; d.stop_box[1] = by0; d.stop_box[2] = bx1; d.stop_box[3] = by1; }
    return d;
}

// What a patch holds until the stream has been waited for: the temporaries of the kernels, the new rows of the free list and, where
// the list changes its length, its successor.
struct PatchHold {
    MapPatchTmp tmp;
    std::vector<uint32_t> seg;
    DevBuf<uint32_t> free_next;
    bool free_moves = false;
    uint64_t n_free_next = 0;
};

// the free cells of rows y0 .. y1 of grid_host (already edited) in place of the old ones: in place where the count is the same,
// else into a new list (prefix and suffix copied on the device)
int patch_free_list(mcl_engine *h, int y0, int y1, PatchHold &k)
{
    const size_t W = (size_t)h->W;
    const uint64_t a = h->free_row[(size_t)y0], b = h->free_row[(size_t)y1 + 1];
    std::vector<uint64_t> row_at((size_t)(y1 - y0) + 2);
    for (int y = y0; y <= y1; ++y) {
        row_at[(size_t)(y - y0)] = a + k.seg.size();
        const int8_t *row = h->grid_host.data() + (size_t)y * W;
        for (size_t x = 0; x < W; ++x)
            if (row[x] == 0) k.seg.push_back((uint32_t)((size_t)y * W + x));
    }
    row_at[(size_t)(y1 - y0) + 1] = a + k.seg.size();
    k.n_free_next = h->n_free - (b - a) + k.seg.size();
    const size_t u32 = sizeof(uint32_t);
    if (k.seg.size() == b - a) {
        if (!k.seg.empty()) HIPCHK(h, hipMemcpyAsync(h->d_free.p + a, k.seg.data(), k.seg.size() * u32, hipMemcpyHostToDevice, h->stream));
    } else {
        k.free_moves = true;
        if (k.n_free_next) {
            MCL_TRY(k.free_next.reserve(h, (size_t)k.n_free_next));
            if (a) HIPCHK(h, hipMemcpyAsync(k.free_next.p, h->d_free.p, a * u32, hipMemcpyDeviceToDevice, h->stream));
            if (!k.seg.empty()) HIPCHK(h, hipMemcpyAsync(k.free_next.p + a, k.seg.data(), k.seg.size() * u32, hipMemcpyHostToDevice, h->stream));
            if (h->n_free > b)
                HIPCHK(h, hipMemcpyAsync(k.free_next.p + a + k.seg.size(), h->d_free.p + b, (h->n_free - b) * u32, hipMemcpyDeviceToDevice, h->stream));
        }
    }
    const int64_t delta = (int64_t)k.seg.size() - (int64_t)(b - a);
    for (int y = y0; y <= y1 + 1; ++y) h->free_row[(size_t)y] = row_at[(size_t)(y - y0)];
    for (size_t y = (size_t)y1 + 2; y <= (size_t)h->H; ++y) h->free_row[y] = (uint64_t)((int64_t)h->free_row[y] + delta);
    return MCL_OK;
}

// everything a patch enqueues on the stream (the caller waits for it, whatever this returns)
int patch_enqueue(mcl_engine *h, const int8_t *cells, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t row_stride,
                  const PatchDiff &d, const MapPatchPlan &plan, bool lf, int lf_reach, int lf_K, PatchHold &k)
{
    HIPCHK(h, hipMemcpy2DAsync(h->d_grid.p + (size_t)y0 * h->W + x0, (size_t)h->W, cells, (size_t)row_stride, width, height, hipMemcpyHostToDevice, h->stream));
    if (d.free_changed) MCL_TRY(patch_free_list(h, (int)y0, (int)(y0 + height - 1), k));
    if (!d.changed_stop) return MCL_OK;
    MCL_TRY(launch_patch_skip_field(h, plan.win, k.tmp));
    if (h->d_distq[0])
        for (int q = 0; q < 4; ++q) MCL_TRY(launch_patch_quadrant(h, q, plan.quad[q], k.tmp));
    if (h->d_distw) MCL_TRY(launch_patch_wedges(h, plan.win, plan.quad, k.tmp));      // (behind the isotropic field: its row tables read dist == 0)
    if (lf) MCL_TRY(launch_patch_lfield(h, plan.lf, lf_reach, lf_K, k.tmp));
    return MCL_OK;
}

}  // namespace

int mcl_update_map_region(mcl_engine_t *h, const int8_t *cells, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height, uint32_t row_stride,
                          mcl_map_patch_stats_t *st)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!cells || width == 0 || height == 0 || row_stride < width) return fail(h, MCL_ERR_INVALID_ARG, "map patch: a null pointer, an empty rectangle or row_stride < width");
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "map patch: no map is set");
    if ((uint64_t)x0 + width > (uint64_t)h->W || (uint64_t)y0 + height > (uint64_t)h->H) return fail(h, MCL_ERR_INVALID_ARG, "map patch: the rectangle leaves the map");
    const PatchDiff d = patch_diff(h, cells, x0, y0, width, height, row_stride);
    mcl_map_patch_stats_t s{};
    s.changed_cells = d.changed; s.changed_stop_cells = d.changed_stop;
    s.window[2] = s.window[3] = s.lf_window[2] = s.lf_window[3] = -1;
    s.free_cells = (int64_t)h->n_free;
    const auto done = [&](int rc) {
        s.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (st) *st = s;
        return rc;
    };
    if (!d.changed) return done(MCL_OK);                    // nothing launched, nothing voided
    const bool lf = h->lf_on && h->lf_K >= 0 && d.changed_stop;
    int lf_K = 0, lf_reach = 0;
    if (lf) lf_reach_of(h, lf_K, lf_reach);
    MapPatchPlan plan{};
    if (d.changed_stop) {
        if (!map_patch_plan(h->W, h->H, d.stop_box, lf ? lf_reach : 0, plan)) return fail(h, MCL_ERR_INVALID_ARG, "map patch: no window (internal)");
        std::memcpy(s.window, plan.win, sizeof(plan.win));
        std::memcpy(s.lf_window, plan.lf, sizeof(plan.lf));
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // what mcl_set_map voids (the particles, the beams and what depends on the range or the resolution alone stay)
    graph_reset(h);
    recov_unset(h);
    h->weighted = false;
    h->mix_n = 0;
    h->ltd_ready = false;
    h->map_epoch++;
    if (lf) h->lf_epoch++;
    h->have_map = false;                 // until the stream has run dry without an error: a failure leaves "map not set", never half a patch
    for (uint32_t j = 0; j < height; ++j)
        std::memcpy(h->grid_host.data() + (size_t)(y0 + j) * h->W + x0, cells + (size_t)j * row_stride, width);
    PatchHold k;
    int rc = patch_enqueue(h, cells, x0, y0, width, height, row_stride, d, plan, lf, lf_reach, lf_K, k);
    const hipError_t e = hipStreamSynchronize(h->stream);              // the one host wait; `cells`, k.seg and the temporaries are free after it
    if (rc == MCL_OK && e != hipSuccess) rc = fail(h, MCL_ERR_HIP, std::string("map patch: ") + hipGetErrorString(e));
    if (rc) return done(rc);
    if (d.free_changed) {
        if (k.free_moves) h->d_free = std::move(k.free_next);
        h->n_free = k.n_free_next;
    }
    s.free_cells = (int64_t)h->n_free;
    h->have_map = true;
    if (h->kld_on) {                     // (as mcl_set_map: the bin bitmap and its counters start clean)
        rc = kld_alloc(h);
        if (rc) { h->have_map = false; return done(rc); }
    }
    return done(MCL_OK);
}

int mcl_get_map_table(mcl_engine_t *h, int32_t which, void *out, size_t n_bytes, size_t *needed)
{
    if (!h) return MCL_ERR_INVALID_ARG;
    if (!h->have_map) return fail(h, MCL_ERR_NOT_READY, "no map is set");
    const size_t field = (size_t)h->Hp * h->Wps;
    const void *src = nullptr;
    size_t need = 0;
    if (which == MCL_MAP_TABLE_GRID) { src = h->d_grid.p; need = (size_t)h->W * h->H; }
    else if (which == MCL_MAP_TABLE_SKIP) { src = h->d_dist.p; need = field; }
    else if (which == MCL_MAP_TABLE_SKIP_NIBBLES) { src = h->d_dist4.p; need = field / 2; }
    else if (which >= MCL_MAP_TABLE_QUADRANT0 && which < MCL_MAP_TABLE_QUADRANT0 + 4) {
        src = h->d_distq[which - MCL_MAP_TABLE_QUADRANT0].p; need = field;
        if (!src) return fail(h, MCL_ERR_NOT_READY, "this map has no quadrant fields");
    }
    else if (which == MCL_MAP_TABLE_FREE_CELLS) { src = h->d_free.p; need = (size_t)h->n_free * sizeof(uint32_t); }
    else return fail(h, MCL_ERR_INVALID_ARG, "no such map table");
    if (needed) *needed = need;
    if (!out) return MCL_OK;
    if (n_bytes != need) return fail(h, MCL_ERR_INVALID_ARG, "the table has *needed bytes");
    if (!need) return MCL_OK;
    return read_back(h, {{out, src, need}});
}
