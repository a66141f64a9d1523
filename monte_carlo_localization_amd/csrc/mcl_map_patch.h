// mcl_map_patch.h -- the kernels of mcl_update_map_region: every map-derived table rebuilt inside a window of
// the map, in integers, to the bytes mcl_set_map would have put there.  A window is given by its origin and extent; what a kernel
// reads beyond its window (stop cells, row tables, column distances) comes through an EXTENDED region with a pitch of its own,
// sized by the window and the table's reach (kPatchReach), never by the map.  The rules are those of mcl_host_math.hip
// (build_distance_field, build_directional_field), mcl_wedge.h and mcl_lfield.h; the brute-force shape is k_lf_cols / k_lf_rows'.
#pragma once

namespace mcl {

// a skip of 255 (the cap) is what every squared gap of 254^2 or more gives: no stop cell further than this, per axis, can lower a
// value, and a search may stop there
constexpr int kPatchReach = 254;
constexpr int kPatchCap2 = kPatchReach * kPatchReach;

struct PatchWin { int x0, y0, w, h; };          // origin and extent, in the cells of the table it is a window of

// stop cell of the padded grid (padded cell (xp, yp) reads grid cell (max(xp - 1, 0), max(yp - 1, 0))); everything outside is stop
__device__ inline bool patch_stop(const int8_t *__restrict__ grid, int W, int Wp, int Hp, int xp, int yp)
{
    if (xp < 0 || yp < 0 || xp >= Wp || yp >= Hp) return true;
    return grid[(size_t)max(yp - 1, 0) * W + max(xp - 1, 0)] > 50;
}

// ---- isotropic field: the 3 x 3 dilation of the stop set over the extended region e (which may hold the one-cell border outside
// the padded grid; a source further out than that border is never the nearest), then the two passes
__global__ __launch_bounds__(256) void k_patch_stop_mask(const int8_t *__restrict__ grid, int W, int Wp, int Hp, PatchWin e, uint8_t *__restrict__ mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= e.w) return;
    const int x = e.x0 + i, y = e.y0 + j;
    bool s = false;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) s = s || patch_stop(grid, W, Wp, Hp, x + dx, y + dy);
    mask[(size_t)j * e.w + i] = s ? 1 : 0;
}

// column pass: g = |dy| to the nearest dilated stop of the same column, exact below kPatchReach, else kPatchReach.  One thread per
// cell of (columns of e) x (rows of the window wy0 .. wy0 + wh - 1).
__global__ __launch_bounds__(256) void k_patch_iso_cols(const uint8_t *__restrict__ mask, PatchWin e, int wy0, int wh, uint8_t *__restrict__ g)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= e.w || j >= wh) return;
    const int r = wy0 + j - e.y0;                                 // the cell's row in e
    int d = kPatchReach;
    for (int k = 0; k < kPatchReach; ++k) {
        const bool up = r - k >= 0 && mask[(size_t)(r - k) * e.w + i];
        const bool dn = r + k < e.h && mask[(size_t)(r + k) * e.w + i];
        if (up || dn) { d = k; break; }
        if (r - k < 0 && r + k >= e.h) break;
    }
    g[(size_t)j * e.w + i] = (uint8_t)d;
}

// row pass: min(floor(sqrt(min over dx of dx^2 + g^2)) + 1, 255), 0 on a stop cell of the padded grid
__global__ __launch_bounds__(256) void k_patch_iso_rows(const uint8_t *__restrict__ g, PatchWin e, const int8_t *__restrict__ grid, int W, int Wp, int Hp,
                                                       PatchWin win, int Wps, uint8_t *__restrict__ dist)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= win.w) return;
    const int x = win.x0 + i, y = win.y0 + j;
    const uint8_t *row = g + (size_t)j * e.w;
    const int c = x - e.x0;
    int best = kPatchCap2;
    for (int dx = 0; dx < kPatchReach && dx * dx < best; ++dx) {
        if (c - dx >= 0) { const int v = row[c - dx]; best = min(best, dx * dx + v * v); }
        if (c + dx < e.w) { const int v = row[c + dx]; best = min(best, dx * dx + v * v); }
    }
    int val = 0;
    if (!patch_stop(grid, W, Wp, Hp, x, y)) val = best >= kPatchCap2 ? 255 : wedge_isqrt(best) + 1;
    dist[(size_t)y * Wps + x] = (uint8_t)val;
}

// the nibble copy of rows y0 .. y0 + h - 1, bytes b0 .. b0 + bw - 1 of every row (two cells a byte; Wps is even)
__global__ __launch_bounds__(256) void k_patch_nibbles(const uint8_t *__restrict__ dist, int Wps, int b0, int y0, int bw, uint8_t *__restrict__ dist4)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= bw) return;
    const size_t k = ((size_t)(y0 + blockIdx.y) * Wps) / 2 + b0 + i;
    dist4[k] = (uint8_t)(min((int)dist[2 * k], 15) | (min((int)dist[2 * k + 1], 15) << 4));
}

// ---- quadrant fields (build_directional_field): hq = the gap in x to the nearest stop ahead in the same row (the cell just
// outside the grid is one), 0 in the row beyond the grid, held at kPatchReach; rows win.y0 .. of an extended region of eh rows that
// starts at ey0 and lies ahead (sy) of the window
__global__ __launch_bounds__(256) void k_patch_quad_rows(const int8_t *__restrict__ grid, int W, int Wp, int Hp, int sx, PatchWin win, int ey0, int eh,
                                                        uint8_t *__restrict__ hq)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= win.w || j >= eh) return;
    const int x = win.x0 + i, y = ey0 + j;
    int hv = 0;
    if (y >= 0 && y < Hp) {
        hv = kPatchReach;
        for (int k = 0; k <= kPatchReach; ++k)
            if (patch_stop(grid, W, Wp, Hp, x + sx * k, y)) { hv = max(k - 1, 0); break; }
    }
    hq[(size_t)j * win.w + i] = (uint8_t)hv;
}

__global__ __launch_bounds__(256) void k_patch_quad_cols(const uint8_t *__restrict__ hq, const int8_t *__restrict__ grid, int W, int Wp, int Hp, int sy,
                                                        PatchWin win, int ey0, int eh, int Wps, uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= win.w) return;
    const int x = win.x0 + i, y = win.y0 + j;
    int best = kPatchCap2;
    for (int k = 0; k <= kPatchReach + 1; ++k) {
        const int gy = max(k - 1, 0);
        if (gy * gy >= best) break;
        const int r = y + sy * k - ey0;
        if (r < 0 || r >= eh) break;
        const int hv = hq[(size_t)r * win.w + i];
        best = min(best, gy * gy + hv * hv);
    }
    int val = 0;
    if (!patch_stop(grid, W, Wp, Hp, x, y)) val = best >= kPatchCap2 ? 255 : wedge_isqrt(best) + 1;
    out[(size_t)y * Wps + x] = (uint8_t)val;
}

// ---- wedge fields: k_row_tables over the region e of the padded grid, in e's own coordinates and pitch (next / previous stop of a
// row inside e: e.w / -1 when there is none).  With e the window widened by kWedgeR and clipped to the grid, the per-cell
// functions of mcl_wedge.h see in e what they would see in the whole grid: an edge of e that is not an edge of the grid is
// further from every window cell than they look, and an edge that is one ends the tables where the grid's end.
__global__ void k_patch_row_tables(const uint8_t *__restrict__ dist, int Wps, PatchWin e, int32_t *__restrict__ nxt, int32_t *__restrict__ prv)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= e.h) return;
    const uint8_t *row = dist + (size_t)(e.y0 + j) * Wps + e.x0;
    int last = -1;
    for (int x = 0; x < e.w; ++x) { if (row[x] == 0) last = x; prv[(size_t)j * e.w + x] = last; }
    int next = e.w;
    for (int x = e.w - 1; x >= 0; --x) { if (row[x] == 0) next = x; nxt[(size_t)j * e.w + x] = next; }
}

template <bool TIGHT>
__global__ __launch_bounds__(256) void k_patch_wedge_field(const int32_t *__restrict__ nxt, const int32_t *__restrict__ prv, PatchWin e, PatchWin win, int Wps,
                                                          const WedgeRow *__restrict__ rows, WedgeCone cone, uint8_t *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= win.w) return;
    const int x = win.x0 + i, y = win.y0 + j;
    const int v = TIGHT ? wedge_skip_cell_tight(nxt, prv, e.w, e.h, x - e.x0, y - e.y0, rows, cone)
                        : wedge_skip_cell(nxt, prv, e.w, e.h, x - e.x0, y - e.y0, rows);
    out[(size_t)y * Wps + x] = (uint8_t)(v == 0 ? 255 : (v > 127 ? 127 : v));
}

// the window's cells of a wedge field into its mirrored, ringed copy (k_ring_field's mapping; ring, padding and tail stay)
__global__ __launch_bounds__(256) void k_patch_ring_field(const uint8_t *__restrict__ src, int Wp, int Hp, int Wps, int pitch, int sxp, int syp, PatchWin win,
                                                         uint8_t *__restrict__ dst)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= win.w) return;
    const int x = win.x0 + i, y = win.y0 + j;
    const int mx = sxp ? x : Wp - 1 - x, my = syp ? y : Hp - 1 - y;
    dst[(size_t)(my + 2) * pitch + mx + 2] = src[(size_t)y * Wps + x];
}

// ---- likelihood field: k_lf_cols over (columns ex0 .. ex0 + ew - 1) x (rows of the window), k_lf_rows over the window
__global__ __launch_bounds__(256) void k_patch_lf_cols(const int8_t *__restrict__ grid, int W, int H, int reach, int ex0, int ew, int wy0, int wh,
                                                      uint16_t *__restrict__ g)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= ew || j >= wh) return;
    const int x = ex0 + i, y = wy0 + j;
    int d = reach;
    for (int k = 0; k < reach; ++k) {
        const bool up = y - k >= 0 && grid[(size_t)(y - k) * W + x] > 50;
        const bool dn = y + k < H && grid[(size_t)(y + k) * W + x] > 50;
        if (up || dn) { d = k; break; }
        if (y - k < 0 && y + k >= H) break;
    }
    g[(size_t)j * ew + i] = (uint16_t)d;
}

__global__ __launch_bounds__(256) void k_patch_lf_rows(const uint16_t *__restrict__ g, int ex0, int ew, int W, int reach, int K, PatchWin win,
                                                      uint16_t *__restrict__ D)
{
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (i >= win.w) return;
    const int x = win.x0 + i, y = win.y0 + j;
    const uint16_t *row = g + (size_t)j * ew;
    const int c = x - ex0;
    int best = K;
    for (int dx = 0; dx < reach && dx * dx < best; ++dx) {
        if (c - dx >= 0) { const int v = row[c - dx]; best = min(best, dx * dx + v * v); }
        if (c + dx < ew) { const int v = row[c + dx]; best = min(best, dx * dx + v * v); }
    }
    D[(size_t)y * W + x] = (uint16_t)best;
}

}  // namespace mcl
