// mcl_field_build.h -- the wedge fields (mcl_wedge.h) built on the device at mcl_set_map: k_ring_field, k_row_tables, k_wedge_field*.
#pragma once

namespace mcl {

// The copy of wedge field k that k_rays_sweep<.., GLOBAL> probes in place (mcl_rays_sweep.h): (Hp + 4) rows of `pitch` bytes holding
// the padded grid MIRRORED in the axes along which the wedge's rays run backwards (sxp / syp = 0), at offset (2, 2); everything
// else -- the two-cell ring around it and the row padding -- stop.  Every ray of the wedge runs towards +x, +y in this frame.
// The tail of stop rows behind the field is left by the memset of the allocation (mcl_set_map).
__global__ __launch_bounds__(256) void k_ring_field(const uint8_t *__restrict__ src, int Wp, int Hp, int Wps, int pitch, int sxp, int syp,
                                                   uint8_t *__restrict__ dst)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;          // destination column / row
    if (x >= pitch) return;
    const int mx = x - 2, my = y - 2;                                             // cell of the mirrored padded grid
    uint8_t v = 0xFF;
    if (mx >= 0 && mx < Wp && my >= 0 && my < Hp) v = src[(size_t)(syp ? my : Hp - 1 - my) * Wps + (sxp ? mx : Wp - 1 - mx)];
    dst[(size_t)y * pitch + x] = v;
}

// one thread per row of the padded grid: next / previous stop cell in the row (dist == 0 marks a stop)
__global__ void k_row_tables(const uint8_t *__restrict__ dist, int Wp, int Hp, int Wps, int32_t *__restrict__ nxt, int32_t *__restrict__ prv)
{
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= Hp) return;
    const uint8_t *row = dist + (size_t)y * Wps;
    int last = -1;
    for (int x = 0; x < Wp; ++x) { if (row[x] == 0) last = x; prv[(size_t)y * Wp + x] = last; }
    int next = Wp;
    for (int x = Wp - 1; x >= 0; --x) { if (row[x] == 0) next = x; nxt[(size_t)y * Wp + x] = next; }
}

__global__ __launch_bounds__(256) void k_wedge_field(const int32_t *__restrict__ nxt, const int32_t *__restrict__ prv, int Wp, int Hp, int Wps,
                                                    const WedgeRow *__restrict__ rows, uint8_t *__restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= Wp || y >= Hp) return;
    // stored in k_rays_cell's LDS encoding: stop -> 0xFF (-1 as a signed byte), skips capped at 127
    const int v = wedge_skip_cell(nxt, prv, Wp, Hp, x, y, rows);
    out[(size_t)y * Wps + x] = (uint8_t)(v == 0 ? 255 : (v > 127 ? 127 : v));
}

// the same field under the tight rule (mcl_wedge.h: the distance travelled inside the wedge), the same encoding
__global__ __launch_bounds__(256) void k_wedge_field_tight(const int32_t *__restrict__ nxt, const int32_t *__restrict__ prv, int Wp, int Hp, int Wps,
                                                          const WedgeRow *__restrict__ rows, WedgeCone cone, uint8_t *__restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= Wp || y >= Hp) return;
    const int v = wedge_skip_cell_tight(nxt, prv, Wp, Hp, x, y, rows, cone);
    out[(size_t)y * Wps + x] = (uint8_t)(v == 0 ? 255 : (v > 127 ? 127 : v));
}

}  // namespace mcl
