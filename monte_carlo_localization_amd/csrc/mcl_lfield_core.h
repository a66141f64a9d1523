// mcl_lfield_core.h -- the per-beam arithmetic of the likelihood-field model (LF4 / LF5): what k_lfield
// (mcl_lfield.h, the update and the pose query) and the lattice search (mcl_search.h) share, so that a particle and a lattice pose
// at the same place get the same bits.  No kernels here: every translation unit with device code may include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mcl {

// Lf is staged in LDS below this many entries (32 KiB: five 256-thread workgroups per CU); a larger K reads it from global memory.
constexpr int kLfLdsEntries = 8192;

// a pose coordinate in cell units
__device__ __forceinline__ double lf_cell_coord(double x, double origin, double inv_res) { return (x - origin) * inv_res; }

// The table value of one beam of a pose at (px, py) cells with heading (s, c) = sincos(theta): the end point of beam b = (r cos a
// / res, r sin a / res) is (px + c b.x - s b.y, py + s b.x + c b.y) (LF4, the rotation form), its cell by floor; off the map
// (or NaN) it reads `off` = Lf[K].
__device__ __forceinline__ float lf_beam_value(const double2 b, double s, double c, double px, double py, double W, double H, int Wi,
                                               const uint16_t *D, const float *lf, float off)
{
    const double fx = floor(fma(c, b.x, fma(-s, b.y, px)));
    const double fy = floor(fma(s, b.x, fma(c, b.y, py)));
    float v = off;
    if (fx >= 0.0 && fx < W && fy >= 0.0 && fy < H)       // (false for NaN: off the map)
        v = lf[D[(size_t)(int)fy * (size_t)Wi + (size_t)(int)fx]];
    return v;
}

// What lf_beam_dist returns off the map (or for NaN): above every D (<= 65535) and never below Ka (<= 65536; BS1)
constexpr uint32_t kLfOffMap = 0x10000u;

// lf_beam_value's end cell (the same two FMA pairs, floors and bounds test), returning D[cell] itself, or kLfOffMap off the map:
// the value of the beam is lf[D] (off the map Lf[K]), and it agrees (BS1) iff D < Ka.
__device__ __forceinline__ uint32_t lf_beam_dist(const double2 b, double s, double c, double px, double py, double W, double H, int Wi,
                                                 const uint16_t *D)
{
    const double fx = floor(fma(c, b.x, fma(-s, b.y, px)));
    const double fy = floor(fma(s, b.x, fma(c, b.y, py)));
    uint32_t d = kLfOffMap;
    if (fx >= 0.0 && fx < W && fy >= 0.0 && fy < H)       // (false for NaN: off the map)
        d = D[(size_t)(int)fy * (size_t)Wi + (size_t)(int)fx];
    return d;
}

}  // namespace mcl
