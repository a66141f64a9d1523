// mcl_kernels.h — the HIP kernels of the particle-filter update (gfx950 / CDNA4, wave64): the list of the per-stage headers.
//
//   K5  k_scan_*            exact uint64 inclusive scan of fixed-point weights (resample CDF)             mcl_scan.h
//   K6+K1+K2 k_resample_motion   threshold -> CDF search -> parent gather -> motion + noise                mcl_resample.h
//   K3  k_rays<MODE>        fused ray cast + beam-model log-likelihood  (the dominant kernel)             mcl_rays_*.h
//   K4  k_reduce_max / k_weights / k_final_*   max-subtracted weights, fixed-point weights, sums          mcl_weights.h
//   K7  (fused into k_weights) weighted pose sums
//
// Reference rows: R = cpp:656-665, M = cpp:449-503, Q/C/E = cpp:506-650,
// N = cpp:678-686, P = cpp:696-716.
#pragma once
#include "mcl_types.h"
#include <type_traits>
#include "mcl_ray_core.h"
#include "mcl_device_math.h"
#include "mcl_wedge.h"
#include "mcl_motion.h"
#include "mcl_sort_key.h"
#include "mcl_compact_guide.h"

// Each stage header is included from here only, inside the context of the includes above.  The order of these includes is the order
// of the kernels in the code object (tools/kernel_compare.py compares it with a parent's): a new header goes where its kernels are to lie.
#include "mcl_scan.h"
#include "mcl_resample.h"
#include "mcl_init.h"
#include "mcl_rays_basic.h"
#include "mcl_field_build.h"
#include "mcl_order.h"
#include "mcl_rays_lists.h"         // (mcl_rays_legacy.h in its place, under MCL_LEGACY_RAY_KERNELS)
#include "mcl_weights.h"
#include "mcl_rays_sweep.h"
#include "mcl_rays_deskew.h"        // (per-beam sensor offsets)
#include "mcl_map_patch.h"          // (last: the windowed field builders of a map patch; off the update path)
