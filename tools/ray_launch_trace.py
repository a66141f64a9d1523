#!/usr/bin/env python3
"""Every branch of the ray stage's host code (launch_rays and what prepares for it), once each at small sizes (run on a GPU box; test
infrastructure, like tests/).

Per scenario one line: the kernel the last ray stage ran, the variant triple of mcl_get_ray_kernel_variant, and a SHA-256 over the raw
bytes of the log-weights, the particles and (after an update) the resample indices -- and the ray steps where they are kept.  Two
builds of the library (MCL_LIB=<the other build>) run the same scenarios and must print the same lines; run under
`rocprofv3 --kernel-trace --output-format csv -- python tools/ray_launch_trace.py`, their kernel traces must also hold the same
ordered list of (kernel, grid, workgroup, LDS bytes): `ray_launch_trace.py compare <parent's kernel_trace.csv> <change's>` says so,
in dispatch order over the whole process (equal there is equal per scenario), and that the parent's trace reached every kernel form
of REQUIRED.  tests/test_gpu_ray_launch_forms.py runs the same scenarios against the oracle.

usage: ray_launch_trace.py [legacy]        (legacy: the two scenarios of libmcl_hip_engine_legacy.so only; default: all the others)
       ray_launch_trace.py compare <kernel_trace.csv of the parent> <kernel_trace.csv of the change> [legacy]
"""
import csv
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import scan_geometries as scg                                     # noqa: E402
import side_geometries as sg                                      # noqa: E402

SWEEP, SKIP, MARCH, QUAD, CELL = "k_rays_sweep", "k_rays_skip", "k_rays_march", "k_rays_quad", "k_rays_cell"


def S(name, kernel, variant=(0, 0, 0), n=4096, beams="even", updates=1, call="update", max_range_m=12.0, env=None, **cfg):
    return dict(name=name, kernel=kernel, variant=tuple(variant), n=n, beams=beams, updates=updates, call=call, max_range_m=max_range_m,
                env=dict(env or {}), cfg=cfg)


# ray_kernel is named by its enumerator's value (include/mcl_hip_engine.h): 1 march, 2 skip, 3 quad, 4 cell, 5 sweep; absent: AUTO.
# The variant triple: (0 LDS windows / 1 global fields / 2 hybrid, turned directions (REC), two rays per lane (PAIRS)).
# 13 m on the 0.05 m map = 260 px: beyond the 243 px an LDS window holds and the 255 a one-byte step index does.
SCENARIOS = [
    S("tiny_tail", SKIP, n=2048, updates=3),                                     # direct table, k_tiny_tail
    S("graph_tail", SKIP, n=32768, updates=3),                                   # the captured tail of a small update
    S("march", MARCH, n=1500, ray_kernel=1),
    S("skip_r1", SKIP, n=1500, ray_kernel=2, rays_per_lane=1),
    S("skip_r4", SKIP, n=1500, ray_kernel=2, rays_per_lane=4),
    S("sweep_pairs", SWEEP, (0, 1, 1), ray_kernel=5),                            # first update of a fresh set: PAIRS + the windowed far pass
    S("sweep_rec", SWEEP, (0, 1, 0), updates=2, ray_kernel=5),
    S("sweep_fetched", SWEEP, (0, 0, 0), n=1500, beams="jitter", updates=2, ray_kernel=5),
    # members of tests/scan_geometries.py by name: 45 degrees of scan (thirteen of a lane's sixteen wedges hold no beam), and 1600 beams with
    # virtual beams whose 1920 table columns leave REC no room in LDS (fetched directions)
    S("sweep_narrow", SWEEP, (0, 1, 1), beams="narrow_rear", ray_kernel=5),
    S("sweep_fetched_padded", SWEEP, (0, 0, 0), n=1500, beams="rec1600", ray_kernel=5),
    S("sweep_global_rec", SWEEP, (1, 1, 1), ray_kernel=5, env={"MCL_SWEEP_GLOBAL": "1", "MCL_SWEEP_HYBRID": "0"}),
    S("sweep_global_fetched", SWEEP, (1, 0, 0), n=1500, beams="jitter", ray_kernel=5, env={"MCL_SWEEP_GLOBAL": "1", "MCL_SWEEP_HYBRID": "0"}),
    S("sweep_hybrid", SWEEP, (2, 1, 0), updates=2, max_range_m=13.0, ray_kernel=5, env={"MCL_SWEEP_HYBRID": "2"}),
    S("long_range_steps", SWEEP, (1, 1, 1), n=1500, max_range_m=13.0, ray_kernel=5, keep_ray_steps=1, env={"MCL_SWEEP_HYBRID": "0"}),
    S("sort_radix", SWEEP, (0, 1, 0), updates=3, ray_kernel=5, env={"MCL_SORT": "radix"}),
    S("sort_hist", SWEEP, (0, 1, 0), n=1500, updates=2, ray_kernel=5, env={"MCL_SORT": "hist"}),
    S("three_updates", SWEEP, (0, 1, 0), updates=3, ray_kernel=5),               # no stale layout / stale layout / + the prep fold
    S("no_stale_layout", SWEEP, (0, 1, 0), updates=3, ray_kernel=5, env={"MCL_NO_STALE_LAYOUT": "1"}),
    S("no_prep_fold", SWEEP, (0, 1, 0), updates=3, ray_kernel=5, env={"MCL_NO_PREP_FOLD": "1"}),
    S("no_bucket_cuts", SWEEP, (0, 1, 0), updates=3, ray_kernel=5, env={"MCL_NO_BUCKET_CUTS": "1"}),
    S("count_sweep", SWEEP, (0, 1, 0), updates=2, ray_kernel=5, debug_count_probes=1),
    S("count_global", SWEEP, (1, 1, 1), ray_kernel=5, debug_count_probes=1, env={"MCL_SWEEP_GLOBAL": "1", "MCL_SWEEP_HYBRID": "0"}),
    S("count_skip", SKIP, n=1500, ray_kernel=2, debug_count_probes=1),
    S("stage_rays", SWEEP, (0, 1, 1), call="stage_rays", ray_kernel=5),
    # two shards on one device: the staged resample (stage_resample_launch) meets no layout / the stale layout / + the prep fold
    S("group_staged", SWEEP, (0, 1, 0), call="group", updates=3, ray_kernel=5),
    S("legacy_quad", QUAD, ray_kernel=3),
    S("legacy_cell", CELL, n=1500, updates=2, ray_kernel=4),
]
ACTION = (0.05, 0.0, 0.01)
# kernel forms (spaces removed) the parent's trace must hold for the comparison to mean something
REQUIRED = ["k_tiny_tail<", "k_rays_march<false>", "k_rays_skip<1,false,false>", "k_rays_skip<4,false,false>", "k_rays_skip<1,true,false>",
            "k_rays_skip<1,false,true>", "k_rays_skip<1,true,true>", "k_rays_sweep<false,false,false,false,false>",
            "k_rays_sweep<false,false,true,false,false>", "k_rays_sweep<false,false,true,true,false>", "k_rays_sweep<false,true,false,false,false>",
            "k_rays_sweep<false,true,true,true,false>", "k_rays_sweep<false,false,true,false,true>", "k_rays_sweep<true,false,true,false,false>",
            "k_rays_sweep<true,false,true,true,false>", "k_rays_sweep<true,true,true,true,false>", "k_rays_far<false>", "k_rays_far<true>",
            "k_rays_fix<false>", "k_rays_exact<false>", "k_combine_logw", "k_prep_small", "k_particle_prep", "k_cell_bbox", "k_tile_compact",
            "k_sort_hist", "k_sort_keys", "k_sort_gather", "k_unit_table", "k_unit_sums", "k_sweep_plan", "k_far_count", "k_bbox_init"]
REQUIRED_LEGACY = ["k_rays_quad<false>", "k_rays_cell<false>", "k_slice_means", "k_fix_overflow", "k_gather_logw", "k_hist_clear"]


def inputs(orc, sc):
    """(geometry, oracle map, beam angles, scan from the geometry's true pose, particles around it): fixed seeds"""
    g = sg.small()
    om = orc.OracleMap(g.data, g.resolution, g.origin_x, g.origin_y, max_range_m=sc["max_range_m"])
    rng = np.random.default_rng(5)
    if sc["beams"] in scg.NAMES:
        ang = scg.family()[sc["beams"]].copy()
    elif sc["beams"] == "even":
        ang = (-0.75 * np.pi + np.arange(181) * (1.5 * np.pi / 180)).astype(np.float32)
    else:
        ang = np.sort(-0.75 * np.pi + (np.arange(61) + rng.uniform(-0.4, 0.4, 61)) * (1.5 * np.pi / 60)).astype(np.float32)
    pose = np.array(g.true_pose)
    scan, _ = orc.cast_many(om, np.full(ang.size, pose[0]), np.full(ang.size, pose[1]), pose[2] + ang.astype(np.float64))
    p = pose[:, None] + rng.normal(0, 1, (3, sc["n"])) * np.array([[0.15], [0.15], [0.2]])
    return g, om, ang, scan.astype(np.float32), p


def run(engine_mod, orc, sc):
    """One scenario on a fresh engine: dict(kernel, variant, particles, logw, idx or None, steps or None, om, ang, scan)"""
    g, om, ang, scan, p = inputs(orc, sc)
    saved = {k: os.environ.get(k) for k in sc["env"]}
    os.environ.update(sc["env"])                                  # (read at mcl_create)
    try:
        if sc["call"] == "group":
            return run_group(engine_mod.Group([0, 0], max_particles=sc["n"] // 2, seed=11, max_range_m=sc["max_range_m"], **sc["cfg"]),
                             sc, g, om, ang, scan, p)
        e = engine_mod.Engine(max_particles=sc["n"], seed=11, max_range_m=sc["max_range_m"], **sc["cfg"])
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        e.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
        e.set_beam_angles(ang)
        e.set_particles(p, np.full(sc["n"], 1.0 / sc["n"]))
        for _ in range(sc["updates"]):
            e.stage_rays(scan) if sc["call"] == "stage_rays" else e.update(ACTION, scan)
        v = e.ray_kernel_variant()
        return dict(kernel=e.ray_kernel_name(), variant=(2 if v["hybrid"] else int(v["global_fields"]), int(v["turned_directions"]), int(v["pairs"])),
                    particles=e.get_particles(), logw=e.log_weights(), idx=e.resample_indices() if sc["call"] == "update" else None,
                    steps=e.ray_steps() if sc["cfg"].get("keep_ray_steps") else None, om=om, ang=ang, scan=scan)
    finally:
        e.close()


def run_group(grp, sc, g, om, ang, scan, p):
    """The same on a two-shard group of one device (sc["n"] particles in all): kernel and variant of the last shard's engine, particles
    and log-weights of the shards one behind the other"""
    try:
        grp.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
        grp.set_beam_angles(ang)
        grp.set_particles(p, np.full(sc["n"], 1.0 / sc["n"]))
        for _ in range(sc["updates"]):
            grp.update(ACTION, scan)
        e = grp.engine(grp.size - 1)
        v = e.ray_kernel_variant()
        return dict(kernel=e.ray_kernel_name(), variant=(2 if v["hybrid"] else int(v["global_fields"]), int(v["turned_directions"]), int(v["pairs"])),
                    particles=grp.get_particles(), logw=np.concatenate([grp.engine(i).log_weights() for i in range(grp.size)]),
                    idx=None, steps=None, om=om, ang=ang, scan=scan)
    finally:
        grp.close()


def launches(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"].split("(")[0].replace("void ", "").replace(" ", ""), int(r["Grid_Size_X"]), int(r["Workgroup_Size_X"]),
             int(r["LDS_Block_Size"])) for r in rows]


def compare(parent, change, legacy):
    a, b = launches(parent), launches(change)
    missing = [k for k in (REQUIRED_LEGACY if legacy else REQUIRED) if not any(k in row[0] for row in a)]
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    print(f"launches: parent {len(a)}, change {len(b)}; ordered lists {'equal' if first is None else f'DIFFER from dispatch {first}: {a[first:first + 1]} / {b[first:first + 1]}'}"
          f"; kernel forms not reached by the parent's trace: {missing or 'none'}")
    sys.exit(0 if first is None and not missing else 1)


def main():
    if sys.argv[1:2] == ["compare"]:
        compare(sys.argv[2], sys.argv[3], sys.argv[4:] == ["legacy"])
    from monte_carlo_localization_amd import engine
    from oracle import oracle as orc
    orc.build()
    legacy = sys.argv[1:] == ["legacy"]
    bad = 0
    for sc in SCENARIOS:
        if (sc["kernel"] in (QUAD, CELL)) != legacy:
            continue
        r = run(engine, orc, sc)
        h = hashlib.sha256()
        for a in (r["logw"], r["particles"], r["idx"], r["steps"]):
            if a is not None:
                h.update(np.ascontiguousarray(a).tobytes())
        reached = r["kernel"] == sc["kernel"] and (r["kernel"] != SWEEP or r["variant"] == sc["variant"])
        bad += not reached
        print(f"scenario {sc['name']:22s} n {sc['n']:6d} updates {sc['updates']} {r['kernel']:13s} variant {r['variant']} "
              f"{'reached' if reached else 'NOT REACHED: wanted ' + sc['kernel'] + ' ' + str(sc['variant'])} sha256 {h.hexdigest()}", flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
