#!/usr/bin/env python3
"""Measurements behind profiles/odometry_motion.md, one GPU.

usage: tools/odometry_motion.py [--quick] [--out FILE.json]

1. stage 0 (resampling + motion) and the whole update at 4M x 1081, 262 144 x 1081 and 2000 x 61 for the REFERENCE, DIFF and
   OMNI models (median of the timed updates).  MCL_LIB=<another build of the library> measures that build's REFERENCE model (the
   parent commit's, for the comparison); models the loaded library does not have are left out.
2. the closed loop of tests/test_gpu_motion_model.py at 1M x 1081: per-step tracking error of the three models.
3. a standing robot (zero action, 50 updates, 65 536 particles) with floors 0 and (0.005 m, 0.005 rad): distinct poses left."""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from monte_carlo_localization_amd import engine, maps, synth  # noqa: E402


def make(m, ang, n, **cfg):
    e = engine.Engine(max_particles=n, **cfg)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    return e


def timings(m, scan_full, n, step, model, warm, reps):
    ang = synth.beam_angles(angle_step=step)
    e = make(m, ang, n, seed=5)
    e.init_particles_pose((0.0, 0.0, 0.0), n)
    if model != "reference":
        e.set_motion_model(model)
    scan = scan_full[::step].copy()
    t0, tot = [], []
    for k in range(warm + reps):
        e.update((0.1, 0.0, 0.02), scan)
        if k >= warm:
            t = e.stage_timings()
            t0.append(t[0]); tot.append(t[5])
    e.close()
    return dict(n=n, beams=int(ang.size), model=model, stage0_ms=float(np.median(t0)), update_ms=float(np.median(tot)))


def closed_loop(m, n, model):
    import motion_ref as mr
    from oracle import oracle as orc
    orc.build()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    ang = synth.beam_angles()
    a64 = ang.astype(np.float64)
    e = make(m, ang, n, seed=11)
    truth = np.zeros((3, 1))
    e.init_particles_gaussian((0.0, 0.0, 0.0), np.diag([0.25, 0.25, 0.16]), n)
    if model != "reference":
        e.set_motion_model(model)
    errs = []
    for k in range(60):
        act = (0.1, 0.02 if model == "omni" else 0.0, 0.015 if k < 20 else (-0.015 if k < 40 else 0.02))
        truth = mr.compose(act, truth)
        x, y, th = truth[:, 0]
        scan, _ = orc.cast_many(om, np.full(a64.size, x), np.full(a64.size, y), th + a64)
        e.update((act[0], 0.0, act[2]) if model == "reference" else act, np.asarray(scan, np.float32))
        pose = e.expected_pose()
        errs.append(math.hypot(pose[0] - x, pose[1] - y))
    e.close()
    return dict(model=model, n=n, err_m=[round(v, 4) for v in errs])


def standing(m, scan_full, floors):
    n, ang = 65536, synth.beam_angles()
    e = make(m, ang, n, seed=3)
    e.init_particles_gaussian((0.0, 0.0, 0.0), np.diag([0.04, 0.04, 0.01]), n)
    e.set_motion_model("diff", floor_trans_m=floors[0], floor_rot_rad=floors[1])
    left = []
    for k in range(50):
        e.update((0.0, 0.0, 0.0), scan_full)
        if k in (0, 9, 49):
            left.append(int(np.unique(e.get_particles(), axis=1).shape[1]))
    e.close()
    return dict(floors=floors, distinct_after_1_10_50=left)


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    have_odo = hasattr(engine.load_library(), "mcl_set_motion_model")
    models = ("reference", "diff", "omni") if have_odo else ("reference",)
    res = dict(lib=engine.LIB_PATH, timings=[], loop=[], standing=[])
    for n, step in ((1 << 22, 1), (262144, 1), (2000, 18)):
        for model in models:
            r = timings(m, scan, n, step, model, 3, 5 if quick else 20)
            print(json.dumps(r), flush=True)
            res["timings"].append(r)
    if have_odo:
        for model in models:
            r = closed_loop(m, 1 << 20, model)
            print(json.dumps(dict(model=model, final=r["err_m"][-1], worst=max(r["err_m"]), mean=round(float(np.mean(r["err_m"])), 4))), flush=True)
            res["loop"].append(r)
        for floors in ((0.0, 0.0), (0.005, 0.005)):
            r = standing(m, scan, floors)
            print(json.dumps(r), flush=True)
            res["standing"].append(r)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
