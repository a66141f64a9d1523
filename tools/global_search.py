#!/usr/bin/env python3
"""The global search (mcl_global_search) on one MI355X, on the Spielberg map; profiles/global_search.md is
written from the parts.

  python tools/global_search.py timing [--out DIR] [--stride 2] [--headings 72]
      ms per search (host wall around the call, which ends in its one host wait; median of REPS after WARMUP) with beam_stride 1
      and 10 over the full 1081-beam scan, and -- in the same process, alternating -- what the engine offered before for the same
      question: a likelihood-field engine holding as many poses from mcl_init_global, one mcl_sensor_update (its k_lfield event
      time and the host wall).  ns per pose x used beam of both.
  python tools/global_search.py found [--out DIR] [--poses 20] [--particles 262144]
      for random free true poses with oracle-cast scans: is the robot found (expected pose within 0.5 m and 0.2 rad) after search
      (beam_stride 10) + seed (mixture of the 16 best hits) + 3 updates, and after mcl_init_global + 3 updates, at equal particle
      count, the robot standing still
  python tools/global_search.py report --out DIR
      profiles/global_search.md from DIR/gs_timing.json and DIR/gs_found.json
  python tools/global_search.py timing|found|report --refine [--out DIR]
      the same three parts for the pose refinement (mcl_refine_poses); profiles/pose_refine.md is written from them.
      timing: ms to refine the 16 best hits of a search at the default window (9 x 9 x 21 poses each) with all 1081 beams, and
      -- alternating, same process -- the route the engine offered before: the same window poses formed in numpy, scored by
      mcl_score_poses (one chunk of at most 65536), best pose / mean / covariance reduced in numpy.
      found: search + refine + seed (mixture of the refined means and covariances) + 3 updates against search + seed (the hits and
      a hand-picked covariance) + 3 updates, same poses, scans, particle count and engine seed as the plain `found`.

build/ is not tracked; the JSON parts go to build/global_search by default."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 2, 5
FOUND_XY_M, FOUND_TH_RAD = 0.5, 0.2


def _world():
    from monte_carlo_localization_amd import maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32).copy()
    return m, synth.beam_angles(angle_step=1), scan


def _engine(n, m, ang, seed=42):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=n, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    e.set_likelihood_field()
    return e


def _median(v):
    return float(np.median(np.asarray(v, np.float64)))


def timing(args):
    from monte_carlo_localization_amd import engine
    m, ang, scan = _world()
    cells, _ = engine.host_search_lattice(m.data, m.resolution, m.origin_x, m.origin_y, stride_cells=args.stride)
    n_poses = cells.size * args.headings
    s = _engine(64, m, ang)
    b = _engine(n_poses, m, ang)
    b.init_global(n_poses)
    out = dict(map="Spielberg_map", stride_cells=args.stride, n_headings=args.headings, n_positions=int(cells.size), n_poses=int(n_poses),
               beams=int(scan.size), warmup=WARMUP, reps=REPS, cases=[])
    for bs in (1, 10):
        masked = scan.copy()
        masked[np.arange(scan.size) % bs != 0] = np.nan
        search_ms, base_ms, base_kernel_ms, st = [], [], [], None
        for it in range(WARMUP + REPS):                      # alternating, same process, same box
            t0 = time.perf_counter()
            hits, st = s.global_search(scan, max_hits=16, stride_cells=args.stride, n_headings=args.headings, beam_stride=bs)
            t1 = time.perf_counter()
            b.sensor_update(masked)
            t2 = time.perf_counter()
            if it >= WARMUP:
                search_ms.append((t1 - t0) * 1e3)
                base_ms.append((t2 - t1) * 1e3)
                base_kernel_ms.append(float(b.ray_kernel_ms()))          # (the sensor stage's kernel: k_lfield here)
        t0 = time.perf_counter()
        s.global_search(scan, max_hits=0, stride_cells=args.stride, n_headings=args.headings, beam_stride=bs)
        count_only_ms = (time.perf_counter() - t0) * 1e3
        work = n_poses * st["used_beams"]
        out["cases"].append(dict(beam_stride=bs, used_beams=st["used_beams"], n_hits=st["n_hits"], device_bytes=st["device_bytes"],
                                 search_wall_ms=search_ms, search_wall_ms_median=_median(search_ms),
                                 search_count_only_wall_ms=count_only_ms,
                                 baseline_wall_ms=base_ms, baseline_wall_ms_median=_median(base_ms),
                                 baseline_lfield_event_ms=base_kernel_ms, baseline_lfield_event_ms_median=_median(base_kernel_ms),
                                 search_ns_per_pose_beam=_median(search_ms) * 1e6 / work,
                                 baseline_wall_ns_per_pose_beam=_median(base_ms) * 1e6 / work,
                                 baseline_lfield_ns_per_pose_beam=_median(base_kernel_ms) * 1e6 / work,
                                 best_hit=[float(v) for v in hits[0]["pose"]] if len(hits) else None))
        print(json.dumps(out["cases"][-1]), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "gs_timing.json"), "w"), indent=1)


def _err(pose, truth):
    d = float(np.hypot(pose[0] - truth[0], pose[1] - truth[1]))
    a = float(abs((pose[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi))
    return d, a


def found(args):
    from monte_carlo_localization_amd import engine
    from oracle import oracle as orc
    orc.build()
    m, ang, _ = _world()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    rng = np.random.default_rng(2024)
    free = np.flatnonzero(np.asarray(m.data).ravel() == 0)
    res = float(np.float32(m.resolution))
    W = m.data.shape[1]
    n = args.particles
    a, g = _engine(n, m, ang, seed=7), _engine(n, m, ang, seed=7)
    rows = []
    still = (0.0, 0.0, 0.0)
    for i in range(args.poses):
        c = int(rng.choice(free))
        truth = np.array([m.origin_x + (c % W + rng.random()) * res, m.origin_y + (c // W + rng.random()) * res, rng.uniform(-np.pi, np.pi)])
        dirs = truth[2] + ang.astype(np.float64)
        scan = orc.cast_many(om, np.full(dirs.size, truth[0]), np.full(dirs.size, truth[1]), dirs)[0].astype(np.float32)
        t0 = time.perf_counter()
        hits, st = a.global_search(scan, max_hits=16, beam_stride=10)
        search_ms = (time.perf_counter() - t0) * 1e3
        row = dict(truth=[float(v) for v in truth], used_beams=st["used_beams"], n_hits=st["n_hits"], search_wall_ms=search_ms)
        if len(hits):
            counts = engine.seed_counts(hits["log_likelihood"], n)
            step = 2 * res
            a.init_particles_mixture(hits["pose"], np.diag([step * step, step * step, (2 * np.pi / 72) ** 2]), counts)
            for _ in range(3):
                a.update(still, scan)
            d, t = _err(a.expected_pose(), truth)
            row.update(search_err_m=d, search_err_rad=t, search_found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD),
                       best_hit_err=list(_err(hits[0]["pose"], truth)))
        else:
            row.update(search_found=False)
        g.init_global(n)
        for _ in range(3):
            g.update(still, scan)
        d, t = _err(g.expected_pose(), truth)
        row.update(global_err_m=d, global_err_rad=t, global_found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(map="Spielberg_map", particles=n, poses=args.poses, found_xy_m=FOUND_XY_M, found_th_rad=FOUND_TH_RAD, rows=rows,
               search_found=sum(r["search_found"] for r in rows), global_found=sum(r["global_found"] for r in rows))
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "gs_found.json"), "w"), indent=1)


def _numpy_refine(e, seeds, scan, res, half_xy=4, half_theta=10, step_xy_cells=0.5, step_theta_rad=np.pi / 360):
    """What a host had to do for the refinement's answer before mcl_refine_poses: the window in numpy (rule R1), mcl_score_poses in
    chunks, the best pose (R3), mean and covariance (R4) in numpy.  Returns (best, mean, cov) per seed."""
    ax, at = np.arange(-half_xy, half_xy + 1), np.arange(-half_theta, half_theta + 1)
    dt, dy, dx = (v.ravel() for v in np.meshgrid(at, ax, ax, indexing="ij"))
    d = np.stack([dx, dy, dt], axis=1)
    step = np.array([step_xy_cells * res, step_xy_cells * res, step_theta_rad])
    poses = (np.asarray(seeds, np.float64)[:, None, :] + d[None].astype(np.float64) * step).reshape(-1, 3)
    ll = np.concatenate([e.score_poses(poses[s:s + 65536], scan)["log_likelihood"] for s in range(0, len(poses), 65536)])
    V = ll.reshape(len(seeds), -1)
    q = (d * d).sum(axis=1)
    out = []
    for m in range(len(seeds)):
        wb = np.lexsort((np.arange(q.size), q, -V[m]))[0]
        w = np.exp(V[m] - V[m, wb]) if np.isfinite(V[m, wb]) else np.zeros(q.size)
        S = w.sum()
        u = (d - d[wb]).astype(np.float64)
        mu = (w[:, None] * u).sum(axis=0) / S if S > 0 else np.zeros(3)
        Cm = (w[:, None, None] * u[:, :, None] * u[:, None, :]).sum(axis=0) / S - np.outer(mu, mu) if S > 0 else np.zeros((3, 3))
        best = poses[m * q.size + wb]
        out.append((best, best + step * mu, np.outer(step, step) * Cm + np.diag(step * step / 12.0)))
    return out


def refine_timing(args):
    m, ang, scan = _world()
    res = float(np.float32(m.resolution))
    e = _engine(64, m, ang)
    hits, _ = e.global_search(scan, max_hits=16, stride_cells=args.stride, n_headings=args.headings, beam_stride=10)
    seeds = hits["pose"].copy()
    refine_ms, numpy_ms, st = [], [], None
    for it in range(WARMUP + REPS):                          # alternating, same process, same box
        t0 = time.perf_counter()
        r, st = e.refine_poses(seeds, scan)
        t1 = time.perf_counter()
        ref = _numpy_refine(e, seeds, scan, res)
        t2 = time.perf_counter()
        if it >= WARMUP:
            refine_ms.append((t1 - t0) * 1e3)
            numpy_ms.append((t2 - t1) * 1e3)
    agree = all(np.array_equal(r[i]["best"], ref[i][0]) for i in range(len(seeds)))
    out = dict(map="Spielberg_map", beams=int(scan.size), seeds=int(len(seeds)), warmup=WARMUP, reps=REPS, n_win=st["n_win"],
               n_poses=st["n_poses"], used_beams=st["used_beams"], device_bytes=st["device_bytes"], refine_wall_ms=refine_ms,
               refine_wall_ms_median=_median(refine_ms), numpy_route_wall_ms=numpy_ms, numpy_route_wall_ms_median=_median(numpy_ms),
               refine_ns_per_pose_beam=_median(refine_ms) * 1e6 / (st["n_poses"] * st["used_beams"]), same_best_pose=bool(agree),
               max_mean_diff=float(max(np.abs(r[i]["mean"] - ref[i][1]).max() for i in range(len(seeds)))),
               weight_sums=[float(v) for v in r["weight_sum"]])
    print(json.dumps(out), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "gs_refine_timing.json"), "w"), indent=1)


def refine_found(args):
    """`found` with a second engine that refines the hits before it seeds; the poses, scans and hits are the same"""
    from monte_carlo_localization_amd import engine
    from oracle import oracle as orc
    orc.build()
    m, ang, _ = _world()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    rng = np.random.default_rng(2024)
    free = np.flatnonzero(np.asarray(m.data).ravel() == 0)
    res = float(np.float32(m.resolution))
    W = m.data.shape[1]
    n = args.particles
    a, b = _engine(n, m, ang, seed=7), _engine(n, m, ang, seed=7)
    rows = []
    still = (0.0, 0.0, 0.0)
    for i in range(args.poses):
        c = int(rng.choice(free))
        truth = np.array([m.origin_x + (c % W + rng.random()) * res, m.origin_y + (c // W + rng.random()) * res, rng.uniform(-np.pi, np.pi)])
        dirs = truth[2] + ang.astype(np.float64)
        scan = orc.cast_many(om, np.full(dirs.size, truth[0]), np.full(dirs.size, truth[1]), dirs)[0].astype(np.float32)
        hits, st = a.global_search(scan, max_hits=16, beam_stride=10)
        row = dict(truth=[float(v) for v in truth], used_beams=st["used_beams"], n_hits=st["n_hits"], search_found=False, refine_found=False)
        if len(hits):
            step = 2 * res
            a.init_particles_mixture(hits["pose"], np.diag([step * step, step * step, (2 * np.pi / 72) ** 2]),
                                     engine.seed_counts(hits["log_likelihood"], n))
            t0 = time.perf_counter()
            r, rst = b.refine_poses(hits["pose"], scan)
            refine_ms = (time.perf_counter() - t0) * 1e3
            b.init_particles_mixture(r["mean"], r["cov"], engine.seed_counts(r["best_log_likelihood"], n))
            for _ in range(3):
                a.update(still, scan)
                b.update(still, scan)
            d, t = _err(a.expected_pose(), truth)
            row.update(search_err_m=d, search_err_rad=t, search_found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD),
                       best_hit_err=list(_err(hits[0]["pose"], truth)))
            d, t = _err(b.expected_pose(), truth)
            k = int(np.argmax(r["best_log_likelihood"]))
            row.update(refine_err_m=d, refine_err_rad=t, refine_found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD), refine_wall_ms=refine_ms,
                       best_refined_err=list(_err(r[k]["best"], truth)), refined_of_best_hit_err=list(_err(r[0]["best"], truth)),
                       used_beams_refine=rst["used_beams"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(map="Spielberg_map", particles=n, poses=args.poses, found_xy_m=FOUND_XY_M, found_th_rad=FOUND_TH_RAD, rows=rows,
               search_found=sum(r["search_found"] for r in rows), refine_found=sum(r["refine_found"] for r in rows))
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "gs_refine_found.json"), "w"), indent=1)


def refine_report(args):
    t = json.load(open(os.path.join(args.out, "gs_refine_timing.json")))
    f = json.load(open(os.path.join(args.out, "gs_refine_found.json")))
    both = [r for r in f["rows"] if "refine_err_m" in r]
    L = ["# Pose refinement on one MI355X (Spielberg map)", "",
         "Written by `tools/global_search.py report --refine` from one `timing --refine` and one `found --refine` run; every number "
         "below is measured.  Commands:", "",
         "    python tools/global_search.py timing --refine", "    python tools/global_search.py found --refine",
         "    python tools/global_search.py report --refine", "",
         "## Wall time", "",
         f"{t['seeds']} seeds (the best hits of a default search with beam_stride 10) x the default window of {t['n_win']} poses = "
         f"{t['n_poses']} poses, {t['beams']}-beam scan ({t['used_beams']} used beams).  Host wall around the call, median of {t['reps']} "
         f"after {t['warmup']}, both routes alternating in one process.", "",
         "| route | ms |", "|---|---|",
         f"| `mcl_refine_poses` (seed upload, score kernel, reduction kernel, {t['seeds']} records back, its one host wait) | {t['refine_wall_ms_median']:.3f} |",
         f"| before: the window in numpy, `mcl_score_poses` (one chunk), best / mean / covariance in numpy | {t['numpy_route_wall_ms_median']:.3f} |", "",
         f"`mcl_refine_poses`: {t['refine_ns_per_pose_beam']:.5f} ns per pose·beam; {t['device_bytes'] / 2**10:.0f} KiB of device buffers.  "
         f"Both routes name the same best pose for every seed: {t['same_best_pose']}; largest difference of a mean component: "
         f"{t['max_mean_diff']:.3g}.  `mcl_score_poses` also casts the expected scan of every pose for its agreement counts, which the "
         "refinement does not need.", "",
         "## Is the robot found?", "",
         f"{f['poses']} random free poses (the poses, scans and engine seed of `profiles/global_search.md`), the robot standing still, "
         f"{f['particles']} particles; found = expected pose within {f['found_xy_m']} m and {f['found_th_rad']} rad after 3 updates.", "",
         f"- search (beam_stride 10) + mixture of the 16 best hits with a hand-picked covariance + 3 updates: **{f['search_found']} / {f['poses']}**",
         f"- search + `mcl_refine_poses` of the 16 hits (default window, every beam) + mixture of the refined means and covariances, "
         f"counts from the refined scores + 3 updates: **{f['refine_found']} / {f['poses']}**"]
    near = [r for r in both if r["best_hit_err"][0] < f["found_xy_m"] and r["best_hit_err"][1] < f["found_th_rad"]]
    if both:
        L += [f"- refinement wall per pose: median {_median([r['refine_wall_ms'] for r in both]):.3f} ms",
              f"- poses where the best hit was already within {f['found_xy_m']} m and {f['found_th_rad']} rad: {len(near)} / {len(both)}"]
        L += [f"  - truth ({r['truth'][0]:.1f}, {r['truth'][1]:.1f}): the best hit {r['best_hit_err'][0]:.3f} m, {r['best_hit_err'][1]:.4f} rad off; "
              f"its refined best pose {r['refined_of_best_hit_err'][0]:.3f} m, {r['refined_of_best_hit_err'][1]:.4f} rad off" for r in near]
    L += ["", "## Reading", "",
          "- Neither figure is a threshold.  The refinement can only sharpen a hit that is near the true pose: where none of the 16 "
          "hits is, it sharpens a wrong one.  The found rate is a property of search + seed on ONE scan of a standing robot, not of "
          "the kernels.",
          "- The refined scores use every beam and the search's every tenth, so `seed_counts` concentrates the cloud on fewer "
          "components after the refinement.", ""]
    open(os.path.join(ROOT, "profiles", "pose_refine.md"), "w").write("\n".join(L))


def report(args):
    t = json.load(open(os.path.join(args.out, "gs_timing.json")))
    f = json.load(open(os.path.join(args.out, "gs_found.json")))
    L = ["# Global search on one MI355X (Spielberg map)", "",
         "Written by `tools/global_search.py report` from one `timing` and one `found` run; every number below is measured.", "",
         f"Lattice: stride {t['stride_cells']} cells, {t['n_headings']} headings: {t['n_positions']} positions, {t['n_poses']} poses; "
         f"{t['beams']}-beam scan.  Search: host wall around `mcl_global_search` (16 hits; score kernel, candidate marking, sort of "
         f"the whole volume, read-back, its one host wait), median of {t['reps']} after {t['warmup']}.  Before: a likelihood-field "
         "engine holding as many poses from `mcl_init_global`, one `mcl_sensor_update` of the same readings (host wall, and the "
         "event time of `k_lfield` alone).  Both in one process, alternating.", "",
         "| beam_stride | used beams | search ms | search, count only ms | sensor_update ms | k_lfield ms | search ns / pose·beam | k_lfield ns / pose·beam | local maxima |",
         "|---|---|---|---|---|---|---|---|---|"]
    for c in t["cases"]:
        L.append(f"| {c['beam_stride']} | {c['used_beams']} | {c['search_wall_ms_median']:.2f} | {c['search_count_only_wall_ms']:.2f} | "
                 f"{c['baseline_wall_ms_median']:.2f} | {c['baseline_lfield_event_ms_median']:.2f} | {c['search_ns_per_pose_beam']:.5f} | "
                 f"{c['baseline_lfield_ns_per_pose_beam']:.5f} | {c['n_hits']} |")
    L += ["", f"Device memory of the search's buffers: {t['cases'][0]['device_bytes'] / 2**20:.0f} MiB.", "",
          "## Is the robot found?", "",
          f"{f['poses']} random free poses, oracle-cast 1081-beam scans, the robot standing still, {f['particles']} particles; found = expected "
          f"pose within {f['found_xy_m']} m and {f['found_th_rad']} rad after 3 updates.", "",
          f"- search (beam_stride 10) + mixture of the 16 best hits + 3 updates: **{f['search_found']} / {f['poses']}**",
          f"- `mcl_init_global` + 3 updates: **{f['global_found']} / {f['poses']}**",
          f"- search wall per pose: median {_median([r['search_wall_ms'] for r in f['rows']]):.2f} ms",
          f"- true poses whose scan has fewer than 40 usable beams of the {t['beams'] // 10 + 1} candidates (most readings at max range; "
          f"free cells off the track are drawn too): {sum(r['used_beams'] < 40 for r in f['rows'])} / {f['poses']}, "
          f"found by the search among them: {sum(r['search_found'] for r in f['rows'] if r['used_beams'] < 40)}", "",
          "## Reading", "",
          "- Per pose·beam the lattice kernel is several times faster than `k_lfield` on a uniform cloud of the same size (the table: "
          "search wall, which includes marking, sort and read-back, against `k_lfield`'s event time alone).  `search, count only` "
          "(max_hits = 0: no sort, no hit read-back) is one call, not a median; the difference to the full search is the sort of the "
          "whole volume and the copies.",
          "- With beam_stride 10 the per-pose·beam figure is worse than with every beam: the marking pass, the sort and the fixed "
          "costs do not shrink with the beams.",
          "- The found rate says how often search + seed localises from ONE scan with the robot standing still; it is not a property "
          "of the kernel.  A true pose is generally not a lattice pose, and a scan with few usable beams fits many poses.", ""]
    open(os.path.join(ROOT, "profiles", "global_search.md"), "w").write("\n".join(L))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["timing", "found", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "global_search"))
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--headings", type=int, default=72)
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--particles", type=int, default=262144)
    ap.add_argument("--refine", action="store_true", help="the part for the pose refinement (profiles/pose_refine.md)")
    args = ap.parse_args()
    parts = dict(timing=refine_timing, found=refine_found, report=refine_report) if args.refine else dict(timing=timing, found=found, report=report)
    parts[args.part](args)


if __name__ == "__main__":
    main()
