#!/usr/bin/env python3
"""The global search over a scan sequence (mcl_global_search_sequence) on one MI355X, on the Spielberg map;
profiles/sequence_search.md is written from the parts.

  python tools/sequence_search.py timing [--out DIR] [--scans 3] [--stride 2] [--headings 72]
      ms per mcl_global_search_sequence over S scans of all 1081 beams (host wall around the call, which ends in its one host
      wait; median, minimum and maximum of REPS after WARMUP) and -- in the same process, alternating -- the only route to the
      same volume before: S mcl_global_search calls, S read-backs of the volume, the sum on the host.  Also S single searches
      alone, and, for the cost per scan, the score kernel alone (max_hits = 0: no sort, no hit read-back) for 1 ... S scans.
  python tools/sequence_search.py found [--out DIR] [--poses 20] [--particles 262144]
      the found-of-20 protocol of profiles/global_search.md (same map, same draws of the true poses, same particle count and engine
      seed): search (beam_stride 10) + refinement of the 16 hits on the anchor scan + mixture seed + 3 updates with the robot
      standing still, with S = 1, 2 and 4 scans taken half a metre apart along a straight drive that ends at the true pose; the
      odometry exact, and with noise of ODOM_SIGMA per half-metre step, accumulated.
  python tools/sequence_search.py report --out DIR
      profiles/sequence_search.md from DIR/seq_timing.json and DIR/seq_found.json

build/ is not tracked; the JSON parts go to build/sequence_search by default."""
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
STEP_M = 0.5
ODOM_SIGMA = (0.02, 0.02, 0.01)          # m, m, rad per half-metre step


def _world():
    from monte_carlo_localization_amd import maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    return m, synth.beam_angles(angle_step=1)


def _engine(n, m, ang, seed=42):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=n, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    e.set_likelihood_field()
    return e


def _stats(v):
    v = np.asarray(v, np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()), all=[float(x) for x in v])


def _drive(truth, S):
    """S poses half a metre apart on a straight line that ends at `truth`, oldest first"""
    c, s = np.cos(truth[2]), np.sin(truth[2])
    return np.array([[truth[0] - c * STEP_M * (S - 1 - i), truth[1] - s * STEP_M * (S - 1 - i), truth[2]] for i in range(S)])


def timing(args):
    from monte_carlo_localization_amd import engine
    m, ang = _world()
    S = args.scans
    e = _engine(64, m, ang)
    odom = _drive(np.zeros(3), S)
    scans = e.expected_scans(odom)                           # what the robot sees along the drive (the ray stage's cast)
    rel = engine.relative_poses(odom)
    f = dict(stride_cells=args.stride, n_headings=args.headings)
    one_bytes = None
    seq_ms, old_ms, three_ms, same = [], [], [], None
    for it in range(WARMUP + REPS):                          # alternating, same process, same box
        t0 = time.perf_counter()
        for s in range(S):
            e.global_search(scans[s], max_hits=16, **f)
        t1 = time.perf_counter()
        if one_bytes is None:
            one_bytes = e.search_bytes()
        total = None
        for s in range(S):
            # (the old route can only sum volumes of the SAME lattice poses: it answers the question for a robot that stood still)
            e.global_search(scans[s], max_hits=0, **f)
            v = e.search_scores()
            total = v if total is None else total + v
        t2 = time.perf_counter()
        hits, st = e.global_search_sequence(scans, rel, max_hits=16, **f)
        t3 = time.perf_counter()
        if it >= WARMUP:
            three_ms.append((t1 - t0) * 1e3)
            old_ms.append((t2 - t1) * 1e3)
            seq_ms.append((t3 - t2) * 1e3)
    # the identity on this lattice (SQ7), and that a still robot's sequence is the host's sum
    v1 = (e.global_search(scans[-1], max_hits=0, **f), e.search_scores())[1]
    v2 = (e.global_search_sequence(scans[-1:], np.zeros((1, 3)), max_hits=0, **f), e.search_scores())[1]
    same = bool(np.array_equal(v1.view(np.uint64), v2.view(np.uint64)))
    del v1, v2
    # the score kernel's cost per scan: no sort, no hit read-back
    single_score, seq_score = [], {n: [] for n in range(1, S + 1)}
    for it in range(WARMUP + REPS):
        t0 = time.perf_counter()
        e.global_search(scans[-1], max_hits=0, **f)
        t1 = time.perf_counter()
        if it >= WARMUP:
            single_score.append((t1 - t0) * 1e3)
        for n in range(1, S + 1):
            t0 = time.perf_counter()
            e.global_search_sequence(scans[S - n:], rel[S - n:], max_hits=0, **f)
            t1 = time.perf_counter()
            if it >= WARMUP:
                seq_score[n].append((t1 - t0) * 1e3)
    out = dict(map="Spielberg_map", scans=S, step_m=STEP_M, stride_cells=args.stride, n_headings=args.headings, n_positions=st["n_positions"],
               n_poses=st["n_poses"], beams=int(scans.shape[1]), used_beams=st["used_beams"], n_hits=st["n_hits"], warmup=WARMUP, reps=REPS,
               sequence_wall_ms=_stats(seq_ms), searches_readbacks_sum_wall_ms=_stats(old_ms), searches_alone_wall_ms=_stats(three_ms),
               single_count_only_wall_ms=_stats(single_score),
               sequence_count_only_wall_ms={str(n): _stats(v) for n, v in seq_score.items()},
               single_search_bytes=int(one_bytes), sequence_search_bytes=int(e.search_bytes()), identity_on_this_lattice=same,
               best_hit=[float(v) for v in hits[0]["pose"]] if len(hits) else None)
    print(json.dumps(out), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "seq_timing.json"), "w"), indent=1)


def _err(pose, truth):
    d = float(np.hypot(pose[0] - truth[0], pose[1] - truth[1]))
    a = float(abs((pose[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi))
    return d, a


ARMS = [(1, False), (2, False), (4, False), (2, True), (4, True)]        # (scans, noisy odometry)


def found(args):
    from monte_carlo_localization_amd import engine
    from oracle import oracle as orc
    orc.build()
    m, ang = _world()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    rng = np.random.default_rng(2024)                        # the draws of tools/global_search.py found
    noise = np.random.default_rng(77)
    grid = np.asarray(m.data)
    free = np.flatnonzero(grid.ravel() == 0)
    res = float(np.float32(m.resolution))
    H, W = grid.shape
    n = args.particles
    engines = {arm: _engine(n, m, ang, seed=7) for arm in ARMS}
    rows, still, Smax = [], (0.0, 0.0, 0.0), max(a[0] for a in ARMS)
    for i in range(args.poses):
        c = int(rng.choice(free))
        truth = np.array([m.origin_x + (c % W + rng.random()) * res, m.origin_y + (c // W + rng.random()) * res, rng.uniform(-np.pi, np.pi)])
        path = _drive(truth, Smax)
        scans = np.stack([orc.cast_many(om, np.full(ang.size, p[0]), np.full(ang.size, p[1]), p[2] + ang.astype(np.float64))[0]
                          for p in path]).astype(np.float32)
        col, row_ = np.floor((path[:, 0] - m.origin_x) / res).astype(int), np.floor((path[:, 1] - m.origin_y) / res).astype(int)
        inside = (col >= 0) & (col < W) & (row_ >= 0) & (row_ < H)
        on_free = [bool(inside[k] and grid[row_[k], col[k]] == 0) for k in range(Smax)]
        # odometry: the true steps plus noise per step, accumulated from the oldest pose on
        steps = noise.normal(0.0, ODOM_SIGMA, (Smax - 1, 3))
        noisy = [np.zeros(3)]
        for k in range(Smax - 1):
            p = noisy[-1]
            d = np.array([STEP_M, 0.0, 0.0]) + steps[k]
            noisy.append(np.array([p[0] + np.cos(p[2]) * d[0] - np.sin(p[2]) * d[1], p[1] + np.sin(p[2]) * d[0] + np.cos(p[2]) * d[1], p[2] + d[2]]))
        noisy = np.array(noisy)
        row = dict(truth=[float(v) for v in truth], path_on_free_cells=on_free, arms={})
        for arm in ARMS:
            S, is_noisy = arm
            e = engines[arm]
            odom = noisy[Smax - S:] if is_noisy else path[Smax - S:]
            rel = engine.relative_poses(odom)
            t0 = time.perf_counter()
            hits, st = e.global_search_sequence(scans[Smax - S:], rel, max_hits=16, beam_stride=10)
            ms = (time.perf_counter() - t0) * 1e3
            r = dict(used_beams=st["used_beams"], n_hits=st["n_hits"], search_wall_ms=ms, found=False)
            if len(hits):
                ref, _ = e.refine_poses(hits["pose"], scans[-1])
                e.init_particles_mixture(ref["mean"], ref["cov"], engine.seed_counts(ref["best_log_likelihood"], n))
                for _ in range(3):
                    e.update(still, scans[-1])
                d, t = _err(e.expected_pose(), truth)
                r.update(err_m=d, err_rad=t, found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD), best_hit_err=list(_err(hits[0]["pose"], truth)),
                         best_hit_near=bool(_err(hits[0]["pose"], truth)[0] < FOUND_XY_M and _err(hits[0]["pose"], truth)[1] < FOUND_TH_RAD),
                         any_hit_near=bool(any(_err(h["pose"], truth)[0] < FOUND_XY_M and _err(h["pose"], truth)[1] < FOUND_TH_RAD for h in hits)))
            row["arms"][f"{S}{'n' if is_noisy else ''}"] = r
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(map="Spielberg_map", particles=n, poses=args.poses, found_xy_m=FOUND_XY_M, found_th_rad=FOUND_TH_RAD, step_m=STEP_M,
               odom_sigma=list(ODOM_SIGMA), rows=rows)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "seq_found.json"), "w"), indent=1)


def report(args):
    t = json.load(open(os.path.join(args.out, "seq_timing.json")))
    f = json.load(open(os.path.join(args.out, "seq_found.json")))
    S = t["scans"]

    def ms(d):
        return f"{d['median']:.2f} ({d['min']:.2f} - {d['max']:.2f})"

    L = ["# Global search over a scan sequence on one MI355X (Spielberg map)", "",
         "Written by `tools/sequence_search.py report` from one `timing` and one `found` run; every number below is measured.  Commands:", "",
         "    python tools/sequence_search.py timing", "    python tools/sequence_search.py found", "    python tools/sequence_search.py report", "",
         "## Wall time", "",
         f"Lattice: stride {t['stride_cells']} cells, {t['n_headings']} headings: {t['n_positions']} positions, {t['n_poses']} poses.  {S} scans of "
         f"{t['beams']} beams ({t['used_beams']} used in all) taken {t['step_m']} m apart on a straight drive that ends at the map's origin pose.  "
         f"Host wall around the calls, median (minimum - maximum) of {t['reps']} after {t['warmup']}; the routes alternate in one process, and "
         "the spread between the repetitions is the run-to-run noise the differences below are read against.", "",
         "| route | ms |", "|---|---|",
         f"| `mcl_global_search_sequence`, {S} scans, 16 hits | {ms(t['sequence_wall_ms'])} |",
         f"| before: {S} x `mcl_global_search` (no hits), {S} read-backs of the volume, the sum in numpy | {ms(t['searches_readbacks_sum_wall_ms'])} |",
         f"| {S} x `mcl_global_search` alone, 16 hits each (no volume leaves the device, so no summed volume either) | {ms(t['searches_alone_wall_ms'])} |", "",
         "The score kernel alone (max_hits = 0: marking, but no sort and no hit read-back):", "",
         "| call | ms |", "|---|---|",
         f"| `mcl_global_search` | {ms(t['single_count_only_wall_ms'])} |"]
    for n in range(1, S + 1):
        L.append(f"| `mcl_global_search_sequence`, {n} scan{'s' if n > 1 else ''} | {ms(t['sequence_count_only_wall_ms'][str(n)])} |")
    c = t["sequence_count_only_wall_ms"]
    per_scan = (c[str(S)]["median"] - c["1"]["median"]) / (S - 1) if S > 1 else float("nan")
    L += ["", f"Each further scan costs {per_scan:.2f} ms; the single search's whole count-only call takes {t['single_count_only_wall_ms']['median']:.2f} ms.  "
          f"One scan at the anchor gives the single search's volume bit for bit on this lattice: {t['identity_on_this_lattice']}.", "",
          "## Memory", "",
          f"The search's buffers after the single searches: {t['single_search_bytes'] / 2**20:.1f} MiB; after the sequence searches: "
          f"{t['sequence_search_bytes'] / 2**20:.1f} MiB ({t['sequence_search_bytes'] - t['single_search_bytes']} bytes more: the beam lists of {S} scans, "
          "the offsets table, the list bounds).  The volume, the sort keys and the indices do not grow with the number of scans.", "",
          "## Is the robot found?", "",
          f"{f['poses']} random free poses (the draws, particle count {f['particles']} and engine seed of `profiles/global_search.md`); the scans are "
          f"cast by the oracle {f['step_m']} m apart along a straight drive that ends at the true pose, whether or not the earlier poses lie on free "
          "cells.  Search (beam_stride 10) + `mcl_refine_poses` of the 16 hits on the latest scan + mixture seed + 3 updates standing still; found = "
          f"expected pose within {f['found_xy_m']} m and {f['found_th_rad']} rad.  Noisy odometry: each {f['step_m']} m step off by N(0, "
          f"{f['odom_sigma'][0]} m) along and across and N(0, {f['odom_sigma'][2]} rad) in heading, accumulated.", "",
          "| scans | odometry | found | best hit near the truth | a hit near the truth | median search ms |", "|---|---|---|---|---|---|"]
    for key in f["rows"][0]["arms"]:
        arms = [r["arms"][key] for r in f["rows"]]
        L.append(f"| {key.rstrip('n')} | {'noisy' if key.endswith('n') else 'exact'} | **{sum(a['found'] for a in arms)} / {f['poses']}** | "
                 f"{sum(a.get('best_hit_near', False) for a in arms)} | {sum(a.get('any_hit_near', False) for a in arms)} | "
                 f"{float(np.median([a['search_wall_ms'] for a in arms])):.2f} |")
    off = sum(not all(r["path_on_free_cells"]) for r in f["rows"])
    L += ["", f"True poses whose drive of {len(f['rows'][0]['path_on_free_cells'])} poses leaves the free cells (the random pose faces a wall less "
          f"than {(len(f['rows'][0]['path_on_free_cells']) - 1) * f['step_m']} m behind it, or lies off the track): {off} / {f['poses']}; the oracle casts "
          "from such a pose all the same, and the scan it returns is what it is.", "",
          "## Reading", "",
          "- The counts are one run of one protocol, reported as they came; none is a threshold.  Compare the rows with one another: "
          "whether further scans raise the count in this protocol is read off the table, not assumed.  The draws are random free "
          "cells, many of them off the track, where every scan of the drive has few usable beams "
          "(`profiles/global_search.md`); a straight drive of a metre and a half in the same surroundings adds little that the "
          "last scan does not already hold.",
          "- `near` = within the found radius.  Where no hit is near the truth the refinement and the seed cannot recover it.", ""]
    open(os.path.join(ROOT, "profiles", "sequence_search.md"), "w").write("\n".join(L))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["timing", "found", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "sequence_search"))
    ap.add_argument("--scans", type=int, default=3)
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--headings", type=int, default=72)
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--particles", type=int, default=262144)
    args = ap.parse_args()
    dict(timing=timing, found=found, report=report)[args.part](args)


if __name__ == "__main__":
    main()
