#!/usr/bin/env python3
"""The refinement over a scan sequence (mcl_refine_poses_sequence) on one MI355X, on Spielberg with the Hokuyo's
1081 beams.  Writes profiles/sequence_refine.md from two parts.

Timing: the set-up of profiles/pruned_sequence_search.md -- scans half a metre apart on a straight drive that ends at the map's
origin pose, the 16 hits of mcl_global_search_sequence_pruned as seeds, the default window (9 x 9 x 21), warm.  Three routes to
the summed volume, timed in one process, (a) and (b) alternating:

  (a) one refine_poses_sequence call
  (b) S calls of refine_poses on the same seeds, one per scan: the single-scan kernel doing the same per-beam work (the yardstick
      for cost; its records are NOT the sequence's: each call scores its scan as if it were taken at the anchor)
  (c) the only earlier route to the same records: score_poses over RS2's poses in chunks of 65536, a host fold, host_refine_reduce

with three scans, with six, and with every tenth beam; every row on an engine of its own, so that its bytes are that row's alone.

Found: the found-of-20 protocol of profiles/global_search.md as tools/sequence_search.py runs it over a sequence (same map, same
draws of the true poses, same particle count and engine seed, scans cast by the oracle half a metre apart along a straight drive
that ends at the true pose, exact odometry): search (mcl_global_search_sequence_pruned, beam_stride 10, 16 hits) + refinement +
mixture seed + 3 updates standing still, with the refinement on the anchor scan alone (mcl_refine_poses) beside the refinement
over the sequence (mcl_refine_poses_sequence), for 2, 3 and 4 scans.

  python tools/sequence_refine.py [--reps 20] [--warmup 3] [--poses 20] [--particles 262144] [--out FILE] [--json FILE]

Host wall time around calls that end in their own host wait, median (minimum - maximum).  Nothing here is a pass/fail number."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_M = 0.5
FOUND_XY_M, FOUND_TH_RAD = 0.5, 0.2
FOUND_SCANS = (2, 3, 4)


def stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def drive(truth, S):
    """S poses half a metre apart on a straight line that ends at `truth`, oldest first (tools/sequence_search.py)"""
    c, s = np.cos(truth[2]), np.sin(truth[2])
    return np.array([[truth[0] - c * STEP_M * (S - 1 - i), truth[1] - s * STEP_M * (S - 1 - i), truth[2]] for i in range(S)])


def world():
    from monte_carlo_localization_amd import maps, synth
    return maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz")), synth.beam_angles(angle_step=1)


def make_engine(n, m, ang, seed=42):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=n, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    e.set_likelihood_field()
    return e


def route_c(engine, e, res, seeds, scans, rel, beam_stride):
    """the volume and the records from score_poses at RS2's poses"""
    off = engine.host_refine_sequence_offsets(seeds, rel)
    nx = 2 * engine.default_refine_config().half_xy + 1
    out = np.zeros(len(seeds), engine.REFINE_DTYPE)
    masked = np.array(scans, np.float32)
    masked[:, np.arange(masked.shape[1]) % beam_stride != 0] = np.nan
    win = np.concatenate([engine.host_refine_window(s, res) for s in seeds])
    n_win = len(win) // len(seeds)
    it = (np.arange(len(win)) % n_win) // (nx * nx)
    m = np.arange(len(win)) // n_win
    total = np.zeros(len(win))
    for s in range(len(scans)):
        poses = np.stack([win[:, 0] + off[m, it, s, 0], win[:, 1] + off[m, it, s, 1], off[m, it, s, 2]], axis=1)
        acc = np.concatenate([e.score_poses(poses[k:k + 65536], masked[s])["log_likelihood"] for k in range(0, len(poses), 65536)])
        total = total + acc
    vol = total.reshape(len(seeds), n_win)
    for k, seed in enumerate(seeds):
        out[k] = engine.host_refine_reduce(seed, res, vol[k])
    return out, vol


def timing(reps, warmup):
    from monte_carlo_localization_amd import engine
    m, ang = world()
    sc = engine.default_search_config()
    rows = []
    for S, beam_stride in ((3, 1), (6, 1), (3, 10)):
        e = make_engine(64, m, ang)                           # an engine per row: its refine_bytes are this row's alone
        odom = drive(np.zeros(3), S)
        scans = e.expected_scans(odom)
        rel = engine.relative_poses(odom)
        hits, _ = e.global_search_sequence_pruned(scans, rel, max_hits=16, beam_stride=beam_stride)
        seeds = hits["pose"]
        a = lambda: e.refine_poses_sequence(seeds, scans, rel, beam_stride=beam_stride)
        b = lambda: [e.refine_poses(seeds, scans[s], beam_stride=beam_stride) for s in range(S)]
        for _ in range(warmup):
            a(), b()
        ta, tb = [], []
        for _ in range(reps):                                 # alternating
            t = time.perf_counter(); a(); ta.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); b(); tb.append((time.perf_counter() - t) * 1e3)
        tc = []
        for _ in range(max(3, reps // 4)):
            t = time.perf_counter(); rc, vc = route_c(engine, e, m.resolution, seeds, scans, rel, beam_stride); tc.append((time.perf_counter() - t) * 1e3)
        ra, st = a()
        va = e.refine_scores()
        same = bool(np.array_equal(va.view(np.uint64), vc.view(np.uint64)) and
                    all(np.array_equal(ra[k], rc[k]) for k in ("best", "best_log_likelihood", "seed_log_likelihood", "best_index")))
        rows.append(dict(scans=S, beam_stride=beam_stride, seeds=len(seeds), n_win=st["n_win"], n_poses=st["n_poses"], used_beams=st["used_beams"],
                         stride_cells=int(sc.stride_cells), n_headings=int(sc.n_headings), a=stats(ta), b=stats(tb), c=stats(tc),
                         bytes=e.refine_bytes(), identical=same))
        print(json.dumps(rows[-1]), flush=True)
        e.close()
    return rows


def err(pose, truth):
    d = float(np.hypot(pose[0] - truth[0], pose[1] - truth[1]))
    a = float(abs((pose[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi))
    return d, a


def near(pose, truth):
    d, a = err(pose, truth)
    return bool(d < FOUND_XY_M and a < FOUND_TH_RAD)


def found(n_poses, n):
    from monte_carlo_localization_amd import engine
    from oracle import oracle as orc
    orc.build()
    m, ang = world()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    rng = np.random.default_rng(2024)                        # the draws of tools/global_search.py found
    free = np.flatnonzero(np.asarray(m.data).ravel() == 0)
    res = float(np.float32(m.resolution))
    W = np.asarray(m.data).shape[1]
    Smax = max(FOUND_SCANS)
    engines = {(S, chain): make_engine(n, m, ang, seed=7) for S in FOUND_SCANS for chain in ("anchor", "sequence")}
    rows, still = [], (0.0, 0.0, 0.0)
    for i in range(n_poses):
        c = int(rng.choice(free))
        truth = np.array([m.origin_x + (c % W + rng.random()) * res, m.origin_y + (c // W + rng.random()) * res, rng.uniform(-np.pi, np.pi)])
        path = drive(truth, Smax)
        scans = np.stack([orc.cast_many(om, np.full(ang.size, p[0]), np.full(ang.size, p[1]), p[2] + ang.astype(np.float64))[0]
                          for p in path]).astype(np.float32)
        row = dict(truth=[float(v) for v in truth], arms={})
        for S in FOUND_SCANS:
            rel = engine.relative_poses(path[Smax - S:])
            sub = scans[Smax - S:]
            for chain in ("anchor", "sequence"):
                e = engines[(S, chain)]
                hits, st = e.global_search_sequence_pruned(sub, rel, max_hits=16, beam_stride=10)
                r = dict(n_hits=int(len(hits)), used_beams=st["used_beams"], found=False, any_hit_near=False, top_component_near=False)
                if len(hits):
                    t0 = time.perf_counter()
                    ref, _ = e.refine_poses(hits["pose"], sub[-1]) if chain == "anchor" else e.refine_poses_sequence(hits["pose"], sub, rel)
                    r["refine_wall_ms"] = (time.perf_counter() - t0) * 1e3
                    counts = engine.seed_counts(ref["best_log_likelihood"], n)
                    e.init_particles_mixture(ref["mean"], ref["cov"], counts)
                    for _ in range(3):
                        e.update(still, sub[-1])
                    k = int(np.argmax(counts))
                    d, t = err(e.expected_pose(), truth)
                    r.update(err_m=d, err_rad=t, found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD), any_hit_near=any(near(h["pose"], truth) for h in hits),
                             top_component_near=near(ref[k]["best"], truth), components_seeded=int((counts > 0).sum()))
                row["arms"][f"{S} {chain}"] = r
        rows.append(row)
        print(json.dumps(row), flush=True)
    for e in engines.values():
        e.close()
    return dict(particles=n, poses=n_poses, rows=rows)


def measuring_flags(argv):
    """the command line without --out / --json and their values: where the files go changes no figure"""
    keep, skip = [], False
    for a in argv:
        if skip:
            skip = False
        elif a in ("--out", "--json"):
            skip = True
        elif not a.startswith(("--out=", "--json=")):
            keep.append(a)
    return keep


def report(rows, f, reps, warmup, out):
    def ms(d):
        return f"{d['median']:.2f} ({d['min']:.2f} - {d['max']:.2f})"

    r0 = rows[0]
    L = ["# The refinement over a scan sequence beside the single-scan one, on one MI355X", "",
         "Written by `tools/sequence_refine.py`; every number below is measured.  Command:", "",
         "    python " + " ".join(["tools/sequence_refine.py"] + measuring_flags(sys.argv[1:])), "",
         "## Wall time", "",
         f"Spielberg, 1081 beams, the {r0['seeds']} hits of `mcl_global_search_sequence_pruned` (stride {r0['stride_cells']} x {r0['n_headings']} headings) "
         f"as seeds, the default window ({r0['n_win']} poses a seed, {r0['n_poses']} in all).  The scans are taken {STEP_M} m apart on a straight drive "
         "that ends at the map's origin pose (the set-up of `profiles/pruned_sequence_search.md`).  Host wall time around calls that end in their own "
         f"host wait, median (minimum - maximum) of {reps} after {warmup} warm calls, (a) and (b) alternating in one process; (c) {max(3, reps // 4)} "
         "times.  (a) one `mcl_refine_poses_sequence`; (b) S calls of `mcl_refine_poses`, one per scan -- the same per-beam work by the single-scan "
         "kernel, not the same records; (c) `mcl_score_poses` over RS2's poses in chunks of 65536, a host fold, `mcl_host_refine_reduce` -- the only "
         "earlier route to the same records.  KiB is `mcl_get_refine_bytes` of the row's own engine, which made these calls alone.  Nothing here is a "
         "pass/fail number.", "",
         "| scans | beam_stride | beams used | (a) ms | (b) ms | (c) ms | refine KiB | (a) = (c) bit for bit |", "|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        L.append(f"| {r['scans']} | {r['beam_stride']} | {r['used_beams']} | {ms(r['a'])} | {ms(r['b'])} | {ms(r['c'])} | {r['bytes'] / 2**10:.0f} | "
                 f"{'yes' if r['identical'] else 'NO'} |")
    L.append("")
    for r in rows:
        spread = r["b"]["max"] - r["b"]["min"]
        over = r["a"]["median"] - r["b"]["median"]
        L.append(f"- {r['scans']} scans, beam_stride {r['beam_stride']}: (a) - (b) = {over:+.2f} ms at the medians; the run-to-run spread of (b) "
                 f"(maximum - minimum) is {spread:.2f} ms.  " + ("(a) does not exceed (b) beyond that spread." if over <= spread else
                                                                  "(a) EXCEEDS (b) by more than that spread."))
    if f:
        L += ["", "## Is the robot found?", "",
              f"{f['poses']} random free poses (the draws, particle count {f['particles']} and engine seed of `profiles/global_search.md`); the scans are cast "
              f"by the oracle {STEP_M} m apart along a straight drive that ends at the true pose, exact odometry (`tools/sequence_search.py`'s protocol).  "
              "`mcl_global_search_sequence_pruned` (beam_stride 10, 16 hits) + refinement of the hits at the default window with every beam + mixture "
              f"seed by `seed_counts` + 3 updates standing still; found = expected pose within {FOUND_XY_M} m and {FOUND_TH_RAD} rad.  Anchor: "
              "`mcl_refine_poses` on the latest scan, the chain documented before; sequence: `mcl_refine_poses_sequence` on all scans.  Both chains "
              "get the same hits.", "",
              "| scans | refinement | found | a hit near the truth | the component with most particles near the truth | median components seeded | "
              "median refinement ms |", "|---:|---|---|---:|---:|---:|---:|"]
        for key in f["rows"][0]["arms"]:
            arms = [r["arms"][key] for r in f["rows"]]
            S, chain = key.split()
            L.append(f"| {S} | {chain} | **{sum(a['found'] for a in arms)} / {f['poses']}** | {sum(a['any_hit_near'] for a in arms)} | "
                     f"{sum(a['top_component_near'] for a in arms)} | {float(np.median([a.get('components_seeded', 0) for a in arms])):.0f} | "
                     f"{float(np.median([a['refine_wall_ms'] for a in arms if 'refine_wall_ms' in a] or [float('nan')])):.2f} |")
        L += ["", "- The counts are one run of one protocol, reported as they came; none is a threshold.  `near` = within the found radius.  Where no hit "
              "is near the truth neither refinement can recover it; the two chains differ only in how the hits are re-ranked and sharpened.",
              "- What the sequence refinement is for is the case of `tests/test_gpu_refine_sequence.py`: two congruent corridors, where the anchor-scan "
              "refinement gives each 500 of 1000 particles and the sequence refinement gives the true one all 1000."]
    L.append("")
    open(out, "w").write("\n".join(L))
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--poses", type=int, default=20, help="true poses of the found protocol (0: leave it out)")
    ap.add_argument("--particles", type=int, default=262144)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_refine.md"))
    ap.add_argument("--json", default=None, help="also keep the raw figures here")
    a = ap.parse_args()
    rows = timing(a.reps, a.warmup)
    f = found(a.poses, a.particles) if a.poses > 0 else None
    if a.json:
        json.dump(dict(timing=rows, found=f), open(a.json, "w"), indent=1)
    report(rows, f, a.reps, a.warmup, a.out)


if __name__ == "__main__":
    main()
