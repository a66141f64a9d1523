#!/usr/bin/env python3
"""The pose refinement under the beam model (mcl_refine_poses_beam) on one MI355X, on the Spielberg map with the
Hokuyo's 1081 beams; profiles/beam_refine.md is written from the parts.

  python tools/beam_refine.py timing [--out DIR] [--seeds 16]
      ms per call (host wall around the call, which ends in its one host wait; median of REPS after WARMUP) for --seeds seeds (the
      hits of one mcl_global_search_beam on the recorded scan) x the default 1701-pose window, at beam_stride 1 and 10; in the same
      process, alternating with it, the only route the engine offered before to the same records: mcl_host_refine_window,
      mcl_score_poses under the beam model in chunks of 65536 poses, mcl_host_refine_reduce per seed.  The records of both
      routes are compared.
  python tools/beam_refine.py found [--out DIR] [--poses 20] [--particles 262144]
      the found-of-20 protocol of profiles/global_search.md / beam_search.md (same poses, scans, particle count, engine seed):
      mcl_global_search_beam (beam_stride 10) -> mcl_refine_poses_beam -> mixture of the refined means -> 3 updates, once on an
      engine that runs the beam model throughout (the field off) and once on the engine of the recorded chain (the field on for
      the updates), where the refinement is the only difference from profiles/beam_search.md
  python tools/beam_refine.py meta [--out DIR]
      the kernels' register / scratch figures from the built library (tools/kernel_meta.py) into DIR/br_meta.json
  python tools/beam_refine.py report --out DIR
      profiles/beam_refine.md from DIR/br_timing.json, DIR/br_found.json and DIR/br_meta.json; a part that is missing is reported
      as not measured

build/ is not tracked; the JSON parts go to build/beam_refine by default."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 3, 20
FOUND_XY_M, FOUND_TH_RAD = 0.5, 0.2
CHUNK = 65536
RECORDED_FOUND = 3                                           # profiles/beam_search.md: beam search + field refinement


def _world():
    from monte_carlo_localization_amd import maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32).copy()
    return m, synth.beam_angles(angle_step=1), scan


def _engine(n, m, ang, seed=42, field=False):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=n, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    if field:
        e.set_likelihood_field()
    return e


def _median(v):
    return float(np.median(np.asarray(v, np.float64)))


def chunked_route(engine, e, seeds, res, scan, beam_stride, e_strided=None):
    """the records by the route before mcl_refine_poses_beam; (records, ms of mcl_score_poses alone, level-3 rays)"""
    poses = np.concatenate([engine.host_refine_window(s, res) for s in seeds])
    q, obs = (e, scan) if beam_stride == 1 else (e_strided, scan[::beam_stride].copy())
    ll, score_ms, level3 = [], 0.0, 0
    for s0 in range(0, len(poses), CHUNK):
        t0 = time.perf_counter()
        ll.append(q.score_poses(poses[s0:s0 + CHUNK], obs)["log_likelihood"])
        score_ms += (time.perf_counter() - t0) * 1e3
        level3 += q.query_counters()["level3_rays"]
    V = np.concatenate(ll).reshape(len(seeds), -1)
    out = np.zeros(len(seeds), engine.REFINE_DTYPE)
    for k in range(len(seeds)):
        out[k] = engine.host_refine_reduce(seeds[k], res, V[k])
    return out, score_ms, level3


def timing(args):
    from monte_carlo_localization_amd import engine
    m, ang, scan = _world()
    e = _engine(64, m, ang)
    hits, _ = e.global_search_beam(scan, max_hits=args.seeds, beam_stride=10)
    seeds = np.ascontiguousarray(hits["pose"], np.float64)
    assert len(seeds) == args.seeds, f"the search gave {len(seeds)} hits"
    out = dict(map="Spielberg_map", seeds=int(args.seeds), beams=int(scan.size), warmup=WARMUP, reps=REPS, runs={})
    for stride in (1, 10):
        e10 = _engine(64, m, ang[::stride].copy()) if stride > 1 else None
        new_ms, old_ms, old_score_ms, st, same = [], [], [], None, True
        for it in range(WARMUP + REPS):                      # alternating, same process, same box
            t0 = time.perf_counter()
            r, st = e.refine_poses_beam(seeds, scan, beam_stride=stride)
            t1 = time.perf_counter()
            ro, sms, level3 = chunked_route(engine, e, seeds, m.resolution, scan, stride, e10)
            t2 = time.perf_counter()
            same = same and bool(np.array_equal(r["best_index"], ro["best_index"])) and \
                r["best_log_likelihood"].tobytes() == ro["best_log_likelihood"].tobytes() and level3 == st["level3_rays"]
            if it >= WARMUP:
                new_ms.append((t1 - t0) * 1e3)
                old_ms.append((t2 - t1) * 1e3)
                old_score_ms.append(sms)
        run = dict(stats=st, new_wall_ms=new_ms, new_wall_ms_median=_median(new_ms), chunked_wall_ms=old_ms,
                   chunked_wall_ms_median=_median(old_ms), chunked_score_only_ms_median=_median(old_score_ms),
                   factor=_median(old_ms) / _median(new_ms), factor_score_only=_median(old_score_ms) / _median(new_ms),
                   same_records=same, level3_share=st["level3_rays"] / st["rays"],
                   chunked_intermediate_bytes=int(st["rays"]) * 2 + int(st["n_poses"]) * (24 + 24))
        out["runs"][str(stride)] = run
        print(json.dumps(dict(beam_stride=stride, **{k: v for k, v in run.items() if not k.endswith("_ms")})), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "br_timing.json"), "w"), indent=1)


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
    res = float(np.float32(m.resolution))
    free = np.flatnonzero(np.asarray(m.data).ravel() == 0)
    W = m.data.shape[1]
    n = args.particles
    still = (0.0, 0.0, 0.0)
    out = dict(map="Spielberg_map", particles=n, poses=args.poses, found_xy_m=FOUND_XY_M, found_th_rad=FOUND_TH_RAD,
               recorded_found=RECORDED_FOUND, chains={})
    for name, field in (("beam model throughout", False), ("field updates, as recorded", True)):
        rng = np.random.default_rng(2024)                    # the poses of profiles/global_search.md, for either chain
        b = _engine(n, m, ang, seed=7, field=field)
        rows = []
        for i in range(args.poses):
            c = int(rng.choice(free))
            truth = np.array([m.origin_x + (c % W + rng.random()) * res, m.origin_y + (c // W + rng.random()) * res, rng.uniform(-np.pi, np.pi)])
            dirs = truth[2] + ang.astype(np.float64)
            scan = orc.cast_many(om, np.full(dirs.size, truth[0]), np.full(dirs.size, truth[1]), dirs)[0].astype(np.float32)
            hits, st = b.global_search_beam(scan, max_hits=16, beam_stride=10)
            row = dict(truth=[float(v) for v in truth], n_hits=st["n_hits"], found=False)
            if len(hits):
                t0 = time.perf_counter()
                r, rst = b.refine_poses_beam(hits["pose"], scan)
                row["refine_wall_ms"] = (time.perf_counter() - t0) * 1e3
                row["level3_share"] = rst["level3_rays"] / rst["rays"]
                b.init_particles_mixture(r["mean"], r["cov"], engine.seed_counts(r["best_log_likelihood"], n))
                for _ in range(3):
                    b.update(still, scan)
                d, t = _err(b.expected_pose(), truth)
                best = r[int(np.argmax(r["best_log_likelihood"]))]["best"]
                row.update(err_m=d, err_rad=t, found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD), best_refined_err=list(_err(best, truth)),
                           any_hit_near=bool(any(e[0] < FOUND_XY_M and e[1] < FOUND_TH_RAD for e in (_err(h["pose"], truth) for h in hits))))
            rows.append(row)
            print(json.dumps(dict(chain=name, **row)), flush=True)
        out["chains"][name] = dict(rows=rows, found=sum(r["found"] for r in rows))
        b.close()
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "br_found.json"), "w"), indent=1)


def meta(args):
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_meta.py"),
                          os.path.join(ROOT, "monte_carlo_localization_amd", "libmcl_hip_engine.so"),
                          "--out", os.path.join(args.out, "dev.co")], capture_output=True, text=True, cwd=ROOT).stdout
    out = {}
    for line in txt.splitlines():
        mm = re.match(r"\S*?(k_refine_\w+|k_query_rays|k_query_exact)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+vspill\s+(\d+)\s+sspill\s+(\d+)\s+lds\s+(\d+)\s+scratch\s+(\d+)", line)
        if mm:
            out[mm.group(1)] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "lds", "scratch"), map(int, mm.groups()[1:])))
    for name in os.listdir(args.out):
        if name.startswith("dev.co"):
            os.remove(os.path.join(args.out, name))
    json.dump(out, open(os.path.join(args.out, "br_meta.json"), "w"), indent=1)
    print(json.dumps(out))


def _load(args, name):
    p = os.path.join(args.out, name)
    return json.load(open(p)) if os.path.exists(p) else None


def report(args):
    t, f, k = _load(args, "br_timing.json"), _load(args, "br_found.json"), _load(args, "br_meta.json")
    L = ["# Pose refinement under the beam model on one MI355X (Spielberg map)", "",
         "Written by `tools/beam_refine.py report` from one `timing` and one `found` run on the GPU and the `meta` part (the built "
         "library's metadata); every number below is measured."]
    if not t:
        L += ["", "The call time and the factor against `mcl_score_poses` in chunks: **not measured**."]
    else:
        r1, r10 = t["runs"]["1"], t["runs"]["10"]
        st = r1["stats"]
        L += ["",
              f"{t['seeds']} seeds (the hits of one `mcl_global_search_beam` on the recorded scan) x the default window of {st['n_win']} poses = "
              f"{st['n_poses']} poses, {t['beams']}-beam scan.  Host wall around each route, which ends in a host wait; median of {t['reps']} "
              f"after {t['warmup']}, the two routes alternating in one process.  The chunked route is what the engine offered before: "
              "`mcl_host_refine_window`, `mcl_score_poses` under the beam model in chunks of 65536 poses, `mcl_host_refine_reduce` per seed.", "",
              "| beam_stride | used beams | rays | `mcl_refine_poses_beam` ms | chunked route ms | of which `mcl_score_poses` ms | factor (whole route) | factor (`mcl_score_poses` alone) | level-3 share of rays | same records |",
              "|---|---|---|---|---|---|---|---|---|---|"]
        for s, r in (("1", r1), ("10", r10)):
            q = r["stats"]
            L.append(f"| {s} | {q['used_beams']} | {q['rays']} | {r['new_wall_ms_median']:.2f} | {r['chunked_wall_ms_median']:.2f} | "
                     f"{r['chunked_score_only_ms_median']:.2f} | {r['factor']:.1f} | {r['factor_score_only']:.1f} | {100 * r['level3_share']:.1f} % | "
                     f"{'yes' if r['same_records'] else 'NO'} |")
        verdict = "faster than" if r1["factor_score_only"] > 1.0 and r10["factor_score_only"] > 1.0 else "NOT faster than"
        L += ["",
              f"**The new call is {verdict} the chunked route at both strides** (the acceptance condition; no time was fixed in advance).  "
              f"At beam_stride 1 the chunked route stores and reads back {r1['chunked_intermediate_bytes'] / 2**20:.0f} MiB of steps, uploaded poses and "
              f"score records that the new call never forms.  Device memory of the refinement's buffers: {st['device_bytes'] / 2**10:.0f} KiB.  "
              "\"Same records\": best_index and best_log_likelihood of every seed agree bit for bit between the routes in every repetition, and both "
              "decide the same number of rays by the literal march."]
    if k and "k_refine_beam_score" in k:
        L += ["", "## The kernel's registers", "", "From the gfx950 code object of the built library (`tools/kernel_meta.py`):", "",
              "| kernel | VGPR | AGPR | SGPR | VGPR spills | SGPR spills | LDS bytes | scratch bytes / lane |", "|---|---|---|---|---|---|---|---|"]
        for name in ("k_refine_beam_score", "k_refine_beam_rows", "k_refine_reduce", "k_query_rays", "k_query_exact"):
            if name in k:
                v = k[name]
                L.append(f"| {name} | {v['vgpr']} | {v['agpr']} | {v['sgpr']} | {v['vspill']} | {v['sspill']} | {v['lds']} | {v['scratch']} |")
    else:
        L += ["", "The kernel's register figures: **not measured**."]
    if not f:
        L += ["", "The found-of-20 count: **not measured**."]
    else:
        L += ["", "## Is the robot found?", "",
              f"The protocol of `profiles/global_search.md` and `profiles/beam_search.md` ({f['poses']} random free poses from the same generator, "
              f"oracle-cast 1081-beam scans, the robot standing still, {f['particles']} particles, engine seed 7, found = expected pose within "
              f"{f['found_xy_m']} m and {f['found_th_rad']} rad after 3 updates): `mcl_global_search_beam` (beam_stride 10), `mcl_refine_poses_beam` "
              "(every beam), the mixture of the refined means, 3 updates.", "",
              "| chain | found |", "|---|---|",
              f"| beam search + field `mcl_refine_poses` + field updates (recorded, `profiles/beam_search.md`) | {f['recorded_found']} / {f['poses']} |"]
        for name, c in f["chains"].items():
            L.append(f"| beam search + `mcl_refine_poses_beam`, {name} | **{c['found']} / {f['poses']}** |")
        for name, c in f["chains"].items():
            rows = [r for r in c["rows"] if "refine_wall_ms" in r]
            L += ["", f"- {name}: poses with one of the 16 hits within the found radius: {sum(r.get('any_hit_near', False) for r in rows)} / {f['poses']}; "
                      f"with the best refined pose within it: {sum(r['best_refined_err'][0] < f['found_xy_m'] and r['best_refined_err'][1] < f['found_th_rad'] for r in rows)} / {f['poses']}; "
                      f"refinement wall per pose (16 seeds, every beam): median {_median([r['refine_wall_ms'] for r in rows]):.2f} ms; "
                      f"level-3 share of its rays: median {100 * _median([r['level3_share'] for r in rows]):.1f} %"]
        L += ["", "No count was promised: the figure says how often search + refine + seed localises from ONE scan of a standing robot, and what the "
                  "mixed-model refinement of the recorded chain cost or gained."]
    L.append("")
    open(os.path.join(ROOT, "profiles", "beam_refine.md"), "w").write("\n".join(L))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["timing", "found", "meta", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "beam_refine"))
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--particles", type=int, default=262144)
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dict(timing=timing, found=found, meta=meta, report=report)[args.part](args)


if __name__ == "__main__":
    main()
