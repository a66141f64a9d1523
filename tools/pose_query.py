#!/usr/bin/env python3
"""Times the pose query (Engine.expected_scans / Engine.score_poses) on the Spielberg map with 1081 beams at
K = 1, 16, 1024, 65536 poses, beside the only route there was before it -- a second engine doing set_particles + sensor_update +
ray_steps + log_weights at the same K -- and writes profiles/pose_query.md.  Each figure is the median (and minimum) wall time of
the whole call or route, host wait included, over --reps runs after --warmup untimed ones.

With --bench FILE.json (written by this tool's --run-bench, see below) the file also records `python bench.py` steady state of
this tree against the parent commit's, measured in the same session.

usage: tools/pose_query.py [--reps 20] [--warmup 3] [--out profiles/pose_query.md] [--bench FILE.json]
       tools/pose_query.py --run-bench PARENT_TREE --bench FILE.json     (three alternating bench.py runs of each tree)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KS = (1, 16, 1024, 65536)


def timed(f, reps, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def run_bench(parent, out, steps=20, warmup=3, repeats=3):
    """bench.py of the parent tree and of this one, alternating, `repeats` times each: the update_ms of every run"""
    res = {"parent": [], "this": []}
    for _ in range(repeats):
        for name, tree in (("parent", parent), ("this", ROOT)):
            line = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=tree,
                                  capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1]
            r = json.loads(line)
            res[name].append({k: r[k] for k in r if isinstance(r[k], (int, float)) and ("ms" in k or k in ("value", "score"))})
            print(name, res[name][-1], flush=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_query.md"))
    ap.add_argument("--bench", default=None)
    ap.add_argument("--run-bench", default=None, metavar="PARENT_TREE")
    args = ap.parse_args()
    if args.run_bench:
        return run_bench(os.path.abspath(args.run_bench), args.bench)
    import __graft_entry__ as g
    g.build()
    from monte_carlo_localization_amd import engine, maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    ang = synth.beam_angles()
    rows = []
    for K in KS:
        poses = synth.tracking_cloud(np.random.default_rng(K), K).T.copy()          # (K, 3) around the scan's true pose
        q = engine.Engine(max_particles=16, seed=5)
        q.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        q.set_beam_angles(ang)
        t_scan = timed(lambda: q.expected_scans(poses), args.reps, args.warmup)
        t_steps = timed(lambda: q.lib.mcl_query_scans(q._h, engine._p(q._query_poses(poses)), K, None, None), args.reps, args.warmup)
        t_score = timed(lambda: q.score_poses(poses, scan), args.reps, args.warmup)
        l3 = q.query_counters()
        q.close()
        t = engine.Engine(max_particles=K, seed=5, keep_ray_steps=1)
        t.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        t.set_beam_angles(ang)
        pc, w = np.ascontiguousarray(poses.T), np.full(K, 1.0 / K)

        def route():
            t.set_particles(pc, w)
            t.sensor_update(scan)
            t.ray_steps()
            t.log_weights()

        t_route = timed(route, args.reps, args.warmup)
        t.close()
        rows.append((K, t_scan, t_steps, t_score, t_route, l3["device_bytes"]))
        print(rows[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("# Pose query: time per call\n\n")
        f.write("Written by `tools/pose_query.py` on one MI355X (Spielberg map, 1081 beams, poses drawn around the scan's true pose). "
                f"Host-synchronous wall time of the whole call, median / minimum of {args.reps} runs after {args.warmup} untimed ones. "
                "`expected_scans` returns K x 1081 float ranges (the copy to host memory is part of the call); `cast only` is "
                "`mcl_query_scans` with both outputs NULL (the kernels and the one host wait); `score_poses` returns K records. "
                "`twin route` is what there was before: a second engine with `keep_ray_steps`, `set_particles` + `sensor_update` + "
                "`ray_steps` + `log_weights` at the same K (it also returns K x 1081 steps).\n\n")
        f.write("| K | expected_scans ms | cast only ms | score_poses ms | twin route ms | query buffers MiB |\n|---:|---:|---:|---:|---:|---:|\n")
        for K, a, b, c, d, nbytes in rows:
            f.write(f"| {K} | {a[0]:.3f} / {a[1]:.3f} | {b[0]:.3f} / {b[1]:.3f} | {c[0]:.3f} / {c[1]:.3f} | {d[0]:.3f} / {d[1]:.3f} | {nbytes / 2**20:.1f} |\n")
        if args.bench and os.path.exists(args.bench):
            res = json.load(open(args.bench))
            f.write("\n## `python bench.py --gpus 1 --steps 20 --warmup 3`: this tree against the parent commit\n\n"
                    "Same machine, same session, the two trees alternating; an engine that never queries allocates nothing for the "
                    "query, and no kernel of the update changed.\n\n")
            keys = sorted({k for runs in res.values() for r in runs for k in r})
            f.write("| tree | run | " + " | ".join(keys) + " |\n|---|---:|" + "---:|" * len(keys) + "\n")
            for name in ("parent", "this"):
                for i, r in enumerate(res[name]):
                    f.write(f"| {name} | {i + 1} | " + " | ".join(f"{r.get(k, float('nan')):.4f}" for k in keys) + " |\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
