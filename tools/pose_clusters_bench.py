#!/usr/bin/env python3
"""Times mcl_pose_clusters (Engine.pose_clusters) on the Spielberg map and writes profiles/pose_clusters.md:
the median wall time of the call (it ends with its one host wait) at the stock 2000 x 61, at 262 144 and 4 194 304 tracking
after an update, and at 4 194 304 uniform straight after init_global; then the kernel_meta lines of the clustering kernels.

usage: tools/pose_clusters_bench.py [--reps 20] [--out profiles/pose_clusters.md] [--only NAME]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases():
    from monte_carlo_localization_amd import synth
    return [
        ("stock 2000 x 61, after 1 update from init_global", 2000, 18, "global", 1),
        ("262 144 tracking, after 1 update (1081 beams)", 262144, 1, "tracking", 1),
        ("4 194 304 tracking, after 1 update (1081 beams)", 4194304, 1, "tracking", 1),
        ("4 194 304 uniform, straight after init_global", 4194304, 1, "global", 0),
    ], synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_clusters.md"))
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from monte_carlo_localization_amd import engine, maps
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan_all = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    rows = []
    cs, synth = cases()
    for name, n, step, kind, updates in cs:
        if args.only and args.only not in name:
            continue
        ang = synth.beam_angles(angle_step=step)
        e = engine.Engine(max_particles=n, seed=5)
        e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        e.set_beam_angles(ang)
        if kind == "tracking":
            e.set_particles(synth.tracking_cloud(np.random.default_rng(5), n), np.full(n, 1.0 / n))
        else:
            e.init_global(n)
        for _ in range(updates):
            e.update((0.1, 0.0, 0.02) if kind == "tracking" else (0.0, 0.0, 0.0), scan_all[::step].copy())
        _, info = e.pose_clusters(16)                  # the first call allocates
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            _, info = e.pose_clusters(16)
            ts.append((time.perf_counter() - t0) * 1e3)
        top, _ = e.pose_clusters(1)
        rows.append((name, float(np.median(ts)), float(np.min(ts)), info["n_clusters"], int(top[0]["n_bins"]) if top.size else 0))
        print(rows[-1], flush=True)
        e.close()
    obj = os.path.join(ROOT, "monte_carlo_localization_amd", "csrc", "_build", "libmcl_hip_engine.so", "mcl_cluster.o")
    meta = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_meta.py"), obj, "--out", "/tmp/mcl_cluster.co"],
                          capture_output=True, text=True).stdout
    meta = "\n".join(l for l in meta.splitlines() if "k_clu_" in l)
    with open(args.out, "w") as f:
        f.write("# mcl_pose_clusters: time per call\n\n")
        f.write("Written by `tools/pose_clusters_bench.py` on one MI355X (Spielberg map, default cluster config 0.5 m x 0.5 m x 10 deg, "
                f"max_clusters 16). Wall time of the whole call, its one host wait included; median and minimum of {args.reps} calls "
                "after a first one that allocates.\n\n")
        f.write("| case | median ms | min ms | clusters | bins of the heaviest |\n|---|---:|---:|---:|---:|\n")
        for r in rows:
            f.write(f"| {r[0]} | {r[1]:.3f} | {r[2]:.3f} | {r[3]} | {r[4]} |\n")
        f.write("\n## kernel_meta\n\n```\n" + meta + "\n```\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
