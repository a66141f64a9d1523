#!/usr/bin/env python3
"""What the sensor mount (mcl_set_sensor_mount) costs an update on one MI355X, on the Spielberg map with bench.py's
scan and action and the tracking cloud; profiles/sensor_mount.md is written from the parts.

  python tools/sensor_mount.py bench --parent-tree DIR [--rounds R] [--out DIR]
      `python bench.py --gpus 1 --steps 20 --warmup 3` in this tree and in a checkout of the parent commit with its library built
      (its own binding beside its own library), R rounds in turn (every second round in the other order), each in a fresh
      process: no mount is set, so the two launch the same kernels (SM5) and the difference is held against the parent's own
      spread over its rounds
  python tools/sensor_mount.py measure [--rounds R] [--out DIR]
      R rounds of the configurations below in turn (every second round in reverse order), each in a fresh child process
  python tools/sensor_mount.py child --config NAME [--sizes N,N] --json FILE
      one configuration (what `measure` starts; also the command to put behind `rocprofv3 --kernel-trace --stats
      --output-format csv -d OUT/prof/<config>_<N> --` with --sizes N for the per-kernel times, in a run of its own)
  python tools/sensor_mount.py report [--out DIR]
      profiles/sensor_mount.md from OUT/bench.json, OUT/sensor_mount.json and, when present, OUT/prof/<config>_<N>/**/*kernel_stats.csv

Configurations, at 262 144 x 1081 and 4 194 304 x 1081:
  beam_off / beam_on   the beam model, no mount / mount (0.27, 0, 0)
  lf_off / lf_on       the likelihood field, no mount / mount (0.27, 0, 0)
  two_single           two lidars the old way: two full updates per step, each with one 1081-beam scan (mount off)
  two_fused            two lidars: update(front scan, front mount) + sensor_update_fuse(rear scan, rear mount) per step

build/ is not tracked; the parts go to build/sensor_mount by default."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION = (0.05, 0.0, 0.01)
SIZES = (262144, 4194304)
WARMUP, STEPS = 3, 20
FRONT, REAR = (0.27, 0.0, 0.0), (-0.27, 0.0, 3.141592653589793)
CONFIGS = ("beam_off", "beam_on", "lf_off", "lf_on", "two_single", "two_fused")
NAMES = dict(beam_off="beam model, no mount", beam_on="beam model, mount (0.27, 0, 0)", lf_off="likelihood field, no mount",
             lf_on="likelihood field, mount (0.27, 0, 0)", two_single="two single-scan updates per step (no mount)",
             two_fused="update(front) + sensor_update_fuse(rear) per step")
KERNELS = ("k_mount_poses", "k_particle_prep", "k_prep_small", "k_sort_", "k_hist_", "k_cell_bbox", "k_tile_compact", "k_unit_",
           "k_resample", "k_rays_sweep", "k_lfield", "k_add_logw", "k_combine_logw")


def child(config, sizes, path):
    sys.path.insert(0, ROOT)
    from monte_carlo_localization_amd import engine, maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    ang = synth.beam_angles(angle_step=1)
    out = []
    for n in sizes:
        e = engine.Engine(max_particles=n, seed=42)
        e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        e.set_beam_angles(ang)
        if config.startswith("lf"):
            e.set_likelihood_field()
        if config.endswith("_on"):
            e.set_sensor_mount(FRONT)
        e.set_particles(synth.tracking_cloud(np.random.default_rng(42), n), np.full(n, 1.0 / n))

        def step():
            if config == "two_single":
                e.update(ACTION, scan)
                e.update((0.0, 0.0, 0.0), scan)
            elif config == "two_fused":
                e.set_sensor_mount(FRONT)
                e.update(ACTION, scan)
                e.set_sensor_mount(REAR)
                e.sensor_update_fuse(scan)
            else:
                e.update(ACTION, scan)              # (ends in a device synchronise: the result block is read back)
        for _ in range(WARMUP):
            step()
        rows = []
        for _ in range(STEPS):
            t0 = time.perf_counter()
            step()
            rows.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, kernel_ms=e.ray_kernel_ms(),
                             kernel="k_lfield" if config.startswith("lf") else e.ray_kernel_name()))
        e.close()
        r = dict(config=config, n=n, beams=int(ang.size), update_ms=float(np.median([x["wall_ms"] for x in rows])),
                 kernel_ms=float(np.median([x["kernel_ms"] for x in rows])), kernel=rows[-1]["kernel"], rows=rows)
        print(f"{config} {n}: {r['update_ms']:.3f} ms per step, sensor kernel {r['kernel_ms']:.3f} ms ({r['kernel']})", flush=True)
        out.append(r)
    if path:
        json.dump(out, open(path, "w"))


def measure(out, rounds):
    runs = []
    for r in range(rounds):
        for config in (CONFIGS if r % 2 == 0 else CONFIGS[::-1]):
            path = os.path.join(out, f"child_{config}_{r}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--config", config, "--json", path], check=True, timeout=600)
            for c in json.load(open(path)):
                c["round"] = r
                runs.append(c)
    json.dump(dict(rounds=rounds, runs=runs), open(os.path.join(out, "sensor_mount.json"), "w"))


def bench(out, parent_tree, rounds):
    if not os.path.exists(os.path.join(parent_tree, "monte_carlo_localization_amd", "libmcl_hip_engine.so")):
        sys.exit(f"{parent_tree}: no built checkout of the parent commit (monte_carlo_localization_amd/libmcl_hip_engine.so)")
    runs = []
    for r in range(rounds):
        for which in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            env.pop("MCL_LIB", None)
            tree = parent_tree if which == "parent" else ROOT
            p = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP)],
                               check=True, timeout=900, env=env, cwd=tree, capture_output=True, text=True)
            line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
            print(f"round {r} {which}: {line['ms_per_step']:.4f} ms per step", flush=True)
            runs.append(dict(round=r, which=which, ms_per_step=line["ms_per_step"], value=line["value"]))
    json.dump(dict(rounds=rounds, runs=runs), open(os.path.join(out, "bench.json"), "w"))


def _kernels(out, tag):
    found = glob.glob(os.path.join(out, "prof", tag, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None
    rows = []
    for row in csv.DictReader(open(found[0])):
        name = row["Name"].split("(")[0].replace("void ", "").replace("mcl::", "")
        if any(k in name for k in KERNELS) or "radix" in name.lower() or "onesweep" in name.lower():
            rows.append((name[:70], int(row["Calls"]), float(row["AverageNs"]) / 1e3))
    return rows


def _spread(v):
    return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


def report(out):
    L = ["# Sensor mount: what it costs an update on one MI355X", "",
         "Written by `tools/sensor_mount.py` (bench, measure, report) from one MI355X run; the notes are by hand.", ""]
    bp = os.path.join(out, "bench.json")
    L += ["## No mount against the parent commit (`python bench.py --gpus 1 --steps 20 --warmup 3`, 4 194 304 x 1081)", ""]
    if os.path.exists(bp):
        b = json.load(open(bp))
        this = [r["ms_per_step"] for r in b["runs"] if r["which"] == "this"]
        par = [r["ms_per_step"] for r in b["runs"] if r["which"] == "parent"]
        L += [f"{b['rounds']} rounds, the two libraries in turn (every second round in the other order), each run a fresh process; ms "
              "per step, median over the rounds (least .. greatest).", "",
              "| library | ms per step |", "|---|---:|", f"| parent commit | {_spread(par)} |", f"| this commit, no mount | {_spread(this)} |", ""]
    else:
        L += ["Not measured.", ""]
    mp = os.path.join(out, "sensor_mount.json")
    if os.path.exists(mp):
        t = json.load(open(mp))
        L += ["## Mount off against mount (0.27, 0, 0), and two lidars", "",
              f"Spielberg map, bench.py's scan and action, the tracking cloud, seed 42, 1081 beams.  ms: host wall time of a step (every "
              f"call in it ends in a device synchronise), median of {STEPS} steps after {WARMUP} warm-up steps; sensor kernel: the "
              f"HIP-event time between EV_K0 and EV_K1 of the step's last sensor stage.  {t['rounds']} rounds of the configurations in turn "
              "(every second round in reverse order), each in a fresh process; the median over the rounds (least .. greatest).", ""]
        for n in SIZES:
            L += [f"### {n} x 1081", "", "| configuration | step ms | sensor kernel ms | kernel |", "|---|---:|---:|---|"]
            for config in CONFIGS:
                rs = [r for r in t["runs"] if r["config"] == config and r["n"] == n]
                if rs:
                    L.append(f"| {NAMES[config]} | {_spread([r['update_ms'] for r in rs])} | {_spread([r['kernel_ms'] for r in rs])} | `{rs[0]['kernel']}` |")
            L.append("")
    L += ["## Per-kernel times (rocprofv3 --kernel-trace --stats, one run per configuration, separate from the timing runs)", ""]
    any_k = False
    for n in SIZES:
        for config in CONFIGS:
            ks = _kernels(out, f"{config}_{n}")
            if ks:
                any_k = True
                L += [f"{NAMES[config]} at {n} x 1081, calls x mean us:", ""] + [f"- `{name}`: {calls} x {us:.1f}" for name, calls, us in ks] + [""]
    if not any_k:
        L += ["Not measured.", ""]
    open(os.path.join(ROOT, "profiles", "sensor_mount.md"), "w").write("\n".join(L))
    print("wrote profiles/sensor_mount.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["bench", "measure", "child", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "sensor_mount"))
    ap.add_argument("--parent-tree", default=None, help="bench: a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--config", choices=list(CONFIGS))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.part == "bench":
        if not a.parent_tree:
            sys.exit("bench needs --parent-tree")
        bench(a.out, os.path.abspath(a.parent_tree), a.rounds)
    elif a.part == "measure":
        measure(a.out, a.rounds)
    elif a.part == "child":
        child(a.config, [int(v) for v in a.sizes.split(",")], a.json)
    else:
        report(a.out)


if __name__ == "__main__":
    main()
