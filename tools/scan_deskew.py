#!/usr/bin/env python3
"""What scan de-skew (mcl_set_beam_offsets) costs an update on one MI355X, on the Spielberg map with bench.py's
scan and action and the tracking cloud; profiles/scan_deskew.md is written from the parts.

  python tools/scan_deskew.py bench --parent-tree DIR [--rounds R] [--out DIR]
      `python bench.py --gpus 1 --steps 20 --warmup 3` in this tree and in a checkout of the parent commit with its library built
      (its own binding beside its own library), R rounds in turn (every second round in the other order), each in a fresh
      process: no offsets are set, so the two launch the same kernels (DS6) and the difference is held against the parent's own
      spread over its rounds
  python tools/scan_deskew.py measure --parent-tree DIR [--rounds R] [--out DIR]
      R rounds of the configurations below in turn (every second round in reverse order), each in a fresh child process; the
      `parent_*` configurations run this file's child in the parent's tree, against the parent's binding and library
  python tools/scan_deskew.py child --config NAME [--sizes NxB,NxB] [--tree DIR] --json FILE
      one configuration (what `measure` starts; also the command to put behind `rocprofv3 --kernel-trace --stats --output-format
      csv -d OUT/prof/<config> --` with one size for the per-kernel times, in a run of its own)
  python tools/scan_deskew.py report [--out DIR]
      profiles/scan_deskew.md from OUT/bench.json and OUT/scan_deskew.json

Configurations, at 2000 x 61, 4000 x 61, 262 144 x 1081 and (first round only) 4 194 304 x 1081:
  parent_beam / parent_lf   the parent commit, beam model / likelihood field (it has no offsets)
  beam_off / lf_off         this commit, offsets off
  beam_on / lf_on           this commit, a constant-twist table set before every update (the setter is inside the timed step, as a
                            node calls it at scan rate)
  setter                    mcl_set_beam_offsets alone, while offsets are on: the host time of a call (table formation on the host and
                            one asynchronous copy; it does not wait for the device)
  query                     mcl_score_poses over 65 536 poses with the same beams: the per-ray cost of one origin per pose on the
                            same field, what k_rays_deskew's per-ray cost is held against

build/ is not tracked; the parts go to build/scan_deskew by default."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION = (0.05, 0.0, 0.01)
SIZES = ((2000, 61), (4000, 61), (262144, 1081), (4194304, 1081))
ONCE = (4194304, 1081)
WARMUP, STEPS = 3, 20
TWIST = (0.175, 0.0, 0.12)             # 7 m/s and 4.8 rad/s over a 25 ms sweep
CONFIGS = ("parent_beam", "beam_off", "beam_on", "parent_lf", "lf_off", "lf_on", "setter", "query")
NAMES = dict(parent_beam="beam model, parent commit", beam_off="beam model, offsets off", beam_on="beam model, offsets on",
             parent_lf="likelihood field, parent commit", lf_off="likelihood field, offsets off", lf_on="likelihood field, offsets on")


def child(config, sizes, path, tree):
    sys.path.insert(0, tree)
    from monte_carlo_localization_amd import engine, maps, synth
    m = maps.load_npz(os.path.join(tree, "tests", "golden", "map_Spielberg_map.npz"))
    full = np.load(os.path.join(tree, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    out = []
    for n, B in sizes:
        step_b = 1080 // (B - 1)
        ang, scan = synth.beam_angles(angle_step=step_b), full[::step_b].copy()
        assert ang.size == B and scan.size == B
        e = engine.Engine(max_particles=n, seed=42)
        e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        e.set_beam_angles(ang)
        if "lf" in config:
            e.set_likelihood_field()
        e.set_particles(synth.tracking_cloud(np.random.default_rng(42), n), np.full(n, 1.0 / n))
        on = config in ("beam_on", "lf_on", "setter")
        off = engine.host_scan_motion_offsets(TWIST, B) if on else None
        rows = []
        if config == "query":
            poses = np.ascontiguousarray(synth.tracking_cloud(np.random.default_rng(7), 65536).T)
            for k in range(WARMUP + STEPS):
                t0 = time.perf_counter()
                e.score_poses(poses, scan)
                if k >= WARMUP:
                    rows.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, kernel_ms=0.0, kernel="k_query_rays"))
        elif config == "setter":
            e.set_beam_offsets(off)
            e.update(ACTION, scan)
            for k in range(200):
                t0 = time.perf_counter()
                e.lib.mcl_set_beam_offsets(e._h, off.ctypes.data, B)           # (the C call alone: no numpy conversion around it)
                rows.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, kernel_ms=0.0, kernel="-"))
                if k % 20 == 19:
                    e.update(ACTION, scan)                                  # (drains the stream: the copies do not pile up)
        else:
            def step():
                if on:
                    e.set_beam_offsets(off)
                e.update(ACTION, scan)                  # (ends in a device synchronise: the result block is read back)
            for _ in range(WARMUP):
                step()
            for _ in range(STEPS):
                t0 = time.perf_counter()
                step()
                rows.append(dict(wall_ms=(time.perf_counter() - t0) * 1e3, kernel_ms=e.ray_kernel_ms(),
                                 kernel="k_lfield" if "lf" in config else e.ray_kernel_name()))
        e.close()
        r = dict(config=config, n=n, beams=B, update_ms=float(np.median([x["wall_ms"] for x in rows])),
                 kernel_ms=float(np.median([x["kernel_ms"] for x in rows])), kernel=rows[-1]["kernel"])
        print(f"{config} {n} x {B}: {r['update_ms']:.4f} ms per step, sensor kernel {r['kernel_ms']:.4f} ms ({r['kernel']})", flush=True)
        out.append(r)
    if path:
        json.dump(out, open(path, "w"))


def measure(out, parent_tree, rounds):
    runs = []
    for r in range(rounds):
        for config in (CONFIGS if r % 2 == 0 else CONFIGS[::-1]):
            tree = parent_tree if config.startswith("parent") else ROOT
            sizes = [s for s in SIZES if s != ONCE or r == 0]
            if config in ("setter", "query"):
                sizes = [(4000, 61), (262144, 1081)]
            path = os.path.join(out, f"child_{config}_{r}.json")
            env = dict(os.environ)
            env.pop("MCL_LIB", None)
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--config", config, "--tree", tree, "--json", path,
                            "--sizes", ",".join(f"{n}x{B}" for n, B in sizes)], check=True, timeout=600, env=env)
            for c in json.load(open(path)):
                c["round"] = r
                runs.append(c)
    json.dump(dict(rounds=rounds, runs=runs), open(os.path.join(out, "scan_deskew.json"), "w"))


def bench(out, parent_tree, rounds):
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


def _spread(v, digits=3):
    return f"{np.median(v):.{digits}f} ({min(v):.{digits}f} .. {max(v):.{digits}f})"


def report(out):
    L = ["# Scan de-skew: what per-beam sensor offsets cost an update on one MI355X", "",
         "Written by `tools/scan_deskew.py` (bench, measure, report) from one MI355X run; the notes are by hand.", ""]
    bp = os.path.join(out, "bench.json")
    L += ["## Offsets off against the parent commit (`python bench.py --gpus 1 --steps 20 --warmup 3`, 4 194 304 x 1081)", ""]
    if os.path.exists(bp):
        b = json.load(open(bp))
        this = [r["ms_per_step"] for r in b["runs"] if r["which"] == "this"]
        par = [r["ms_per_step"] for r in b["runs"] if r["which"] == "parent"]
        L += [f"{b['rounds']} rounds, the two libraries in turn (every second round in the other order), each run a fresh process; ms "
              "per step, median over the rounds (least .. greatest).", "",
              "| library | ms per step |", "|---|---:|", f"| parent commit | {_spread(par)} |", f"| this commit, offsets off | {_spread(this)} |", ""]
    else:
        L += ["Not measured.", ""]
    mp = os.path.join(out, "scan_deskew.json")
    if os.path.exists(mp):
        t = json.load(open(mp))
        L += ["## Per-update time: the parent, offsets off, offsets on", "",
              f"Spielberg map, bench.py's scan (every 18th beam of it at 61 beams) and action, the tracking cloud, seed 42.  ms: host wall "
              f"time of a step (the setter call, where offsets are on, and an update that ends in a device synchronise), median of "
              f"{STEPS} steps after {WARMUP} warm-up steps; sensor kernel: the HIP-event time between EV_K0 and EV_K1.  {t['rounds']} "
              "rounds of the configurations in turn (every second round in reverse order), each in a fresh process; the median over the "
              "rounds (least .. greatest); 4 194 304 x 1081 in the first round only.", ""]
        for n, B in SIZES:
            L += [f"### {n} x {B}", "", "| configuration | step ms | sensor kernel ms | kernel |", "|---|---:|---:|---|"]
            for config in CONFIGS[:6]:
                rs = [r for r in t["runs"] if r["config"] == config and r["n"] == n and r["beams"] == B]
                if rs:
                    L.append(f"| {NAMES[config]} | {_spread([r['update_ms'] for r in rs])} | {_spread([r['kernel_ms'] for r in rs])} | `{rs[0]['kernel']}` |")
            L.append("")
        L += ["## The setter alone, and the pose query's cost per ray", ""]
        for n, B in ((4000, 61), (262144, 1081)):
            rs = [r for r in t["runs"] if r["config"] == "setter" and r["beams"] == B]
            if rs:
                L.append(f"- `mcl_set_beam_offsets` with offsets on, {B} beams: {_spread([r['update_ms'] * 1e3 for r in rs], 1)} us of host time per call "
                         "(median of 200 calls; no device wait).")
            rs = [r for r in t["runs"] if r["config"] == "query" and r["beams"] == B]
            if rs:
                ms = [r["update_ms"] for r in rs]
                L.append(f"- `mcl_score_poses`, 65 536 poses x {B} beams: {_spread(ms)} ms per call, {np.median(ms) * 1e9 / (65536 * B):.1f} ps per ray "
                         "(copies and the scoring kernels included).")
            rs = [r for r in t["runs"] if r["config"] == "beam_on" and r["beams"] == B and r["n"] == (4000 if B == 61 else 262144)]
            if rs:
                k = float(np.median([r["kernel_ms"] for r in rs]))
                L.append(f"- `k_rays_deskew`, {rs[0]['n']} particles x {B} beams: {k:.3f} ms, {k * 1e9 / (rs[0]['n'] * B):.1f} ps per ray.")
        L.append("")
    open(os.path.join(ROOT, "profiles", "scan_deskew.md"), "w").write("\n".join(L))
    print("wrote profiles/scan_deskew.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["bench", "measure", "child", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "scan_deskew"))
    ap.add_argument("--parent-tree", default=None, help="bench, measure: a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--config", choices=list(CONFIGS))
    ap.add_argument("--sizes", default=",".join(f"{n}x{B}" for n, B in SIZES))
    ap.add_argument("--tree", default=ROOT, help="child: the tree whose binding and library are measured")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.part in ("bench", "measure"):
        if not a.parent_tree or not os.path.exists(os.path.join(a.parent_tree, "monte_carlo_localization_amd", "libmcl_hip_engine.so")):
            sys.exit(f"{a.part} needs --parent-tree: a checkout of the parent commit with monte_carlo_localization_amd/libmcl_hip_engine.so built")
        (bench if a.part == "bench" else measure)(a.out, os.path.abspath(a.parent_tree), a.rounds)
    elif a.part == "child":
        child(a.config, [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")], a.json, os.path.abspath(a.tree))
    else:
        report(a.out)


if __name__ == "__main__":
    main()
