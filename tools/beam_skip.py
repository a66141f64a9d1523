#!/usr/bin/env python3
"""What beam skipping (mcl_set_beam_skip) costs an update on one MI355X, on the Spielberg map with bench.py's scan
and action and the tracking cloud; profiles/beam_skip.md is written from the parts.  Four configurations at 262 144 x 1081 and
4 194 304 x 1081:

  a  the likelihood field alone, on a checkout of the parent commit (--parent-tree: its tree with its library built)
  b  this tree, beam skipping off
  c  beam skipping on with no beam skipped (threshold 0: a beam is kept as soon as one particle agrees)
  d  beam skipping on, AMCL's defaults, with the sector of the tests shortened to 0.4 of its ranges

  python tools/beam_skip.py measure --parent-tree DIR [--rounds R] [--out DIR]
      R rounds of a, b, c, d in turn (every second round in the order d, c, b, a), every configuration in a fresh child process,
      so that drift of the machine and what ran just before fall on all four alike; the spread of a over its rounds is what b is
      held against
  python tools/beam_skip.py child --tree DIR --config a|b|c|d [--sizes N,N] --json FILE
      one configuration (what `measure` starts; also the command to put behind `rocprofv3 --kernel-trace --stats
      --output-format csv -d OUT/prof/<config>_<N> --` with --sizes N for the split over the three kernels, in a run of its own)
  python tools/beam_skip.py report [--out DIR]
      profiles/beam_skip.md from OUT/beam_skip.json and, when present, OUT/prof/<config>_<N>/**/*kernel_stats.csv

build/ is not tracked; the parts go to build/beam_skip by default."""
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
NAMES = dict(a="likelihood field alone, parent commit", b="this commit, beam skipping off",
             c="beam skipping on, no beam skipped (threshold 0)", d="beam skipping on, the tests' sector shortened")


def child(tree, config, sizes, path):
    sys.path.insert(0, tree)
    from monte_carlo_localization_amd import engine, maps, synth
    assert os.path.realpath(engine.__file__).startswith(os.path.realpath(tree)), engine.__file__
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    ang = synth.beam_angles(angle_step=1)
    if config == "d":
        scan[int(0.28 * scan.size):int(0.39 * scan.size)] *= np.float32(0.4)
    out = []
    for n in sizes:
        e = engine.Engine(max_particles=n, seed=42)
        e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        e.set_beam_angles(ang)
        e.set_likelihood_field()
        if config == "c":
            e.set_beam_skip(threshold=0.0)
        elif config == "d":
            e.set_beam_skip()
        e.set_particles(synth.tracking_cloud(np.random.default_rng(42), n), np.full(n, 1.0 / n))
        for _ in range(WARMUP):
            e.update(ACTION, scan)
        rows = []
        for _ in range(STEPS):
            t0 = time.perf_counter()
            e.update(ACTION, scan)                  # (ends in a device synchronise: the result block is read back)
            wall = (time.perf_counter() - t0) * 1e3
            row = dict(wall_ms=wall, kernel_ms=e.ray_kernel_ms())
            if config in "cd":
                st = e.beam_skip_state()
                row.update(n_used=st["n_used"], n_kept=st["n_kept"], n_skipped=st["n_skipped"], integrate_all=st["integrate_all"])
            rows.append(row)
        e.close()
        med = lambda k: float(np.median([r[k] for r in rows]))
        r = dict(config=config, n=n, beams=int(ang.size), update_ms=med("wall_ms"), kernel_ms=med("kernel_ms"), rows=rows)
        print(f"{config} {n}: {r['update_ms']:.3f} ms per update, sensor kernels {r['kernel_ms']:.3f} ms", flush=True)
        out.append(r)
    if path:
        json.dump(out, open(path, "w"))


def measure(out, parent_tree, rounds):
    if not os.path.exists(os.path.join(parent_tree, "monte_carlo_localization_amd", "libmcl_hip_engine.so")):
        sys.exit(f"{parent_tree}: no built checkout of the parent commit (monte_carlo_localization_amd/libmcl_hip_engine.so)")
    runs = []
    for r in range(rounds):
        for config in ("abcd" if r % 2 == 0 else "dcba"):
            tree = parent_tree if config == "a" else ROOT
            path = os.path.join(out, f"child_{config}_{r}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--tree", tree, "--config", config, "--json", path],
                           check=True, timeout=600)
            for c in json.load(open(path)):
                c["round"] = r
                runs.append(c)
    json.dump(dict(rounds=rounds, runs=runs), open(os.path.join(out, "beam_skip.json"), "w"))


def _kernels(out, config):
    found = glob.glob(os.path.join(out, "prof", config, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None
    rows = []
    for row in csv.DictReader(open(found[0])):
        if "lfield" in row["Name"] or "lf_skip" in row["Name"]:
            rows.append((row["Name"].split("(")[0], int(row["Calls"]), float(row["AverageNs"]) / 1e3))
    return rows


def report(out):
    t = json.load(open(os.path.join(out, "beam_skip.json")))
    L = ["# Beam skipping for the likelihood field: what it costs an update on one MI355X", "",
         "Written by `tools/beam_skip.py` (measure, report) from one MI355X run; the notes are by hand.", "",
         f"Spielberg map, bench.py's scan and action, the tracking cloud, seed 42, 1081 beams.  ms: host wall time of `mcl_update` "
         f"(it ends in a device synchronise), median of {STEPS} updates after {WARMUP} warm-up updates; sensor kernels: the HIP-event "
         f"time between EV_K0 and EV_K1 (`mcl_get_ray_kernel_ms`: `k_lfield`, or the three kernels of §4.24).  {t['rounds']} rounds "
         "of a, b, c, d in turn (every second round in reverse order), each configuration in a fresh process; per configuration "
         "the median over the rounds and, in brackets, the least and the greatest round.", ""]
    for n in SIZES:
        L += [f"## {n} x 1081", "", "| | configuration | update ms | sensor kernels ms | beams skipped / used |", "|---|---|---:|---:|---:|"]
        for config in "abcd":
            rs = [r for r in t["runs"] if r["config"] == config and r["n"] == n]
            if not rs:
                continue
            u, k = [r["update_ms"] for r in rs], [r["kernel_ms"] for r in rs]
            sk = "" if config in "ab" else "%d / %d%s" % (np.median([x["n_skipped"] for r in rs for x in r["rows"]]), rs[0]["rows"][0]["n_used"],
                                                          " (integrate_all)" if any(x["integrate_all"] for r in rs for x in r["rows"]) else "")
            L.append(f"| {config} | {NAMES[config]} | {np.median(u):.3f} ({min(u):.3f} .. {max(u):.3f}) | "
                     f"{np.median(k):.3f} ({min(k):.3f} .. {max(k):.3f}) | {sk} |")
        L.append("")
    L += ["## The three kernels (rocprofv3 --kernel-trace --stats, one run per configuration, separate from the timing runs)", ""]
    any_k = False
    for n in SIZES:
        for config in "bcd":
            ks = _kernels(out, f"{config}_{n}")
            if ks:
                any_k = True
                L += [f"{config} ({NAMES[config]}) at {n} x 1081, calls x mean us:", ""] + [f"- `{name}`: {calls} x {us:.1f}" for name, calls, us in ks] + [""]
    if not any_k:
        L += ["Not measured.", ""]
    open(os.path.join(ROOT, "profiles", "beam_skip.md"), "w").write("\n".join(L))
    print("wrote profiles/beam_skip.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["measure", "child", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "beam_skip"))
    ap.add_argument("--parent-tree", default=None, help="measure: a checkout of the parent commit with its library built")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tree", default=ROOT, help="child: the tree whose package and library are measured")
    ap.add_argument("--config", choices=list("abcd"))
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.part == "measure":
        if not a.parent_tree:
            sys.exit("measure needs --parent-tree")
        measure(a.out, os.path.abspath(a.parent_tree), a.rounds)
    elif a.part == "child":
        child(os.path.abspath(a.tree), a.config, [int(v) for v in a.sizes.split(",")], a.json)
    else:
        report(a.out)


if __name__ == "__main__":
    main()
