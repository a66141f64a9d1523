#!/usr/bin/env python3
"""The likelihood-field sensor model (mcl_set_likelihood_field) against the beam model on one MI355X, on the
Spielberg map; profiles/likelihood_field.md is written from the parts.

  python tools/likelihood_field_bench.py timing [--out DIR] [--only NAME] [--tag TAG]
      ms per update (host wall, median) of both models at 2000 x 61, 262 144 x 1081 and 4 194 304 x 1081 (tracking, and the first
      update from a uniform cloud), the sensor kernel's event time and the field build (mcl_set_likelihood_field, host wall)
  python tools/likelihood_field_bench.py global [--out DIR]
      global localisation from a uniform 1M cloud under both models (the run of tests/test_gpu_likelihood_field.py): updates until
      the pose error is below 0.5 m / 0.1 rad, and the pose clusters along the way
  python tools/likelihood_field_bench.py report --out DIR
      profiles/likelihood_field.md from DIR/lf_timing.json, DIR/lf_global.json and, when present, the kernel statistics of
      rocprofv3 --kernel-trace --stats runs of `timing --only NAME --tag MODEL` written under DIR/prof/<NAME>_<MODEL>/

build/ is not tracked; the JSON parts go to build/likelihood_field by default."""
import argparse
import csv
import glob
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACTION = (0.05, 0.0, 0.01)                 # bench.py's action, with its scan (the golden scan from the origin)
CASES = [                                  # name, particles, beam step, regime
    ("2000x61", 2000, 18, "tracking"),
    ("262144x1081", 262144, 1, "tracking"),
    ("4194304x1081", 4194304, 1, "tracking"),
    ("4194304x1081_uniform", 4194304, 1, "uniform"),
]
WARMUP, STEPS, UNIFORM_REPS = 3, 20, 5
# the localisation run of tests/test_gpu_likelihood_field.py::test_global_localisation
LOC_N, LOC_SEED, LOC_START, LOC_ACTION, LOC_UPDATES = 1 << 20, 81, (-46.19, 29.66, -3.02), (0.05, 0.0, 0.01), 40


def _world(step):
    from monte_carlo_localization_amd import maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)[::step].copy()
    return m, synth.beam_angles(angle_step=step), scan


def _engine(n, m, ang, lf, seed=42):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=n, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    if lf:
        e.set_likelihood_field()
    return e


def _run_case(name, n, step, regime, lf):
    from monte_carlo_localization_amd import synth
    m, ang, scan = _world(step)
    e = _engine(n, m, ang, lf)
    rows = []

    def one():
        t0 = time.perf_counter()
        e.update(ACTION, scan)
        wall = (time.perf_counter() - t0) * 1e3
        rows.append(dict(wall_ms=wall, stages=[float(v) for v in e.stage_timings()], kernel_ms=e.ray_kernel_ms(),
                         kernel=None if lf else e.ray_kernel_name()))

    if regime == "tracking":
        e.set_particles(synth.tracking_cloud(np.random.default_rng(42), n), np.full(n, 1.0 / n))
        for _ in range(WARMUP):
            e.update(ACTION, scan)
        for _ in range(STEPS):
            one()
    else:
        e.init_global(n)
        e.update(ACTION, scan)                 # sizes every lazily allocated buffer
        for _ in range(UNIFORM_REPS):
            e.init_global(n)
            one()
    e.close()
    med = lambda k: float(np.median([r[k] for r in rows]))
    return dict(name=name, n=n, beams=int(ang.size), regime=regime, model="likelihood_field" if lf else "beam",
                update_ms=med("wall_ms"), kernel_ms=med("kernel_ms"), sensor_stage_ms=float(np.median([r["stages"][3] for r in rows])),
                kernel=rows[-1]["kernel"] or "k_lfield", rows=rows)


def field_build():
    m, ang, _ = _world(1)
    e = _engine(64, m, ang, False)
    ts = []
    for _ in range(7):
        e.set_likelihood_field(False)
        t0 = time.perf_counter()
        e.set_likelihood_field()
        ts.append((time.perf_counter() - t0) * 1e3)
    K = int(e.likelihood_table().size - 1)
    e.close()
    return dict(map="Spielberg_map", W=int(m.data.shape[1]), H=int(m.data.shape[0]), K=K, wall_ms=ts, median_ms=float(np.median(ts[1:])))


def timing(out, only, tag):
    res = dict(cases=[], field_build=None)
    for name, n, step, regime in CASES:
        if only and only != name:
            continue
        for lf in (False, True):
            if tag and tag != ("likelihood_field" if lf else "beam"):
                continue
            r = _run_case(name, n, step, regime, lf)
            print(f"{name} {r['model']}: {r['update_ms']:.3f} ms per update, {r['kernel']} {r['kernel_ms']:.3f} ms", flush=True)
            res["cases"].append(r)
    if not only:
        res["field_build"] = field_build()
        print(f"field build (Spielberg, K = {res['field_build']['K']}): {res['field_build']['median_ms']:.3f} ms", flush=True)
    json.dump(res, open(os.path.join(out, f"lf_timing{'_' + only if only else ''}{'_' + tag if tag else ''}.json"), "w"))


def global_run(out):
    from oracle import oracle as orc
    m, ang, _ = _world(1)
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    runs = []
    for lf in (False, True):
        e = _engine(LOC_N, m, ang, lf, seed=LOC_SEED)
        e.init_global(LOC_N)
        truth = np.array(LOC_START, np.float64).reshape(3, 1)
        rows, found = [], None
        for k in range(LOC_UPDATES):
            truth = orc.motion_model(truth, LOC_ACTION, np.zeros((1, 3)))
            x, y, th = truth[:, 0]
            scan, _ = orc.cast_many(om, np.full(ang.size, x), np.full(ang.size, y), th + ang.astype(np.float64))
            e.update(LOC_ACTION, scan)
            pose = e.expected_pose()
            d = math.hypot(pose[0] - x, pose[1] - y)
            dth = abs((pose[2] - th + math.pi) % (2 * math.pi) - math.pi)
            cl, info = e.pose_clusters(3)
            rows.append(dict(update=k + 1, err_m=d, err_rad=dth, ms=e.stage_timings()[5], n_clusters=info["n_clusters"],
                             top=[dict(weight=float(c["weight"]), mean=[float(v) for v in c["mean"]], n=int(c["n_particles"])) for c in cl]))
            if found is None and d < 0.5 and dth < 0.1:
                found = k + 1
        runs.append(dict(model="likelihood_field" if lf else "beam", found_after=found, rows=rows))
        print(f"global {runs[-1]['model']}: within 0.5 m / 0.1 rad after {found} updates; last error {rows[-1]['err_m']:.3f} m", flush=True)
        e.close()
    json.dump(dict(n=LOC_N, seed=LOC_SEED, start=LOC_START, action=LOC_ACTION, runs=runs), open(os.path.join(out, "lf_global.json"), "w"))


def _stats(out, name, model):
    """{kernel name: (calls, average us, total us)} of the rocprofv3 --stats run of one case and model, or None"""
    found = glob.glob(os.path.join(out, "prof", f"{name}_{model}", "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        return None
    st = {}
    for row in csv.DictReader(open(found[0])):
        st[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3, float(row["TotalDurationNs"]) / 1e3)
    return st


def _kernel_of(st, prefix):
    hits = [(k, v) for k, v in st.items() if prefix in k]
    if not hits:
        return None
    calls = sum(v[0] for _, v in hits)
    total = sum(v[2] for _, v in hits)
    return calls, total / calls, total


def report(out):
    L = ["# Likelihood-field sensor model against the beam model on one MI355X", "",
         "Written by `tools/likelihood_field_bench.py` (timing, global, report) from one MI355X run; the notes are by hand.", ""]
    tp = os.path.join(out, "lf_timing.json")
    if os.path.exists(tp):
        t = json.load(open(tp))
        L += ["## Update time", "",
              f"Spielberg map, bench.py's scan and action, seed 42.  ms: host wall time of `mcl_update`, median of {STEPS} updates after "
              f"{WARMUP} warm-up updates (tracking), or of {UNIFORM_REPS} first updates straight after `init_global` (uniform).  "
              "Sensor kernel: its HIP-event time inside the update (`mcl_get_ray_kernel_ms`: `k_lfield`, or the beam model's ray "
              "kernel; at 2000 x 61 the beam model runs the three-launch small update, whose whole tail that figure is), and its share "
              "of the update.", "",
              "| size | regime | beam model ms | likelihood field ms | speed-up | beam ray kernel (ms, share) | k_lfield (ms, share) |",
              "|---|---|---:|---:|---:|---|---|"]
        by = {(c["name"], c["model"]): c for c in t["cases"]}
        for name, n, step, regime in CASES:
            b, f = by.get((name, "beam")), by.get((name, "likelihood_field"))
            if not (b and f):
                continue
            L.append(f"| {n} x {b['beams']} | {regime} | {b['update_ms']:.3f} | {f['update_ms']:.3f} | {b['update_ms'] / f['update_ms']:.2f} | "
                     f"{b['kernel']} {b['kernel_ms']:.3f} ({b['kernel_ms'] / b['update_ms']:.0%}) | "
                     f"{f['kernel_ms']:.3f} ({f['kernel_ms'] / f['update_ms']:.0%}) |")
        fb = t.get("field_build")
        if fb:
            L += ["", f"Field build on {fb['map']} ({fb['W']} x {fb['H']}, K = {fb['K']}): `mcl_set_likelihood_field` takes "
                  f"{fb['median_ms']:.2f} ms host wall (median of {len(fb['wall_ms']) - 1} after a first call of {fb['wall_ms'][0]:.2f} ms; "
                  "the table on the host, two allocations, `k_lf_cols` + `k_lf_rows`, one synchronisation)."]
    else:
        L += ["Update times: not measured."]
    L += ["", "## Kernel statistics (rocprofv3 --kernel-trace --stats, one run per size and model, separate from the timing run)", ""]
    rows = []
    for name, n, step, regime in CASES:
        sb, sf = _stats(out, name, "beam"), _stats(out, name, "likelihood_field")
        if not (sb and sf):
            continue
        lfk = _kernel_of(sf, "k_lfield")
        ray = _kernel_of(sb, "k_rays_sweep") or _kernel_of(sb, "k_rays_skip")
        tot_b, tot_f = sum(v[2] for v in sb.values()), sum(v[2] for v in sf.values())
        cols = _kernel_of(sf, "k_lf_cols"), _kernel_of(sf, "k_lf_rows")
        rows.append(f"| {name} | {ray[0]} x {ray[1]:.1f} us ({ray[2] / tot_b:.0%} of kernel time) | "
                    f"{lfk[0]} x {lfk[1]:.1f} us ({lfk[2] / tot_f:.0%} of kernel time) | "
                    f"{(cols[0][1] + cols[1][1]) if all(cols) else float('nan'):.1f} us |")
    if rows:
        L += ["The share is of all kernel time of that run (set-up kernels included).", "",
              "| case | beam model ray kernel: calls x mean | k_lfield: calls x mean | field build kernels (cols + rows) |",
              "|---|---|---|---:|"] + rows
    else:
        L += ["Not measured."]
    L += ["", "## L2 traffic of k_lfield at 4 194 304 x 1081 (rocprofv3 --pmc TCC_HIT_sum TCC_MISS_sum, a run of its own)", ""]
    pm = []
    for name in ("4194304x1081", "4194304x1081_uniform"):
        found = glob.glob(os.path.join(out, "pmc", name, "**", "*counter_collection.csv"), recursive=True)
        if not found:
            continue
        acc = {}
        for row in csv.DictReader(open(found[0])):
            if "k_lfield" in row["Kernel_Name"]:
                acc.setdefault(row["Counter_Name"], []).append(float(row["Counter_Value"]))
        if "TCC_HIT_sum" in acc and "TCC_MISS_sum" in acc:
            h, mi = float(np.median(acc["TCC_HIT_sum"])), float(np.median(acc["TCC_MISS_sum"]))
            pm.append(f"| {name} | {h / 1e6:.1f} M | {mi / 1e6:.1f} M | {mi / (h + mi):.1%} |")
    L += (["Per launch (median over the run's launches); the field is 2000 x 2000 x 2 B = 8 MB, the L2 4 MiB per XCD.", "",
           "| case | L2 hits | L2 misses | miss rate |", "|---|---:|---:|---:|"] + pm) if pm else ["Not measured."]
    gp = os.path.join(out, "lf_global.json")
    L += ["", "## Global localisation on Spielberg", ""]
    if os.path.exists(gp):
        g = json.load(open(gp))
        L += [f"{g['n']} particles from `init_global`, seed {g['seed']}, 1081 beams; the robot starts at {tuple(g['start'])} and moves "
              f"{tuple(g['action'])} per update; scans are the oracle's ray casts from the true pose.  Found: the first update after which "
              "the expected pose is within 0.5 m / 0.1 rad.  Clusters: `pose_clusters` (0.5 m x 0.5 m x 10 degrees), the heaviest three.", "",
              "| model | found after | error at the end m / rad |", "|---|---:|---:|"]
        for r in g["runs"]:
            last = r["rows"][-1]
            L.append(f"| {r['model']} | {r['found_after'] if r['found_after'] else 'not found'} | {last['err_m']:.3f} / {last['err_rad']:.3f} |")
        for r in g["runs"]:
            L += ["", f"### {r['model']}", "", "| update | error m | error rad | clusters | heaviest: weight @ (x, y, heading) | ms |",
                  "|---:|---:|---:|---:|---|---:|"]
            for x in r["rows"]:
                top = "; ".join(f"{c['weight']:.3f} @ ({c['mean'][0]:.2f}, {c['mean'][1]:.2f}, {c['mean'][2]:.2f})" for c in x["top"])
                L.append(f"| {x['update']} | {x['err_m']:.3f} | {x['err_rad']:.3f} | {x['n_clusters']} | {top} | {x['ms']:.2f} |")
    else:
        L += ["Not measured."]
    open(os.path.join(ROOT, "profiles", "likelihood_field.md"), "w").write("\n".join(L) + "\n")
    print("wrote profiles/likelihood_field.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["timing", "global", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "likelihood_field"))
    ap.add_argument("--only", default=None, help="timing: one case by name")
    ap.add_argument("--tag", default=None, choices=[None, "beam", "likelihood_field"], help="timing: one model")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.part == "timing":
        timing(a.out, a.only, a.tag)
    elif a.part == "global":
        global_run(a.out)
    else:
        report(a.out)


if __name__ == "__main__":
    main()
