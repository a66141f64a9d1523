"""Recovery by random-particle injection (mcl_set_recovery) on one MI355X: kidnap runs, spurious firing on a
correct trajectory, and the cost of the injecting resampling kernel; profiles/recovery.md is written from the parts.

  python tools/kidnap_recover.py kidnap   [--out DIR] [--sizes 1048576,4194304] [--alphas 0.001:0.1,...]
  python tools/kidnap_recover.py spurious [--out DIR]
  python tools/kidnap_recover.py cost     [--out DIR]          (run under rocprofv3 --kernel-trace --stats, in a run of its own)
  python tools/kidnap_recover.py report   --out DIR [--stats kernel_stats.csv]

Each part writes DIR/recovery_<part>.json; `report` turns them into profiles/recovery.md."""
import argparse
import csv
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

A = (0.0, 0.0, 0.0)                        # converged here
B = (-46.19, 29.66, -3.02)                 # then the scans come from here
SEED = 0x5EED_0000_0000_0009 + 12345
CONVERGE = 10
KIDNAP_UPDATES = 20


def _setup(n, kld=False, rec=None):
    from monte_carlo_localization_amd import engine, maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    ang = synth.beam_angles()
    e = engine.Engine(max_particles=n, seed=SEED)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    if kld:
        e.set_kld(max_particles=n)
    if rec is not None:
        e.set_recovery(alpha_slow=rec[0], alpha_fast=rec[1])
    return e, m, ang


def _err(e, truth):
    pose = e.expected_pose()
    return math.hypot(pose[0] - truth[0], pose[1] - truth[1]), math.degrees(abs((pose[2] - truth[2] + math.pi) % (2 * math.pi) - math.pi))


def kidnap(out, sizes, alphas):
    from monte_carlo_localization_amd import synth
    runs = []
    for n in sizes:
        for kld in (False, True):
            for rec in [None] + alphas:
                e, m, ang = _setup(n, kld, rec)
                scan_a, scan_b = synth.scan_from_pose(e, m, ang, A), synth.scan_from_pose(e, m, ang, B)
                e.init_particles_pose(A, n)
                rows = []
                for k in range(CONVERGE + KIDNAP_UPDATES):
                    kidnapped = k >= CONVERGE
                    p = e.recovery_state()[2]
                    e.update((0.0, 0.0, 0.0), scan_b if kidnapped else scan_a)
                    d, dth = _err(e, B if kidnapped else A)
                    rows.append(dict(update=k, kidnapped=kidnapped, p=p, injected=e.recovery_state()[3], n=e.n,
                                     err_m=d, err_deg=dth, ms=e.stage_timings()[5]))
                found = next((r["update"] - CONVERGE + 1 for r in rows if r["kidnapped"] and r["err_m"] < 0.25 and r["err_deg"] < 5), None)
                runs.append(dict(n=n, kld=kld, alphas=rec, found_after=found, rows=rows))
                print(f"n={n} kld={kld} rec={rec}: found after {found}; last error {rows[-1]['err_m']:.3f} m "
                      f"{rows[-1]['err_deg']:.2f} deg; injected {sum(r['injected'] for r in rows)}", flush=True)
                e.close()
    json.dump(dict(A=A, B=B, seed=SEED, converge=CONVERGE, runs=runs), open(os.path.join(out, "recovery_kidnap.json"), "w"))


def spurious(out, alphas, n=1 << 20, updates=40):
    """a moving robot, noise-free scans from the true trajectory, the filter tracking it: p per update"""
    from monte_carlo_localization_amd import synth
    from oracle import oracle as orc
    action = (0.1, 0.0, 0.02)             # (forward m, -, turn rad) per update, as mcl_update takes it
    runs = []
    for rec in alphas:
        e, m, ang = _setup(n, False, rec)
        truth = np.array(A, np.float64).reshape(3, 1)
        e.init_particles_pose(A, n)
        rows = []
        for k in range(updates):
            truth = orc.motion_model(truth, action, np.zeros((1, 3)))
            scan = synth.scan_from_pose(e, m, ang, truth[:, 0])
            p = e.recovery_state()[2]
            e.update(action, scan)
            d, dth = _err(e, truth[:, 0])
            rows.append(dict(update=k, p=p, injected=e.recovery_state()[3], err_m=d, err_deg=dth, S=e.recovery_state()[0], F=e.recovery_state()[1]))
        runs.append(dict(alphas=rec, n=n, action=action, rows=rows))
        print(f"spurious rec={rec}: max p {max(r['p'] for r in rows):.3g}, injecting updates {sum(r['injected'] > 0 for r in rows)}, "
              f"last error {rows[-1]['err_m']:.3f} m", flush=True)
        e.close()
    json.dump(dict(runs=runs), open(os.path.join(out, "recovery_spurious.json"), "w"))


def cost(out, n=1 << 22, reps=10):
    """the resampling kernel at 4M for p = 0 (the plain kernel), 0.01, 0.3, 1; and the whole injecting update"""
    from monte_carlo_localization_amd import synth
    e, m, ang = _setup(n, False, (0.001, 0.1))
    scan = synth.scan_from_pose(e, m, ang, A)
    e.init_particles_pose(A, n)
    for _ in range(3):
        e.update((0.0, 0.0, 0.0), scan)
    res = {}
    for p in (0.0, 0.01, 0.3, 1.0):
        ms = []
        for _ in range(reps):
            # converged set, then one update with p forced (the update after it is the ordinary one and is not timed)
            e.set_recovery_state(0.0, 0.0 if p == 0.0 else (-math.inf if p >= 1.0 else math.log1p(-p)))
            t = time.perf_counter()
            e.update((0.0, 0.0, 0.0), scan)
            ms.append(dict(total=(time.perf_counter() - t) * 1e3, resample=e.stage_timings()[0], injected=e.recovery_state()[3]))
            e.init_particles_pose(A, n)
            for _ in range(2):
                e.update((0.0, 0.0, 0.0), scan)
        res[str(p)] = ms
        print(f"p={p}: median total {np.median([r['total'] for r in ms]):.3f} ms, resampling stage "
              f"{np.median([r['resample'] for r in ms]):.3f} ms", flush=True)
    json.dump(dict(n=n, reps=reps, runs=res), open(os.path.join(out, "recovery_cost.json"), "w"))


def report(out, stats):
    lines = ["# Recovery by random-particle injection: kidnap runs and costs on one MI355X", ""]
    kp = os.path.join(out, "recovery_kidnap.json")
    if os.path.exists(kp):
        k = json.load(open(kp))
        lines += [f"Spielberg, 1081 beams, seed {k['seed']:#x}.  The set is initialised around A = {tuple(k['A'])} and converges there "
                  f"over {k['converge']} updates of noise-free scans from A, standing still; from update {k['converge']} on the scans come "
                  f"from B = {tuple(k['B'])} (the robot is carried there).  Pose errors are against A before the kidnap and B after it.  "
                  "ms: host wall time of the update (stage_timings total).", "",
                  "| N | KLD | alpha_slow / alpha_fast | found within 0.25 m / 5 deg after | error at the end m / deg | injected in all |",
                  "|---:|---|---|---:|---:|---:|"]
        for r in k["runs"]:
            last = r["rows"][-1]
            al = "off" if r["alphas"] is None else f"{r['alphas'][0]} / {r['alphas'][1]}"
            lines.append(f"| {r['n']} | {'on' if r['kld'] else 'off'} | {al} | "
                         f"{'not found' if r['found_after'] is None else str(r['found_after']) + ' updates'} | "
                         f"{last['err_m']:.3f} / {last['err_deg']:.2f} | {sum(x['injected'] for x in r['rows'])} |")
        for r in k["runs"]:
            al = "recovery off" if r["alphas"] is None else f"alpha {r['alphas'][0]} / {r['alphas'][1]}"
            lines += ["", f"### N = {r['n']}, KLD {'on' if r['kld'] else 'off'}, {al}", "",
                      "| update | scan from | p | injected | N | error m | error deg | ms |", "|---:|---|---:|---:|---:|---:|---:|---:|"]
            for x in r["rows"][k["converge"] - 2:]:
                lines.append(f"| {x['update']} | {'B' if x['kidnapped'] else 'A'} | {x['p']:.4g} | {x['injected']} | {x['n']} | "
                             f"{x['err_m']:.3f} | {x['err_deg']:.2f} | {x['ms']:.3f} |")
    else:
        lines += ["Kidnap runs: not measured."]
    sp = os.path.join(out, "recovery_spurious.json")
    lines += ["", "## Spurious firing: a moving robot tracked on its true trajectory", ""]
    if os.path.exists(sp):
        s = json.load(open(sp))
        for r in s["runs"]:
            ps = [x["p"] for x in r["rows"]]
            lines += [f"N = {r['n']}, action {tuple(r['action'])} per update, noise-free scans from the true pose, alpha "
                      f"{r['alphas'][0]} / {r['alphas'][1]}: max p {max(ps):.4g}, median p {np.median(ps):.4g}, updates that injected "
                      f"{sum(x['injected'] > 0 for x in r['rows'])} of {len(ps)}, children injected in all {sum(x['injected'] for x in r['rows'])}, "
                      f"pose error at the end {r['rows'][-1]['err_m']:.3f} m.", "",
                      "p per update: " + ", ".join(f"{v:.3g}" for v in ps), ""]
    else:
        lines += ["Not measured."]
    lines += ["", "## Cost of the injecting update at 4194304 particles x 1081 beams", ""]
    cp = os.path.join(out, "recovery_cost.json")
    if os.path.exists(cp):
        c = json.load(open(cp))
        lines += ["Converged tracking set; one update with p forced (set_recovery_state), median of "
                  f"{c['reps']}.  'resampling stage' is the engine's event time from the update's start to the end of the resampling kernel.", "",
                  "| p | injected | update ms (host wall) | resampling stage ms |", "|---:|---:|---:|---:|"]
        for p, ms in c["runs"].items():
            lines.append(f"| {p} | {int(np.median([r['injected'] for r in ms]))} | {np.median([r['total'] for r in ms]):.3f} | "
                         f"{np.median([r['resample'] for r in ms]):.3f} |")
    else:
        lines += ["Not measured."]
    lines += ["", "### Resampling kernels (rocprofv3 --kernel-trace --stats, the cost run above, in a run of its own)", ""]
    if stats and os.path.exists(stats):
        # the dispatches in order: 3 warm-up updates, then per forced p `reps` x (forced update, 2 ordinary updates after a
        # re-initialisation); the forced update's resampling kernel is the plain one for p = 0 and the _rec one otherwise
        import sqlite3
        db = sqlite3.connect(stats)
        ks = list(db.execute("select name, duration from kernels where name like '%k_resample_motion%' order by start"))
        redo = list(db.execute("select count(*), avg(duration), max(duration) from kernels where name like '%k_rays_skip<1, false, false>%'"))[0]
        c = json.load(open(cp)) if os.path.exists(cp) else dict(reps=10, runs={})
        reps = c["reps"]
        plain = [d for n, d in ks if "_rec" not in n]
        rec = [d for n, d in ks if "_rec" in n]
        forced = {"0.0 (k_resample_motion)": plain[3:3 + 3 * reps:3]}
        for i, p in enumerate(("0.01", "0.3", "1.0")):
            forced[f"{p} (k_resample_motion_rec)"] = rec[i * reps:(i + 1) * reps]
        lines += ["| p | kernel us, median | min | max |", "|---|---:|---:|---:|"]
        for p, ds in forced.items():
            lines.append(f"| {p} | {np.median(ds) / 1e3:.1f} | {min(ds) / 1e3:.1f} | {max(ds) / 1e3:.1f} |")
        lines += ["", f"k_rays_skip<1, false, false>, the engine's redo of a whole ray stage after its fix-up lists overflowed, ran "
                  f"{redo[0]} times in this trace (mean {redo[1] / 1e6:.1f} ms, max {redo[2] / 1e6:.1f} ms)."]
    else:
        lines += ["Not measured."]
    open(os.path.join(ROOT, "profiles", "recovery.md"), "w").write("\n".join(lines) + "\n")
    print("wrote profiles/recovery.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kidnap", "spurious", "cost", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "recovery"), help="where the parts write their JSON (build/ is not tracked)")
    ap.add_argument("--sizes", default="1048576,4194304")
    ap.add_argument("--alphas", default="0.001:0.1")
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    alphas = [tuple(float(v) for v in s.split(":")) for s in a.alphas.split(",")]
    if a.part == "kidnap":
        kidnap(a.out, [int(s) for s in a.sizes.split(",")], alphas)
    elif a.part == "spurious":
        spurious(a.out, alphas)
    elif a.part == "cost":
        cost(a.out)
    else:
        report(a.out, a.stats)


if __name__ == "__main__":
    main()
