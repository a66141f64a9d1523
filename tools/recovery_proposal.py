"""Recovery from a pose mixture (mcl_set_recovery_proposal) on one MI355X beside recovery from free space: the
twelve kidnap rows of profiles/recovery.md rerun, each beside the same run with Engine.propose_from_scan before every update whose
p > 0; the cost of the injecting update at 4M x 1081 under both sources; the resampling kernels and the ray stage's redo from a
kernel trace.  profiles/recovery_proposal.md is written from the parts.

  python tools/recovery_proposal.py kidnap [--out DIR] [--sizes 1048576,4194304] [--alphas 0.001:0.1,0.01:0.5]
  python tools/recovery_proposal.py cost   [--out DIR] [--reps 5]      (once plainly; once more under rocprofv3 --kernel-trace --stats --output-format csv,
                                                                       in a run of its own, for the kernel times)
  python tools/recovery_proposal.py report --out DIR [--stats kernel_trace.csv]

Each part writes DIR/recovery_proposal_<part>.json."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kidnap_recover import A, B, CONVERGE, KIDNAP_UPDATES, SEED, _err, _setup    # noqa: E402  (the runs of profiles/recovery.md)

SEARCH = dict(beam_stride=10, stride_cells=4)          # the thinned search of tests/test_gpu_recovery_proposal.py
FORCED = (0.01, 0.3, 1.0)


def kidnap(out, sizes, alphas):
    from monte_carlo_localization_amd import synth
    runs = []
    for n in sizes:
        for kld in (False, True):
            for rec in [None] + alphas:
                for propose in ((False,) if rec is None else (False, True)):
                    e, m, ang = _setup(n, kld, rec)
                    scan_a, scan_b = synth.scan_from_pose(e, m, ang, A), synth.scan_from_pose(e, m, ang, B)
                    e.init_particles_pose(A, n)
                    rows, search_ms, rank = [], [], None
                    for k in range(CONVERGE + KIDNAP_UPDATES):
                        kidnapped = k >= CONVERGE
                        scan = scan_b if kidnapped else scan_a
                        p = e.recovery_state()[2]
                        if propose and p > 0:
                            t = time.perf_counter()
                            hits = e.propose_from_scan(scan, **SEARCH)
                            search_ms.append((time.perf_counter() - t) * 1e3)
                            d = np.hypot(hits["pose"][:, 0] - B[0], hits["pose"][:, 1] - B[1])
                            near = np.flatnonzero(d < 0.5)
                            rank = int(near[0]) if near.size else -1
                        e.update((0.0, 0.0, 0.0), scan)
                        d, dth = _err(e, B if kidnapped else A)
                        rows.append(dict(update=k, kidnapped=kidnapped, p=p, injected=e.recovery_state()[3], n=e.n, err_m=d, err_deg=dth,
                                         ms=e.stage_timings()[5]))
                    found = next((r["update"] - CONVERGE + 1 for r in rows if r["kidnapped"] and r["err_m"] < 0.25 and r["err_deg"] < 5), None)
                    runs.append(dict(n=n, kld=kld, alphas=rec, propose=propose, found_after=found, rows=rows, search_ms=search_ms, hit_rank=rank))
                    print(f"n={n} kld={kld} rec={rec} propose={propose}: found after {found}; last error {rows[-1]['err_m']:.3f} m "
                          f"{rows[-1]['err_deg']:.2f} deg; injected {sum(r['injected'] for r in rows)}; searches {len(search_ms)}", flush=True)
                    e.close()
    json.dump(dict(A=A, B=B, seed=SEED, converge=CONVERGE, search=SEARCH, runs=runs), open(os.path.join(out, "recovery_proposal_kidnap.json"), "w"))


def cost(out, n=1 << 22, reps=5):
    """one update with p forced on a converged 4M set, the injected children from free space and from a proposal, in one process"""
    from monte_carlo_localization_amd import synth
    e, m, ang = _setup(n, False, (0.001, 0.1))
    scan = synth.scan_from_pose(e, m, ang, A)
    e.init_particles_pose(A, n)
    for _ in range(3):
        e.update((0.0, 0.0, 0.0), scan)
    hits = e.propose_from_scan(scan, **SEARCH)          # the proposal of the scan at A: what a recovery at A would draw from
    prop = e.recovery_proposal()
    e.set_recovery_proposal(None)
    r, _ = e.refine_poses_beam(hits["pose"], scan)
    res = {}
    for p in FORCED:
        for source in ("uniform", "mixture"):
            ms = []
            for _ in range(reps):
                if source == "mixture":
                    e.set_recovery_proposal(r["mean"], r["cov"])
                e.set_recovery_state(0.0, -math.inf if p >= 1.0 else math.log1p(-p))
                t = time.perf_counter()
                e.update((0.0, 0.0, 0.0), scan)
                ms.append(dict(total=(time.perf_counter() - t) * 1e3, resample=e.stage_timings()[0], injected=e.recovery_state()[3],
                               kernel=e.ray_kernel_name()))
                e.init_particles_pose(A, n)
                for _ in range(2):
                    e.update((0.0, 0.0, 0.0), scan)
            res[f"{p}/{source}"] = ms
            print(f"p={p} {source}: median total {np.median([x['total'] for x in ms]):.3f} ms, resampling stage "
                  f"{np.median([x['resample'] for x in ms]):.3f} ms, ray kernel {ms[-1]['kernel']}", flush=True)
    json.dump(dict(n=n, reps=reps, components=int(prop[0].size), runs=res), open(os.path.join(out, "recovery_proposal_cost.json"), "w"))


def report(out, stats):
    lines = ["# Recovery from a pose mixture beside recovery from free space, on one MI355X", "",
             "Written by `tools/recovery_proposal.py` (kidnap, cost, report).  Nothing here is a pass/fail number: each figure stands beside "
             "the uniform source's in the same run, and beside `profiles/recovery.md` as recorded.", ""]
    kp = os.path.join(out, "recovery_proposal_kidnap.json")
    if os.path.exists(kp):
        k = json.load(open(kp))
        lines += [f"## Kidnap runs", "",
                  f"Spielberg, 1081 beams, seed {k['seed']:#x}; A = {tuple(k['A'])}, {k['converge']} converging updates, then {KIDNAP_UPDATES} "
                  f"updates of scans from B = {tuple(k['B'])}, standing still -- the runs of `profiles/recovery.md`.  'proposal': "
                  f"`propose_from_scan(scan, {', '.join(f'{a}={b}' for a, b in k['search'].items())})` before every update whose p > 0 "
                  "(the search of the model in use, refined, equal weights).  hit rank: the rank of the first hit within 0.5 m of B in the "
                  "last search.", "",
                  "| N | KLD | alpha_slow / alpha_fast | source | found within 0.25 m / 5 deg after | error at the end m / deg | injected in all | "
                  "searches | search + refine ms, median | hit rank |", "|---:|---|---|---|---:|---:|---:|---:|---:|---:|"]
        for r in k["runs"]:
            last = r["rows"][-1]
            al = "off" if r["alphas"] is None else f"{r['alphas'][0]} / {r['alphas'][1]}"
            src = "-" if r["alphas"] is None else ("proposal" if r["propose"] else "free cells")
            sm = f"{np.median(r['search_ms']):.1f}" if r["search_ms"] else "-"
            lines.append(f"| {r['n']} | {'on' if r['kld'] else 'off'} | {al} | {src} | "
                         f"{'not found' if r['found_after'] is None else str(r['found_after']) + ' updates'} | "
                         f"{last['err_m']:.3f} / {last['err_deg']:.2f} | {sum(x['injected'] for x in r['rows'])} | {len(r['search_ms'])} | {sm} | "
                         f"{'-' if r['hit_rank'] is None else r['hit_rank']} |")
        kl = [r for r in k["runs"] if r["kld"] and r["propose"]]
        if kl:
            lines += ["", "`tests/test_gpu_recovery_proposal.py::test_kidnap_with_kld` is the KLD-on row at 65 536 particles with `min_particles` 512.  "
                      "It uses the first pose of its candidate list, B itself; in the KLD-on runs above the thinned search on the scan at B "
                      f"returns a hit within 0.5 m of B at rank {', '.join(sorted({str(r['hit_rank']) for r in kl}))}."]
        lines += ["", "The injecting update of every run (the first update with p > 0):", "",
                  "| N | KLD | alphas | source | p | injected | N of the update | error after it m | update ms |", "|---:|---|---|---|---:|---:|---:|---:|---:|"]
        for r in k["runs"]:
            x = next((x for x in r["rows"] if x["injected"] > 0), None)
            if x:
                lines.append(f"| {r['n']} | {'on' if r['kld'] else 'off'} | {r['alphas'][0]} / {r['alphas'][1]} | "
                             f"{'proposal' if r['propose'] else 'free cells'} | {x['p']:.4g} | {x['injected']} | {x['n']} | {x['err_m']:.3f} | {x['ms']:.3f} |")
    else:
        lines += ["Kidnap runs: not measured."]
    lines += ["", "## Cost of the injecting update at 4194304 particles x 1081 beams", ""]
    cp = os.path.join(out, "recovery_proposal_cost.json")
    c = json.load(open(cp)) if os.path.exists(cp) else None
    if c:
        lines += [f"Converged tracking set at A; one update with p forced (set_recovery_state), median of {c['reps']}, both sources in one "
                  f"process.  The proposal is `propose_from_scan` of the scan at A ({c['components']} components).  'resampling stage' is the "
                  "engine's event time from the update's start to the end of the resampling kernel.", "",
                  "| p | source | injected | update ms (host wall) | resampling stage ms | ray kernel of the update |", "|---:|---|---:|---:|---:|---|"]
        for key, ms in c["runs"].items():
            p, source = key.split("/")
            lines.append(f"| {p} | {source} | {int(np.median([x['injected'] for x in ms]))} | {np.median([x['total'] for x in ms]):.3f} | "
                         f"{np.median([x['resample'] for x in ms]):.3f} | {ms[-1]['kernel']} |")
    else:
        lines += ["Not measured."]
    lines += ["", "### Resampling kernels and the ray stage's redo (rocprofv3 --kernel-trace --stats, the cost run above, in a run of its own)", ""]
    if stats and os.path.exists(stats) and c:
        # the kernel trace as CSV (rocprofv3 --kernel-trace --stats --output-format csv): one row per dispatch
        import csv
        rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"])
                       for r in csv.DictReader(open(stats))), key=lambda r: r[0])
        reps = c["reps"]
        rec = [d for _, d, n in rows if "k_resample_motion_rec" in n]
        mix = [d for _, d, n in rows if "k_resample_motion_mix" in n]
        lines += ["| p | kernel | us, median | min | max |", "|---:|---|---:|---:|---:|"]
        for i, p in enumerate(FORCED):
            for name, ds in (("k_resample_motion_rec", rec[i * reps:(i + 1) * reps]), ("k_resample_motion_mix", mix[i * reps:(i + 1) * reps])):
                if ds:
                    lines.append(f"| {p} | {name} | {np.median(ds) / 1e3:.1f} | {min(ds) / 1e3:.1f} | {max(ds) / 1e3:.1f} |")
        # the redo: k_rays_skip<1, false, false> dispatches, attributed to the source of the injecting update before them
        marks = [(t, n) for t, _, n in rows if "k_resample_motion_rec" in n or "k_resample_motion_mix" in n or "k_rays_skip<1, false, false>" in n]
        redo, cur = {"uniform": [], "mixture": []}, None
        for _, name in marks:
            if "k_resample_motion_rec" in name:
                cur = "uniform"
            elif "k_resample_motion_mix" in name:
                cur = "mixture"
            elif cur:
                redo[cur].append(1)
                cur = None
        n_inj = len(FORCED) * reps
        lines += ["", f"`k_rays_skip<1, false, false>`, the engine's redo of a whole ray stage after its fix-up lists overflowed, followed "
                  f"{len(redo['uniform'])} of the {n_inj} injecting updates from free cells and {len(redo['mixture'])} of the {n_inj} from the proposal."]
        if redo["uniform"] and not redo["mixture"]:
            lines += ["The redo does not appear under the mixture.  That supports the explanation `profiles/recovery.md` calls probable -- "
                      "free-cell poses sit exactly on cell corners, mixture poses come off the lattice -- without isolating it: the mixture's "
                      "children also stand on a few spots instead of all over the map.  The uniform rule is left as it is."]
        elif redo["mixture"]:
            lines += ["The redo still appears under the mixture: poses off the cell lattice do not remove it, so the cell-corner explanation of "
                      "`profiles/recovery.md` is not what causes it (or not alone)."]
    else:
        lines += ["Not measured."]
    open(os.path.join(ROOT, "profiles", "recovery_proposal.md"), "w").write("\n".join(lines) + "\n")
    print("wrote profiles/recovery_proposal.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["kidnap", "cost", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "recovery_proposal"), help="where the parts write their JSON (build/ is not tracked)")
    ap.add_argument("--sizes", default="1048576,4194304")
    ap.add_argument("--alphas", default="0.001:0.1,0.01:0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    alphas = [tuple(float(v) for v in s.split(":")) for s in a.alphas.split(",")]
    if a.part == "kidnap":
        kidnap(a.out, [int(s) for s in a.sizes.split(",")], alphas)
    elif a.part == "cost":
        cost(a.out, reps=a.reps)
    else:
        report(a.out, a.stats)


if __name__ == "__main__":
    main()
