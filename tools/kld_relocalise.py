#!/usr/bin/env python3
"""KLD-adaptive particle count measured on one GPU: a global re-localisation on Spielberg from a uniform
cloud of 4 194 304 particles with 1081 beams, per update N, occupied bins, ms and pose error; then the cost of the bin marking
with the size pinned (KLD on, min = max = 4M, against KLD off in the same process) and the cost at the converged size (the KLD
engine against a plain engine of the same N).  Prints markdown (profiles/kld_relocalise.md is its output).

usage: tools/kld_relocalise.py [--n 4194304] [--updates 30] [--reps 20] [--seed 81] [--out FILE]

Beside the KLD run, an engine without KLD runs the same updates from the same cloud (same seed) and scan: its pose error is the
control column.

ms per update: the engine's stage timings -- events on its stream for a regular update (sum of the five stages), the host's
wall clock around a captured-graph or three-launch small update, whose single stage is the whole update (mcl_get_stage_timings)."""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TRUTH = np.array([-46.19, 29.66, -3.02])    # a pose from which the filter without KLD localises on this map


def engine_for(E, m, ang, cap, seed):
    e = E.Engine(max_particles=cap, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    return e


def update_ms(e):
    t = e.stage_timings()
    return float(t[5]) if t[0] == 0.0 and t[3] == t[5] else float(t[:5].sum())


def pose_err(p):
    return float(np.hypot(p[0] - TRUTH[0], p[1] - TRUTH[1])), float(np.degrees(abs((p[2] - TRUTH[2] + np.pi) % (2 * np.pi) - np.pi)))


def timed(e, scan, reps):
    ms = []
    for _ in range(reps):
        e.update((0.0, 0.0, 0.0), scan)
        ms.append(update_ms(e))
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4194304)
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=81)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from monte_carlo_localization_amd import engine as E, maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    ang = synth.beam_angles()
    lines = []
    say = lines.append

    # 1. global re-localisation with KLD on
    e = engine_for(E, m, ang, args.n, args.seed)
    ctl = engine_for(E, m, ang, args.n, args.seed)
    scan = synth.scan_from_pose(e, m, ang, TRUTH)
    e.init_global(args.n)
    ctl.init_global(args.n)
    k = e.set_kld(min_particles=256, max_particles=args.n)
    say(f"# KLD-adaptive particle count: global re-localisation on Spielberg, {args.n} particles x {ang.size} beams\n")
    say(f"KLD: err {k.err}, z {k.z}, bins {k.bin_x_m} m x {k.bin_y_m} m x {k.n_theta_bins} headings, round_to {k.round_to}, "
        f"shrink_permille {k.shrink_permille}, min {k.min_particles}, max {k.max_particles}; truth pose {TRUTH.tolist()}, "
        "the robot standing still (action 0), noise-free scan from the truth.\n")
    say("| update | N drawn | bins of the draw | N next | ray kernel | ms | pose error m | pose error deg | KLD off: error m / deg |")
    say("|---:|---:|---:|---:|---|---:|---:|---:|---:|")
    for u in range(args.updates):
        e.update((0.0, 0.0, 0.0), scan)
        ctl.update((0.0, 0.0, 0.0), scan)
        bins, n_next = e.kld_state()
        d, dth = pose_err(e.expected_pose())
        cd, cdth = pose_err(ctl.expected_pose())
        say(f"| {u} | {e.n} | {bins} | {n_next} | {e.ray_kernel_name()} | {update_ms(e):.3f} | {d:.3f} | {dth:.2f} | {cd:.3f} / {cdth:.2f} |")
    ctl.close()
    n_conv = e.n
    conv = timed(e, scan, args.reps)
    say("")

    # 2. converged size: the KLD engine against a plain engine of the same N
    plain = engine_for(E, m, ang, max(n_conv, 1), 7)
    plain.set_particles(synth.tracking_cloud(np.random.default_rng(1), n_conv, sig=(0.05, 0.05, 0.02)), np.full(n_conv, 1.0 / n_conv))
    timed(plain, scan, 3)
    ref = timed(plain, scan, args.reps)
    say(f"## Converged size: N = {n_conv}\n")
    say("| engine | ms per update (median of %d) | min | ray kernel |" % args.reps)
    say("|---|---:|---:|---|")
    say(f"| KLD on (converged run) | {np.median(conv):.4f} | {conv.min():.4f} | {e.ray_kernel_name()} |")
    say(f"| plain engine, same N | {np.median(ref):.4f} | {ref.min():.4f} | {plain.ray_kernel_name()} |")
    # the same engine held at that size (min = max = N: no growth, no graph reset, no jump to max_particles on a one-bin draw)
    e.set_kld(min_particles=n_conv, max_particles=n_conv)
    timed(e, scan, 3)
    held = timed(e, scan, args.reps)
    say(f"| KLD on, held at N (min = max) | {np.median(held):.4f} | {held.min():.4f} | {e.ray_kernel_name()} |")
    say("")
    e.close()
    plain.close()

    # 3. KLD on but pinned (min = max = N) against KLD off, same process, alternating
    say(f"## Bin marking at {args.n}: KLD on with the size pinned (min = max = N) against KLD off\n")
    for regime in ("tracking", "uniform"):
        engs = {}
        for name in ("off", "pinned"):
            x = engine_for(E, m, ang, args.n, 11)
            if regime == "tracking":
                x.init_particles_pose(TRUTH, args.n)
            else:
                x.init_global(args.n)
            if name == "pinned":
                x.set_kld(min_particles=args.n, max_particles=args.n)
            engs[name] = x
        res = {name: [] for name in engs}
        for r in range(args.reps):
            for name, x in engs.items():
                if regime == "uniform":              # a fresh uniform cloud every time: the draw's bins are the spread set's
                    x.init_global(args.n)
                x.update((0.0, 0.0, 0.0), scan)
                if r >= 2:
                    res[name].append(update_ms(x))
        off, pin = np.array(res["off"]), np.array(res["pinned"])
        bins = engs["pinned"].kld_state()[0]
        say(f"- {regime} cloud: off {np.median(off):.4f} ms, pinned {np.median(pin):.4f} ms (medians of {off.size}), "
            f"{100.0 * (np.median(pin) / np.median(off) - 1.0):+.2f} %; bins of the last draw {bins}")
        for x in engs.values():
            x.close()
    say("")

    # 4. register figures of the resampling kernel in the library that ran
    lib = os.path.join(ROOT, "monte_carlo_localization_amd", "libmcl_hip_engine.so")
    try:
        meta = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_meta.py"), lib, "--out", "/tmp/mcl_kld_meta.co"],
                              capture_output=True, text=True, timeout=300).stdout
        say("## tools/kernel_meta.py\n")
        say("```")
        for ln in meta.splitlines():
            if "k_resample_motion" in ln or "k_kld_clear" in ln or "k_tiny_tail" in ln:
                say(ln.rstrip())
        say("```")
    except (OSError, subprocess.SubprocessError) as ex:
        say(f"(kernel_meta.py failed: {ex})")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
