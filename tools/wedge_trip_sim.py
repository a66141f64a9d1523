#!/usr/bin/env python3
"""CPU simulation of the probe trips of the beam walk under the two wedge-field rules (csrc/mcl_wedge.h): the Euclidean one
(mcl_host_skip_field_wedge) and the tight one (mcl_host_skip_field_wedge_tight).  No GPU: the fields come from the library's
host twins, the march is numpy.

The cloud is G wave-like groups of 64 particles: a group shares a half cell (the finest unit of the ordering) and
its headings lie within --heading-span rad, as the 64 lanes of a wave of k_rays_sweep do; every particle casts all beams.  The
march follows the walk's rule: the first sample lies the own cell's skip away (at least one), every sample examined is a trip,
the walk ends on a stop byte or when the skip exceeds the samples left.  Printed per rule: trips per ray (the per-lane mean) and
trips per group of 64 (the lock-step cost: the slowest lane of a group, per beam), and whether the hit indices agree.

Fields are built on a crop of the map around the pose: range + 127 (the cap of a device skip) + the cloud's spread, so every
byte a ray can read is what the whole map would give.

usage: wedge_trip_sim.py [--map spielberg|levine|fine025|<file.npz>] [--pose X Y TH] [--range-m 12] [--groups 40]
                         [--sigma-m 0.05] [--sigma-th 0.02] [--beam-step 1] [--seed 0]
"""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAP = 127          # k_wedge_field stores skips capped at 127


def load_map(name, maps):
    base = os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz")
    if name == "spielberg":
        return maps.load_npz(base)
    if name == "fine025":
        return maps.synthetic_fine025(maps.load_npz(base))
    if name == "levine":
        return maps.synthetic_levine()
    return maps.load_npz(name)


def march(F, P, px, py, ang, K):
    """F[k]: padded fields of a crop (uint8, 0 = stop); px, py in crop pixels.  Returns (hit step index, trips) per ray."""
    k = np.floor(ang * (K / (2 * math.pi))).astype(np.int64) % K
    ux, uy = np.cos(ang), np.sin(ang)
    Hp, Wp = F.shape[1:]

    def cell_byte(x, y):
        cx, cy = np.floor(x).astype(np.int64) + 1, np.floor(y).astype(np.int64) + 1
        inside = (cx >= 0) & (cx < Wp) & (cy >= 0) & (cy < Hp)
        return np.where(inside, F[k, np.clip(cy, 0, Hp - 1), np.clip(cx, 0, Wp - 1)], 0)

    s = np.maximum(cell_byte(px, py), 1).astype(np.int64)
    hit = np.full(px.shape, P, np.int64)
    trips = np.zeros(px.shape, np.int64)
    live = s <= P
    while live.any():
        d = cell_byte(px + s * ux, py + s * uy).astype(np.int64)
        trips += live
        stop = live & (d == 0)
        hit[stop] = s[stop] - 1
        s = np.where(live & ~stop, s + d, s)
        live = live & ~stop & (s <= P)
    return hit, trips


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map", default="spielberg")
    ap.add_argument("--pose", type=float, nargs=3, default=(1.09, 0.29, 0.0), metavar=("X", "Y", "TH"))
    ap.add_argument("--range-m", type=float, default=12.0)
    ap.add_argument("--groups", type=int, default=40)
    ap.add_argument("--sigma-m", type=float, default=0.05)
    ap.add_argument("--sigma-th", type=float, default=0.02)
    ap.add_argument("--heading-span", type=float, default=2e-3)
    ap.add_argument("--beam-step", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from monte_carlo_localization_amd import engine, maps, synth
    m = load_map(args.map, maps)
    res = float(m.resolution)
    P = int(args.range_m / res)
    K = engine.WEDGES
    rng = np.random.default_rng(args.seed)
    ang = synth.beam_angles(angle_step=args.beam_step).astype(np.float64)
    G, B = args.groups, ang.size

    # groups: a cell and one of its halves (in x), 64 origins inside it, headings within the span
    gx = (args.pose[0] - m.origin_x + rng.normal(0, args.sigma_m, G)) / res
    gy = (args.pose[1] - m.origin_y + rng.normal(0, args.sigma_m, G)) / res
    half = np.floor(gx * 2) / 2
    px = (half[:, None] + 0.5 * rng.random((G, 64)))
    py = (np.floor(gy)[:, None] + rng.random((G, 64)))
    th = (args.pose[2] + rng.normal(0, args.sigma_th, G))[:, None] + rng.uniform(0, args.heading_span, (G, 64))

    margin = P + CAP + 8
    x0, x1 = int(px.min()) - margin, int(px.max()) + margin + 1
    y0, y1 = int(py.min()) - margin, int(py.max()) + margin + 1
    H, W = m.data.shape
    crop = np.full((y1 - y0, x1 - x0), 100, np.int8)                      # outside the map: stop
    sy0, sy1, sx0, sx1 = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
    crop[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = m.data[sy0:sy1, sx0:sx1]
    print(f"map {args.map}: {W} x {H} @ {res:.4f} m, range {P} px, crop {crop.shape[1]} x {crop.shape[0]}, "
          f"{G} groups x 64 particles x {B} beams = {G * 64 * B} rays", flush=True)

    rx = np.repeat((px - x0).ravel(), B)
    ry = np.repeat((py - y0).ravel(), B)
    ra = (th.ravel()[:, None] + ang[None, :]).ravel()
    results = {}
    for rule, build in (("euclidean", engine.host_skip_field_wedge), ("tight", engine.host_skip_field_wedge_tight)):
        F = np.stack([np.minimum(build(crop, k), CAP) for k in range(K)])
        hit, trips = march(F, P, rx, ry, ra, K)
        per_group = trips.reshape(G, 64, B).max(axis=1)
        results[rule] = (F, hit, trips.mean(), per_group.mean())
        print(f"{rule:10s} trips per ray {trips.mean():.3f}   trips per group of 64 {per_group.mean():.3f}", flush=True)
    Fe, he, te, ge = results["euclidean"]
    Ft, ht, tt, gt = results["tight"]
    print(f"hit index identical on {int((he == ht).sum())} of {he.size} rays; cells with a smaller skip under the tight rule: "
          f"{int((Ft < Fe).sum())}; with a larger one: {int((Ft > Fe).sum())} of {int((Fe > 0).sum())} free cells x wedges")
    print(f"tight / euclidean: per ray {tt / te:.4f}, per group {gt / ge:.4f}")
    return 0 if (he == ht).all() and not (Ft < Fe).any() else 1


if __name__ == "__main__":
    sys.exit(main())
