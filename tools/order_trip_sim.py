#!/usr/bin/env python3
"""CPU simulation of what the ORDER of the particles costs the beam walk: probe trips per ray (the per-lane mean) against probe
trips per wave (the slowest of 64 lanes, which is what a wave pays), for a list of fine-bit settings of the ordering key
(csrc/mcl_sort_key.h).  No GPU: the keys are the host twin's (engine.host_sort_key), the fields the library's
(engine.host_skip_field_wedge_tight), the march is tools/wedge_trip_sim.py's.

A synthetic cloud N(pose, sigma) -- or a real set, --particles FILE.npy (3 x n: `bench.py --dump-outputs DIR` writes
DIR/particles.npy, a sample of the set: give the set's size with --set-size, it decides the layout) -- is keyed under the layout
the engine would make for it (bounding box of its cells, occupied tiles numbered compactly) and sorted; --runs random runs of 64
consecutive slots of the sorted order stand for waves.  Two ways to pair the lanes' rays:
  beam       lane i casts beam j when the wave is at beam j (headings apart -> directions apart);
  direction  what k_rays_sweep does: the wave walks the scan's angular GRID continued over all headings, and every lane casts its
             own beam nearest the grid direction, so the lanes' directions differ by at most half a beam increment whatever their
             headings (a lane without a beam there idles).  Under this pairing finer heading bits have little left to give.

usage: order_trip_sim.py [--map spielberg|levine|fine025|<file.npz>] [--pose X Y TH] [--sigma SX SY STH] [--n 4194304]
                         [--particles FILE.npy] [--set-size N] [--runs 48] [--fine 0,2,6,2:1] [--range-m 12] [--seed 0]
A --fine entry is F or F:FS (FS of the F bits per axis are sub-cell bits; default: the rule, max(F - 2, 0) // 4).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from wedge_trip_sim import CAP, load_map, march          # noqa: E402


def layout_of(px, py, W, H, engine):
    """the layout words and tile map the engine would make for these pixel coordinates (every particle sampled, no window play)"""
    cx = np.clip(np.floor(px).astype(np.int64) + 1, 0, W)
    cy = np.clip(np.floor(py).astype(np.int64) + 1, 0, H)
    ntx, nty = engine.sort_tile_grid(W, H)
    bbox = np.array([cx.min(), cy.min(), cx.max(), cy.max(), 0, 0, 0], np.int32)
    tm = None
    if ntx * nty <= 8192:
        used = np.zeros(ntx * nty, bool)
        used[(cy >> 5) * ntx + (cx >> 5)] = True
        tm = np.full(ntx * nty, int(used.sum()), np.int32)
        tm[used] = np.arange(int(used.sum()), dtype=np.int32)
        bbox[4], bbox[5] = int(used.sum()), 1
    return bbox, tm


def wave_trips(F, P, K, px, py, th, ang, align):
    """(trips per ray, trips per wave and step) of runs x 64 particles; px, py in crop pixels"""
    R, B = px.shape[0], ang.size
    if align == "beam":
        ra = th[:, :, None] + ang[None, None, :]
        has = np.ones(ra.shape, bool)
    else:
        inc = (ang[-1] - ang[0]) / (B - 1)
        # grid directions a0 + g inc over the union of the lanes' scans; lane i's beam for direction g is j = g - round((th_i - th_0) / inc)
        off = np.rint((th - th[:, :1]) / inc).astype(np.int64)
        lo, hi = off.min(axis=1), off.max(axis=1)
        G = B + int((hi - lo).max())
        g = np.arange(G)[None, None, :] + lo[:, None, None]
        j = g - off[:, :, None]
        has = (j >= 0) & (j < B)
        ra = th[:, :, None] + ang[np.clip(j, 0, B - 1)]
    shape = ra.shape
    rx = np.broadcast_to(px[:, :, None], shape)[has]
    ry = np.broadcast_to(py[:, :, None], shape)[has]
    _, t = march(F, P, rx, ry, ra[has], K)
    trips = np.zeros(shape, np.int64)
    trips[has] = t
    per_wave = trips.max(axis=1)
    steps = has.any(axis=1)
    return t.mean(), per_wave[steps].mean() if align == "beam" else per_wave.sum() / (R * B)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--map", default="spielberg")
    ap.add_argument("--pose", type=float, nargs=3, default=(1.09, 0.29, 0.0), metavar=("X", "Y", "TH"))
    ap.add_argument("--sigma", type=float, nargs=3, default=(0.06, 0.035, 0.25), metavar=("SX", "SY", "STH"))
    ap.add_argument("--n", type=int, default=4194304)
    ap.add_argument("--particles")
    ap.add_argument("--set-size", type=int)
    ap.add_argument("--runs", type=int, default=48)
    ap.add_argument("--fine", default="0,2,6,2:1")
    ap.add_argument("--range-m", type=float, default=12.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    from monte_carlo_localization_amd import engine, maps, synth
    m = load_map(args.map, maps)
    res = float(np.float32(m.resolution))
    H, W = m.data.shape
    P, K = int(args.range_m / res), engine.WEDGES
    rng = np.random.default_rng(args.seed)
    ang = synth.beam_angles().astype(np.float64)
    if args.particles:
        p = np.load(args.particles)
        x, y, th = p[0], p[1], p[2]
    else:
        x = args.pose[0] + rng.normal(0, args.sigma[0], args.n)
        y = args.pose[1] + rng.normal(0, args.sigma[1], args.n)
        th = args.pose[2] + rng.normal(0, args.sigma[2], args.n)
    n = x.size
    n_layout = args.set_size or n
    px, py = (x - m.origin_x) / res, (y - m.origin_y) / res
    bbox, tm = layout_of(px, py, W, H, engine)
    print(f"map {args.map}: {W} x {H} @ {res:.4f} m, range {P} px; {n} particles (layout for {n_layout}), box {bbox[:4].tolist()}, "
          f"{int(bbox[4])} tiles; {args.runs} runs x 64 particles x {ang.size} beams", flush=True)

    margin = P + CAP + 8
    x0, x1 = int(np.floor(px.min())) - margin, int(np.floor(px.max())) + margin + 1
    y0, y1 = int(np.floor(py.min())) - margin, int(np.floor(py.max())) + margin + 1
    crop = np.full((y1 - y0, x1 - x0), 100, np.int8)                      # outside the map: stop
    sy0, sy1, sx0, sx1 = max(y0, 0), min(y1, H), max(x0, 0), min(x1, W)
    crop[sy0 - y0:sy1 - y0, sx0 - x0:sx1 - x0] = m.data[sy0:sy1, sx0:sx1]
    F = np.stack([np.minimum(engine.host_skip_field_wedge_tight(crop, k), CAP) for k in range(K)])

    starts = rng.integers(0, n - 64, args.runs)            # the same slots for every setting
    print("  fine  sub-cell bits  key bits | pairing by beam: per ray, per wave | pairing by direction: per ray, per wave")
    base = None
    for entry in args.fine.split(","):
        f, _, fs = entry.partition(":")
        f, fs = int(f), (int(fs) if fs else None)
        keys = engine.host_sort_key(bbox, tm, W, H, px, py, th, fine=f, n_layout=n_layout, fine_sub=fs)
        order = np.argsort(keys, kind="stable")
        sel = order[starts[:, None] + np.arange(64)[None, :]]
        out = [wave_trips(F, P, K, px[sel] - x0, py[sel] - y0, th[sel], ang, a) for a in ("beam", "direction")]
        base = base or out
        fs_eff = fs if fs is not None else max(f - 2, 0) // 4
        print(f"  {f:4d}  {fs_eff:13d}  {engine.SORT_KEY_LOG2 + f:8d} | {out[0][0]:.3f}  {out[0][1]:.3f} ({100 * (out[0][1] / base[0][1] - 1):+.1f} %) | "
              f"{out[1][0]:.3f}  {out[1][1]:.3f} ({100 * (out[1][1] / base[1][1] - 1):+.1f} %)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
