#!/usr/bin/env python3
"""What a map patch (mcl_update_map_region) costs beside mcl_set_map on one MI355X; profiles/map_patch.md is
written from the parts.

  python tools/map_patch.py measure [--parent-lib FILE] [--rounds R] [--out DIR]
      one process, two maps: Spielberg (2000 x 2000, 0.05 m) and the same map with every cell doubled (4000 x 4000, 0.025 m: the
      ringed fields are held).  Per map, R rounds of
        * mcl_set_map with this tree's library and, with --parent-lib, with a libmcl_hip_engine.so built from the parent commit
          (loaded beside this one; only mcl_create / mcl_set_map / mcl_destroy are called on it), in turn;
        * mcl_update_map_region for a 1-cell, a 64 x 64, a 512 x 512 and a whole-map rectangle.  Every patch flips the stop bit of
          the rectangle's two opposite corner cells, so the box of its stop changes -- and with it every window -- is the rectangle;
        * the first mcl_update (262 144 particles x 1081 beams) after a patch and after a mcl_set_map.
  python tools/map_patch.py report [--out DIR]
      profiles/map_patch.md from OUT/map_patch.json

build/ is not tracked; the parts go to build/map_patch by default."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION = (0.05, 0.0, 0.01)
N = 262144
RECTS = (("1 cell", 1), ("64 x 64", 64), ("512 x 512", 512), ("whole map", 0))


def ms_of(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def parent_set_map(path, engine, m, res, ox, oy, cfg):
    """wall ms of mcl_set_map through a library that knows nothing of this tree's binding"""
    lib = C.CDLL(path)
    lib.mcl_create.argtypes = [C.POINTER(engine.Config), C.POINTER(C.c_void_p)]
    lib.mcl_destroy.argtypes = [C.c_void_p]
    lib.mcl_destroy.restype = None
    lib.mcl_set_map.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_double, C.c_double]
    h = C.c_void_p()
    assert lib.mcl_create(C.byref(cfg), C.byref(h)) == 0
    g = np.ascontiguousarray(m, np.int8)
    out = []

    def call():
        assert lib.mcl_set_map(h, g.ctypes.data, g.shape[1], g.shape[0], np.float32(res), ox, oy) == 0
    call()                                                   # the first call of a process pays for the code object
    out.append(ms_of(call))
    lib.mcl_destroy(h)
    return out[0]


def flipped(m, x0, y0, side):
    """the rectangle with the stop bit of its two opposite corner cells flipped (a free cell for a wall and back)"""
    c = m[y0:y0 + side, x0:x0 + side].copy()
    for y, x in {(0, 0), (side - 1, side - 1)}:
        c[y, x] = 0 if c[y, x] > 50 else 100
    return c


def measure(args):
    sys.path.insert(0, ROOT)
    from monte_carlo_localization_amd import engine, maps, synth
    sp = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    ang = synth.beam_angles(angle_step=1)
    cases = (("Spielberg 2000 x 2000", sp.data, sp.resolution),
             ("doubled 4000 x 4000", np.kron(sp.data, np.ones((2, 2), np.int8)).astype(np.int8), sp.resolution / 2))
    result = {"rounds": args.rounds, "maps": []}
    for name, m, res in cases:
        H, W = m.shape
        e = engine.Engine(max_particles=N, seed=42)
        e.set_map(m, res, sp.origin_x, sp.origin_y)         # (warm: the code object, the allocations)
        e.set_beam_angles(ang)
        cloud = synth.tracking_cloud(np.random.default_rng(42), N)
        rec = {"map": name, "P": e.max_range_px, "set_map_ms": [], "parent_set_map_ms": [], "patch": {r[0]: [] for r in RECTS},
               "patch_windows": {}, "update_after_patch_ms": [], "update_after_set_map_ms": [], "update_warm_ms": []}
        for _ in range(args.rounds):
            rec["set_map_ms"].append(ms_of(lambda: e.set_map(m, res, sp.origin_x, sp.origin_y)))
            if args.parent_lib:
                rec["parent_set_map_ms"].append(parent_set_map(args.parent_lib, engine, m, res, sp.origin_x, sp.origin_y, e.cfg))
            cur = m.copy()
            for label, side in RECTS:
                side = side or min(W, H)
                x0, y0 = (0, 0) if side == min(W, H) else (W // 2 - side // 2, H // 2 - side // 2)
                c = flipped(cur, x0, y0, side)
                st = {}
                wall = ms_of(lambda: st.update(e.update_map_region(c, x0, y0)))
                cur[y0:y0 + side, x0:x0 + side] = c
                rec["patch"][label].append({"wall_ms": wall, "ms": st["ms"], "changed_stop_cells": st["changed_stop_cells"]})
                rec["patch_windows"][label] = st["window"]
            # the first update after a patch / after a set_map, and a warm one
            e.set_map(m, res, sp.origin_x, sp.origin_y)
            e.set_particles(cloud, np.full(N, 1.0 / N))
            e.update(ACTION, scan)
            e.update(ACTION, scan)
            rec["update_warm_ms"].append(ms_of(lambda: e.update(ACTION, scan)))
            e.update_map_region(flipped(m, W // 2, H // 2, 1), W // 2, H // 2)
            rec["update_after_patch_ms"].append(ms_of(lambda: e.update(ACTION, scan)))
            e.update(ACTION, scan)
            e.set_map(m, res, sp.origin_x, sp.origin_y)
            rec["update_after_set_map_ms"].append(ms_of(lambda: e.update(ACTION, scan)))
        e.close()
        result["maps"].append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "map_patch.json"), "w") as f:
        json.dump(result, f, indent=1)


def span(v):
    return f"{min(v):.2f} .. {max(v):.2f}" if v else "-"


def report(args):
    r = json.load(open(os.path.join(args.out, "map_patch.json")))
    L = ["# Map patches beside `mcl_set_map`", "",
         "`python tools/map_patch.py measure --parent-lib <parent's libmcl_hip_engine.so>` then `report`: one process on one MI355X, "
         f"{r['rounds']} rounds, wall milliseconds of the calls (lowest .. highest of the rounds).  A patch flips the stop bit of the "
         "two opposite corner cells of its rectangle, so its windows are those of the whole rectangle; `ms` is the call's own "
         "statistic, the wall time includes the binding.", ""]
    for m in r["maps"]:
        best_set = min(m["set_map_ms"])
        L += [f"## {m['map']} (MAX_RANGE_PX {m['P']})", "",
              "| call | wall ms | share of `mcl_set_map` (lowest of each) |", "|---|---|---|",
              f"| `mcl_set_map`, parent commit | {span(m['parent_set_map_ms'])} | |",
              f"| `mcl_set_map`, this commit | {span(m['set_map_ms'])} | 1 |"]
        for label, _ in RECTS:
            w = [p["wall_ms"] for p in m["patch"][label]]
            win = m["patch_windows"][label]
            L.append(f"| `mcl_update_map_region`, {label} (window {win[2] - win[0] + 1} x {win[3] - win[1] + 1}) | {span(w)} | {min(w) / best_set:.3f} |")
        L += ["", "| first `mcl_update` (262 144 x 1081) | wall ms |", "|---|---|",
              f"| after a one-cell patch | {span(m['update_after_patch_ms'])} |",
              f"| after `mcl_set_map` | {span(m['update_after_set_map_ms'])} |",
              f"| warm (third update after `mcl_set_map`) | {span(m['update_warm_ms'])} |", ""]
    path = os.path.join(ROOT, "profiles", "map_patch.md")
    notes = os.path.join(args.out, "notes.md")
    if os.path.exists(notes):
        L += open(notes).read().rstrip("\n").split("\n") + [""]
    open(path, "w").write("\n".join(L))
    print(path)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["measure", "report"])
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "map_patch"))
    a = ap.parse_args()
    {"measure": measure, "report": report}[a.mode](a)
