#!/usr/bin/env python3
"""The global search under the beam model (mcl_global_search_beam) on one MI355X, on the Spielberg map;
profiles/beam_search.md is written from the parts.

  python tools/beam_search.py timing [--out DIR] [--stride 2] [--headings 72] [--chunks 16]
      ms per search (host wall around the call, which ends in its one host wait; median of REPS after WARMUP) over the full
      1081-beam scan with beam_stride 1 and one run with beam_stride 10; in the same process the only route the engine offered
      before for these scores, mcl_score_poses under the beam model in chunks of 65536 lattice poses (--chunks of them, spread
      over the lattice, scaled to the whole lattice), and mcl_global_search (likelihood field) on the same lattice.
  python tools/beam_search.py once [--stride 2] [--headings 72]
      one warm-up and one search, nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the split between
      k_beam_table, k_beam_table_exact, k_beam_score and the rest (halve the totals: two calls)
  python tools/beam_search.py kernels --stats FILE [--out DIR]
      the per-kernel totals of that run's kernel_stats.csv into DIR/bs_kernels.json
  python tools/beam_search.py found [--out DIR] [--poses 20] [--particles 262144]
      the found-of-20 protocol of profiles/global_search.md / pose_refine.md (same poses, scans, particle count, engine seed) with
      this search (beam_stride 10) in the likelihood-field search's place: search + mcl_refine_poses (which still uses the field)
      + mixture of the refined means + 3 updates
  python tools/beam_search.py report --out DIR
      profiles/beam_search.md from DIR/bs_timing.json, DIR/bs_found.json and, when there, DIR/bs_kernels.json and
      DIR/bs_distance.json; a part that is missing is reported as not measured
  python tools/beam_search.py distance --log FILE [--out DIR]
      DIR/bs_distance.json ({"1081": [oracle share, engine share], "55": [...]}) from the lines test_distance_from_query_scans
      of tests/test_gpu_search_beam.py prints (FILE: the output of `pytest -s`)

build/ is not tracked; the JSON parts go to build/beam_search by default."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, REPS = 1, 3
FOUND_XY_M, FOUND_TH_RAD = 0.5, 0.2
CHUNK = 65536


def _world():
    from monte_carlo_localization_amd import maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    scan = np.load(os.path.join(ROOT, "tests", "golden", "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32).copy()
    return m, synth.beam_angles(angle_step=1), scan


def _engine(n, m, ang, seed=42, field=False):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=n, seed=seed)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    if field:
        e.set_likelihood_field()
    return e


def _median(v):
    return float(np.median(np.asarray(v, np.float64)))


def timing(args):
    from monte_carlo_localization_amd import engine
    m, ang, scan = _world()
    cells, xy = engine.host_search_lattice(m.data, m.resolution, m.origin_x, m.origin_y, stride_cells=args.stride)
    theta = engine.host_search_headings(n_headings=args.headings)
    n_pos, n_poses = cells.size, cells.size * args.headings
    g = engine.host_search_beam_grid(ang, args.headings)
    e, f = _engine(64, m, ang), _engine(64, m, ang, field=True)
    kw = dict(max_hits=16, stride_cells=args.stride, n_headings=args.headings)
    beam_ms, field_ms, st = [], [], None
    for it in range(WARMUP + REPS):                          # alternating, same process, same box
        t0 = time.perf_counter()
        hits, st = e.global_search_beam(scan, **kw)
        t1 = time.perf_counter()
        f.global_search(scan, **kw)
        t2 = time.perf_counter()
        if it >= WARMUP:
            beam_ms.append((t1 - t0) * 1e3)
            field_ms.append((t2 - t1) * 1e3)
    t0 = time.perf_counter()
    _, st10 = e.global_search_beam(scan, beam_stride=10, **kw)
    stride10_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    e.global_search_beam(scan, **dict(kw, max_hits=0))
    count_only_ms = (time.perf_counter() - t0) * 1e3
    # the yardstick: mcl_score_poses under the beam model, chunks of 65536 lattice poses spread over the volume
    starts = np.linspace(0, n_poses - CHUNK, args.chunks).astype(np.int64)
    e.score_poses(np.column_stack([xy[:64], np.full(64, theta[0])]), scan)                      # warm-up
    chunk_ms, same = [], 0
    V = e.search_scores() if args.compare else None
    for s0 in starts:
        i = np.arange(s0, s0 + CHUNK)
        poses = np.column_stack([xy[i % n_pos], theta[i // n_pos]])
        t0 = time.perf_counter()
        sc = e.score_poses(poses, scan)
        chunk_ms.append((time.perf_counter() - t0) * 1e3)
        if V is not None:
            same += int(np.count_nonzero(sc["log_likelihood"] == V[i]))
    scaled = _median(chunk_ms) * n_poses / CHUNK
    out = dict(map="Spielberg_map", stride_cells=args.stride, n_headings=args.headings, n_positions=int(n_pos), n_poses=int(n_poses),
               beams=int(scan.size), grid_angles=g["M"], max_dev=g["max_dev"], warmup=WARMUP, reps=REPS, stats=st, stats_stride10=st10,
               beam_wall_ms=beam_ms, beam_wall_ms_median=_median(beam_ms), beam_stride10_wall_ms=stride10_ms,
               beam_count_only_wall_ms=count_only_ms, field_wall_ms=field_ms, field_wall_ms_median=_median(field_ms),
               chunks=int(args.chunks), chunk_wall_ms=chunk_ms, chunk_wall_ms_median=_median(chunk_ms), yardstick_scaled_ms=scaled,
               factor=scaled / _median(beam_ms), same_score_share=(same / (CHUNK * len(starts)) if V is not None else None),
               best_hit=[float(v) for v in hits[0]["pose"]] if len(hits) else None)
    print(json.dumps(out), flush=True)
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "bs_timing.json"), "w"), indent=1)


def once(args):
    m, ang, scan = _world()
    e = _engine(64, m, ang)
    for _ in range(2):
        t0 = time.perf_counter()
        _, st = e.global_search_beam(scan, max_hits=16, stride_cells=args.stride, n_headings=args.headings)
        print(json.dumps(dict(wall_ms=(time.perf_counter() - t0) * 1e3, **st)), flush=True)


def kernels(args):
    rows = list(csv.DictReader(open(args.stats)))
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        short = next((k for k in ("k_beam_table_exact", "k_beam_table", "k_beam_score", "k_beam_rows", "k_search_mark") if k in name), None)
        if short is None:
            short = "radix sort (rocPRIM)" if "rocprim" in name else None
        if short is None:
            continue                                             # the map's and the beams' set-up: not part of a search
        d = out.setdefault(short, dict(calls=0, total_ms=0.0))
        d["calls"] += int(r["Calls"])
        d["total_ms"] += float(r["TotalDurationNs"]) * 1e-6
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "bs_kernels.json"), "w"), indent=1)
    print(json.dumps(out))


def distance(args):
    import re
    out = {}
    for line in open(args.log):
        m = re.search(r"beam table vs (float-angle rays, oracle|mcl_query_scans, engine): B=(\d+) share=([0-9.eE+-]+)", line)
        if m:
            out.setdefault(m.group(2), [None, None])[0 if "oracle" in m.group(1) else 1] = float(m.group(3))
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "bs_distance.json"), "w"), indent=1)
    print(json.dumps(out))


def _err(pose, truth):
    d = float(np.hypot(pose[0] - truth[0], pose[1] - truth[1]))
    a = float(abs((pose[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi))
    return d, a


def found(args):
    from monte_carlo_localization_amd import engine
    from oracle import oracle as orc
    orc.build()
    m, ang, _ = _world()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    rng = np.random.default_rng(2024)
    free = np.flatnonzero(np.asarray(m.data).ravel() == 0)
    res = float(np.float32(m.resolution))
    W = m.data.shape[1]
    n = args.particles
    b = _engine(n, m, ang, seed=7, field=True)
    rows = []
    still = (0.0, 0.0, 0.0)
    for i in range(args.poses):
        c = int(rng.choice(free))
        truth = np.array([m.origin_x + (c % W + rng.random()) * res, m.origin_y + (c // W + rng.random()) * res, rng.uniform(-np.pi, np.pi)])
        dirs = truth[2] + ang.astype(np.float64)
        scan = orc.cast_many(om, np.full(dirs.size, truth[0]), np.full(dirs.size, truth[1]), dirs)[0].astype(np.float32)
        t0 = time.perf_counter()
        hits, st = b.global_search_beam(scan, max_hits=16, beam_stride=10)
        search_ms = (time.perf_counter() - t0) * 1e3
        row = dict(truth=[float(v) for v in truth], n_hits=st["n_hits"], search_wall_ms=search_ms, found=False)
        if len(hits):
            r, _ = b.refine_poses(hits["pose"], scan)
            b.init_particles_mixture(r["mean"], r["cov"], engine.seed_counts(r["best_log_likelihood"], n))
            for _ in range(3):
                b.update(still, scan)
            d, t = _err(b.expected_pose(), truth)
            row.update(err_m=d, err_rad=t, found=bool(d < FOUND_XY_M and t < FOUND_TH_RAD), best_hit_err=list(_err(hits[0]["pose"], truth)),
                       any_hit_near=bool(any(e[0] < FOUND_XY_M and e[1] < FOUND_TH_RAD for e in (_err(h["pose"], truth) for h in hits))))
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = dict(map="Spielberg_map", particles=n, poses=args.poses, found_xy_m=FOUND_XY_M, found_th_rad=FOUND_TH_RAD, rows=rows,
               found=sum(r["found"] for r in rows))
    os.makedirs(args.out, exist_ok=True)
    json.dump(out, open(os.path.join(args.out, "bs_found.json"), "w"), indent=1)


def _load(args, name):
    p = os.path.join(args.out, name)
    return json.load(open(p)) if os.path.exists(p) else None


def report(args):
    t, f, k, d = _load(args, "bs_timing.json"), _load(args, "bs_found.json"), _load(args, "bs_kernels.json"), _load(args, "bs_distance.json")
    L = ["# Global search under the beam model on one MI355X (Spielberg map)", "",
         "Written by `tools/beam_search.py report` from one `timing` and one `found` run, one `once` run under "
         "`rocprofv3 --kernel-trace --stats` for the kernel split and the `distance` part; every number below is measured."]
    if not t:
        L += ["", "The call time, the factor against `mcl_score_poses` in chunks and the time beside `mcl_global_search`: **not measured**."]
    else:
        st = t["stats"]
        L += ["",
             f"Lattice: stride {t['stride_cells']} cells, {t['n_headings']} headings: {t['n_positions']} positions, {t['n_poses']} poses; "
             f"{t['beams']}-beam scan on a grid of {t['grid_angles']} angles (worst deviation of a beam angle {t['max_dev']:.2e} rad).  "
             f"The table is made in {st['n_tiles']} tiles of {st['tile_positions']} positions (256 MiB); {st['level3_rays']} of "
             f"{t['n_positions'] * t['grid_angles']} table rays were decided by the literal march.  Host wall around each call, median of "
             f"{t['reps']} after {t['warmup']}, the calls alternating in one process.", "",
             "| call | ms |", "|---|---|",
             f"| `mcl_global_search_beam`, every beam ({st['used_beams']} used), 16 hits | {t['beam_wall_ms_median']:.1f} |",
             f"| the same, max_hits 0 (no sort, one call) | {t['beam_count_only_wall_ms']:.1f} |",
             f"| the same, beam_stride 10 ({t['stats_stride10']['used_beams']} used beams, one call) | {t['beam_stride10_wall_ms']:.1f} |",
             f"| `mcl_global_search` (likelihood field) on the same lattice, every beam | {t['field_wall_ms_median']:.1f} |",
             f"| `mcl_score_poses` under the beam model, one chunk of {CHUNK} lattice poses (median of {t['chunks']} chunks spread over the volume) | {t['chunk_wall_ms_median']:.1f} |",
             f"| ... scaled to the {t['n_poses']} poses of the lattice | {t['yardstick_scaled_ms']:.0f} |", "",
             f"**The beam search takes 1 / {t['factor']:.0f} of the only route the engine offered before for these scores** (target: at most a tenth).  "
             f"Device memory of the search's buffers: {st['device_bytes'] / 2**20:.0f} MiB."]
    if t and t.get("same_score_share") is not None:
        L += ["", f"Share of the yardstick's poses whose `mcl_score_poses` log-likelihood equals the volume's entry bit for bit: "
                  f"{t['same_score_share']:.4f} (B3: not a parity, the float angles sit off the grid)."]
    if k:
        tot = sum(v["total_ms"] for v in k.values())
        L += ["", "## Where the time goes", "",
              "Kernel totals of two searches under `rocprofv3 --kernel-trace --stats`, halved:", "", "| kernel | calls / search | ms / search | share |",
              "|---|---|---|---|"]
        for name, v in sorted(k.items(), key=lambda kv: -kv[1]["total_ms"]):
            L.append(f"| {name} | {v['calls'] / 2:g} | {v['total_ms'] / 2:.2f} | {100 * v['total_ms'] / tot:.1f} % |")
    def sh(v):
        return "not measured" if v is None else f"{v:.5f}"
    if not k:
        L += ["", "The split between table, exact march and score: **not measured**."]
    if not f:
        L += ["", "The found-of-20 count: **not measured**."]
    if d:
        L += ["", "## Distance from `mcl_query_scans`", "",
              "Share of table entries that differ from the step `mcl_query_scans` reports for the same pose and beam "
              "(tests/test_gpu_search_beam.py: every position of the stride-2 lattice of its 120 x 90 map, 4 headings):", "",
              "| scan | oracle alone (grid angle against theta_k + (double)a_j) | engine (table against `mcl_query_scans`) | bound |", "|---|---|---|---|",
              f"| 1081 beams, every 8th | {sh(d.get('1081', [None, None])[0])} | {sh(d.get('1081', [None, None])[1])} | 0.01 |",
              f"| 55 beams | {sh(d.get('55', [None, None])[0])} | {sh(d.get('55', [None, None])[1])} | 0.05 |"]
    if f:
        L += ["", "## Is the robot found?", "",
              f"The protocol of `profiles/pose_refine.md` ({f['poses']} random free poses, oracle-cast 1081-beam scans, the robot standing still, "
              f"{f['particles']} particles, found = expected pose within {f['found_xy_m']} m and {f['found_th_rad']} rad after 3 updates), with "
              "`mcl_global_search_beam` (beam_stride 10) in the likelihood-field search's place; the refinement and the updates still use the field.", "",
              f"- beam search + `mcl_refine_poses` + mixture + 3 updates: **{f['found']} / {f['poses']}** (recorded with the likelihood-field search: 5 / 20)",
              f"- poses with one of the 16 hits within the found radius: {sum(r.get('any_hit_near', False) for r in f['rows'])} / {f['poses']}; "
              f"with the best hit within it: {sum(bool(r.get('best_hit_err')) and r['best_hit_err'][0] < f['found_xy_m'] and r['best_hit_err'][1] < f['found_th_rad'] for r in f['rows'])} / {f['poses']}",
              f"- search wall per pose: median {_median([r['search_wall_ms'] for r in f['rows']]):.1f} ms", "",
              "No count was promised: the figure says how often search + refine + seed localises from ONE scan of a standing robot."]
    L.append("")
    open(os.path.join(ROOT, "profiles", "beam_search.md"), "w").write("\n".join(L))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["timing", "once", "kernels", "found", "distance", "report"])
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "beam_search"))
    ap.add_argument("--stride", type=int, default=2)
    ap.add_argument("--headings", type=int, default=72)
    ap.add_argument("--chunks", type=int, default=16)
    ap.add_argument("--compare", action="store_true", help="timing: also count the yardstick's scores that equal the volume's bit for bit")
    ap.add_argument("--poses", type=int, default=20)
    ap.add_argument("--particles", type=int, default=262144)
    ap.add_argument("--log", help="distance: the output of pytest -s tests/test_gpu_search_beam.py")
    ap.add_argument("--stats", help="kernels: the kernel_stats.csv of a rocprofv3 run of `once`")
    args = ap.parse_args()
    dict(timing=timing, once=once, kernels=kernels, found=found, distance=distance, report=report)[args.part](args)


if __name__ == "__main__":
    main()
