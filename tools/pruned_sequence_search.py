#!/usr/bin/env python3
"""The pruned search over a scan sequence (mcl_global_search_sequence_pruned) on one MI355X beside
mcl_global_search_sequence in the same process, on Spielberg with the Hokuyo's 1081 beams: the protocol of
profiles/sequence_search.md -- scans half a metre apart on a straight drive that ends at the map's origin pose, the default lattice
(stride 2 x 72 headings), max_hits 16 -- with three scans, then with one and with six, and with every tenth beam.  Per setting the
exhaustive call's time and bytes, and for block 2, 4 and 8 the pruned call's time, bytes, pairs scored of pairs, rounds and guard
fallbacks, and whether its hits are the exhaustive call's byte for byte.  Writes profiles/pruned_sequence_search.md.

  python tools/pruned_sequence_search.py [--reps 5] [--warmup 2] [--out FILE] [--json FILE]

Host wall time around a call (each call ends in a host wait), median (minimum - maximum) of --reps after --warmup.  The two calls
run on two engines of one process, so that each engine's mcl_get_search_bytes is what a node that makes only that call holds.
Nothing here is a pass/fail number."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEP_M = 0.5
SINGLE_RECORD = (17578, 1125000)         # pairs scored of pairs of the single-scan pruned search (profiles/pruned_search.md)


def timed(f, warmup, reps):
    for _ in range(warmup):
        f()
    ms, r = [], None
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t) * 1e3)
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms))), r


def drive(S):
    """S poses half a metre apart on a straight line that ends at the origin pose, oldest first (tools/sequence_search.py)"""
    return np.array([[-STEP_M * (S - 1 - i), 0.0, 0.0] for i in range(S)])


def make_engine(m, ang):
    from monte_carlo_localization_amd import engine
    e = engine.Engine(max_particles=64, seed=42)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    e.set_likelihood_field()
    return e


def run(reps, warmup):
    from monte_carlo_localization_amd import engine, maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    ang = synth.beam_angles(angle_step=1)
    ex, pe = make_engine(m, ang), make_engine(m, ang)
    rows = []
    for S, fields in ((3, {}), (1, {}), (6, {}), (3, dict(beam_stride=10))):
        odom = drive(S)
        scans = ex.expected_scans(odom)                      # what the robot sees along the drive (the ray stage's cast)
        rel = engine.relative_poses(odom)
        ex_ms, (want, st) = timed(lambda: ex.global_search_sequence(scans, rel, max_hits=16, **fields), warmup, reps)
        ex_bytes = ex.search_bytes()
        for block in (8, 4, 2):                              # the default first: its MiB is then that of a node which uses it alone
            ms, (got, ps) = timed(lambda: pe.global_search_sequence_pruned(scans, rel, max_hits=16, block=block, **fields), warmup, reps)
            same = got.tobytes() == want[:len(got)].tobytes() and len(got) == min(16, st["n_hits"])
            rows.append(dict(scans=S, beam_stride=fields.get("beam_stride", 1), used_beams=ps["used_beams"], block=block, exhaustive_ms=ex_ms,
                             exhaustive_bytes=ex_bytes, ms=ms, bytes=pe.search_bytes(), call_bytes=ps["device_bytes"], pairs=ps["pairs"],
                             scored=ps["pairs_scored"], rounds=ps["rounds"], guard=ps["guard_fallbacks"], identical=bool(same),
                             n_poses=ps["n_poses"], n_positions=ps["n_positions"], best=[float(v) for v in got[0]["pose"]] if len(got) else None))
            print(json.dumps(rows[-1]), flush=True)
    ex.close()
    pe.close()
    return rows


def report(rows, reps, warmup, out):
    def ms(d):
        return f"{d['median']:.2f} ({d['min']:.2f} - {d['max']:.2f})"

    r0 = rows[0]
    L = ["# The pruned search over a scan sequence beside the exhaustive one, on one MI355X", "",
         "Written by `tools/pruned_sequence_search.py`; every number below is measured.  Command:", "",
         "    python tools/pruned_sequence_search.py", "",
         f"Spielberg, 1081 beams, stride 2 x 72 headings ({r0['n_positions']} positions, {r0['n_poses']} poses), `max_hits` 16, the default first "
         f"round.  The scans are taken {STEP_M} m apart on a straight drive that ends at the map's origin pose (the protocol of "
         f"`profiles/sequence_search.md`).  Host wall time around a call, median (minimum - maximum) of {reps} after {warmup}; the exhaustive "
         "and the pruned call run on two engines of one process, and MiB is each engine's `mcl_get_search_bytes` after the row's calls "
         "(the pruned engine's buffers grow over the rows -- the largest pair buffers and store so far stay -- so the first row, block 8, "
         "is what a node that makes only the default call holds).  Nothing here is a pass/fail number.", "",
         "| scans | beams used | block | `mcl_global_search_sequence` ms | `mcl_global_search_sequence_pruned` ms | pairs scored / pairs | rounds | "
         "guard | exhaustive MiB | pruned MiB | hits identical |", "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        L.append(f"| {r['scans']} | {r['used_beams']} | {r['block']} | {ms(r['exhaustive_ms'])} | {ms(r['ms'])} | {r['scored']} / {r['pairs']} "
                 f"({100.0 * r['scored'] / r['pairs']:.2f} %) | {r['rounds']} | {r['guard']} | {r['exhaustive_bytes'] / 2**20:.0f} | "
                 f"{r['bytes'] / 2**20:.0f} | {'yes' if r['identical'] else 'NO'} |")
    slower = [r for r in rows if r["ms"]["median"] >= r["exhaustive_ms"]["median"]]
    L += ["", "## Reading", "",
          f"- The single-scan pruned search scores {SINGLE_RECORD[0]} of {SINGLE_RECORD[1]} pairs at block 8 "
          f"({100.0 * SINGLE_RECORD[0] / SINGLE_RECORD[1]:.2f} %, `profiles/pruned_search.md`): its default first round, 1 / 64 of the "
          "pairs, and no further one.  The fractions above are what the sum of per-scan bounds needs on this drive, read beside that "
          "figure.  No ratio was fixed in advance."]
    if slower:
        L.append("- The pruned call is NOT faster than the exhaustive one at: " +
                 "; ".join(f"{r['scans']} scans, beam_stride {r['beam_stride']}, block {r['block']} ({r['ms']['median']:.2f} ms against "
                           f"{r['exhaustive_ms']['median']:.2f} ms)" for r in slower) + ".")
    else:
        L.append("- The pruned call is faster than the exhaustive one at every setting above.")
    if not all(r["identical"] for r in rows):
        L.append("- SOME HITS DIFFER from the exhaustive call's: see the last column.")
    L.append("")
    open(out, "w").write("\n".join(L))
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pruned_sequence_search.md"))
    ap.add_argument("--json", default=None, help="also keep the raw figures here")
    a = ap.parse_args()
    rows = run(a.reps, a.warmup)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    report(rows, a.reps, a.warmup, a.out)


if __name__ == "__main__":
    main()
