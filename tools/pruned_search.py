"""The global search with exact pruning (mcl_global_search_pruned) on one MI355X beside mcl_global_search in the
same process, on Spielberg with the Hokuyo's 1081 beams: time, bytes, pairs scored / pairs, rounds and the split between the bound
pass and the scoring rounds, for the default lattice with all beams and with every tenth, for propose_from_scan's thinned search,
for block 4 and 8, for several first rounds, and for a scan with few usable beams; then a kidnap run under the likelihood field
with propose_from_scan(pruned=False) beside pruned=True.  Writes profiles/pruned_search.md.

  python tools/pruned_search.py [--reps 5] [--kidnap-n 65536] [--json FILE]

Nothing here is a pass/fail number.  The split between the bound pass and the scoring rounds: beside every call the tool times
the same call with first_pairs = 1 and max_hits = 1 -- the bound pass, the sort of the pairs and rounds of few pairs -- and reports
that call's rounds and pairs with its time."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kidnap_recover import A, B, SEED, _err    # noqa: E402

THINNED = dict(beam_stride=10, stride_cells=4)          # propose_from_scan's search in profiles/recovery_proposal.md


def timed(f, reps):
    f()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), r


def setup(n=1024):
    from monte_carlo_localization_amd import engine, maps, synth
    m = maps.load_npz(os.path.join(ROOT, "tests", "golden", "map_Spielberg_map.npz"))
    ang = synth.beam_angles()
    e = engine.Engine(max_particles=n, seed=SEED)
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    e.set_beam_angles(ang)
    e.set_likelihood_field(True)
    return e, m, ang


def searches(reps):
    from monte_carlo_localization_amd import engine, synth
    e, m, ang = setup()
    scan = synth.scan_from_pose(e, m, ang, B)
    few = np.full(scan.size, np.nan, np.float32)
    few[::120] = scan[::120]                              # 10 usable beams: the bound is loose
    rows = []
    cases = [("stride 2 x 72, all beams", scan, {}), ("stride 2 x 72, every tenth beam", scan, dict(beam_stride=10)),
             ("thinned (stride 4, every tenth beam)", scan, THINNED), ("stride 2 x 72, 10 usable beams", few, {})]
    for name, obs, fields in cases:
        ex_ms, (want, st) = timed(lambda: e.global_search(obs, max_hits=16, **fields), reps)
        ex_bytes = st["device_bytes"]
        for block in (4, 8):
            for first in (0, 256, 4096, 65536):
                f = lambda: e.global_search_pruned(obs, max_hits=16, block=block, first_pairs=first, **fields)   # noqa: E731
                ms, (got, ps) = timed(f, reps)
                same = got.tobytes() == want[:len(got)].tobytes() and len(got) == min(16, st["n_hits"])
                # the bound pass, the pairs' sort and a round of one pair: what a call costs before its rounds
                b_ms, _ = timed(lambda: e.global_search_pruned(obs, max_hits=1, block=block, first_pairs=1, **fields), reps)
                _, one = e.global_search_pruned(obs, max_hits=1, block=block, first_pairs=1, **fields)
                rows.append(dict(case=name, block=block, first_pairs=first, exhaustive_ms=ex_ms, exhaustive_bytes=ex_bytes, ms=ms,
                                 bytes=ps["device_bytes"], pairs=ps["pairs"], scored=ps["pairs_scored"], rounds=ps["rounds"],
                                 guard=ps["guard_fallbacks"], identical=bool(same), n_poses=ps["n_poses"], n_positions=ps["n_positions"],
                                 first_round_call_ms=b_ms, first_round_call_rounds=one["rounds"], first_round_call_scored=one["pairs_scored"]))
                print(rows[-1], flush=True)
    # the share of live lanes of a wave per block: positions / (pairs' blocks * S * S)
    lanes = {}
    for block in (2, 4, 8):
        for stride in (2, 4):
            plan = engine.host_search_blocks(m.data, block=block, stride_cells=stride)
            lanes[f"{block}/{stride}"] = (int(plan["blocks"][:, 2].sum()), int(plan["n_blocks"]) * 64, int(plan["n_blocks"]) * block * block)
    e.close()
    return rows, lanes


def kidnap(n, updates=20, converge=10):
    """the KLD-on kidnap run of profiles/recovery_proposal.md under the likelihood field: propose_from_scan before every update whose
    p > 0, with the exhaustive and with the pruned search"""
    from monte_carlo_localization_amd import synth
    out = []
    for pruned in (False, True):
        e, m, ang = setup(n)
        e.set_kld(min_particles=512, max_particles=n)
        e.set_recovery(alpha_slow=0.001, alpha_fast=0.1)
        scan_a, scan_b = synth.scan_from_pose(e, m, ang, A), synth.scan_from_pose(e, m, ang, B)
        e.init_particles_pose(A, n)
        search_ms, upd_ms, found = [], [], None
        for k in range(converge + updates):
            scan = scan_b if k >= converge else scan_a
            if e.recovery_state()[2] > 0:
                t = time.perf_counter()
                e.propose_from_scan(scan, pruned=pruned, **THINNED)
                search_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            e.update((0.0, 0.0, 0.0), scan)
            upd_ms.append((time.perf_counter() - t) * 1e3)
            d, dth = _err(e, B if k >= converge else A)
            if k >= converge and found is None and d < 0.25 and dth < 5:
                found = k - converge + 1
        out.append(dict(pruned=pruned, n=n, found_after=found, err_m=d, err_deg=dth, searches=len(search_ms),
                        search_ms=float(np.median(search_ms)) if search_ms else None, update_ms=float(np.median(upd_ms)), n_end=e.n))
        print(out[-1], flush=True)
        e.close()
    return out


def report(rows, lanes, kid):
    L = ["# The global search with exact pruning beside the exhaustive search, on one MI355X", "",
         "Written by `tools/pruned_search.py`.  Spielberg, 1081 beams, the scan cast at B of `profiles/recovery.md`, `max_hits` 16, host "
         "wall time of a call (median), both searches in one process.  Nothing here is a pass/fail number.  'before the rounds': a call "
         "with `first_pairs` 1 and `max_hits` 1 -- the bound pass, the sort of the pairs and rounds of few pairs (its rounds and pairs in "
         "brackets).  bytes: what the call's own buffers have asked for by then (they grow over the rows of one process: the largest "
         "store so far stays).", "",
         "| case | block | first_pairs | exhaustive ms | pruned ms | before the rounds ms (rounds, pairs) | pairs scored / pairs | rounds | "
         "exhaustive MiB | pruned MiB | guard | hits identical |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        L.append(f"| {r['case']} | {r['block']} | {r['first_pairs']} | {r['exhaustive_ms']:.2f} | {r['ms']:.2f} | {r['first_round_call_ms']:.2f} "
                 f"({r['first_round_call_rounds']}, {r['first_round_call_scored']}) | {r['scored']} / {r['pairs']} "
                 f"({100.0 * r['scored'] / r['pairs']:.2f} %) | {r['rounds']} | {r['exhaustive_bytes'] / 2**20:.0f} | {r['bytes'] / 2**20:.0f} | "
                 f"{r['guard']} | {'yes' if r['identical'] else 'NO'} |")
    L += ["", "## Live lanes of a wave per block", "", "| block / stride_cells | positions | lanes of the waves (64 per block) | share live | "
          "entries of the store (S x S per block) | share live |", "|---|---:|---:|---:|---:|---:|"]
    for k, (pos, l64, lss) in lanes.items():
        L.append(f"| {k} | {pos} | {l64} | {100.0 * pos / l64:.1f} % | {lss} | {100.0 * pos / lss:.1f} % |")
    L += ["", "## Kidnap under the likelihood field, KLD on", "",
          "A converged set at A, then scans from B, standing still; `propose_from_scan(scan, beam_stride=10, stride_cells=4)` before every "
          "update whose p > 0, with the exhaustive search and with `pruned=True`.", "",
          "| N | search | found within 0.25 m / 5 deg after | error at the end m / deg | searches | search + refine ms, median | update ms, median | N at the end |",
          "|---:|---|---:|---:|---:|---:|---:|---:|"]
    for r in kid:
        L.append(f"| {r['n']} | {'pruned' if r['pruned'] else 'exhaustive'} | {r['found_after']} | {r['err_m']:.3f} / {r['err_deg']:.2f} | "
                 f"{r['searches']} | {'-' if r['search_ms'] is None else format(r['search_ms'], '.2f')} | {r['update_ms']:.2f} | {r['n_end']} |")
    open(os.path.join(ROOT, "profiles", "pruned_search.md"), "w").write("\n".join(L) + "\n")
    print("wrote profiles/pruned_search.md")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kidnap-n", type=int, default=65536)
    ap.add_argument("--json", default=None, help="also keep the raw figures here")
    a = ap.parse_args()
    rows, lanes = searches(a.reps)
    kid = kidnap(a.kidnap_n)
    if a.json:
        json.dump(dict(rows=rows, lanes=lanes, kidnap=kid), open(a.json, "w"))
    report(rows, lanes, kid)


if __name__ == "__main__":
    main()
