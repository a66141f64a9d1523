"""Python / numpy restatement of the pose refinement over a scan sequence (include/mcl_hip_engine.h, DESIGN.md §4.23, rules RS1, RS2,
RS4) and the fixtures its tests share.  A plain helper module (like refine_ref.py): no device, no engine.

  offsets:  RS1 with math.cos / math.sin per (seed, window heading), then numpy's rounded multiplies and adds
  poses:    RS2: one IEEE add per coordinate of R1's window and the table
  fold:     RS4: ((+0.0 + acc_0) + acc_1) + ... in scan order
  twin:     the two congruent corridors of tests/test_gpu_search_sequence.py, re-exported, and TWIN_WINDOW

TWIN_WINDOW = half_xy 1, a quarter-cell step, half_theta 2 (45 poses).  The seeds are cell centres and a quarter-cell step never
puts a window pose on a cell edge, so the statement tests/lfield_ref.py reports no ambiguous beam for it (0 as well for half_xy 3,
step 0.3, half_theta 3; half_xy 2 at step 0.25 and the default window reach the half cell and have 40 and 360).

The fixture of the independent statement (SEEDS[0], FIXTURE_WINDOW, REL2, perturbed scans) was confirmed on the CPU as it
stands: tests/test_refine_sequence_host.py asserts the cap (ambiguous beams at most 1e-5 of all beams, or 2) before the device is
held to the statement, so neither rel nor the window headings had to be changed."""
import math

import numpy as np

import refine_ref as rr
from test_gpu_search_sequence import (REL2, REL3, REL5, REL_OFF, TRUTH_CELL, TWIN_CELL, cell_pose, exact_scan, fold,  # noqa: F401
                                      perturbed, twin_map)

TWIN_WINDOW = dict(half_xy=1, step_xy_cells=0.25, half_theta=2)
REL16 = np.array([[-0.05 * (15 - s), 0.01 * ((s * 7) % 5 - 2), 0.02 * ((s * 3) % 7 - 3)] for s in range(15)] + [[0.0, 0.0, 0.0]])


def offsets(seeds, rel, **fields):
    """RS1: (M, nt, S, 3)"""
    c = rr.cfg_of(**fields)
    ht, st = c["half_theta"], c["step_theta_rad"]
    seeds, rel = np.atleast_2d(np.asarray(seeds, np.float64)), np.atleast_2d(np.asarray(rel, np.float64))
    out = np.empty((len(seeds), 2 * ht + 1, len(rel), 3))
    for m, seed in enumerate(seeds):
        for it in range(2 * ht + 1):
            t = np.float64(it - ht) * np.float64(st)             # rounded
            th = np.float64(seed[2]) + t                         # rounded: R1's heading
            c_, s_ = np.float64(math.cos(th)), np.float64(math.sin(th))
            out[m, it, :, 0] = c_ * rel[:, 0] - s_ * rel[:, 1]
            out[m, it, :, 1] = s_ * rel[:, 0] + c_ * rel[:, 1]
            out[m, it, :, 2] = th + rel[:, 2]
    return out


def scan_poses(window, off, **fields):
    """RS2: (S, n_win, 3), the pose of every scan at every window pose of ONE seed.  window: (n_win, 3) by R1; off: (nt, S, 3)"""
    c = rr.cfg_of(**fields)
    nx = 2 * c["half_xy"] + 1
    it = np.arange(len(window)) // (nx * nx)
    S = off.shape[1]
    out = np.empty((S, len(window), 3))
    for s in range(S):
        out[s, :, 0] = window[:, 0] + off[it, s, 0]
        out[s, :, 1] = window[:, 1] + off[it, s, 1]
        out[s, :, 2] = off[it, s, 2]
    return out


def twin_seeds():
    """[twin, truth]: the lattice poses in corridor A and in corridor B (the truth), heading 0"""
    return np.array([cell_pose(*TWIN_CELL), cell_pose(*TRUTH_CELL)])


def twin_scans(m, ang):
    """the two scans of the twin case: from outside B's mouth, then from the truth (the anchor)"""
    from test_gpu_search_sequence import EARLIER_COL
    return np.stack([exact_scan(m, ang, cell_pose(EARLIER_COL, TRUTH_CELL[1])), exact_scan(m, ang, cell_pose(*TRUTH_CELL))])


def statement(lr, m, ang, scans, seeds, rel, max_range, **fields):
    """per seed: (summed volume, per-scan (log-weights, alternatives, ambiguous beams)) of tests/lfield_ref.py at RS2's poses"""
    D, Lf = lr.field(m.data, m.resolution), lr.table(m.resolution)
    off = offsets(seeds, rel, **fields)
    out = []
    for k, seed in enumerate(np.atleast_2d(seeds)):
        poses = scan_poses(rr.window(seed, m.resolution, **fields), off[k], **fields)
        ref = [lr.log_weights(np.ascontiguousarray(poses[s].T), ang, scans[s], D, Lf, m.resolution, m.origin_x, m.origin_y, max_range)
               for s in range(len(scans))]
        out.append((fold([r[0] for r in ref]), ref))
    return out
