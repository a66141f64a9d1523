"""Python / numpy restatement of the pose refinement (include/mcl_hip_engine.h, DESIGN.md §4.14, rules R1, R3, R4) and the small
fixture its tests share: the statement mcl_host_refine_* and the device are held to.  A plain helper module (like lfield_ref.py):
no device, no engine.

  window:   R1 in numpy's fp64 (a multiply and an add, each rounded)
  best:     R3 as a sort key in Python
  moments:  R4 with math.fsum (correctly rounded sums) and math.exp
  fixture:  the 120 x 90 map at 0.05 m of tests/test_gpu_global_search.py, restated; a scan cast by the oracle from a known pose
            P* and moved by about a millimetre (fixed seed)"""
import math

import numpy as np

from side_geometries import odd_scan, perturbed_scan, scan_at  # noqa: F401  (the fixture's helpers, shared by geometry)

RES = np.float32(0.05)
OX, OY = -3.0, -2.25
MAX_RANGE = 12.0
W, H = 120, 90
DEFAULT = dict(half_xy=4, half_theta=10, step_xy_cells=0.5, step_theta_rad=math.pi / 360.0)


class SmallMap:
    """120 x 90 cells at 0.05 m: an outer wall with two gaps (beams leave the map there), interior walls, a pillar, a post of one
    cell, unknown cells"""

    def __init__(self):
        g = np.zeros((H, W), np.int8)
        g[0, :] = g[-1, :] = 100
        g[:, 0] = g[:, -1] = 100
        g[0, 30:40] = 0
        g[40:50, -1] = 0
        g[30, 20:70] = 100
        g[30:75, 85] = 100
        g[55:60, 40:45] = 100
        g[64, 64] = 100
        g[60:80, 5:15] = -1
        g[10:14, 100:110] = -1
        self.data, self.resolution, self.origin_x, self.origin_y = g, RES, OX, OY


def angles(orc, B):
    """B beams over the Hokuyo's 270 degrees (B = 1: the first of them)"""
    full = orc.beam_angles()
    return full[np.linspace(0, full.size - 1, B).round().astype(int)].copy() if B > 1 else full[:1].copy()


# The seed of fixtures (a) and (b): the pose of the stride-2 search lattice at cell (col 25, row 15) -- free, in the asymmetric
# lower left of the map -- and heading k = 58 of 72 (S2: (2 k - 72) pi / 72 = 110 degrees).  P* = that pose moved by (+0.6 cell,
# -0.4 cell, +1.7 degrees), the offsets the design of this feature proposed; the scan is cast from P*.
#
# What had to be chosen otherwise, by the statement of tests/lfield_ref.py alone (tests/test_refine_host.py asserts both
# conditions): the window of the fixture is FIXTURE_WINDOW = the default steps with half_theta = 3 (9 x 9 x 7 = 567 poses), and k
# is 58.  With the default half_theta = 10 condition (a) cannot hold for ANY lattice seed: a lattice position is a cell centre, so
# every odd multiple of the half-cell step puts the pose exactly on a cell edge; lattice headings are multiples of 5 degrees, the
# window's of 0.5 degrees and the 61 beams' of 4.5 degrees, so in 21 consecutive headings some beam points along a map axis (to
# the float32 rounding of its angle), and its end point then lies on that edge too: 36 to 180 ambiguous beams for every seed that
# was tried.  theta + a_j is a multiple of 90 degrees iff (k + it) % 9 == 0 for some j, so 7 consecutive headings avoid it when
# k % 9 == 4: k = 58, it in [-3, 3].  Then no beam is ambiguous and (b) holds with the proposed offsets (best = (0, 0, +3) steps
# from the seed, P* at (1.2, -0.8, 3.4) steps).  The default window is still held to mcl_score_poses bit for bit by the GPU tests.
LATTICE_POSE = (OX + 25.5 * float(RES), OY + 15.5 * float(RES), (2 * 58 - 72) * (math.pi / 72))
P_STAR = (LATTICE_POSE[0] + 0.6 * float(RES), LATTICE_POSE[1] - 0.4 * float(RES), LATTICE_POSE[2] + math.radians(1.7))
P_STAR_STEPS = (1.2, -0.8, 3.4)                 # P* - seed in window steps (half a cell, half a cell, half a degree)
FIXTURE_WINDOW = dict(half_theta=3)
# the three seeds of the GPU tests: the lattice pose, a pose off the map, a pose inside the interior wall (row 30, col 40)
SEEDS = np.array([LATTICE_POSE,
                  (OX - 0.3, OY + 1.0, 0.3),
                  (OX + 40.5 * float(RES), OY + 30.5 * float(RES), -2.0)])


def cfg_of(**fields):
    c = dict(DEFAULT)
    c.update(fields)
    return c


def steps(resolution, **fields):
    """(sx, sx, step_theta): sx formed once, from the float resolution widened to double"""
    c = cfg_of(**fields)
    sx = c["step_xy_cells"] * float(np.float32(resolution))
    return sx, sx, c["step_theta_rad"]


def offsets(**fields):
    """integer offsets (dix, diy, dit) of every window pose from the window centre, in window-index order (ix fastest)"""
    c = cfg_of(**fields)
    hx, ht = c["half_xy"], c["half_theta"]
    dt, dy, dx = np.meshgrid(np.arange(-ht, ht + 1), np.arange(-hx, hx + 1), np.arange(-hx, hx + 1), indexing="ij")
    return np.stack([dx.ravel(), dy.ravel(), dt.ravel()], axis=1).astype(np.int64)


def window(seed, resolution, **fields):
    """R1: (n_win, 3) poses"""
    d = offsets(**fields).astype(np.float64)
    st = steps(resolution, **fields)
    out = np.empty_like(d)
    for a in range(3):
        t = d[:, a] * st[a]                      # rounded
        out[:, a] = float(seed[a]) + t           # rounded
    return out


def best(scores, **fields):
    """R3: the window index of the best pose"""
    d = offsets(**fields)
    q = (d * d).sum(axis=1)
    s = np.asarray(scores, np.float64)
    assert not np.isnan(s).any()
    return min(range(s.size), key=lambda w: (-s[w], int(q[w]), w))


def moments(seed, resolution, scores, **fields):
    """R4 with correctly rounded sums: (best pose, mean, cov, S)"""
    d = offsets(**fields)
    st = steps(resolution, **fields)
    s = [float(v) for v in np.asarray(scores, np.float64)]
    wb = best(scores, **fields)
    win = window(seed, resolution, **fields)
    u = d - d[wb]
    w = [0.0 if v == -math.inf else math.exp(v - s[wb]) for v in s]
    S = math.fsum(w)
    m, C = [0.0] * 3, [[0.0] * 3 for _ in range(3)]
    if S > 0.0:
        m = [math.fsum(w[i] * float(u[i, a]) for i in range(len(w))) / S for a in range(3)]
        for a in range(3):
            for b in range(3):
                C[a][b] = math.fsum(w[i] * float(u[i, a] * u[i, b]) for i in range(len(w))) / S - m[a] * m[b]
    mean = np.array([win[wb, a] + st[a] * m[a] for a in range(3)])
    cov = np.array([[st[a] * st[b] * C[a][b] + (st[a] * st[a] / 12.0 if a == b else 0.0) for b in range(3)] for a in range(3)])
    return win[wb], mean, cov, S


def tolerances(resolution, **fields):
    """(mean tolerance (3,), cov tolerance (3, 3), weight-sum tolerance).  Recursive summation of n terms bounded by
    sum w (2 h_a)(2 h_b) errs by at most (n - 1) 2^-53 of that; exp within 1-2 ulp and the m_a m_b subtraction add a few more:
    about 4 (n + 4) 2^-53.  32 n 2^-53 leaves a factor 8; times the extent of the window in the entry's units."""
    c = cfg_of(**fields)
    n_win = (2 * c["half_xy"] + 1) ** 2 * (2 * c["half_theta"] + 1)
    base = 32.0 * n_win * 2.0 ** -53
    ext = np.array([2 * c["half_xy"] + 1, 2 * c["half_xy"] + 1, 2 * c["half_theta"] + 1], np.float64) * np.array(steps(resolution, **fields))
    return base * ext, base * np.outer(ext, ext), base
