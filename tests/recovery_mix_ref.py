"""Restatement of the recovery proposal (mcl_set_recovery_proposal; include/mcl_hip_engine.h P1-P3) in numpy and
Python integers: the thresholds of a weighted mixture, the factors, and the poses of the children an update injects from it.
Philox, bits53, the per-child coin / pick and the injection threshold are those of test_recovery_host.py; the Cholesky factor and
normalize_angle those of motion_ref.py."""
import math

import numpy as np

from motion_ref import cholesky, normalize_angle
from test_recovery_host import MASK, TWO53, bits53, child_draws, philox4x32, threshold  # noqa: F401  (re-exported for the tests)

MAX_COMPONENTS = 4096


def thresholds(weights):
    """P2: t_k = floor((s_k / s_M) 2^53) of the in-order double prefix sums for k < M - 1, t_{M-1} = 2^53; ValueError where P1 refuses"""
    w = [float(v) for v in weights]
    if not 1 <= len(w) <= MAX_COMPONENTS:
        raise ValueError("component count")
    if any(not math.isfinite(v) or v < 0.0 for v in w):
        raise ValueError("weight")
    total = 0.0
    for v in w:
        total += v
    if not math.isfinite(total) or not total > 0.0:
        raise ValueError("sum of the weights")
    out, s = [], 0.0
    for v in w:
        s += v
        out.append(int(math.floor((s / total) * 2 ** 53)))
    out[-1] = TWO53
    return out


def factors(means, covs):
    """(M, 9): mean x, y, theta, L00 L10 L11 L20 L21 L22; ValueError where P1 refuses"""
    m = np.asarray(means, np.float64).reshape(-1, 3)
    c = np.asarray(covs, np.float64).reshape(-1, 3, 3)
    if not np.isfinite(m).all():
        raise ValueError("mean")
    out = np.empty((m.shape[0], 9))
    for k in range(m.shape[0]):
        L = cholesky(c[k])
        out[k] = [m[k, 0], m[k, 1], m[k, 2], L[0, 0], L[1, 0], L[1, 1], L[2, 0], L[2, 1], L[2, 2]]
    return out


def component_of(pick, thr):
    """the first k with pick < t_k (pick < 2^53 = t_{M-1}: there always is one)"""
    t = np.array(thr, np.uint64)
    return np.searchsorted(t, np.asarray(pick, np.uint64), side="right").astype(np.int64)


def mix_normals(seed, upd, g):
    """P3: the three normals of children g of update upd -- streams 10 (n0, n1) and 11 (n2), G1's Box-Muller"""
    g = np.asarray(g, np.uint64)
    lo, hi = g & MASK, g >> np.uint64(32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    two_m53 = 1.0 / 9007199254740992.0
    o = philox4x32(lo, upd, 10, hi, k0, k1)
    u1 = (bits53(o[0], o[1]) + np.uint64(1)).astype(np.float64) * two_m53
    u2 = bits53(o[2], o[3]).astype(np.float64) * two_m53
    rad = np.sqrt(-2.0 * np.log(u1))
    n0, n1 = rad * np.cos(2.0 * math.pi * u2), rad * np.sin(2.0 * math.pi * u2)
    o = philox4x32(lo, upd, 11, hi, k0, k1)
    u1 = (bits53(o[0], o[1]) + np.uint64(1)).astype(np.float64) * two_m53
    u2 = bits53(o[2], o[3]).astype(np.float64) * two_m53
    n2 = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * math.pi * u2)
    return n0, n1, n2


def injected_poses(seed, upd, g, pick, thr, fac):
    """(poses (3, n), component (n,)) of the injected children g (global indices) whose stream-8 second halves are `pick`"""
    k = component_of(pick, thr)
    f = np.asarray(fac, np.float64)[k]
    n0, n1, n2 = mix_normals(seed, upd, g)
    x = f[:, 0] + f[:, 3] * n0
    y = f[:, 1] + (f[:, 4] * n0 + f[:, 5] * n1)
    th = normalize_angle(f[:, 2] + (f[:, 6] * n0 + f[:, 7] * n1 + f[:, 8] * n2))
    return np.stack([x, y, th]), k
