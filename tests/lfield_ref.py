"""numpy restatement of the likelihood-field sensor model (include/mcl_hip_engine.h): the statement the
engine's field, table and log-weights are held to.  A plain helper module (like clusters_ref.py): no device, no engine.

  field:  D = min(d2, K), d2 the integer squared distance to the nearest occupied cell, from scipy's exact EDT (the indices of the
          nearest feature, squared in integers)
  table:  Lf in Python's double (math.exp / math.log are the C library's), rounded to float32 once
  logw:   the end point of every used beam in fp64, its cell by floor, K off the map; the in-order fp64 sum (np.cumsum adds in
          order).  An end point within AMBIG cell of a cell edge is ambiguous -- any fp64 formulation may put it on either side --
          and for a particle with such a beam every sum over the candidate cells is listed."""
import math

import numpy as np
from scipy import ndimage

AMBIG = 1e-6


def K_of(max_occ_dist_m, resolution):
    q = max_occ_dist_m / float(np.float32(resolution))
    return math.ceil(q * q)


def field(grid, resolution, max_occ_dist_m=2.0):
    K = K_of(max_occ_dist_m, resolution)
    occ = np.asarray(grid) > 50
    if not occ.any():
        return np.full(occ.shape, K, np.uint16)
    _, (iy, ix) = ndimage.distance_transform_edt(~occ, return_indices=True)
    yy, xx = np.indices(occ.shape)
    d2 = (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2
    return np.minimum(d2, K).astype(np.uint16)


def table(resolution, z_hit=0.5, z_rand=0.5, sigma_hit_m=0.2, max_occ_dist_m=2.0, max_range_m=12.0, squash_factor=2.2):
    K = K_of(max_occ_dist_m, resolution)
    res = float(np.float32(resolution))
    res2, den, rnd, inv = res * res, 2.0 * sigma_hit_m * sigma_hit_m, z_rand / max_range_m, 1.0 / squash_factor
    out = np.empty(K + 1, np.float32)
    for k in range(K + 1):
        e = math.exp(-(k * res2) / den) if k < K else math.exp(-(max_occ_dist_m * max_occ_dist_m) / den)
        p = z_hit * e + rnd
        out[k] = np.float32(math.log(p) * inv if p > 0.0 else -math.inf)
    return out


def used_beams(angles, ranges, max_range_m):
    """(angle, range) of the beams that count (LF3), in beam order, both widened to double"""
    r = np.asarray(ranges, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = (r >= 0.0) & (r < max_range_m)
    return np.asarray(angles, np.float32).astype(np.float64)[keep], r[keep]


def _lookup(cx, cy, D):
    """D at the cells (cx, cy) (floats or ints), -1 off the map"""
    H, W = D.shape
    with np.errstate(invalid="ignore"):
        inside = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
    idx = np.where(inside, cy * W + cx, 0).astype(np.int64)
    return np.where(inside, D.ravel()[idx].astype(np.int64), -1)


def log_weights(p, angles, ranges, D, Lf, resolution, ox, oy, max_range_m, chunk=2048):
    """(logw, alternatives, ambiguous beams per particle): logw per particle (LF5); alternatives maps a particle with an ambiguous
    beam to the sorted list of every in-order sum over its candidate cells (the engine's value must be one of them)."""
    p = np.asarray(p, np.float64)
    a, r = used_beams(angles, ranges, max_range_m)
    K = Lf.size - 1
    lf = Lf.astype(np.float64)
    res = float(np.float32(resolution))
    N = p.shape[1]
    logw = np.zeros(N)
    alts, n_amb = {}, np.zeros(N, np.int64)
    if a.size == 0:
        return logw, alts, n_amb
    for s in range(0, N, chunk):
        q = p[:, s:s + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            ang = q[2][:, None] + a[None, :]
            fx = (q[0][:, None] + r[None, :] * np.cos(ang) - ox) / res
            fy = (q[1][:, None] + r[None, :] * np.sin(ang) - oy) / res
            d = _lookup(np.floor(fx), np.floor(fy), D)
            vals = lf[np.where(d < 0, K, d)]
            amb = (np.abs(fx - np.round(fx)) < AMBIG) | (np.abs(fy - np.round(fy)) < AMBIG)
        logw[s:s + q.shape[1]] = np.cumsum(np.concatenate([np.zeros((q.shape[1], 1)), vals], axis=1), axis=1)[:, -1]
        n_amb[s:s + q.shape[1]] = amb.sum(axis=1)
        for i in np.flatnonzero(amb.any(axis=1)):
            alts[s + int(i)] = _alternatives(fx[i], fy[i], amb[i], vals[i], D, lf, K)
    return logw, alts, n_amb


def _alternatives(fx, fy, amb, vals, D, lf, K):
    sums = {0.0}
    for j in range(vals.size):
        if amb[j]:
            xs = {math.floor(fx[j] - AMBIG), math.floor(fx[j] + AMBIG)}
            ys = {math.floor(fy[j] - AMBIG), math.floor(fy[j] + AMBIG)}
            vs = set()
            for x in xs:
                for y in ys:
                    d = int(_lookup(np.array([x]), np.array([y]), D)[0])
                    vs.add(float(lf[K if d < 0 else d]))
        else:
            vs = {float(vals[j])}
        sums = {t + v for t in sums for v in vs}
    return sorted(sums)
