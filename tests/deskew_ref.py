"""numpy restatement of scan de-skew (include/mcl_hip_engine.h): the constant-twist table of per-beam sensor
offsets (DM1, DM2), the effective angles and direction pairs (DS1), the beam origins (DS2), the likelihood field's pairs (DS5), and
the de-skewed log-weights under both models -- the beam model's through the oracle's cast_many per ray and the table sum in Q3's
order (DS3, DS4), the likelihood field's through lfield_ref's field, table and ambiguity rule.  A plain helper module (like
lfield_ref.py): no device, no engine; it imports oracle.oracle (handed in) and lfield_ref and changes neither."""
import numpy as np

import lfield_ref as lr


# ---- DM1 / DM2
def twist_delta(motion, tau):
    """DM1: the base's pose after the twist `motion` = (u, v, w) integrated over tau (an array), in its frame at tau = 0"""
    u, v, w = (float(k) for k in motion)
    tau = np.asarray(tau, np.float64)
    th = tau * w
    small = np.abs(th) < 1e-8
    safe = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th * th / 6.0, np.sin(safe) / safe)
    Bc = np.where(small, th / 2.0, (1.0 - np.cos(safe)) / safe)
    return np.stack([tau * (A * u - Bc * v) + 0.0, tau * (Bc * u + A * v) + 0.0, th + 0.0])


def stamps(n_beams, t=None):
    if t is not None:
        return np.asarray(t, np.float64)
    return np.arange(n_beams, dtype=np.float64) / (n_beams - 1) if n_beams > 1 else np.zeros(1)


def scan_motion_offsets(motion, n_beams, t=None, t_ref=1.0, mount=None):
    """(3, B): o_j = m^-1 o Delta(t_j - t_ref) o m (DM2); no mount: Delta itself"""
    d = twist_delta(motion, stamps(n_beams, t) - t_ref)
    if mount is None:
        return d
    mx, my, mth = (float(k) for k in mount)
    s, c = np.sin(d[2]), np.cos(d[2])
    xs, ys = d[0] + (c * mx - s * my), d[1] + (s * mx + c * my)
    sm, cm = np.sin(mth), np.cos(mth)
    ex, ey = xs - mx, ys - my
    return np.stack([(cm * ex + sm * ey) + 0.0, (cm * ey - sm * ex) + 0.0, d[2]])      # (+ 0.0: never -0)


# ---- DS1, DS2, DS5
def effective_angles(angles, offsets):
    """DS1: a'_j = (float)((double)a_j + dtheta_j)"""
    return (np.asarray(angles, np.float32).astype(np.float64) + np.asarray(offsets, np.float64)[2]).astype(np.float32)


def directions(eff):
    """(2, B): (cos, sin) of the widened float angle"""
    a = np.asarray(eff, np.float32).astype(np.float64)
    return np.stack([np.cos(a), np.sin(a)])


def origins(sensor_poses, offsets):
    """DS2: (x, y), each (n, B), in the rule's order"""
    p, o = np.asarray(sensor_poses, np.float64), np.asarray(offsets, np.float64)
    with np.errstate(invalid="ignore"):
        s, c = np.sin(p[2])[:, None], np.cos(p[2])[:, None]
        return p[0][:, None] + (c * o[0][None, :] - s * o[1][None, :]), p[1][:, None] + (s * o[0][None, :] + c * o[1][None, :])


def lf_pairs(ranges, offsets, dirs, resolution):
    """DS5: (2, B) in cells, for every beam (used or not)"""
    r = np.asarray(ranges, np.float32).astype(np.float64)
    inv = 1.0 / float(np.float32(resolution))
    o = np.asarray(offsets, np.float64)
    with np.errstate(invalid="ignore"):
        return np.stack([(o[0] + r * dirs[0]) * inv, (o[1] + r * dirs[1]) * inv])


# ---- DS3 / DS4: the beam model
def steps_at(orc, om, ox, oy, theta_s, eff):
    """DS3: cast_many's step of every ray from the origins (n, B) at theta_s_i + (double)a'_j"""
    n, B = ox.shape
    a = np.asarray(theta_s, np.float64)[:, None] + np.asarray(eff, np.float32).astype(np.float64)[None, :]
    return orc.cast_many(om, np.ascontiguousarray(ox).ravel(), np.ascontiguousarray(oy).ravel(), a.ravel())[1].reshape(n, B).astype(np.int64)


def table_sum(L, rows, steps):
    """DS4 in Q3's order: lane l adds beams l, l + 64, ... in fp64, then the butterfly over the 64 lanes (xor 32, 16, .. 1)"""
    n, B = steps.shape
    vals = np.asarray(L, np.float32)[np.asarray(rows, np.int64)[None, :], steps].astype(np.float64)
    lanes = np.zeros((n, 64))
    with np.errstate(invalid="ignore"):
        for j0 in range(0, B, 64):
            k = min(64, B - j0)
            lanes[:, :k] = lanes[:, :k] + vals[:, j0:j0 + k]
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ o]
    return lanes[:, 0].copy()


def beam_log_weights(orc, om, L, scan, ox, oy, theta_s, eff):
    """(logw (n,), steps (n, B)) of the de-skewed beam model at the origins given"""
    st = steps_at(orc, om, ox, oy, theta_s, eff)
    return table_sum(L, orc.obs_index(scan, om), st), st


# ---- DS5 with LF3-LF5: the likelihood field
def lf_log_weights(sensor_poses, eff, ranges, offsets, D, Lf, resolution, origin_x, origin_y, max_range_m):
    """lfield_ref.log_weights with DS5's pairs: (logw, alternatives, ambiguous beams per particle).  The end point of a used beam is
    the sensor pose composed with its pair; cell by floor, K off the map, the in-order fp64 sum; an end point within lr.AMBIG of a
    cell edge is ambiguous and every sum over its candidate cells is listed."""
    p = np.asarray(sensor_poses, np.float64)
    r = np.asarray(ranges, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = (r >= 0.0) & (r < max_range_m)
    K = Lf.size - 1
    lf = Lf.astype(np.float64)
    res = float(np.float32(resolution))
    N = p.shape[1]
    logw, alts, n_amb = np.zeros(N), {}, np.zeros(N, np.int64)
    if not keep.any():
        return logw, alts, n_amb
    pairs = lf_pairs(ranges, offsets, directions(eff), resolution)[:, keep]      # cells
    with np.errstate(invalid="ignore", over="ignore"):
        s, c = np.sin(p[2])[:, None], np.cos(p[2])[:, None]
        fx = (p[0][:, None] - origin_x) / res + (c * pairs[0][None, :] - s * pairs[1][None, :])
        fy = (p[1][:, None] - origin_y) / res + (s * pairs[0][None, :] + c * pairs[1][None, :])
        d = lr._lookup(np.floor(fx), np.floor(fy), D)
        vals = lf[np.where(d < 0, K, d)]
        amb = (np.abs(fx - np.round(fx)) < lr.AMBIG) | (np.abs(fy - np.round(fy)) < lr.AMBIG)
    logw[:] = np.cumsum(np.concatenate([np.zeros((N, 1)), vals], axis=1), axis=1)[:, -1]
    n_amb[:] = amb.sum(axis=1)
    for i in np.flatnonzero(amb.any(axis=1)):
        alts[int(i)] = lr._alternatives(fx[i], fy[i], amb[i], vals[i], D, lf, K)
    return logw, alts, n_amb


def lf_agree_counts(sensor_poses, eff, ranges, offsets, D, Ka, resolution, origin_x, origin_y, max_range_m):
    """beam_skip_ref.counts at DS5's end points: (lo, hi, ambiguous) -- the agreement counts (BS1, BS2) of the used beams as a band"""
    p = np.asarray(sensor_poses, np.float64)
    r = np.asarray(ranges, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = (r >= 0.0) & (r < max_range_m)
    res = float(np.float32(resolution))
    pairs = lf_pairs(ranges, offsets, directions(eff), resolution)[:, keep]
    with np.errstate(invalid="ignore", over="ignore"):
        s, c = np.sin(p[2])[:, None], np.cos(p[2])[:, None]
        fx = (p[0][:, None] - origin_x) / res + (c * pairs[0][None, :] - s * pairs[1][None, :])
        fy = (p[1][:, None] - origin_y) / res + (s * pairs[0][None, :] + c * pairs[1][None, :])
        d = lr._lookup(np.floor(fx), np.floor(fy), D)
        amb = (np.abs(fx - np.round(fx)) < lr.AMBIG) | (np.abs(fy - np.round(fy)) < lr.AMBIG)
    agree = (d >= 0) & (d < Ka)
    lo, n_amb = (agree & ~amb).sum(axis=0), amb.sum(axis=0)
    return lo, lo + n_amb, int(n_amb.sum())


# ---- the fixtures the two test files share (tests/test_scan_deskew_host.py checks their preconditions without a device)
MOTION = (0.175, 0.02, 0.12)          # 7 m/s over a 25 ms sweep, a little sideways, 6.9 degrees of turn: 3.5 cells of the 0.05 m maps
MOUNT = (0.27, 0.05, 0.4)
LF_N = 4097


def table_of(B, k=0, mount=None):
    """the k-th table of a chain of updates: another twist, another reference time (the end, the middle, the start of the sweep)"""
    motion = (MOTION[0] + 0.02 * k, MOTION[1] - 0.03 * k, MOTION[2] - 0.05 * k)
    return scan_motion_offsets(motion, B, t_ref=(1.0, 0.5, 0.0)[k % 3], mount=mount)


def sm2(m, p):
    """SM2 in numpy, in the rule's order (the sensor poses of base poses)"""
    with np.errstate(invalid="ignore"):
        s, c = np.sin(p[2]), np.cos(p[2])
        return np.stack([p[0] + (c * m[0] - s * m[1]), p[1] + (s * m[0] + c * m[1]), p[2] + m[2]])


def shorten(scan, lo=0.28, hi=0.39):
    s = scan.copy()
    s[int(lo * s.size):int(hi * s.size)] *= np.float32(0.4)
    return s


def lf_fixture(sg, orc, g, ang, mount=None):
    """(base poses (3, LF_N), scan, offsets) of the likelihood-field tests: a tight cloud around the true pose, the scan cast from
    the true sensor pose with odd readings and a shortened sector, the first table"""
    p0 = sg.cloud_around(g, np.random.default_rng(5), LF_N, sig_cells=(1.0, 1.0), sig_theta=0.05)
    pose = g.true_pose if mount is None else tuple(sm2(mount, np.array(g.true_pose).reshape(3, 1))[:, 0])
    scan = sg.odd_scan(shorten(sg.perturbed_scan(orc, g.oracle(orc), ang, pose, seed=g.perturb_seed)))
    return p0, scan, table_of(ang.size, 0, mount)


def moving_scan(orc, om, ang, pose, offsets, ox=None, oy=None):
    """the scan a moving sensor takes: beam j cast from its own origin (DS2 of the true sensor pose `pose`; ox / oy (B,): origins
    given instead, e.g. the engine's own) at pose.theta + (double)a'_j; (ranges, steps)"""
    eff = effective_angles(ang, offsets)
    if ox is None:
        x, y = origins(np.array(pose, np.float64).reshape(3, 1), offsets)
        ox, oy = x[0], y[0]
    a = float(pose[2]) + eff.astype(np.float64)
    r, st = orc.cast_many(om, np.ascontiguousarray(ox), np.ascontiguousarray(oy), a)
    return r.astype(np.float32), st.astype(np.int64)
