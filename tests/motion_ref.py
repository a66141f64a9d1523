"""Restatement of the odometry motion models and the Gaussian pose initialisation (include/mcl_hip_engine.h M2-M5 / G1,
DESIGN.md §4.11) in numpy + math, written from the spec and not from the engine's source: what the engine's host functions
and kernels are tested against.  Never shipped."""
import math

import numpy as np

PI = math.pi
DEFAULT_ALPHAS = (0.2, 0.2, 0.2, 0.2, 0.2)


def norm(z):
    return math.atan2(math.sin(z), math.cos(z))


def adiff(a, b):
    a, b = norm(a), norm(b)
    d1 = a - b
    d2 = 2.0 * PI - abs(d1)
    if d1 > 0.0:
        d2 = -d2
    return d1 if abs(d1) < abs(d2) else d2


def scalars(model, action, alphas=DEFAULT_ALPHAS, floors=(0.0, 0.0)):
    """M3: the 8 per-update scalars of model "diff" / "omni"."""
    dx, dy, dth = (float(v) for v in action)
    a1, a2, a3, a4, a5 = alphas
    ft, fr = floors
    trans = math.sqrt(dx * dx + dy * dy)
    if model == "diff":
        rot1 = 0.0 if trans < 0.01 else math.atan2(dy, dx)
        rot2 = adiff(dth, rot1)
        r1n = min(abs(adiff(rot1, 0.0)), abs(adiff(rot1, PI)))
        r2n = min(abs(adiff(rot2, 0.0)), abs(adiff(rot2, PI)))
        s1 = math.sqrt(a1 * r1n ** 2 + a2 * trans ** 2 + fr ** 2)
        st = math.sqrt(a3 * trans ** 2 + a4 * r1n ** 2 + a4 * r2n ** 2 + ft ** 2)
        s2 = math.sqrt(a1 * r2n ** 2 + a2 * trans ** 2 + fr ** 2)
        return np.array([rot1, trans, rot2, s1, st, s2, 0.0, 0.0])
    assert model == "omni"
    rot, bearing = dth, math.atan2(dy, dx)
    st = math.sqrt(a3 * trans ** 2 + a1 * rot ** 2 + ft ** 2)
    sr = math.sqrt(a4 * rot ** 2 + a2 * trans ** 2 + fr ** 2)
    ss = math.sqrt(a1 * rot ** 2 + a5 * trans ** 2 + ft ** 2)
    return np.array([bearing, trans, rot, st, sr, ss, 0.0, 0.0])


def normalize_angle(a):
    """the engine's: subtract / add 2 pi while outside [-pi, pi]"""
    a = np.array(a, np.float64)
    for _ in range(64):
        hi = a > PI
        if not hi.any():
            break
        a[hi] -= 2.0 * PI
    for _ in range(64):
        lo = a < -PI
        if not lo.any():
            break
        a[lo] += 2.0 * PI
    return a


def sample(model, action, p, normals, alphas=DEFAULT_ALPHAS, floors=(0.0, 0.0)):
    """M5: children of the poses p (3, n) with the normals (n, 3)."""
    s = scalars(model, action, alphas, floors)
    p = np.asarray(p, np.float64)
    n0, n1, n2 = (np.asarray(normals, np.float64).reshape(-1, 3)[:, k] for k in range(3))
    x, y, th = p[0], p[1], p[2]
    if model == "diff":
        r1 = s[0] - s[3] * n0
        t = s[1] - s[4] * n1
        r2 = s[2] - s[5] * n2
        return np.stack([x + t * np.cos(th + r1), y + t * np.sin(th + r1), normalize_angle(th + (r1 + r2))])
    t = s[1] + s[3] * n0
    r = s[2] + s[4] * n1
    sd = s[5] * n2
    b = s[0] + th
    return np.stack([x + (t * np.cos(b) + sd * np.sin(b)), y + (t * np.sin(b) - sd * np.cos(b)), normalize_angle(th + r)])


def compose(action, p):
    """The noise-free composition of the poses p (3, n) with a robot-frame displacement (dx, dy, dtheta)."""
    dx, dy, dth = action
    p = np.asarray(p, np.float64)
    c, s = np.cos(p[2]), np.sin(p[2])
    return np.stack([p[0] + dx * c - dy * s, p[1] + dx * s + dy * c, normalize_angle(p[2] + dth)])


def cholesky(cov):
    """G1: the lower factor of a symmetric positive semi-definite 3 x 3 covariance; ValueError where the engine refuses."""
    A = np.asarray(cov, np.float64).reshape(3, 3)
    if not np.isfinite(A).all():
        raise ValueError("non-finite")
    amax = np.abs(A).max()
    if (np.abs(A - A.T) > 1e-12 * amax).any():
        raise ValueError("not symmetric")
    tol = 1e-12 * max(A[0, 0], A[1, 1], A[2, 2], 0.0)
    L = np.zeros((3, 3))
    for j in range(3):
        p = A[j, j] - sum(L[j, k] * L[j, k] for k in range(j))
        if abs(p) <= tol:
            continue
        if p < 0.0:
            raise ValueError("not positive semi-definite")
        L[j, j] = math.sqrt(p)
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    return L


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (the engine's generator; checked against oracle.eng_philox4x32 in the tests)."""
    c = [np.asarray(v, np.uint64) & np.uint64(0xFFFFFFFF) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    M0, M1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def _bits53(a, b):
    return ((a << np.uint64(32)) | b) >> np.uint64(11)


def init_normals(seed, init_idx, first, n):
    """The three normals of particle g = first .. first + n - 1 of initialisation init_idx: Philox streams 5 (n0, n1) and 6 (n2),
    Box-Muller with u1 = (bits53 + 1) 2^-53, u2 = bits53 2^-53."""
    g = np.arange(first, first + n, dtype=np.uint64)
    lo, hi = g & np.uint64(0xFFFFFFFF), g >> np.uint64(32)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    two_m53 = 1.0 / 9007199254740992.0
    o = philox4x32(lo, init_idx, 5, hi, k0, k1)
    u1 = (_bits53(o[0], o[1]) + np.uint64(1)).astype(np.float64) * two_m53
    u2 = _bits53(o[2], o[3]).astype(np.float64) * two_m53
    rad = np.sqrt(-2.0 * np.log(u1))
    n0, n1 = rad * np.cos(2.0 * PI * u2), rad * np.sin(2.0 * PI * u2)
    o = philox4x32(lo, init_idx, 6, hi, k0, k1)
    u1 = (_bits53(o[0], o[1]) + np.uint64(1)).astype(np.float64) * two_m53
    u2 = _bits53(o[2], o[3]).astype(np.float64) * two_m53
    n2 = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * PI * u2)
    return np.stack([n0, n1, n2], axis=1)


def init_gaussian(seed, init_idx, mean, cov, first, n):
    """G1: the particles (3, n) of mcl_init_particles_gaussian."""
    L = cholesky(cov)
    nrm = init_normals(seed, init_idx, first, n)
    n0, n1, n2 = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    return np.stack([mean[0] + L[0, 0] * n0, mean[1] + (L[1, 0] * n0 + L[1, 1] * n1),
                     normalize_angle(mean[2] + (L[2, 0] * n0 + L[2, 1] * n1 + L[2, 2] * n2))])


def cov_band_ok(p, mean, cov):
    """Every entry of the sample covariance of p (3, n) about `mean` within 6 sqrt((Sii Sjj + Sij^2) / n) of Sij: the 6-sigma
    band of the estimator of a Gaussian's covariance.  Returns (ok, worst ratio)."""
    S = np.asarray(cov, np.float64).reshape(3, 3)
    d = np.asarray(p, np.float64) - np.asarray(mean, np.float64)[:, None]
    n = d.shape[1]
    got = d @ d.T / n
    worst = 0.0
    for i in range(3):
        for j in range(3):
            band = 6.0 * math.sqrt((S[i, i] * S[j, j] + S[i, j] ** 2) / n)
            worst = max(worst, abs(got[i, j] - S[i, j]) / band)
    return worst <= 1.0, worst
