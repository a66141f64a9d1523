"""Recovery by random-particle injection, host side (no GPU): mcl_host_recovery_step against a `math` statement of the rules in
include/mcl_hip_engine.h, the injection threshold at its edges, the refused configurations, the defaults and the
ctypes mirror of mcl_recovery_config_t.  The numpy statements of the per-child draw (Philox streams 8 and 9, the free-cell rule)
live here too; tests/test_gpu_recovery.py checks the device against them."""
import math

import numpy as np
import pytest

NAN = float("nan")
INF = float("inf")
TWO53 = 2 ** 53
MCL_ERR_INVALID_ARG = -1


# ---- statements of the header's rules (C's exp / log1p: +inf on overflow, log1p(-1) = -inf)
def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def _log1p(x):
    return -INF if x == -1.0 else math.log1p(x)


def logaddexp(a, b):
    hi, lo = (a, b) if a > b else (b, a)
    if hi == -INF:
        return -INF
    return hi + math.log1p(_exp(lo - hi))


def likelihood(max_logw, sum_w, denom, n_beams, per_beam):
    l = -INF if max_logw == -INF else max_logw + math.log(sum_w) - math.log(denom)
    return l / n_beams if per_beam else l


def fold(a_s, a_f, S, F, l):
    if math.isnan(l):
        return S, F
    S = l if math.isnan(S) else logaddexp(S + _log1p(-a_s), l + math.log(a_s))
    F = l if math.isnan(F) else logaddexp(F + _log1p(-a_f), l + math.log(a_f))
    return S, F


def p_of(S, F):
    if math.isnan(S) or math.isnan(F) or S == -INF:
        return 0.0
    return min(max(1.0 - _exp(F - S), 0.0), 1.0)


def threshold(p):
    """T = floor(p * 2^53): the exact scaling (p * 2^53 is a power-of-two multiple of a double)"""
    return int(math.floor(p * TWO53))


def step(a_s, a_f, per_beam, S, F, reset, max_logw, sum_w, denom, n_beams):
    if reset:
        S = F = NAN
    S, F = fold(a_s, a_f, S, F, likelihood(max_logw, sum_w, denom, n_beams, per_beam))
    return S, F, p_of(S, F)


# ---- the per-child draw (Philox4x32-10 as the engine and the oracle compute it, vectorised)
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & MASK, p1 & MASK, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & MASK, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c


def bits53(a, b):
    return ((a << np.uint64(32)) | b) >> np.uint64(11)


def child_draws(seed, upd, n, first=0):
    """(coin, pick, heading bits) of children first .. first + n - 1 of update `upd`: streams 8 (coin, pick) and 9 (heading)"""
    g = np.arange(first, first + n, dtype=np.uint64)
    lo, hi = g & MASK, g >> np.uint64(32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    v = philox4x32(lo, upd, 8, hi, k0, k1)
    t = philox4x32(lo, upd, 9, hi, k0, k1)
    return bits53(v[0], v[1]), bits53(v[2], v[3]), bits53(t[0], t[1])


def free_cells(grid):
    return np.flatnonzero(np.asarray(grid).ravel() == 0).astype(np.uint64)


def injected_poses(pick, hbits, free, W, resolution, ox, oy):
    """x = col * res + ox, y = row * res + oy for cell = free[umulhi(pick << 11, n_free)]; theta = (h * 2^-53 - 0.5) * 2 pi"""
    nf = len(free)
    # umulhi(pick << 11, nf) = floor(pick * nf / 2^53), exact in Python integers
    at = np.array([(int(k) * nf) >> 53 for k in pick], np.int64)
    cell = free[at]
    row, col = (cell // np.uint64(W)).astype(np.float64), (cell % np.uint64(W)).astype(np.float64)
    res = np.float64(np.float32(resolution))
    x = col * res + np.float64(ox)
    y = row * res + np.float64(oy)
    th = (hbits.astype(np.float64) * np.float64(2.0 ** -53) - np.float64(0.5)) * np.float64(2.0 * math.pi)
    return np.stack([x, y, th])


# ---- tests
@pytest.fixture(scope="module")
def eng(engine_mod):
    return engine_mod


def ulps(a, b):
    if math.isnan(a) or math.isnan(b):
        return 0 if (math.isnan(a) and math.isnan(b)) else 1 << 62
    if a == b:
        return 0
    if math.isinf(a) or math.isinf(b):
        return 1 << 62
    ia, ib = (np.array([v]).view(np.int64)[0] for v in (a, b))
    ia, ib = (int(v) if v >= 0 else -(int(v) & 0x7FFFFFFFFFFFFFFF) for v in (ia, ib))
    return abs(ia - ib)


def test_defaults_and_mirror(eng):
    import ctypes as C
    c = eng.default_recovery_config()
    assert (c.alpha_slow, c.alpha_fast, c.per_beam, c.reserved) == (0.001, 0.1, 1, 0)
    assert C.sizeof(eng.RecoveryConfig) == 24
    c2 = eng.default_recovery_config(alpha_slow=0.01, per_beam=0)
    assert (c2.alpha_slow, c2.alpha_fast, c2.per_beam) == (0.01, 0.1, 0)
    with pytest.raises(AttributeError):
        eng.default_recovery_config(alpha=0.1)


STATES = [(NAN, NAN), (NAN, -0.2), (-0.2, NAN), (-0.2, -0.2), (-0.3, -0.1), (-0.1, -0.3), (-INF, -0.5), (-0.5, -INF),
          (-INF, -INF), (-2500.0, -2400.0), (3.0, -7.5)]
SCALARS = [(-12.5, 37.25, 1000.0), (0.0, 1.0, 1.0), (-INF, 0.0, 512.0), (-INF, NAN, 512.0), (NAN, 3.0, 100.0),
           (-1e5, 4.0e6, 4194304.0), (-3.25, 0.5, 0.75), (2.0, 1.0, 1e-300)]


@pytest.mark.parametrize("per_beam", [0, 1])
@pytest.mark.parametrize("alphas", [(0.001, 0.1), (0.05, 1.0), (0.2, 0.5)])
def test_step_matches_statement(eng, per_beam, alphas):
    """every state (unset, -inf, finite) x scalar triple (finite, -inf max, NaN) x reset flag x beam count, within 2 ulp"""
    a_s, a_f = alphas
    c = eng.default_recovery_config(alpha_slow=a_s, alpha_fast=a_f, per_beam=per_beam)
    checked = 0
    for S, F in STATES:
        for mx, sw, d in SCALARS:
            for reset in (0, 1):
                for B in (1, 61, 1081):
                    got = eng.host_recovery_step(c, S, F, reset, mx, sw, d, B)
                    want = step(a_s, a_f, per_beam, S, F, reset, mx, sw, d, B)
                    for g, w, what in zip(got, want, ("S", "F", "p")):
                        assert ulps(g, w) <= 2, (what, S, F, mx, sw, d, reset, B, g, w)
                    checked += 1
    assert checked == len(STATES) * len(SCALARS) * 2 * 3


def test_step_rules(eng):
    c = eng.default_recovery_config()                          # 0.001, 0.1, per beam
    nan = math.isnan
    # unset state: seeded by l itself, p = 0 (S == F)
    S, F, p = eng.host_recovery_step(c, NAN, NAN, 0, -108.1, 1.0, 1.0, 1081)
    l0 = -108.1 / 1081
    assert S == F == l0 and p == 0.0
    # -inf likelihood: both averages fall, F faster; p > 0
    S2, F2, p2 = eng.host_recovery_step(c, S, F, 0, -INF, 0.0, 1000.0, 1081)
    assert S2 < S and F2 < S2 and 0.0 < p2 < 1.0
    assert S2 == S + math.log1p(-0.001) and F2 == F + math.log1p(-0.1)
    # -inf from unset: S = F = -inf, p = 0 (S = -inf)
    assert eng.host_recovery_step(c, NAN, NAN, 0, -INF, 0.0, 10.0, 1081) == (-INF, -INF, 0.0)
    # NaN likelihood leaves the state alone (also an unset one)
    assert eng.host_recovery_step(c, S2, F2, 0, NAN, 1.0, 10.0, 1081) == (S2, F2, p2)
    r = eng.host_recovery_step(c, NAN, NAN, 0, NAN, 1.0, 10.0, 1081)
    assert nan(r[0]) and nan(r[1]) and r[2] == 0.0
    # reset: the averages restart from l
    assert eng.host_recovery_step(c, S2, F2, 1, -108.1, 1.0, 1.0, 1081)[:2] == (l0, l0)
    # a kept update: D is the previous sum of weights -- l = m + log(sum_w) - log(D)
    raw = eng.default_recovery_config(per_beam=0)
    assert eng.host_recovery_step(raw, NAN, NAN, 0, -3.0, 20.0, 40.0, 1081)[0] == -3.0 + math.log(20.0) - math.log(40.0)
    # per_beam divides by B
    assert eng.host_recovery_step(c, NAN, NAN, 0, -3.0, 20.0, 40.0, 7)[0] == (-3.0 + math.log(20.0) - math.log(40.0)) / 7
    # p clamps: F above S gives 0, F = -inf gives 1
    assert eng.host_recovery_step(raw, -5.0, -1.0, 0, NAN, 1.0, 1.0, 1)[2] == 0.0
    assert eng.host_recovery_step(raw, -5.0, -INF, 0, NAN, 1.0, 1.0, 1)[2] == 1.0
    # alpha_fast = 1: F is the last l
    c1 = eng.default_recovery_config(alpha_fast=1.0, per_beam=0)
    assert eng.host_recovery_step(c1, -1.0, -1.0, 0, -9.0, 1.0, 1.0, 1)[1] == -9.0


def test_threshold_edges():
    assert threshold(1.0) == TWO53                      # every coin (< 2^53) injects
    assert threshold(0.0) == 0
    assert threshold(0.5) == TWO53 // 2
    assert threshold(2.0 ** -53) == 1
    assert threshold(2.0 ** -54) == 0                   # below one part in 2^53: no injection, the plain kernel
    assert threshold(1e-300) == 0
    p = math.nextafter(1.0, 0.0)
    assert threshold(p) == TWO53 - 1
    # the scaling is exact: T / 2^53 == p for every p that is a multiple of 2^-53
    for p in (0.3, 0.01, 1.0 / 3.0, 0.999):
        t = threshold(p)
        assert t <= p * TWO53 < t + 1


def test_philox_statement_matches_oracle(orc):
    seed, upd = 0x1234_5678_9ABC_DEF0 + 7, 5
    n = 40
    coin, pick, hb = child_draws(seed, upd, n, first=(1 << 32) - 20)       # across the high word of the counter
    for i in range(n):
        g = (1 << 32) - 20 + i
        o = orc.eng_philox4x32((g & 0xFFFFFFFF, upd, 8, g >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(coin[i]) == ((int(o[0]) << 32 | int(o[1])) >> 11)
        assert int(pick[i]) == ((int(o[2]) << 32 | int(o[3])) >> 11)
        t = orc.eng_philox4x32((g & 0xFFFFFFFF, upd, 9, g >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(hb[i]) == ((int(t[0]) << 32 | int(t[1])) >> 11)


def test_injected_heading_range():
    th = injected_poses(np.array([0, 1], np.uint64), np.array([0, TWO53 - 1], np.uint64), np.array([0], np.uint64), 4, 0.05, 0, 0)[2]
    assert th[0] == -math.pi and th[1] < math.pi


@pytest.mark.parametrize("field,value", [("alpha_slow", 0.0), ("alpha_slow", -0.1), ("alpha_slow", 0.1), ("alpha_slow", 0.2),
                                         ("alpha_slow", NAN), ("alpha_fast", 1.5), ("alpha_fast", INF), ("alpha_fast", NAN),
                                         ("per_beam", 2), ("per_beam", -1), ("reserved", 1)])
def test_refused_configs(eng, field, value):
    c = eng.default_recovery_config(**{field: value})
    with pytest.raises(eng.EngineError) as ex:
        eng.host_recovery_step(c, NAN, NAN, 0, -1.0, 1.0, 1.0, 1)
    assert ex.value.status == MCL_ERR_INVALID_ARG


def test_refused_arguments(eng):
    c = eng.default_recovery_config()
    for denom, B in ((0.0, 10), (-1.0, 10), (NAN, 10), (1.0, 0)):
        with pytest.raises(eng.EngineError):
            eng.host_recovery_step(c, NAN, NAN, 0, -1.0, 1.0, denom, B)
