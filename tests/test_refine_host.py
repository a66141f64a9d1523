"""The host restatements of the pose refinement (mcl_host_refine_window / mcl_host_refine_reduce, DESIGN.md §4.14, rules R1, R3, R4
of include/mcl_hip_engine.h) against the Python statement tests/refine_ref.py, without a device; and the two conditions the
fixture of tests/test_gpu_refine.py must meet, decided by the statement tests/lfield_ref.py alone."""
import ctypes as C
import math

import numpy as np
import pytest

import lfield_ref as lr
import refine_ref as rr

WINDOWS = [(0, 0), (1, 0), (0, 3), (4, 10)]
SEED = rr.LATTICE_POSE


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- R1
@pytest.mark.parametrize("hxy,hth", WINDOWS)
def test_window_is_r1(engine_mod, hxy, hth):
    for seed, extra in ((SEED, {}), ((-0.0, 1e6 + 0.1, -7.5), dict(step_xy_cells=0.3, step_theta_rad=0.0123))):
        got = engine_mod.host_refine_window(seed, rr.RES, half_xy=hxy, half_theta=hth, **extra)
        want = rr.window(seed, rr.RES, half_xy=hxy, half_theta=hth, **extra)
        assert got.shape == want.shape == ((2 * hxy + 1) ** 2 * (2 * hth + 1), 3)
        assert np.array_equal(bits(got), bits(want))
    # ix is the fastest index, then iy, then it; the centre is the seed
    c = (hth * (2 * hxy + 1) + hxy) * (2 * hxy + 1) + hxy
    w = engine_mod.host_refine_window(SEED, rr.RES, half_xy=hxy, half_theta=hth)
    assert np.array_equal(w[c], np.array(SEED))
    if hxy:
        assert w[1, 0] > w[0, 0] and w[1, 1] == w[0, 1] and w[2 * hxy + 1, 1] > w[0, 1]


def test_default_config(engine_mod):
    c = engine_mod.default_refine_config()
    assert (c.half_xy, c.half_theta, c.step_xy_cells, c.step_theta_rad, c.beam_stride) == (4, 10, 0.5, math.pi / 360, 1)
    assert list(c.reserved) == [0, 0, 0] and engine_mod.refine_window_size(c) == 1701
    assert C.sizeof(engine_mod.RefineConfig) == 40 and engine_mod.REFINE_DTYPE.itemsize == 152


REFUSED = [dict(half_xy=-1), dict(half_theta=-1), dict(step_xy_cells=0.0), dict(step_xy_cells=-0.5), dict(step_xy_cells=math.inf),
           dict(step_xy_cells=math.nan), dict(step_theta_rad=0.0), dict(step_theta_rad=math.inf), dict(step_theta_rad=math.nan),
           dict(beam_stride=0), dict(reserved=(0, 1, 0)), dict(reserved=(0, 0, 1)),
           dict(half_xy=90, half_theta=1),                 # 181 * 181 * 3 > 32768
           dict(half_xy=0, half_theta=16384),              # 32769
           dict(half_xy=2 ** 30, half_theta=2 ** 30)]


@pytest.mark.parametrize("fields", REFUSED)
def test_refused_configs(engine_mod, fields):
    INVALID = engine_mod.MCL_ERR_INVALID_ARG
    with pytest.raises(engine_mod.EngineError) as ei:
        engine_mod.host_refine_window(SEED, rr.RES, **fields)
    assert ei.value.status == INVALID
    with pytest.raises(engine_mod.EngineError) as ei:
        engine_mod.host_refine_reduce(SEED, rr.RES, np.zeros(1), **fields)
    assert ei.value.status == INVALID


def test_refused_arguments(engine_mod):
    INVALID = engine_mod.MCL_ERR_INVALID_ARG
    for bad in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)):
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_refine_window(bad, rr.RES)
        assert ei.value.status == INVALID
    for res in (0.0, -0.05, math.nan, math.inf):
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_refine_window(SEED, res)
        assert ei.value.status == INVALID
    for scores in (np.zeros(1700), np.full(1701, np.nan), np.full(1701, np.inf)):           # a wrong n_win, NaN, +inf
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_refine_reduce(SEED, rr.RES, scores)
        assert ei.value.status == INVALID
    assert engine_mod.host_refine_window(SEED, rr.RES, half_xy=0, half_theta=16383).shape == (32767, 3)     # the largest window


# ---- R3
def synthetic_cases():
    """(name, window fields, scores): the ties R3 decides"""
    F = dict(half_xy=2, half_theta=1)                       # 5 x 5 x 3 = 75 poses, centre 37
    n, c = 75, 37
    rng = np.random.default_rng(3)
    out = [("all equal", F, np.full(n, -3.25))]
    s = rng.normal(-40.0, 2.0, n)
    s[0] = s[c + 1] = 5.0                                   # q = 9 (a corner) and q = 1
    out.append(("two maxima, different q", F, s.copy()))
    s = rng.normal(-40.0, 2.0, n)
    s[c + 5] = s[c - 5] = s[c + 1] = s[c + 25] = 5.0        # q = 1 four times: the lowest index (c - 5) wins
    out.append(("equal q", F, s.copy()))
    s = rng.normal(-40.0, 2.0, n)
    s[::3] = -np.inf
    s[c] = -np.inf
    out.append(("-inf entries", F, s.copy()))
    out.append(("void", F, np.full(n, -np.inf)))
    s = np.full(n, -np.inf)
    s[11] = -7.0
    out.append(("one hot", F, s.copy()))
    for hxy, hth in WINDOWS:
        f = dict(half_xy=hxy, half_theta=hth)
        k = (2 * hxy + 1) ** 2 * (2 * hth + 1)
        out.append((f"random {hxy} {hth}", f, rng.normal(-30.0, 3.0, k)))
        out.append((f"flat steps {hxy} {hth}", f, np.round(rng.normal(-30.0, 1.0, k))))       # many exact ties
    return out


CASES = synthetic_cases()


@pytest.mark.parametrize("name,fields,scores", CASES, ids=[c[0] for c in CASES])
def test_best_is_r3(engine_mod, name, fields, scores):
    r = engine_mod.host_refine_reduce(SEED, rr.RES, scores, **fields)
    wb = rr.best(scores, **fields)
    n = scores.size
    centre = (n - 1) // 2
    assert int(r["best_index"]) == wb
    assert np.array_equal(bits(r["best"]), bits(rr.window(SEED, rr.RES, **fields)[wb]))
    assert bits(r["best_log_likelihood"]) == bits(scores[wb]) and bits(r["seed_log_likelihood"]) == bits(scores[centre])
    if name in ("all equal", "void"):
        assert wb == centre
    if name == "two maxima, different q":
        assert wb == centre + 1
    if name == "equal q":
        assert wb == centre - 5


# ---- R4
@pytest.mark.parametrize("name,fields,scores", CASES, ids=[c[0] for c in CASES])
def test_moments_are_r4(engine_mod, name, fields, scores):
    r = engine_mod.host_refine_reduce(SEED, rr.RES, scores, **fields)
    best, mean, cov, S = rr.moments(SEED, rr.RES, scores, **fields)
    tol_mean, tol_cov, tol_s = rr.tolerances(rr.RES, **fields)
    err_mean, err_cov, err_s = np.abs(r["mean"] - mean), np.abs(r["cov"] - cov), abs(float(r["weight_sum"]) - S)
    print(name, "mean err / tol", (err_mean / tol_mean).max(), "cov err / tol", (err_cov / tol_cov).max(), "S err", err_s, tol_s)
    assert np.all(err_mean <= tol_mean) and np.all(err_cov <= tol_cov) and err_s <= tol_s
    assert np.array_equal(r["cov"], r["cov"].T)
    st = np.array(rr.steps(rr.RES, **fields))
    if name in ("void", "one hot") or scores.size == 1:
        # one pose (or none) carries the weight: mean = best, cov = the box term alone
        assert float(r["weight_sum"]) == (0.0 if name == "void" else 1.0)
        assert np.array_equal(bits(r["mean"]), bits(r["best"]))
        assert np.array_equal(r["cov"], np.diag(st * st / 12.0))
    if name == "void":
        assert np.array_equal(r["mean"], np.array(SEED)) and r["best_log_likelihood"] == -np.inf
    if name == "all equal":
        assert float(r["weight_sum"]) == scores.size
    # G1 accepts it
    L = engine_mod.host_gaussian_factor(r["cov"])
    assert np.all(np.diag(L) > 0.0)


def test_reduce_is_repeatable(engine_mod):
    s = CASES[-2][2]
    a, b = (engine_mod.host_refine_reduce(SEED, rr.RES, s, **CASES[-2][1]) for _ in range(2))
    assert a.tobytes() == b.tobytes()


# ---- the fixture of tests/test_gpu_refine.py, decided by tests/lfield_ref.py alone
@pytest.fixture(scope="module")
def fixture_volume(orc):
    m = rr.SmallMap()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    ang = rr.angles(orc, 61)
    obs = rr.perturbed_scan(orc, om, ang, rr.P_STAR)
    D, Lf = lr.field(m.data, m.resolution), lr.table(m.resolution)
    win = rr.window(rr.LATTICE_POSE, rr.RES, **rr.FIXTURE_WINDOW)
    want, alts, n_amb = lr.log_weights(np.ascontiguousarray(win.T), ang, obs, D, Lf, m.resolution, rr.OX, rr.OY, rr.MAX_RANGE)
    return ang, obs, want, alts, n_amb


def test_fixture_has_no_ambiguous_beam(fixture_volume):
    """(a): no used beam of any window pose ends within 1e-6 cell of a cell edge"""
    ang, obs, want, alts, n_amb = fixture_volume
    assert lr.used_beams(ang, obs, rr.MAX_RANGE)[0].size == 61
    assert int(n_amb.sum()) == 0 and not alts


def test_fixture_best_is_near_the_true_pose(fixture_volume):
    """(b): the R3-best of the statement's volume lies within 2 steps in x and y and 1 step in theta of P*"""
    ang, obs, want, alts, n_amb = fixture_volume
    d = rr.offsets(**rr.FIXTURE_WINDOW)[rr.best(want, **rr.FIXTURE_WINDOW)]
    err = np.abs(d - np.array(rr.P_STAR_STEPS))
    print("best offset", d, "P* at", rr.P_STAR_STEPS)
    assert err[0] <= 2.0 and err[1] <= 2.0 and err[2] <= 1.0
    # (P_STAR_STEPS is P* - seed in steps)
    st = np.array(rr.steps(rr.RES))
    assert np.allclose((np.array(rr.P_STAR) - np.array(rr.LATTICE_POSE)) / st, rr.P_STAR_STEPS, atol=1e-6)
