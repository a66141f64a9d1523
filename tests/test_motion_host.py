"""The odometry motion models and the Gaussian initialisation on the host (mcl_host_motion_scalars, mcl_host_motion_sample,
mcl_host_gaussian_factor) against tests/motion_ref.py, the restatement written from the spec.  No device."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import motion_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("diff", "omni")

# zero motion, trans on both sides of 0.01, pure rotation, straight reverse, a diagonal, dtheta near +-pi, lateral slip
ACTIONS = [(0.0, 0.0, 0.0), (0.0099, 0.0, 0.0), (0.0101, 0.0, 0.0), (0.007, 0.007, 0.01), (0.0072, 0.0072, 0.01),
           (0.0, 0.0, 0.3), (0.0, 0.0, -1.2), (-0.1, 0.0, 0.0), (-0.25, 0.0, 0.02), (0.1, 0.1, 0.05), (-0.1, 0.07, -0.05),
           (0.05, 0.0, math.pi - 1e-9), (0.05, 0.0, -math.pi + 1e-9), (0.05, 0.0, 3.2), (0.1, 0.02, 0.0), (0.1, -0.02, 0.01),
           (1.5, 0.0, 0.4), (0.1, 0.0, 0.02)]


def alpha_sets():
    sets = [dict(), dict(floor_trans_m=0.005, floor_rot_rad=0.005), dict(alpha1=0.05, alpha2=0.3, alpha3=0.7, alpha4=0.01, alpha5=0.4)]
    for k in range(5):
        sets.append({f"alpha{i + 1}": (0.2 if i == k else 0.0) for i in range(5)})      # every alpha zero but one
    return sets


def ref_args(over):
    al = tuple(over.get(f"alpha{i + 1}", 0.2) for i in range(5))
    return al, (over.get("floor_trans_m", 0.0), over.get("floor_rot_rad", 0.0))


def test_scalars_equal_the_restatement(engine_mod):
    for model, over, act in itertools.product(MODELS, alpha_sets(), ACTIONS):
        cfg = engine_mod.default_motion_config(model=model, **over)
        got = engine_mod.host_motion_scalars(cfg, act)
        al, fl = ref_args(over)
        want = mr.scalars(model, act, al, fl)
        np.testing.assert_allclose(got, want, rtol=1e-15, atol=1e-15, err_msg=f"{model} {over} {act}")
        assert got[6] == 0.0 and got[7] == 0.0


def test_reverse_gets_no_half_turn_of_noise(engine_mod):
    cfg = engine_mod.default_motion_config(model="diff")
    fwd = engine_mod.host_motion_scalars(cfg, (0.1, 0.0, 0.0))
    rev = engine_mod.host_motion_scalars(cfg, (-0.1, 0.0, 0.0))
    assert abs(abs(rev[0]) - math.pi) < 1e-12                       # rot1 = pi: the robot "turns round" ...
    np.testing.assert_allclose(rev[3:6], fwd[3:6], rtol=0, atol=1e-12)   # ... and gets the noise of the forward move, not pi of it


def _poses(rng, n):
    return np.stack([rng.uniform(-30, 30, n), rng.uniform(-30, 30, n), rng.uniform(-math.pi, math.pi, n)])


def _assert_poses(got, want, tol=1e-13, msg=""):
    np.testing.assert_allclose(got[:2], want[:2], rtol=tol, atol=tol, err_msg=msg)
    d = (got[2] - want[2] + math.pi) % (2 * math.pi) - math.pi          # headings modulo 2 pi
    assert (np.abs(d) <= tol + tol * np.abs(want[2])).all(), msg
    assert (np.abs(got[2]) <= math.pi).all()


def test_sample_equals_the_restatement(engine_mod):
    rng = np.random.default_rng(1)
    n = 4096
    p, nrm = _poses(rng, n), rng.normal(size=(n, 3))
    for model, over, act in itertools.product(MODELS, alpha_sets()[:3], ACTIONS):
        cfg = engine_mod.default_motion_config(model=model, **over)
        got = engine_mod.host_motion_sample(cfg, act, p, nrm)
        al, fl = ref_args(over)
        _assert_poses(got, mr.sample(model, act, p, nrm, al, fl), msg=f"{model} {over} {act}")


def test_no_noise_is_the_composition_of_pose_and_action(engine_mod):
    rng = np.random.default_rng(2)
    n = 2048
    p, nrm = _poses(rng, n), rng.normal(size=(n, 3))
    zero = {f"alpha{i + 1}": 0.0 for i in range(5)}
    for model in MODELS:
        cfg = engine_mod.default_motion_config(model=model, **zero)
        for act in [(0.1, 0.0, 0.02), (0.1, 0.05, -0.3), (-0.2, 0.01, 0.1), (0.0, 0.0, 0.5), (0.3, -0.2, 0.0)]:
            want = mr.compose(act, p)
            _assert_poses(mr.sample(model, act, p, nrm, (0.0,) * 5), want, tol=1e-12, msg=f"ref {model} {act}")
            _assert_poses(engine_mod.host_motion_sample(cfg, act, p, nrm), want, tol=1e-12, msg=f"{model} {act}")


def test_diff_straight_equals_the_reference_straight_branch(orc, engine_mod):
    rng = np.random.default_rng(3)
    n = 2048
    p = _poses(rng, n)
    act = (0.1, 0.0, 0.0)
    ref = orc.motion_model(p, act, np.zeros((n, 3)), disp=(0.0, 0.0, 0.0))
    _assert_poses(mr.sample("diff", act, p, np.zeros((n, 3))), ref)
    _assert_poses(engine_mod.host_motion_sample(engine_mod.default_motion_config(), act, p, np.zeros((n, 3))), ref)


def test_config_refusals(engine_mod):
    lib = engine_mod.load_library()
    out, act = np.empty(8), np.array([0.1, 0.0, 0.0])
    pa, po = act.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    good = engine_mod.default_motion_config()
    assert (good.model, good.alpha1, good.alpha5, good.floor_trans_m, good.floor_rot_rad) == (engine_mod.MOTION_DIFF, 0.2, 0.2, 0.0, 0.0)
    assert lib.mcl_host_motion_scalars(ctypes.byref(good), pa, po) == 0
    bad = [dict(model=3), dict(model=-1), dict(model="reference"), dict(reserved=1), dict(alpha1=-0.1), dict(alpha4=float("nan")),
           dict(alpha5=float("inf")), dict(floor_trans_m=-1.0), dict(floor_rot_rad=float("nan"))]
    for over in bad:
        c = engine_mod.default_motion_config(**over)
        assert lib.mcl_host_motion_scalars(ctypes.byref(c), pa, po) == -1, over
        assert lib.mcl_host_motion_sample(ctypes.byref(c), pa, po, po, ctypes.c_int64(1), po) == -1, over
    assert lib.mcl_host_motion_scalars(None, pa, po) == -1
    assert lib.mcl_host_motion_scalars(ctypes.byref(good), pa, None) == -1
    assert lib.mcl_host_motion_scalars(ctypes.byref(good), None, po) == -1
    # a non-finite action is passed through
    assert np.isnan(engine_mod.host_motion_scalars(good, (float("nan"), 0.0, 0.0))[1])


def test_cholesky_factor_and_refusals(engine_mod):
    rng = np.random.default_rng(4)
    for _ in range(50):
        A = rng.normal(size=(3, 3))
        cov = A @ A.T
        L = engine_mod.host_gaussian_factor(cov)
        np.testing.assert_allclose(L, mr.cholesky(cov), rtol=1e-13, atol=1e-13)
        np.testing.assert_allclose(L @ L.T, cov, rtol=1e-12, atol=1e-12)
    assert np.array_equal(engine_mod.host_gaussian_factor(np.diag([0.25, 0.25, 0.16])), np.diag([0.5, 0.5, 0.4]))   # exact
    assert np.array_equal(engine_mod.host_gaussian_factor(np.zeros((3, 3))), np.zeros((3, 3)))
    nan, inf = float("nan"), float("inf")
    bad = [np.diag([0.25, -0.25, 0.1]), np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]),         # not PSD
           np.array([[1.0, 0.1, 0.0], [0.2, 1.0, 0.0], [0.0, 0.0, 1.0]]),                                      # not symmetric
           np.diag([1.0, nan, 1.0]), np.diag([inf, 1.0, 1.0])]
    for cov in bad:
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_gaussian_factor(cov)
        assert ei.value.status == -1
        with pytest.raises(ValueError):
            mr.cholesky(cov)


def test_rank_deficient_covariance_gives_one_heading(engine_mod):
    cov = np.array([[0.09, 0.03, 0.0], [0.03, 0.04, 0.0], [0.0, 0.0, 0.0]])
    L = engine_mod.host_gaussian_factor(cov)
    assert (L[2] == 0.0).all() and L[0, 0] > 0 and L[1, 1] > 0
    np.testing.assert_allclose(L, mr.cholesky(cov), rtol=1e-13, atol=1e-13)
    p = mr.init_gaussian(5, 0, (1.0, 2.0, 0.7), cov, 0, 4096)
    assert (p[2] == 0.7).all() and np.unique(p[0]).size == 4096


def test_numpy_philox_is_the_oracles(orc):
    for g, idx, stream, seed in [(0, 0, 5, 1), (12345, 3, 6, 0xDEADBEEFCAFE), ((1 << 32) + 7, 9, 0, 42), (99, 1, 8, (1 << 63) + 5)]:
        want = orc.eng_philox4x32((g & 0xFFFFFFFF, idx, stream, g >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        got = mr.philox4x32(np.array([g & 0xFFFFFFFF]), idx, stream, g >> 32, seed & 0xFFFFFFFF, seed >> 32)
        assert [int(v[0]) for v in got] == [int(v) for v in want]


def test_init_restatement(orc):
    """diag(0.25, 0.25, 0.16) is mcl_init_particles_pose's cloud; the sample covariance of the restatement at 2^20 lies in the
    6-sigma band of the estimator (the assertion the GPU test makes of the device's particles)."""
    pose = (0.3, -1.2, 0.5)
    np.testing.assert_allclose(mr.init_gaussian(77, 2, pose, np.diag([0.25, 0.25, 0.16]), 100, 5000), orc.eng_init_pose(77, 2, pose, 100, 5000),
                               rtol=1e-13, atol=1e-13)
    cov = np.array([[0.30, 0.12, 0.004], [0.12, 0.20, -0.003], [0.004, -0.003, 0.0025]])
    p = mr.init_gaussian(2024, 0, pose, cov, 0, 1 << 20)
    ok, worst = mr.cov_band_ok(p, pose, cov)
    print("worst |S_ij - Sigma_ij| / band:", worst)
    assert ok, worst


def test_motion_config_layout_matches_header(engine_mod, tmp_path):
    probe = tmp_path / "probe.c"
    fields = ["model", "reserved", "alpha1", "alpha2", "alpha3", "alpha4", "alpha5", "floor_trans_m", "floor_rot_rad"]
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcl_hip_engine.h"\n'
                     'int main(void){printf("%zu", sizeof(mcl_motion_config_t));'
                     + "".join(f'printf(" %zu", offsetof(mcl_motion_config_t, {f}));' for f in fields) +
                     'printf(" %d %d %d\\n", MCL_MOTION_REFERENCE, MCL_MOTION_DIFF, MCL_MOTION_OMNI);return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    M = engine_mod.MotionConfig
    want = [ctypes.sizeof(M)] + [getattr(M, f).offset for f in fields] + [engine_mod.MOTION_REFERENCE, engine_mod.MOTION_DIFF, engine_mod.MOTION_OMNI]
    assert got == want
