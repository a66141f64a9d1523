"""The sensor mount's host functions (mcl_host_sensor_mount / _unmount / _mount_cov, DESIGN.md §4.25, rules SM1 / SM2) without a
GPU: against numpy's statement of SM2, the round trip, the covariance map against J S J^T, SM1's refusals, and the new names in the
header and in EXPORTS."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOUNTS = [(0.27, 0.0, 0.0), (-0.4, 0.3, 2.5), (0.0, 0.0, -np.pi)]
RTOL = 1e-13
N = 4096


def poses():
    rng = np.random.default_rng(20250607)
    p = np.empty((3, N))
    p[0] = rng.uniform(-60.0, 60.0, N)
    p[1] = rng.uniform(-45.0, 45.0, N)
    p[2] = rng.uniform(-np.pi, np.pi, N)
    p[2, :4] = [np.pi, -np.pi, 0.0, -0.0]
    return p


def sm2(m, p):
    """SM2 in numpy, in the rule's order"""
    mx, my, mth = m
    s, c = np.sin(p[2]), np.cos(p[2])
    return np.stack([p[0] + (c * mx - s * my), p[1] + (s * mx + c * my), p[2] + mth])


def bound(m, coord):
    # three roundings (two products' difference, the sum) and a libm sincos within 1 ulp, about 4x in hand
    return 2.0 ** -50 * (np.abs(coord) + abs(m[0]) + abs(m[1]))


@pytest.mark.parametrize("m", MOUNTS)
def test_mount_matches_numpy(engine_mod, m):
    p = poses()
    got, ref = engine_mod.host_sensor_mount(m, p), sm2(m, p)
    assert np.array_equal(got[2].view(np.uint64), ref[2].view(np.uint64))          # one IEEE add
    for k in (0, 1):
        assert np.all(np.abs(got[k] - ref[k]) <= bound(m, ref[k])), k


@pytest.mark.parametrize("m", MOUNTS)
def test_unmount_inverts_mount(engine_mod, m):
    p = poses()
    back = engine_mod.host_sensor_unmount(m, engine_mod.host_sensor_mount(m, p))
    for k in (0, 1):
        assert np.all(np.abs(back[k] - p[k]) <= 2.0 * bound(m, p[k])), k
    # the heading: (theta + mtheta) - mtheta, two rounded adds at the size of the larger operand
    assert np.all(np.abs(back[2] - p[2]) <= 2.0 ** -52 * (np.abs(p[2]) + abs(m[2])))


def test_zero_mount_is_the_identity(engine_mod):
    p = poses()
    for m in [(0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)]:
        got = engine_mod.host_sensor_mount(m, p)
        assert np.array_equal(got[0], p[0]) and np.array_equal(got[1], p[1]) and np.array_equal(got[2], p[2])
        assert np.array_equal(engine_mod.host_sensor_unmount(m, p), p)


@pytest.mark.parametrize("m", MOUNTS)
def test_covariance_map(engine_mod, m):
    rng = np.random.default_rng(7)
    for _ in range(32):
        A = rng.normal(size=(3, 3)) * [0.3, 0.3, 0.1]
        S = A @ A.T
        pose = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-np.pi, np.pi)])
        s, c = np.sin(pose[2]), np.cos(pose[2])
        J = np.array([[1.0, 0.0, -(s * m[0] + c * m[1])], [0.0, 1.0, c * m[0] - s * m[1]], [0.0, 0.0, 1.0]])
        got = engine_mod.host_sensor_mount_cov(m, pose, S)
        np.testing.assert_allclose(got, J @ S @ J.T, rtol=RTOL, atol=RTOL * np.abs(J @ S @ J.T).max())
        # to the base frame: the inverse's Jacobian at the sensor pose is the inverse matrix, so the covariance comes back
        sp = engine_mod.host_sensor_mount(m, pose.reshape(3, 1))[:, 0]
        th = sp[2] - m[2]
        s, c = np.sin(th), np.cos(th)
        Ji = np.array([[1.0, 0.0, s * m[0] + c * m[1]], [0.0, 1.0, -(c * m[0] - s * m[1])], [0.0, 0.0, 1.0]])
        back = engine_mod.host_sensor_mount_cov(m, sp, got, to_base=True)
        np.testing.assert_allclose(back, Ji @ got @ Ji.T, rtol=RTOL, atol=RTOL * np.abs(back).max())
        np.testing.assert_allclose(back, S, rtol=1e-9, atol=1e-9 * np.abs(S).max())


def test_refusals_are_sm1(engine_mod):
    lib = engine_mod.load_library()
    p, out = poses(), np.empty((3, N))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ok = np.array([0.1, 0.2, 2.0 * np.pi])
    assert lib.mcl_host_sensor_mount(ptr(ok), ptr(p), N, ptr(out)) == 0
    ok[2] = -2.0 * np.pi
    assert lib.mcl_host_sensor_unmount(ptr(ok), ptr(p), N, ptr(out)) == 0
    cov, o9 = np.eye(3), np.empty(9)
    for bad in [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 0, np.nan), (0, 0, np.nextafter(2.0 * np.pi, 7.0)),
                (0, 0, -np.nextafter(2.0 * np.pi, 7.0))]:
        b = np.array(bad, np.float64)
        assert lib.mcl_host_sensor_mount(ptr(b), ptr(p), N, ptr(out)) == -1, bad
        assert lib.mcl_host_sensor_unmount(ptr(b), ptr(p), N, ptr(out)) == -1, bad
        assert lib.mcl_host_sensor_mount_cov(ptr(b), ptr(p[:, 0].copy()), ptr(cov), 0, ptr(o9)) == -1, bad
    ok[2] = 0.5
    assert lib.mcl_host_sensor_mount(None, ptr(p), N, ptr(out)) == -1
    assert lib.mcl_host_sensor_mount(ptr(ok), None, N, ptr(out)) == -1
    assert lib.mcl_host_sensor_mount(ptr(ok), ptr(p), N, None) == -1
    assert lib.mcl_host_sensor_mount(ptr(ok), ptr(p), 0, ptr(out)) == -1
    assert lib.mcl_host_sensor_mount_cov(ptr(ok), ptr(np.array([0.0, np.nan, 0.0])), ptr(cov), 0, ptr(o9)) == -1
    assert lib.mcl_host_sensor_mount_cov(ptr(ok), ptr(np.zeros(3)), ptr(cov), 2, ptr(o9)) == -1
    # the engine-side setters refuse a null engine before anything else
    assert lib.mcl_set_sensor_mount(None, ptr(ok)) == -1 and lib.mcl_get_sensor_mount(None, ptr(out)) == -1
    assert lib.mcl_sensor_update_fuse(None, None, 0) == -1 and lib.mcl_group_set_sensor_mount(None, ptr(ok)) == -1
    assert lib.mcl_mount_poses(None, ptr(p), N, ptr(out)) == -1 and lib.mcl_get_sensor_poses(None, ptr(out), N) == -1
    with pytest.raises(engine_mod.EngineError):
        engine_mod.host_sensor_mount((0.0, 0.0, 7.0), p)


def test_names_are_exported_and_declared(engine_mod):
    names = ["mcl_set_sensor_mount", "mcl_get_sensor_mount", "mcl_mount_poses", "mcl_get_sensor_poses", "mcl_sensor_update_fuse",
             "mcl_group_set_sensor_mount", "mcl_host_sensor_mount", "mcl_host_sensor_unmount", "mcl_host_sensor_mount_cov"]
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mcl_hip_engine.h")).read(), flags=re.S)
    lib = engine_mod.load_library()
    for n in names:
        assert n in engine_mod.EXPORTS and re.search(r"\b%s\s*\(" % n, src) and hasattr(lib, n), n
