"""Scan de-skew without a GPU: mcl_host_scan_motion_offsets against tests/deskew_ref.py's statement of DM1 / DM2,
the setter's host-side table formation (DS1, DS5's pairs) against the same module, the refusals, the new names in the header and in
EXPORTS, and the preconditions of the fixtures tests/test_gpu_scan_deskew.py works with, on the CPU statement alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deskew_ref as dr
import lfield_ref as lr
import side_geometries as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOUNTS = [None, (0.27, 0.0, 0.0), (-0.4, 0.3, 2.5), (0.0, 0.0, -np.pi)]
B = 61


def bound(motion, tau, mount):
    # DM1 is a libm sine and cosine within 1 ulp, two quotients, two products' difference and a product; DM2 adds a second sincos
    # pair and eight roundings: at most a dozen errors of 2^-53 .. 2^-52 relative to quantities no larger than
    # M = |tau| (|u| + |v|) + 2 (|mx| + |my|), i.e. below 12 * 2^-52 M < 2^-48 M
    m = (0.0, 0.0) if mount is None else mount
    return 2.0 ** -48 * (np.abs(tau) * (abs(motion[0]) + abs(motion[1])) + 2.0 * (abs(m[0]) + abs(m[1])))


def check(engine_mod, motion, n, t=None, t_ref=1.0, mount=None):
    got = engine_mod.host_scan_motion_offsets(motion, n, t=t, t_ref=t_ref, mount=mount)
    want = dr.scan_motion_offsets(motion, n, t=t, t_ref=t_ref, mount=mount)
    tau = dr.stamps(n, t) - t_ref
    assert got.shape == (3, n)
    assert np.array_equal(got[2].view(np.uint64), want[2].view(np.uint64))          # tau w: one IEEE product, whatever the mount
    for k in (0, 1):
        assert np.all(np.abs(got[k] - want[k]) <= bound(motion, tau, mount)), (k, motion, t_ref, mount)
    return got


@pytest.mark.parametrize("mount", MOUNTS)
@pytest.mark.parametrize("t_ref", [0.0, 0.5, 1.0])
def test_zero_twist_is_zeros(engine_mod, mount, t_ref):
    got = engine_mod.host_scan_motion_offsets((0.0, 0.0, 0.0), B, t_ref=t_ref, mount=mount)
    assert np.array_equal(got.view(np.uint64), np.zeros((3, B)).view(np.uint64))     # +0.0, bit for bit


@pytest.mark.parametrize("mount", MOUNTS)
@pytest.mark.parametrize("t_ref", [0.0, 0.5, 1.0])
def test_against_the_statement(engine_mod, mount, t_ref):
    for motion in [(0.175, 0.0, 0.0), (0.1, -0.05, 0.0), (0.0, 0.0, 0.12), (0.0, 0.0, -0.3), dr.MOTION, (-0.2, 0.04, -0.09)]:
        got = check(engine_mod, motion, B, t_ref=t_ref, mount=mount)
        if motion[2] == 0.0 and mount is None:
            # pure translation: the offset is tau (u, v), the heading stays
            tau = dr.stamps(B) - t_ref
            assert np.array_equal(got[0], tau * motion[0] + 0.0) and np.array_equal(got[1], tau * motion[1] + 0.0) and not got[2].any()
    # pure rotation about a mounted sensor: the sensor moves on a circle of radius |m| about the base, its heading turns by theta
    if mount is not None:
        w = 0.12
        got = engine_mod.host_scan_motion_offsets((0.0, 0.0, w), B, t_ref=t_ref, mount=mount)
        th = (dr.stamps(B) - t_ref) * w
        r = np.hypot(mount[0], mount[1])
        # |o_xy| is the chord of the turn, 2 r |sin(theta / 2)|
        assert np.allclose(np.hypot(got[0], got[1]), 2.0 * r * np.abs(np.sin(th / 2.0)), rtol=0, atol=2.0 ** -45 * max(r, 1.0))
        assert np.array_equal(got[2], th + 0.0)


def test_stamps_given_and_defaulted_and_one_beam(engine_mod):
    rng = np.random.default_rng(11)
    t = np.sort(rng.uniform(-0.2, 1.3, B))
    for mount in MOUNTS:
        check(engine_mod, dr.MOTION, B, t=t, t_ref=0.4, mount=mount)
        a = engine_mod.host_scan_motion_offsets(dr.MOTION, B, mount=mount)
        b = engine_mod.host_scan_motion_offsets(dr.MOTION, B, t=np.arange(B) / (B - 1.0), mount=mount)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))                  # the default stamps are j / (B - 1)
        # B = 1: the one stamp is 0
        one = check(engine_mod, dr.MOTION, 1, t_ref=1.0, mount=mount)
        assert np.array_equal(one, check(engine_mod, dr.MOTION, 1, t=np.zeros(1), t_ref=1.0, mount=mount))
        assert one[2, 0] == -dr.MOTION[2]
        assert not engine_mod.host_scan_motion_offsets(dr.MOTION, 1, t_ref=0.0, mount=mount).any()


@pytest.mark.parametrize("mount", MOUNTS)
def test_series_branch(engine_mod, mount):
    # theta on both sides of 1e-8: the stamps put tau w at 0, +-0.5e-8, +-0.99e-8, +-1.01e-8, +-2e-8
    w = 1e-3
    th = np.array([0.0, 0.5e-8, -0.5e-8, 0.99e-8, -0.99e-8, 1.01e-8, -1.01e-8, 2e-8, -2e-8])
    t = th / w
    got = check(engine_mod, (0.175, 0.02, w), th.size, t=t, t_ref=0.0, mount=mount)
    if mount is None:
        # on this side of the branch A and Bc are the series' two terms, formed of exact operations: the same bits as numpy's
        want = dr.scan_motion_offsets((0.175, 0.02, w), th.size, t=t, t_ref=0.0)
        small = np.abs(t * w) < 1e-8
        assert small.sum() == 5 and np.array_equal(got[:, small].view(np.uint64), want[:, small].view(np.uint64))


def test_refusals(engine_mod):
    lib = engine_mod.load_library()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    mo, out, t = np.array(dr.MOTION), np.empty((3, B)), np.linspace(0.0, 1.0, B)
    call = lambda m=mo, mount=None, tt=None, tr=1.0, n=B, o=out: lib.mcl_host_scan_motion_offsets(
        None if m is None else ptr(m), None if mount is None else ptr(mount), None if tt is None else ptr(tt), C.c_double(tr), n,
        None if o is None else ptr(o))
    assert call() == 0 and call(tt=t) == 0
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(3):
            m = mo.copy(); m[k] = bad
            assert call(m=m) == -1, (bad, k)
        tb = t.copy(); tb[7] = bad
        assert call(tt=tb) == -1 and call(tr=bad) == -1
        assert call(mount=np.array([0.1, bad, 0.0])) == -1
    assert call(mount=np.array([0.0, 0.0, 7.0])) == -1                                # SM1: |mtheta| <= 2 pi
    assert call(n=0) == -1 and call(n=-3) == -1 and call(m=None) == -1 and call(o=None) == -1
    with pytest.raises(engine_mod.EngineError):
        engine_mod.host_scan_motion_offsets((0.1, np.nan, 0.0), B)
    # the engine-side calls refuse a null engine before anything else
    assert lib.mcl_set_beam_offsets(None, ptr(out), B) == -1 and lib.mcl_get_beam_offsets(None, ptr(out), None, B, None) == -1
    assert lib.mcl_beam_origins(None, ptr(out), 1, ptr(out)) == -1
    # the table formation: non-finite offsets, null pointers, counts
    ang = np.linspace(-2.0, 2.0, B).astype(np.float32)
    eff, dirs, pairs = np.empty(B, np.float32), np.empty((2, B)), np.empty((2, B))
    off = dr.table_of(B)
    assert lib.mcl_host_beam_offset_table(ptr(ang), ptr(off), B, ptr(eff), ptr(dirs)) == 0
    assert lib.mcl_host_beam_offset_table(ptr(ang), ptr(off), B, None, None) == -1
    assert lib.mcl_host_beam_offset_table(ptr(ang), ptr(off), 0, ptr(eff), ptr(dirs)) == -1
    nf = off.copy(); nf[1, 3] = np.nan
    assert lib.mcl_host_beam_offset_table(ptr(ang), ptr(nf), B, ptr(eff), ptr(dirs)) == -1
    r = np.full(B, 2.0, np.float32)
    assert lib.mcl_host_beam_offset_pairs(ptr(r), ptr(off), ptr(dirs), B, C.c_double(0.05), ptr(pairs)) == 0
    assert lib.mcl_host_beam_offset_pairs(ptr(r), ptr(off), ptr(dirs), B, C.c_double(0.0), ptr(pairs)) == -1
    assert lib.mcl_host_beam_offset_pairs(ptr(r), ptr(off), None, B, C.c_double(0.05), ptr(pairs)) == -1


def test_table_formation_is_ds1_and_ds5(engine_mod, orc):
    for n in (1, 61, 1081):
        ang = sg.angles(orc, n)
        off = dr.table_of(n, 1, dr.MOUNT)
        eff, dirs = engine_mod.host_beam_offset_table(ang, off)
        want = dr.effective_angles(ang, off)
        assert eff.dtype == np.float32 and np.array_equal(eff.view(np.uint32), want.view(np.uint32))      # one add, one rounding to float
        # the pair of the widened float: libm's cosine and sine against numpy's, 1 ulp each
        assert np.all(np.abs(dirs - dr.directions(want)) <= 2.0 ** -52)
        # zero offsets: the beams' own angles, bit for bit
        eff0, _ = engine_mod.host_beam_offset_table(ang, np.zeros((3, n)))
        assert np.array_equal(eff0.view(np.uint32), ang.view(np.uint32))
        r = np.random.default_rng(n).uniform(0.0, 12.0, n).astype(np.float32)
        got = engine_mod.host_beam_offset_pairs(r, off, dirs, 0.05)
        assert np.array_equal(got.view(np.uint64), dr.lf_pairs(r, off, dirs, 0.05).view(np.uint64))        # two products and a sum, IEEE
        # zero offsets: the plain model's pair r c / res
        inv = 1.0 / float(np.float32(0.05))
        got0 = engine_mod.host_beam_offset_pairs(r, np.zeros((3, n)), dirs, 0.05)
        assert np.array_equal(got0[0], r.astype(np.float64) * dirs[0] * inv) and np.array_equal(got0[1], r.astype(np.float64) * dirs[1] * inv)


def test_names_are_exported_and_declared(engine_mod):
    names = ["mcl_set_beam_offsets", "mcl_get_beam_offsets", "mcl_beam_origins", "mcl_host_scan_motion_offsets",
             "mcl_host_beam_offset_table", "mcl_host_beam_offset_pairs"]
    text = open(os.path.join(ROOT, "include", "mcl_hip_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = engine_mod.load_library()
    for n in names:
        assert n in engine_mod.EXPORTS and re.search(r"\b%s\s*\(" % n, src) and hasattr(lib, n), n
    assert re.search(r"MCL_RAYS_DESKEW\s*=\s*6", src) and engine_mod.RAYS_DESKEW == 6
    assert re.search(r"#define\s+MCL_ABI_VERSION\s+1\b", text) and lib.mcl_abi_version() == 1
    for rule in ["DS1", "DS2", "DS3", "DS4", "DS5", "DS6", "DM1", "DM2"]:
        assert rule in text, rule


# ---- the preconditions of tests/test_gpu_scan_deskew.py's fixtures, on the CPU statement alone
@pytest.mark.parametrize("mount", [None, dr.MOUNT])
def test_lf_fixture_stays_within_the_cap(orc, mount):
    g = sg.small()
    ang = sg.angles(orc, 61)
    D, Lf = lr.field(g.data, g.resolution), lr.table(g.resolution, max_range_m=g.max_range_m)
    p0, scan, off = dr.lf_fixture(sg, orc, g, ang, mount)
    sp = p0 if mount is None else dr.sm2(mount, p0)
    used = lr.used_beams(ang, scan, g.max_range_m)[0].size
    assert 40 <= used < 61                                                           # (the odd readings are not used; most beams are)
    for obs in (scan, sg.masked(scan, 2)):
        _, _, n_amb = dr.lf_log_weights(sp, dr.effective_angles(ang, off), obs, off, D, Lf, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
        assert sg.within_cap(n_amb, dr.LF_N * lr.used_beams(ang, obs, g.max_range_m)[0].size), int(n_amb.sum())


def test_moving_scan_differs_from_the_plain_one(orc):
    g = sg.small()
    om = g.oracle(orc)
    ang = sg.angles(orc, 61)
    off = dr.table_of(61, 0)
    assert np.abs(off[:2]).max() > 3.0 * g.res and np.degrees(np.abs(off[2]).max()) > 5.0     # several cells, several degrees
    scan, st = dr.moving_scan(orc, om, ang, g.true_pose, off)
    a = g.true_pose[2] + ang.astype(np.float64)
    plain = orc.cast_many(om, np.full(61, g.true_pose[0]), np.full(61, g.true_pose[1]), a)[1]
    hit = st < om.max_range_px
    assert hit.sum() > 30 and (plain[hit] != st[hit]).sum() >= 10, (int(hit.sum()), int((plain[hit] != st[hit]).sum()))
    # the rows of the scan are the de-skewed steps where a beam hits in range: range = step * res read back through E2
    assert np.array_equal(orc.obs_index(scan, om)[hit], st[hit])
