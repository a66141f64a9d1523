"""The pose refinement on the GPU (mcl_refine_poses, DESIGN.md §4.14, rules R1-R7 of include/mcl_hip_engine.h): the score volume
against mcl_score_poses bit for bit and against the numpy statement tests/lfield_ref.py; the records against the host restatement
mcl_host_refine_reduce; that it finds a known pose; that its result seeds a cloud; that an engine which refines runs the same
updates, bit for bit, as one that never does; the refusals.  The fixture is tests/refine_ref.py's, whose two conditions
tests/test_refine_host.py decides on the CPU."""
import ctypes as C

import numpy as np
import pytest

import lfield_ref as lr
import refine_ref as rr
import side_geometries as sg
from conftest import make_engine, tracking_cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    return rr.SmallMap()


@pytest.fixture(scope="module")
def small_oracle(orc, small):
    return orc.OracleMap(small.data, small.resolution, small.origin_x, small.origin_y)


def lf_engine(engine_mod, m, ang, n=64, **lf_fields):
    e = make_engine(engine_mod, m, ang, n)
    e.set_likelihood_field(True, **lf_fields)
    return e


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def window_scores(engine_mod, e, seeds, obs, beam_stride=1, **fields):
    """mcl_score_poses on the window poses of mcl_host_refine_window: (M, n_win), the readings of the unused beams NaN (R2)"""
    ll, scored, _ = sg.window_scores(engine_mod, e, rr.SmallMap(), seeds, obs, beam_stride, **fields)
    return ll, scored


# ---- 1. the volume is mcl_score_poses, bit for bit; 3. the records are the host restatement's
@pytest.mark.parametrize("M,hxy,hth,B,beam_stride,lf_fields", [
    (1, 0, 0, 61, 1, {}),
    (3, 1, 0, 61, 1, {}),
    (3, 0, 3, 1, 1, {}),
    (1, 4, 10, 1, 1, {}),
    (3, 4, 10, 61, 1, {}),                            # n_win = 1701: no multiple of 64, seeds share waves
    (3, 4, 10, 61, 3, {}),
    (1, 4, 10, 61, 1, dict(max_occ_dist_m=4.6)),      # K = 8464 >= 8192: the table is read from global memory
    (3, 1, 0, 61, 1, dict(max_occ_dist_m=4.6)),
])
def test_volume_is_score_poses_and_records_are_the_restatement(engine_mod, orc, small, small_oracle, M, hxy, hth, B, beam_stride,
                                                               lf_fields):
    ang = rr.angles(orc, B)
    e = lf_engine(engine_mod, small, ang, **lf_fields)
    if lf_fields:
        assert e.likelihood_table().size - 1 >= 8192
    obs = rr.odd_scan(rr.scan_at(orc, small_oracle, ang, rr.P_STAR))
    seeds = rr.SEEDS[:M] if M > 1 else rr.SEEDS[(hxy + hth) % 3:][:1]         # (the single seeds: each of the three in turn)
    fields = dict(half_xy=hxy, half_theta=hth)
    r, st = e.refine_poses(seeds, obs, beam_stride=beam_stride, **fields)
    want, masked = window_scores(engine_mod, e, seeds, obs, beam_stride, **fields)
    n_win = (2 * hxy + 1) ** 2 * (2 * hth + 1)
    assert st["n_win"] == n_win and st["n_poses"] == M * n_win and st["device_bytes"] == e.refine_bytes() > 0
    assert st["used_beams"] == lr.used_beams(ang, masked, rr.MAX_RANGE)[0].size
    got = e.refine_scores()
    assert got.shape == want.shape == (M, n_win)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    if B > 1 and n_win > 100:
        assert np.unique(got).size > 100                   # (a volume, not a constant)
    # the records
    tol_mean, tol_cov, tol_s = rr.tolerances(rr.RES, **fields)
    for m in range(M):
        h = engine_mod.host_refine_reduce(seeds[m], rr.RES, want[m], **fields)
        for name in ("best", "best_log_likelihood", "seed_log_likelihood"):
            assert np.array_equal(bits(r[m][name]), bits(h[name])), (m, name)
        assert int(r[m]["best_index"]) == int(h["best_index"]) == rr.best(want[m], **fields)
        err = (np.abs(r[m]["mean"] - h["mean"]) / tol_mean).max(), (np.abs(r[m]["cov"] - h["cov"]) / tol_cov).max(), \
            abs(float(r[m]["weight_sum"]) - float(h["weight_sum"])) / tol_s
        print("seed", m, "mean / cov / weight_sum error in tolerances:", err)
        assert max(err) <= 1.0
        assert np.array_equal(r[m]["cov"], r[m]["cov"].T)
        engine_mod.host_gaussian_factor(r[m]["cov"])
    # the same state, the same bytes
    r2, _ = e.refine_poses(seeds, obs, beam_stride=beam_stride, **fields)
    assert r.tobytes() == r2.tobytes()
    assert np.array_equal(bits(e.refine_scores()), bits(got))


def test_void_seeds(engine_mod, orc, small, small_oracle):
    """z_rand = 0 and a sigma_hit of a millimetre: Lf is finite for D = 0 alone, so a window none of whose poses has every end
    point inside an occupied cell is all -inf"""
    ang = rr.angles(orc, 61)
    e = lf_engine(engine_mod, small, ang, z_rand=0.0, sigma_hit_m=0.001, max_occ_dist_m=0.1)
    assert np.isinf(e.likelihood_table()[-1])
    obs = rr.perturbed_scan(orc, small_oracle, ang, rr.P_STAR)
    f = dict(half_xy=1, half_theta=1)
    r, _ = e.refine_poses(rr.SEEDS, obs, **f)
    V = e.refine_scores()
    assert not np.isnan(V).any() and np.all(np.isneginf(V[1]))
    want, _ = window_scores(engine_mod, e, rr.SEEDS, obs, **f)
    assert np.array_equal(bits(V), bits(want))
    st = np.array(rr.steps(rr.RES, **f))
    for m in range(3):
        if np.all(np.isneginf(V[m])):
            assert r[m]["weight_sum"] == 0.0 and r[m]["best_log_likelihood"] == -np.inf and r[m]["best_index"] == 13
            assert np.array_equal(r[m]["best"], rr.SEEDS[m]) and np.array_equal(r[m]["mean"], rr.SEEDS[m])
            assert np.array_equal(r[m]["cov"], np.diag(st * st / 12.0))
        h = engine_mod.host_refine_reduce(rr.SEEDS[m], rr.RES, want[m], **f)
        assert int(r[m]["best_index"]) == int(h["best_index"])


# ---- 2. the volume against the independent statement; 4. it finds the pose
def test_volume_is_the_restatement_and_the_pose_is_found(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    obs = rr.perturbed_scan(orc, small_oracle, ang, rr.P_STAR)
    F = rr.FIXTURE_WINDOW
    win = rr.window(rr.LATTICE_POSE, rr.RES, **F)
    D, Lf = lr.field(small.data, small.resolution), lr.table(small.resolution)
    want, alts, n_amb = lr.log_weights(np.ascontiguousarray(win.T), ang, obs, D, Lf, small.resolution, rr.OX, rr.OY, rr.MAX_RANGE)
    assert int(n_amb.sum()) == 0 and not alts               # condition (a), as tests/test_refine_host.py decides it
    e = lf_engine(engine_mod, small, ang)
    r, st = e.refine_poses(rr.LATTICE_POSE, obs, **F)
    got = e.refine_scores()
    assert got.shape == (1, want.size) and np.array_equal(bits(got[0]), bits(want))
    wb = rr.best(want, **F)
    assert int(r[0]["best_index"]) == wb
    err = np.abs(rr.offsets(**F)[wb] - np.array(rr.P_STAR_STEPS))
    assert err[0] <= 2.0 and err[1] <= 2.0 and err[2] <= 1.0  # condition (b)
    assert np.array_equal(bits(r[0]["best"]), bits(win[wb])) and r[0]["best_log_likelihood"] >= r[0]["seed_log_likelihood"]


# ---- 5. it feeds the initialisers
def test_result_seeds_a_cloud(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    e = lf_engine(engine_mod, small, ang, n=512)
    obs = rr.perturbed_scan(orc, small_oracle, ang, rr.P_STAR)
    r, _ = e.refine_poses(rr.SEEDS, obs)
    counts = engine_mod.seed_counts(r["best_log_likelihood"], 512)
    assert counts.sum() == 512 and counts[0] == counts.max()
    e.init_particles_mixture(r["mean"], r["cov"], counts)
    assert e.particle_count() == 512
    p = e.get_particles()
    assert np.isfinite(p).all()
    e.init_particles_gaussian(r[0]["mean"], r[0]["cov"], 512)
    assert e.particle_count() == 512


# ---- 6. read-only
@pytest.mark.parametrize("field_only_round_the_call", [False, True])
def test_refine_leaves_the_updates_alone(engine_mod, orc, small, small_oracle, field_only_round_the_call):
    ang = rr.angles(orc, 61)
    n = 2000
    pose = rr.P_STAR
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=pose, sig=(0.2, 0.2, 0.2))
    scans = [rr.scan_at(orc, small_oracle, ang, (pose[0] + 0.02 * t, pose[1], pose[2])) for t in range(1, 4)]
    a, b = make_engine(engine_mod, small, ang, n), make_engine(engine_mod, small, ang, n)
    if not field_only_round_the_call:
        a.set_likelihood_field(True)
        b.set_likelihood_field(True)
    assert a.refine_bytes() == 0 and b.refine_bytes() == 0
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    for t, scan in enumerate(scans):
        if field_only_round_the_call:                       # (either switch makes the next update plan afresh: a switches too)
            a.set_likelihood_field(True)
            a.set_likelihood_field(False)
            b.set_likelihood_field(True)
        r, st = b.refine_poses(rr.SEEDS[:1 + t], scan, half_xy=1 + t, half_theta=2 * t)
        assert st["device_bytes"] == b.refine_bytes() > 0
        if field_only_round_the_call:
            b.set_likelihood_field(False)
        for e in (a, b):
            e.update((0.02, 0.0, 0.0), scan)
        assert np.array_equal(bits(a.get_particles()), bits(b.get_particles())), t
        assert np.array_equal(bits(a.get_weights()), bits(b.get_weights())), t
    assert a.refine_bytes() == 0
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))


# ---- 7. the refusals
def expect(engine_mod, status, fn, *args, **kw):
    with pytest.raises(engine_mod.EngineError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    return str(ei.value)


def test_refusals(engine_mod, orc, small):
    INVALID, NOT_READY = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY
    ang = rr.angles(orc, 61)
    obs = np.full(61, 1.0, np.float32)
    seeds = rr.SEEDS
    # not ready: no map, no beams, the field off -- the message says which
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.refine_poses, seeds, obs)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    assert "beam" in expect(engine_mod, NOT_READY, e.refine_poses, seeds, obs)
    e.set_beam_angles(ang)
    assert "likelihood-field" in expect(engine_mod, NOT_READY, e.refine_poses, seeds, obs)
    expect(engine_mod, NOT_READY, e.refine_scores)                      # before any call
    assert e.refine_bytes() == 0
    e.set_likelihood_field(True)
    # refused arguments
    for fields in (dict(half_xy=-1), dict(half_theta=-1), dict(step_xy_cells=0.0), dict(step_xy_cells=np.inf), dict(step_theta_rad=0.0),
                   dict(step_theta_rad=np.nan), dict(beam_stride=0), dict(reserved=(0, 0, 1)), dict(reserved=(1, 0, 0)),
                   dict(half_xy=90, half_theta=1), dict(half_xy=0, half_theta=16384)):          # the last two: n_win > 32768
        expect(engine_mod, INVALID, e.refine_poses, seeds, obs, **fields)
    expect(engine_mod, INVALID, e.refine_poses, seeds, obs[:60])        # n_beams != B
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            bad = seeds.copy()
            bad[1, k] = v
            expect(engine_mod, INVALID, e.refine_poses, bad, obs)
    expect(engine_mod, INVALID, e.refine_poses, np.zeros((0, 3)), obs)  # M = 0
    expect(engine_mod, INVALID, e.refine_poses, np.zeros((4097, 3)), obs, half_xy=0, half_theta=0)
    # (M * n_win >= 2^27 cannot be reached through the other bounds: n_win is odd, so at most 4096 * 32767; the engine checks it all the same)
    assert e.refine_bytes() == 0                                        # ... all refused before anything was asked for
    cfg = engine_mod.default_refine_config()
    s = np.ascontiguousarray(seeds.T)
    out, st = np.zeros(3, engine_mod.REFINE_DTYPE), np.zeros(4, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert e.lib.mcl_refine_poses(e._h, C.byref(cfg), None, 3, vp(obs), 61, vp(out), vp(st)) == INVALID       # null seeds
    assert e.lib.mcl_refine_poses(e._h, C.byref(cfg), vp(s), 3, None, 61, vp(out), vp(st)) == INVALID         # null obs
    assert e.lib.mcl_refine_poses(e._h, C.byref(cfg), vp(s), 3, vp(obs), 61, None, vp(st)) == INVALID         # null out
    assert e.lib.mcl_refine_poses(e._h, None, vp(s), 3, vp(obs), 61, vp(out), None) == engine_mod.MCL_OK      # null config and stats
    r, st2 = e.refine_poses(seeds, obs)
    assert r.tobytes() == out.tobytes() and st2["n_win"] == 1701
    # the largest call the bounds allow by M: 4096 seeds, one pose each
    r, st3 = e.refine_poses(np.tile(seeds[0], (4096, 1)), obs, half_xy=0, half_theta=0)
    assert st3["n_poses"] == 4096 and np.all(r["best_index"] == 0) and np.unique(r["best_log_likelihood"]).size == 1
    # a call, then a new map: the volume is gone until the next call
    e.refine_poses(seeds, obs, half_xy=1, half_theta=1)
    assert e.refine_scores().shape == (3, 27)
    expect(engine_mod, INVALID, lambda: e._chk(e.lib.mcl_get_refine_scores(e._h, vp(np.zeros(80)), 80), "mcl_get_refine_scores"))
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    expect(engine_mod, NOT_READY, e.refine_scores)
    e.refine_poses(seeds, obs, half_xy=1, half_theta=1)
    assert e.refine_scores().shape == (3, 27)
    # the field off again: refused again
    e.set_likelihood_field(False)
    expect(engine_mod, NOT_READY, e.refine_poses, seeds, obs)
