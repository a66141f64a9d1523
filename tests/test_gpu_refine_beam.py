"""The pose refinement under the beam model on the GPU (mcl_refine_poses_beam, DESIGN.md §4.18, rules RB1-RB6 of
include/mcl_hip_engine.h): the score volume against mcl_score_poses bit for bit and against the oracle's statement
tests/refine_beam_ref.py; the records against mcl_host_refine_reduce; the cooperative literal march; that the likelihood field's
switch changes nothing; that an engine which refines runs the same updates, bit for bit, as one that never does; the refusals.
The fixture is tests/refine_ref.py's, whose conditions under this model tests/test_refine_beam_host.py decides on the CPU."""
import ctypes as C

import numpy as np
import pytest

import refine_beam_ref as rb
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


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def window_scores(engine_mod, e, seeds, obs, **fields):
    """mcl_score_poses (the field off: the beam model) on the window poses of mcl_host_refine_window, in chunks of <= 65536:
    (M, n_win) log-likelihoods and the rays the literal march decided, summed over the chunks"""
    ll, _, level3 = sg.window_scores(engine_mod, e, rr.SmallMap(), seeds, obs, **fields)
    return ll, level3


def check_records(engine_mod, r, seeds, want, **fields):
    """RB4: the records are mcl_host_refine_reduce of the volume"""
    tol_mean, tol_cov, tol_s = rr.tolerances(rr.RES, **fields)
    for m in range(len(seeds)):
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


# ---- 1. the volume is mcl_score_poses, bit for bit; the records are the host restatement's
CASES = [
    (1, 0, 0, 1, 1),                 # one wave, one live lane
    (1, 0, 0, 61, 1),                # three idle lanes
    (3, 1, 0, 64, 1),                # exactly one round
    (3, 1, 0, 65, 1),                # lane 0 adds twice
    (3, 4, 10, 61, 1),               # 5103 poses, no multiple of 4: idle waves in the last workgroup, seeds share workgroups
    (3, 4, 10, 61, 3),               # stride: against a second engine with angles[::3] and obs[::3]
    (1, 1, 1, 1081, 1),              # 17 rounds, the last with 57 lanes
    (1, 1, 1, 1081, 10),             # 109 used beams
]


def run_case(engine_mod, orc, small, small_oracle, M, hxy, hth, B, beam_stride, field_on=False):
    ang = rr.angles(orc, B)
    e = make_engine(engine_mod, small, ang, 64)             # the field off
    obs = rr.odd_scan(rr.scan_at(orc, small_oracle, ang, rr.P_STAR))
    seeds = rr.SEEDS[:M]
    fields = dict(half_xy=hxy, half_theta=hth)
    n_win = (2 * hxy + 1) ** 2 * (2 * hth + 1)
    if beam_stride == 1:
        want, level3 = window_scores(engine_mod, e, seeds, obs, **fields)
    else:
        e2 = make_engine(engine_mod, small, ang[::beam_stride].copy(), 64)
        want, level3 = window_scores(engine_mod, e2, seeds, obs[::beam_stride].copy(), **fields)
    if field_on:
        e.set_likelihood_field(True)
    r, st = e.refine_poses_beam(seeds, obs, beam_stride=beam_stride, **fields)
    nb = rb.used(B, beam_stride).size
    assert st["n_win"] == n_win and st["n_poses"] == M * n_win and st["device_bytes"] == e.refine_bytes() > 0
    assert st["used_beams"] == nb and st["rays"] == M * n_win * nb
    assert st["level3_rays"] == level3                      # (the same rays take the literal march in both routes)
    got = e.refine_scores()
    assert got.shape == want.shape == (M, n_win)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    if B > 1 and n_win > 100:
        assert np.unique(got).size > 100                   # (a volume, not a constant)
    check_records(engine_mod, r, seeds, want, **fields)
    # the same state, the same bytes
    r2, st2 = e.refine_poses_beam(seeds, obs, beam_stride=beam_stride, **fields)
    assert r.tobytes() == r2.tobytes() and st2 == st
    assert np.array_equal(bits(e.refine_scores()), bits(got))
    return e, r, got, seeds, obs, fields


@pytest.mark.parametrize("M,hxy,hth,B,beam_stride", CASES)
def test_volume_is_score_poses_and_records_are_the_restatement(engine_mod, orc, small, small_oracle, M, hxy, hth, B, beam_stride):
    run_case(engine_mod, orc, small, small_oracle, M, hxy, hth, B, beam_stride)


def test_odd_readings_count(engine_mod, orc, small, small_oracle):
    """RB3 masks nothing: the NaN, +-inf, negative and max-range readings of odd_scan have rows, so the volume differs from
    that of the plain scan and is still finite or -inf"""
    ang = rr.angles(orc, 61)
    e = make_engine(engine_mod, small, ang, 64)
    scan = rr.scan_at(orc, small_oracle, ang, rr.P_STAR)
    f = dict(half_xy=1, half_theta=1)
    e.refine_poses_beam(rr.SEEDS[:1], scan, **f)
    a = e.refine_scores()
    e.refine_poses_beam(rr.SEEDS[:1], rr.odd_scan(scan), **f)
    b = e.refine_scores()
    assert not np.isnan(a).any() and not np.isnan(b).any() and not np.array_equal(bits(a), bits(b))


# ---- 2. the volume against the independent statement (oracle rays); it finds the pose
def test_volume_is_the_restatement_and_the_pose_is_found(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    obs = rr.perturbed_scan(orc, small_oracle, ang, rr.P_STAR)
    F = rr.FIXTURE_WINDOW
    win = rr.window(rr.LATTICE_POSE, rr.RES, **F)
    want = rb.scores(orc, small_oracle, win, ang, obs)
    e = make_engine(engine_mod, small, ang, 64)
    r, st = e.refine_poses_beam(rr.LATTICE_POSE, obs, **F)
    got = e.refine_scores()
    assert got.shape == (1, want.size) and np.array_equal(bits(got[0]), bits(want))
    off = rr.offsets(**F)
    wb = int(np.flatnonzero((off == (0, 0, 3)).all(axis=1))[0])
    assert int(r[0]["best_index"]) == wb == rr.best(want, **F)
    assert np.array_equal(bits(r[0]["best"]), bits(win[wb])) and r[0]["best_log_likelihood"] > r[0]["seed_log_likelihood"]
    # strided, against the statement too
    e.refine_poses_beam(rr.LATTICE_POSE, obs, beam_stride=4, **F)
    assert np.array_equal(bits(e.refine_scores()[0]), bits(rb.scores(orc, small_oracle, win, ang, obs, beam_stride=4)))


# ---- 3. the level-3 path: the cooperative march inside the beam loop
def test_forced_literal_march_gives_the_same_volume(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    obs = rr.odd_scan(rr.scan_at(orc, small_oracle, ang, rr.P_STAR))
    f = dict(half_xy=1, half_theta=1)
    e = make_engine(engine_mod, small, ang, 64)
    x = make_engine(engine_mod, small, ang, 64, debug_force_exact=1)
    r, st = e.refine_poses_beam(rr.SEEDS, obs, **f)
    rx, stx = x.refine_poses_beam(rr.SEEDS, obs, **f)
    assert stx["rays"] == 3 * 27 * 61 and stx["level3_rays"] == stx["rays"]
    assert np.array_equal(bits(x.refine_scores()), bits(e.refine_scores())) and r.tobytes() == rx.tobytes()
    # 13 used beams: fewer flagged lanes than kLaneMarchMin, so the wave marches them one after the other (above: each lane its own)
    e.refine_poses_beam(rr.SEEDS, obs, beam_stride=5, **f)
    _, st5 = x.refine_poses_beam(rr.SEEDS, obs, beam_stride=5, **f)
    assert st5["used_beams"] == 13 and st5["level3_rays"] == st5["rays"] == 3 * 27 * 13
    assert np.array_equal(bits(x.refine_scores()), bits(e.refine_scores()))
    e5 = make_engine(engine_mod, small, ang[::5].copy(), 64)
    want5, _ = window_scores(engine_mod, e5, rr.SEEDS, obs[::5].copy(), **f)
    assert np.array_equal(bits(x.refine_scores()), bits(want5))
    r, st = e.refine_poses_beam(rr.SEEDS, obs, **f)
    # without the flag: the rays the pose query marches literally for the same poses
    want, level3 = window_scores(engine_mod, e, rr.SEEDS, obs, **f)
    assert st["level3_rays"] == level3 < st["rays"]
    assert np.array_equal(bits(e.refine_scores()), bits(want))


def test_edge_poses_take_the_literal_march(engine_mod, orc, small, small_oracle):
    """LATTICE_POSE is a cell centre and the default window steps by half a cell: every pose with an odd x or y offset stands on
    a cell edge, where the guard sends all its rays to the literal march (25 of the 81 positions keep clear of both)"""
    ang = rr.angles(orc, 61)
    obs = rr.perturbed_scan(orc, small_oracle, ang, rr.P_STAR)
    e = make_engine(engine_mod, small, ang, 64)
    _, st = e.refine_poses_beam(rr.LATTICE_POSE, obs)
    assert st["n_win"] == 1701 and st["rays"] == 1701 * 61
    print("level-3 share of the default window:", st["level3_rays"] / st["rays"])
    assert st["level3_rays"] >= (81 - 25) * 21 * 61       # at least the edge poses' rays (25 positions have both offsets even)
    assert st["level3_rays"] < st["rays"]
    want, level3 = window_scores(engine_mod, e, [rr.LATTICE_POSE], obs)
    assert st["level3_rays"] == level3 and np.array_equal(bits(e.refine_scores()), bits(want))


def test_more_than_2_to_the_26_poses(engine_mod, orc, small, small_oracle):
    """M n_win = 4096 x 16767 = 68.7 M poses, within R7's 2^27: a wave per pose is 2^32.03 threads, so the pose index must not come
    from a 32-bit global thread index (it would wrap at 2^26 poses and leave the scores of seeds from 4003 on unwritten) and the
    kernel runs in 17 launches of at most 2^22 poses.  One beam keeps it to 68.7 M rays."""
    ang = rr.angles(orc, 1)
    e = make_engine(engine_mod, small, ang, 64)
    obs = np.array([1.3], np.float32)
    f = dict(half_xy=13, half_theta=11)
    M, n_win = 4096, 27 * 27 * 23
    assert M * n_win > 2 ** 26 and M * n_win < 2 ** 27
    seeds = rr.SEEDS[np.arange(M) % 3] + np.arange(M)[:, None] * np.array([1e-4, -1e-4, 1e-3])
    r, st = e.refine_poses_beam(seeds, obs, **f)
    assert st["n_win"] == n_win and st["n_poses"] == st["rays"] == M * n_win
    V = e.refine_scores()
    assert V.shape == (M, n_win) and not np.isnan(V).any()
    assert np.array_equal(bits(r["best_log_likelihood"]), bits(V.max(axis=1)))
    for k in (0, 250, 251, 4002, 4003, 4095):               # the first, both sides of the first launch's end and of 2^26, the last
        want, l3 = window_scores(engine_mod, e, seeds[k:k + 1], obs, **f)
        assert np.array_equal(bits(V[k]), bits(want[0])), k
        check_records(engine_mod, r[k:k + 1], seeds[k:k + 1], want, **f)
    assert 0 < st["level3_rays"] < st["rays"]


# ---- 4. the field on or off: the same bits; one volume for both refinements
def test_field_on_or_off_same_bits(engine_mod, orc, small, small_oracle):
    M, hxy, hth, B, stride = CASES[4]
    e, r, got, seeds, obs, fields = run_case(engine_mod, orc, small, small_oracle, M, hxy, hth, B, stride)
    f, rf, gotf, _, _, _ = run_case(engine_mod, orc, small, small_oracle, M, hxy, hth, B, stride, field_on=True)
    assert np.array_equal(bits(got), bits(gotf)) and r.tobytes() == rf.tobytes()
    # the field refinement still works on that engine, and the volume is the last call's, of either kind
    small_f = dict(half_xy=1, half_theta=0)
    rl, _ = f.refine_poses(seeds, obs, **small_f)
    assert f.refine_scores().shape == (3, 9)
    lf_volume = f.refine_scores().copy()
    rb_, _ = f.refine_poses_beam(seeds, obs, **fields)
    assert f.refine_scores().shape == (3, 1701) and np.array_equal(bits(f.refine_scores()), bits(got)) and rb_.tobytes() == r.tobytes()
    rl2, _ = f.refine_poses(seeds, obs, **small_f)
    assert np.array_equal(bits(f.refine_scores()), bits(lf_volume)) and rl.tobytes() == rl2.tobytes()
    assert not np.array_equal(bits(rl["best_log_likelihood"]), bits(rb_["best_log_likelihood"]))    # (two models)


# ---- 5. read-only
def test_refine_beam_leaves_the_updates_alone(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    n = 2000
    pose = rr.P_STAR
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=pose, sig=(0.2, 0.2, 0.2))
    scans = [rr.scan_at(orc, small_oracle, ang, (pose[0] + 0.02 * t, pose[1], pose[2])) for t in range(1, 4)]
    a, b = make_engine(engine_mod, small, ang, n), make_engine(engine_mod, small, ang, n)
    assert a.refine_bytes() == 0 and b.refine_bytes() == 0
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    for t, scan in enumerate(scans):
        r, st = b.refine_poses_beam(rr.SEEDS[:1 + t], scan, half_xy=1 + t, half_theta=2 * t)      # (t = 0: the allocating call)
        assert st["device_bytes"] == b.refine_bytes() > 0
        for e in (a, b):
            e.update((0.02, 0.0, 0.0), scan)
        assert np.array_equal(bits(a.get_particles()), bits(b.get_particles())), t
        assert np.array_equal(bits(a.get_weights()), bits(b.get_weights())), t
        assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose())), t
    assert a.refine_bytes() == 0                            # an engine that never calls it asks for nothing
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))


# ---- 6. the refusals
def expect(engine_mod, status, fn, *args, **kw):
    with pytest.raises(engine_mod.EngineError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    return str(ei.value)


def test_refusals(engine_mod, orc, small):
    INVALID, NOT_READY, UNSUPPORTED = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY, -5     # (MCL_ERR_UNSUPPORTED)
    ang = rr.angles(orc, 61)
    obs = np.full(61, 1.0, np.float32)
    seeds = rr.SEEDS
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.refine_poses_beam, seeds, obs)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    assert "beam" in expect(engine_mod, NOT_READY, e.refine_poses_beam, seeds, obs)
    e.set_beam_angles(ang)
    expect(engine_mod, NOT_READY, e.refine_scores)                      # before any call
    for fields in (dict(half_xy=-1), dict(half_theta=-1), dict(step_xy_cells=0.0), dict(step_xy_cells=np.inf), dict(step_theta_rad=0.0),
                   dict(step_theta_rad=np.nan), dict(beam_stride=0), dict(reserved=(0, 0, 1)), dict(reserved=(1, 0, 0)),
                   dict(half_xy=90, half_theta=1), dict(half_xy=0, half_theta=16384)):          # the last two: n_win > 32768
        expect(engine_mod, INVALID, e.refine_poses_beam, seeds, obs, **fields)
    expect(engine_mod, INVALID, e.refine_poses_beam, seeds, obs[:60])   # n_beams != B
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            bad = seeds.copy()
            bad[1, k] = v
            expect(engine_mod, INVALID, e.refine_poses_beam, bad, obs)
    expect(engine_mod, INVALID, e.refine_poses_beam, np.zeros((0, 3)), obs)  # M = 0
    expect(engine_mod, INVALID, e.refine_poses_beam, np.zeros((4097, 3)), obs, half_xy=0, half_theta=0)
    assert e.refine_bytes() == 0                                        # ... all refused before anything was asked for
    cfg = engine_mod.default_refine_config()
    s = np.ascontiguousarray(seeds.T)
    out, st = np.zeros(3, engine_mod.REFINE_DTYPE), np.zeros(6, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    f = e.lib.mcl_refine_poses_beam
    assert f(e._h, C.byref(cfg), None, 3, vp(obs), 61, vp(out), vp(st)) == INVALID       # null seeds
    assert f(e._h, C.byref(cfg), vp(s), 3, None, 61, vp(out), vp(st)) == INVALID         # null obs
    assert f(e._h, C.byref(cfg), vp(s), 3, vp(obs), 61, None, vp(st)) == INVALID         # null out
    assert f(e._h, None, vp(s), 3, vp(obs), 61, vp(out), None) == engine_mod.MCL_OK      # null config and stats
    r, st2 = e.refine_poses_beam(seeds, obs)
    assert r.tobytes() == out.tobytes() and st2["n_win"] == 1701
    # the largest call the bounds allow by M: 4096 seeds, one pose each
    r, st3 = e.refine_poses_beam(np.tile(seeds[0], (4096, 1)), obs, half_xy=0, half_theta=0)
    assert st3["n_poses"] == 4096 and np.all(r["best_index"] == 0) and np.unique(r["best_log_likelihood"]).size == 1
    # a call, then a new map: the volume is gone until the next call
    e.refine_poses_beam(seeds, obs, half_xy=1, half_theta=1)
    assert e.refine_scores().shape == (3, 27)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    expect(engine_mod, NOT_READY, e.refine_scores)
    e.refine_poses_beam(seeds, obs, half_xy=1, half_theta=1)
    assert e.refine_scores().shape == (3, 27)
    e.close()
    # PRODUCT mode
    p = engine_mod.Engine(max_particles=64, weight_mode=engine_mod.WEIGHT_PRODUCT, keep_ray_steps=1)
    p.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    p.set_beam_angles(ang)
    assert "LOG" in expect(engine_mod, INVALID, p.refine_poses_beam, seeds, obs)
    p.close()
    # an engine of a device group
    g = engine_mod.Group([0], max_particles=1024)
    g.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    g.set_beam_angles(ang)
    expect(engine_mod, UNSUPPORTED, g.engine(0).refine_poses_beam, seeds, obs)
    g.close()
