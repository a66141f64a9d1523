"""Recovery by random-particle injection on the GPU (mcl_set_recovery), on the Spielberg map: the injected set of
an update against the stream-8 coins, every injected pose against the free-cell rule bit for bit, every other child against an
engine with recovery off, the log-weights against the spec oracle, the count and the KLD bin count; the averages against
mcl_host_recovery_step after every kind of update; off means off; a kidnapped robot found again; the refusals."""
import math

import numpy as np
import pytest

from conftest import make_engine
from test_kld_host import np_bins
from test_recovery_host import child_draws, free_cells, injected_poses, threshold

pytestmark = pytest.mark.gpu

ACTION = (0.1, 0.0, 0.02)
SEED = 0x5EED_0000_0000_0009 + 12345
P0 = (0.0, 0.0, 0.0)
KIDNAP_B = (-46.19, 29.66, -3.02)          # a pose a global start localises at (tests/test_gpu_kld.py)
NAN = float("nan")


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def force_p(e, p):
    """S = 0, F = log(1 - p): the next update's p is 1 - exp(F - S) (p = 1: F = -inf); returns that p"""
    e.set_recovery_state(0.0, -math.inf if p >= 1.0 else math.log1p(-p))
    return e.recovery_state()[2]


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def world(spielberg, spielberg_oracle, orc):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    return dict(ang=ang, free=free_cells(spielberg.data), om=spielberg_oracle,
                L=orc.eng_log_table(orc.sensor_table(spielberg_oracle.max_range_px)))


# ---- 1. exact injection, every particle
CASES = [
    # n, resampling mode, KLD, forced p, expected path, MCL_NO_COMPACT (dense parent list at a size that would take the compact one)
    (4096, 0, False, 0.3, "tiny", False),
    (4096, 0, False, 1.0, "tiny", False),
    (4096, 1, True, 0.3, "tiny", False),
    (32768, 1, False, 0.3, "graph", False),
    (32768, 0, True, 1.0, "graph", False),
    (65536, 0, False, 0.3, "regular", False),
    (65536, 1, False, 0.3, "regular", True),
    (65536, 0, True, 0.3, "regular", False),
    (65536, 1, False, 1.0, "regular", False),
]


@pytest.mark.parametrize("n,mode,kld,p,path,dense", CASES)
def test_exact_injection(engine_mod, spielberg, orc, world, monkeypatch, n, mode, kld, p, path, dense):
    from monte_carlo_localization_amd import synth
    if dense:
        monkeypatch.setenv("MCL_NO_COMPACT", "1")
    m, ang, om = spielberg, world["ang"], world["om"]
    a = make_engine(engine_mod, m, ang, n, seed=SEED, resample_mode=mode)
    b = make_engine(engine_mod, m, ang, n, seed=SEED, resample_mode=mode)
    scan = synth.scan_from_pose(a, m, ang, P0)
    p0 = synth.tracking_cloud(np.random.default_rng(n + mode), n)
    kcfg = None
    for e in (a, b):
        e.set_particles(p0, np.full(n, 1.0 / n))
        if kld:
            kcfg = e.set_kld(min_particles=n, max_particles=n)
    a.set_recovery()
    # warm-up: the small-update paths need one regular update first; recovery is not triggered (unset, then S == F)
    warm = 1
    for _ in range(warm):
        a.update(ACTION, scan)
        b.update(ACTION, scan)
    assert a.recovery_state()[3] == 0
    parents = a.get_particles()
    assert same_bits(parents, b.get_particles())
    pe = force_p(a, p)
    T = threshold(pe)
    assert T > 0
    a.update(ACTION, scan)
    b.update(ACTION, scan)
    assert path_of(a) == path, (path_of(a), path)
    if n == 65536:
        assert a.compact_list()[1] == (not dense)
    coin, pick, hb = child_draws(SEED, warm, n)
    inj = coin < np.uint64(T)
    if p >= 1.0:
        assert inj.all()
    idx_a, idx_b = a.resample_indices(), b.resample_indices()
    assert np.array_equal(np.flatnonzero(idx_a == -1), np.flatnonzero(inj))
    assert np.array_equal(idx_a[~inj], idx_b[~inj])
    pa, pb = a.get_particles(), b.get_particles()
    want_inj = injected_poses(pick[inj], hb[inj], world["free"], m.data.shape[1], m.resolution, m.origin_x, m.origin_y)
    assert same_bits(pa[:, inj], want_inj), "injected poses differ from the free-cell rule"
    assert same_bits(pa[:, ~inj], pb[:, ~inj]), "a non-injected child differs from the recovery-off engine's"
    logw, _, _ = orc.eng_log_weights(om, pa, ang, orc.obs_index(scan, om), world["L"])
    assert np.array_equal(a.log_weights(), logw)
    assert a.recovery_state()[3] == int(inj.sum())
    if kld:
        drawn = parents[:, np.where(inj, 0, idx_b)].copy()
        drawn[:, inj] = want_inj
        assert a.kld_state()[0] == np_bins(drawn[0], drawn[1], drawn[2], m.data.shape[1], m.data.shape[0], m.resolution,
                                           m.origin_x, m.origin_y, kcfg)
    # the update after the injecting one (ordered by the injected set's layout) is the spec's too
    S, F, p_next, _ = a.recovery_state()
    assert S == F and p_next == 0.0                        # reset by the injecting update, then seeded by its likelihood
    a.update(ACTION, scan)
    assert a.recovery_state()[3] == 0
    pa2 = a.get_particles()
    logw2, _, _ = orc.eng_log_weights(om, pa2, ang, orc.obs_index(scan, om), world["L"])
    assert np.array_equal(a.log_weights(), logw2)
    a.close()
    b.close()


# ---- 2. the averages on the device follow mcl_host_recovery_step
@pytest.mark.parametrize("neff", [0, 1])
def test_state_follows_host_rule(engine_mod, spielberg, world, neff):
    from monte_carlo_localization_amd import synth
    m, ang, n = spielberg, world["ang"], 4096
    e = make_engine(engine_mod, m, ang, n, seed=SEED, resample_neff_permille=neff)
    scan_a = synth.scan_from_pose(e, m, ang, P0)
    scan_b = synth.scan_from_pose(e, m, ang, KIDNAP_B)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(5), n), np.full(n, 1.0 / n))
    cfg = e.set_recovery(alpha_slow=0.05, alpha_fast=0.5)
    steps = ([("move", ACTION, scan_a)] * 3 + [("still", (0.0, 0.0, 0.0), scan_a)] * 3 + [("sensor", None, scan_a)] +
             [("kidnap", (0.0, 0.0, 0.0), scan_b)] * 5 + [("move", ACTION, scan_b)] * 3 + [("sensor", None, scan_b)])
    u = 0
    prev_sw = None
    seen = dict(kept=0, resampled=0, injecting=0, injected=0, sensor=0)
    for kind, act, scan in steps:
        S, F, p, _ = e.recovery_state()
        T = threshold(p)
        if kind == "sensor":
            e.sensor_update(scan)
            kept, resampled = False, False
            seen["sensor"] += 1
        else:
            e.update(act, scan)
            resampled = e.effective_sample_size()[1]
            kept = not resampled
            seen["kept" if kept else "resampled"] += 1
        sc = e.scalars()
        injecting = resampled and T > 0
        denom = prev_sw if kept else float(e.n)
        want = engine_mod.host_recovery_step(cfg, S, F, injecting, sc[0], sc[1], denom, len(ang))
        S2, F2, p2, injected = e.recovery_state()
        for g, w in zip((S2, F2, p2), want):
            assert g == w or (math.isnan(g) and math.isnan(w)), (kind, g, w)
        if injecting:
            seen["injecting"] += 1
            coin = child_draws(SEED, u, e.n)[0]
            assert injected == int((coin < np.uint64(T)).sum())
            seen["injected"] += injected
            assert np.array_equal(np.flatnonzero(e.resample_indices() == -1), np.flatnonzero(coin < np.uint64(T)))
        else:
            assert injected == 0
        if kind != "sensor":
            u += 1
        prev_sw = sc[1]
    assert seen["injecting"] >= 1 and seen["injected"] > 0 and seen["resampled"] >= 1 and seen["sensor"] == 2, seen
    if neff:
        assert seen["kept"] >= 1, seen
    e.close()


# ---- 3. off means off
@pytest.mark.parametrize("n", [4096, 65536])
def test_off_means_off(engine_mod, spielberg, world, n):
    from monte_carlo_localization_amd import synth
    m, ang = spielberg, world["ang"]
    engines = [make_engine(engine_mod, m, ang, n, seed=SEED) for _ in range(3)]
    never, cleared, untriggered = engines
    scan_a = synth.scan_from_pose(never, m, ang, P0)
    scan_b = synth.scan_from_pose(never, m, ang, KIDNAP_B)
    p0 = synth.tracking_cloud(np.random.default_rng(7), n)
    for e in engines:
        e.set_particles(p0, np.full(n, 1.0 / n))
    cleared.set_recovery()
    cleared.set_recovery(False)
    untriggered.set_recovery(alpha_slow=0.05, alpha_fast=0.5)
    for scan in (scan_a, scan_a, scan_b, scan_b, scan_a):
        untriggered.set_recovery_state(0.0, 0.0)            # p = 0: the plain kernel
        for e in engines:
            e.update(ACTION, scan)
        ref = (never.get_particles(), never.resample_indices(), never.log_weights())
        for e in (cleared, untriggered):
            got = (e.get_particles(), e.resample_indices(), e.log_weights())
            for g, r in zip(got, ref):
                assert same_bits(g, r) if g.dtype == np.float64 else np.array_equal(g, r)
            assert e.recovery_state()[3] == 0
    s = cleared.recovery_state()
    assert math.isnan(s[0]) and math.isnan(s[1]) and s[2] == 0.0
    for e in engines:
        e.close()


# ---- 4. a kidnapped robot found again (the parameters are those of profiles/recovery.md)
KIDNAP_N = 1 << 20
KIDNAP_A = (0.0, 0.0, 0.0)
KIDNAP_ALPHAS = (0.001, 0.1)
KIDNAP_K = 20
KIDNAP_CONVERGE = 10


def _err(e, truth):
    pose = e.expected_pose()
    return math.hypot(pose[0] - truth[0], pose[1] - truth[1]), abs((pose[2] - truth[2] + math.pi) % (2 * math.pi) - math.pi)


def test_kidnap_recovery(engine_mod, spielberg, world):
    from monte_carlo_localization_amd import synth
    m, ang, n = spielberg, world["ang"], KIDNAP_N
    results = {}
    for rec in (True, False):
        e = make_engine(engine_mod, m, ang, n, seed=SEED)
        scan_a = synth.scan_from_pose(e, m, ang, KIDNAP_A)
        scan_b = synth.scan_from_pose(e, m, ang, KIDNAP_B)
        e.init_particles_pose(KIDNAP_A, n)
        if rec:
            e.set_recovery(alpha_slow=KIDNAP_ALPHAS[0], alpha_fast=KIDNAP_ALPHAS[1])
        for _ in range(KIDNAP_CONVERGE):
            e.update((0.0, 0.0, 0.0), scan_a)
        d, dth = _err(e, KIDNAP_A)
        assert d < 0.25 and dth < math.radians(5), (rec, d, dth)
        found, injected = None, 0
        for k in range(KIDNAP_K):
            e.update((0.0, 0.0, 0.0), scan_b)
            injected += e.recovery_state()[3]
            d, dth = _err(e, KIDNAP_B)
            if rec and d < 0.25 and dth < math.radians(5):
                found = k + 1
                break
        results[rec] = (found, d, dth, injected)
        e.close()
    assert results[True][0] is not None, results
    assert results[True][3] > 0
    assert results[False][1] > 2.0 and results[False][3] == 0, results


# ---- 5. refusals
def test_refusals(engine_mod, spielberg):
    import ctypes as C
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    # weight_mode PRODUCT
    e = make_engine(engine_mod, spielberg, ang, 1024, seed=3, weight_mode=engine_mod.WEIGHT_PRODUCT)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.set_recovery()
    assert ei.value.status == -5
    e.close()
    # invalid configurations, state without recovery
    e = make_engine(engine_mod, spielberg, ang, 1024, seed=3)
    e.init_particles_pose((0.0, 0.0, 0.0), 1024)
    for bad in (dict(alpha_slow=0.2, alpha_fast=0.1), dict(alpha_fast=1.5), dict(per_beam=2), dict(reserved=1)):
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_recovery(**bad)
        assert ei.value.status == -1
    with pytest.raises(engine_mod.EngineError) as ei:
        e.set_recovery_state(0.0, 0.0)
    assert ei.value.status == -2
    # stage calls and the communicator while it is on
    e.set_recovery()
    with pytest.raises(engine_mod.EngineError) as ei:
        e.set_recovery_state(math.inf, 0.0)
    assert ei.value.status == -1
    obs = synth.scan_from_pose(e, spielberg, ang, (0.0, 0.0, 0.0))
    lib = e.lib
    assert lib.mcl_stage_rays(e._h, obs.ctypes.data_as(C.c_void_p), C.c_int32(obs.size)) == -5
    act = np.array(ACTION)
    assert lib.mcl_stage_keep(e._h, C.c_int64(0), C.c_int64(1024), act.ctypes.data_as(C.c_void_p)) == -5
    assert lib.mcl_stage_weights(e._h, C.c_double(0.0)) == -5
    assert lib.mcl_stage_finish(e._h, np.zeros(5).ctypes.data_as(C.c_void_p)) == -5
    assert "single-engine" in lib.mcl_last_error(e._h).decode()
    uid = (C.c_ubyte * 128)()
    assert lib.mcl_comm_create(e._h, uid, C.c_int32(1), C.c_int32(0)) == -5
    e.set_recovery(False)
    e.update(ACTION, obs)
    e.close()
    # an engine of a device group
    g = engine_mod.Group([0], max_particles=1024)
    with pytest.raises(engine_mod.EngineError) as ei:
        g.engine(0).set_recovery()
    assert ei.value.status == -5
    g.close()
    # a map without free cells: an update that would inject is refused before anything runs; p = 0 updates as before
    grid = np.full((64, 64), 100, np.int8)
    e = engine_mod.Engine(max_particles=256, seed=3)
    e.set_map(grid, 0.05, 0.0, 0.0)
    e.set_beam_angles(ang)
    p0 = np.stack([np.full(256, 1.6), np.full(256, 1.6), np.linspace(-3, 3, 256)])
    e.set_particles(p0, np.full(256, 1.0 / 256))
    e.set_recovery()
    scan = np.full(ang.size, 1.0, np.float32)
    e.update(ACTION, scan)
    before = e.get_particles()
    force_p(e, 1.0)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.update(ACTION, scan)
    assert ei.value.status == -2
    assert same_bits(e.get_particles(), before)
    e.close()
