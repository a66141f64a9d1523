"""Recovery from a pose mixture on the GPU (mcl_set_recovery_proposal; the header's P1-P7), on the Spielberg map
with the golden scan: the injected set of an update against the stream-8 coins and against a twin that injects from free space,
every injected pose against tests/recovery_mix_ref.py, every other child against a twin with recovery off, every log-weight against
the spec oracle, the count and the KLD bin count, on each update path; one shot and what leaves the proposal in place; off is off;
a map without free cells; the sample covariance; the refusals and the getter; a kidnapped robot found again with KLD on."""
import math
import os

import numpy as np
import pytest

import motion_ref as mr
import recovery_mix_ref as ref
from conftest import GOLDEN, make_engine
from test_kld_host import np_bins
from test_recovery_host import child_draws, free_cells, injected_poses, threshold

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0019 + 4321
TOL = 1e-13                                  # tests/test_gpu_motion_model.py's for G1: device log / sincos are not numpy's bit for bit
STEP = 8                                     # 136 of the 1081 beams: 65536 x 136 >= 2^23 rays is still the regular path
ACTIONS = {None: (0.1, 0.0, 0.02), "diff": (0.1, 0.0, 0.02)}
P0 = (0.0, 0.0, 0.0)
KIDNAP_B = (-46.19, 29.66, -3.02)
PATH_OF_N = {4096: "tiny", 32768: "graph", 65536: "regular"}

# M = 4: a full covariance at the origin, a zero-weight component (never drawn: any child near it is a wrong component), one with no
# heading uncertainty, a diagonal one; the means are 17 m to 55 m apart
MIX_MEANS = np.array([[0.0, 0.0, 0.3], [10.03, 19.98, 0.0], [-46.19, 29.66, -3.02], [-29.91, 35.39, 1.0]])
MIX_COVS = np.array([[[0.09, 0.02, 0.01], [0.02, 0.04, -0.005], [0.01, -0.005, 0.05]],
                     np.diag([0.25, 0.25, 0.1]),
                     np.diag([0.0625, 0.04, 0.0]),
                     np.diag([0.01, 0.09, 0.16])])
MIX_W = np.array([2.0, 0.0, 1.0, 1.0])


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def force_p(e, p):
    e.set_recovery_state(0.0, -math.inf if p >= 1.0 else math.log1p(-p))
    return e.recovery_state()[2]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def assert_poses(got, want, msg=""):
    """1e-13 / 1e-13 on every particle, headings modulo 2 pi"""
    np.testing.assert_allclose(got[:2], want[:2], rtol=TOL, atol=TOL, err_msg=msg)
    d = (got[2] - want[2] + math.pi) % (2 * math.pi) - math.pi
    bad = np.abs(d) > TOL + TOL * np.abs(want[2])
    assert not bad.any(), (msg, int(bad.sum()), float(np.abs(d).max()))


class World:
    def __init__(self, orc, om, m):
        from monte_carlo_localization_amd import synth
        self.orc, self.om, self.m = orc, om, m
        self.ang = synth.beam_angles(angle_step=STEP)
        self.scan = np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::STEP].astype(np.float32)
        self.L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
        self.oi = orc.obs_index(self.scan, om)
        self.free = free_cells(m.data)

    def logw(self, parts):
        return self.orc.eng_log_weights(self.om, np.ascontiguousarray(parts), self.ang, self.oi, self.L)[0]

    def free_poses(self, pick, hb):
        m = self.m
        return injected_poses(pick, hb, self.free, m.data.shape[1], m.resolution, m.origin_x, m.origin_y)


@pytest.fixture(scope="module")
def world(orc, spielberg, spielberg_oracle):
    return World(orc, spielberg_oracle, spielberg)


@pytest.fixture(scope="module")
def mix(engine_mod):
    thr, fac = engine_mod.host_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)
    return [int(t) for t in thr], fac


# ---- 1. exact mixture injection, every particle, on every path
@pytest.mark.parametrize("p", [0.3, 1.0])
@pytest.mark.parametrize("odo", [None, "diff"])
@pytest.mark.parametrize("kld", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [4096, 32768, 65536])
def test_exact_mixture_injection(engine_mod, world, mix, n, mode, kld, odo, p):
    from monte_carlo_localization_amd import synth
    w, m = world, world.m
    thr, fac = mix
    a, b, c = (make_engine(engine_mod, m, w.ang, n, seed=SEED, resample_mode=mode) for _ in range(3))    # mixture | recovery off | uniform
    p0 = synth.tracking_cloud(np.random.default_rng(n + mode), n)
    kcfg = None
    for e in (a, b, c):
        e.set_particles(p0, np.full(n, 1.0 / n))
        if kld:
            kcfg = e.set_kld(min_particles=n, max_particles=n)
        if odo:
            e.set_motion_model(odo)
    a.set_recovery()
    c.set_recovery()
    action = ACTIONS[odo]
    for e in (a, b, c):                      # warm-up: the small-update paths need one regular update first
        e.update(action, w.scan)
    parents = a.get_particles()
    assert same_bits(parents, b.get_particles())
    a.set_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)
    pe = force_p(a, p)
    assert force_p(c, p) == pe
    T = threshold(pe)
    assert T > 0
    for e in (a, b, c):
        e.update(action, w.scan)
    assert path_of(a) == PATH_OF_N[n], (path_of(a), n)
    assert a.recovery_proposal() is None     # consumed
    coin, pick, _ = child_draws(SEED, 1, n)
    inj = coin < np.uint64(T)
    if p >= 1.0:
        assert inj.all()
    idx_a, idx_b, idx_c = a.resample_indices(), b.resample_indices(), c.resample_indices()
    assert np.array_equal(np.flatnonzero(idx_a == -1), np.flatnonzero(inj))
    assert np.array_equal(np.flatnonzero(idx_c == -1), np.flatnonzero(inj)), "the uniform source injects another set"
    assert np.array_equal(idx_a[~inj], idx_b[~inj])
    pa, pb = a.get_particles(), b.get_particles()
    g = np.flatnonzero(inj).astype(np.uint64)
    want_inj, comp = ref.injected_poses(SEED, 1, g, pick[inj], thr, fac)
    assert not (comp == 1).any() and set(np.unique(comp)) == {0, 2, 3}
    assert_poses(pa[:, inj], want_inj, "injected poses differ from the mixture rule")
    assert same_bits(pa[2, inj][comp == 2], np.full(int((comp == 2).sum()), MIX_MEANS[2, 2])), "a heading without uncertainty moved"
    assert same_bits(pa[:, ~inj], pb[:, ~inj]), "a non-injected child differs from the recovery-off engine's"
    assert np.array_equal(a.log_weights(), w.logw(pa))
    assert a.recovery_state()[3] == int(inj.sum()) == c.recovery_state()[3]
    if kld:
        drawn = parents[:, np.where(inj, 0, idx_b)].copy()
        drawn[:, inj] = pa[:, inj]           # the engine's own injected poses: bin edges cannot differ
        assert a.kld_state()[0] == np_bins(drawn[0], drawn[1], drawn[2], m.data.shape[1], m.data.shape[0], m.resolution,
                                           m.origin_x, m.origin_y, kcfg)
    # the update after the injecting one is the spec's too
    S, F, p_next, _ = a.recovery_state()
    assert S == F and p_next == 0.0
    a.update(action, w.scan)
    assert a.recovery_state()[3] == 0 and not (a.resample_indices() == -1).any()
    assert np.array_equal(a.log_weights(), w.logw(a.get_particles()))
    for e in (a, b, c):
        e.close()


# ---- 2. one shot, and what leaves the proposal in place (P5)
def test_one_shot_and_persistence(engine_mod, world, mix):
    from monte_carlo_localization_amd import synth
    w, m, n = world, world.m, 4096
    thr, fac = mix
    e = make_engine(engine_mod, m, w.ang, n, seed=SEED)
    p0 = synth.tracking_cloud(np.random.default_rng(2), n)
    e.set_particles(p0, np.full(n, 1.0 / n))
    e.set_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)          # set while recovery is off
    e.update(ACTIONS[None], w.scan)
    assert e.recovery_proposal() is not None
    e.set_recovery()                                             # the recovery config does not clear it
    u = 1
    e.set_recovery_state(0.0, 0.0)                               # T = 0
    e.update(ACTIONS[None], w.scan); u += 1
    assert e.recovery_state()[3] == 0 and e.recovery_proposal() is not None
    force_p(e, 1.0)
    e.sensor_update(w.scan)                                      # no resampling: nothing is consumed
    assert e.recovery_state()[3] == 0 and e.recovery_proposal() is not None
    e.set_particles(p0, np.full(n, 1.0 / n))                     # neither do new particles or the beams
    e.set_beam_angles(w.ang)
    got = e.recovery_proposal()
    assert got is not None and [int(t) for t in got[0]] == thr and same_bits(got[1], fac)
    # the injecting update consumes it ...
    e.update(ACTIONS[None], w.scan)                              # (S, F unset by set_particles: p = 0)
    u += 1
    T = threshold(force_p(e, 0.5))
    e.update(ACTIONS[None], w.scan)
    coin, pick, hb = child_draws(SEED, u, n)
    u += 1
    inj = coin < np.uint64(T)
    g = np.flatnonzero(inj).astype(np.uint64)
    assert np.array_equal(np.flatnonzero(e.resample_indices() == -1), g.astype(np.int64))
    assert_poses(e.get_particles()[:, inj], ref.injected_poses(SEED, u - 1, g, pick[inj], thr, fac)[0], "the consuming update")
    assert e.recovery_proposal() is None
    # ... and the next forced injection follows the free-cell rule bit for bit
    T = threshold(force_p(e, 0.5))
    e.update(ACTIONS[None], w.scan)
    coin, pick, hb = child_draws(SEED, u, n)
    u += 1
    inj = coin < np.uint64(T)
    assert np.array_equal(np.flatnonzero(e.resample_indices() == -1), np.flatnonzero(inj))
    assert same_bits(e.get_particles()[:, inj], w.free_poses(pick[inj], hb[inj]))
    # mcl_set_map clears it
    e.set_recovery_proposal(MIX_MEANS, MIX_COVS)
    assert e.recovery_proposal() is not None
    e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    assert e.recovery_proposal() is None
    # None clears it
    e.set_recovery_proposal(MIX_MEANS, MIX_COVS)
    e.set_recovery_proposal(None)
    assert e.recovery_proposal() is None
    e.close()
    # an update that keeps its particles (adaptive resampling) injects nothing and consumes nothing
    from monte_carlo_localization_amd import synth as sy
    ang = sy.beam_angles(angle_step=18)
    scan = np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::18].astype(np.float32)
    k = make_engine(engine_mod, m, ang, n, seed=SEED, resample_neff_permille=1)
    k.set_particles(sy.tracking_cloud(np.random.default_rng(3), n, sig=(0.05, 0.05, 0.02)), np.full(n, 1.0 / n))
    k.set_recovery()
    k.update((0.0, 0.0, 0.0), scan)
    assert k.effective_sample_size()[0] >= 0.002 * n, "precondition: the next update keeps its particles"
    k.set_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)
    force_p(k, 1.0)
    k.update((0.0, 0.0, 0.0), scan)
    assert not k.effective_sample_size()[1], "precondition: the update kept its particles"
    assert k.recovery_state()[3] == 0 and k.recovery_proposal() is not None
    k.close()


# ---- 3. off is off
@pytest.mark.parametrize("n", [4096, 32768, 65536])
def test_off_is_off(engine_mod, world, n):
    from monte_carlo_localization_amd import synth
    w, m = world, world.m
    plain, untriggered, rec_off = (make_engine(engine_mod, m, w.ang, n, seed=SEED) for _ in range(3))
    p0 = synth.tracking_cloud(np.random.default_rng(7), n)
    for e in (plain, untriggered, rec_off):
        e.set_particles(p0, np.full(n, 1.0 / n))
    untriggered.set_recovery(alpha_slow=0.05, alpha_fast=0.5)
    untriggered.set_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)
    rec_off.set_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)
    for k in range(4):
        untriggered.set_recovery_state(0.0, 0.0)             # p = 0: the plain kernel
        if k == 2:                                           # setting it between updates keeps a warm path warm
            untriggered.set_recovery_proposal(MIX_MEANS[::-1].copy(), MIX_COVS[::-1].copy())
            rec_off.set_recovery_proposal(MIX_MEANS[::-1].copy(), MIX_COVS[::-1].copy())
        for e in (plain, untriggered, rec_off):
            e.update(ACTIONS[None], w.scan)
        ref_out = (plain.get_particles(), plain.resample_indices(), plain.log_weights())
        for e in (untriggered, rec_off):
            got = (e.get_particles(), e.resample_indices(), e.log_weights())
            for g, r in zip(got, ref_out):
                assert same_bits(g, r) if g.dtype == np.float64 else np.array_equal(g, r)
            assert e.recovery_state()[3] == 0 and e.recovery_proposal() is not None
            assert path_of(e) == path_of(plain)
        if k >= 1:
            assert path_of(plain) == PATH_OF_N[n]
    for e in (plain, untriggered, rec_off):
        e.close()


# ---- 4. P6: a map without a free cell
def test_no_free_cell_needed(engine_mod, mix):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    grid = np.full((64, 64), -1, np.int8)                    # every cell unknown
    n = 256
    p0 = np.stack([np.full(n, 1.6), np.full(n, 1.6), np.linspace(-3, 3, n)])
    scan = np.full(ang.size, 1.0, np.float32)
    mean, cov = np.array([[1.5, 1.7, 0.2]]), np.diag([0.01, 0.01, 0.04])[None]
    thr, fac = engine_mod.host_recovery_proposal(mean, cov)
    for with_proposal in (False, True):
        e = engine_mod.Engine(max_particles=n, seed=SEED)
        e.set_map(grid, 0.05, 0.0, 0.0)
        e.set_beam_angles(ang)
        e.set_particles(p0, np.full(n, 1.0 / n))
        e.set_recovery()
        e.update(ACTIONS[None], scan)
        before = e.get_particles()
        if with_proposal:
            e.set_recovery_proposal(mean, cov)
        force_p(e, 1.0)
        if not with_proposal:
            with pytest.raises(engine_mod.EngineError) as ei:
                e.update(ACTIONS[None], scan)
            assert ei.value.status == -2
            assert same_bits(e.get_particles(), before)
        else:
            e.update(ACTIONS[None], scan)
            assert e.recovery_state()[3] == n and (e.resample_indices() == -1).all()
            g = np.arange(n, dtype=np.uint64)
            pick = child_draws(SEED, 1, n)[1]
            assert_poses(e.get_particles(), ref.injected_poses(SEED, 1, g, pick, [int(t) for t in thr], fac)[0])
        e.close()


# ---- 5. the injected cloud has the covariance it was asked for
def test_sample_covariance(engine_mod, world):
    from monte_carlo_localization_amd import synth
    w, n = world, 65536
    mean = np.array([-46.19, 29.66, 0.3])
    cov = np.array([[0.09, 0.03, -0.01], [0.03, 0.16, 0.02], [-0.01, 0.02, 0.04]])
    e = make_engine(engine_mod, w.m, w.ang, n, seed=SEED)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(5), n), np.full(n, 1.0 / n))
    e.set_recovery()
    e.update(ACTIONS[None], w.scan)
    e.set_recovery_proposal(mean[None], cov[None])
    force_p(e, 1.0)
    e.update(ACTIONS[None], w.scan)
    assert e.recovery_state()[3] == n
    p = e.get_particles()
    ok, worst = mr.cov_band_ok(p, mean, cov)
    print("worst covariance entry, in 6-sigma bands:", worst)
    assert ok, worst
    assert np.abs(p.mean(axis=1) - mean).max() < 6.0 * math.sqrt(0.16 / n)
    e.close()


# ---- 6. refusals (P7, P1) and the getter's round trip
def test_refusals_and_getter(engine_mod, spielberg, mix):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    thr, fac = mix
    e = make_engine(engine_mod, spielberg, ang, 1024, seed=3, weight_mode=engine_mod.WEIGHT_PRODUCT)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.set_recovery_proposal(MIX_MEANS, MIX_COVS)
    assert ei.value.status == -5
    e.set_recovery_proposal(None)
    e.close()
    g = engine_mod.Group([0], max_particles=1024)
    with pytest.raises(engine_mod.EngineError) as ei:
        g.engine(0).set_recovery_proposal(MIX_MEANS, MIX_COVS)
    assert ei.value.status == -5
    g.close()
    if engine_mod.Engine.comm_available():
        e = make_engine(engine_mod, spielberg, ang, 1024, seed=3)
        e.init_particles_pose(P0, 1024, 0, 1024)
        e.comm_create(e.comm_unique_id(), 1, 0)
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_recovery_proposal(MIX_MEANS, MIX_COVS)
        assert ei.value.status == -5
        e.comm_destroy()
        e.close()
    e = make_engine(engine_mod, spielberg, ang, 1024, seed=3)
    assert e.recovery_proposal() is None
    e.set_recovery_proposal(MIX_MEANS, MIX_COVS, MIX_W)          # recovery off: allowed
    got = e.recovery_proposal()
    assert [int(t) for t in got[0]] == thr and same_bits(got[1], fac)
    bad_cov = MIX_COVS.copy(); bad_cov[2] = np.diag([1.0, -1.0, 1.0])
    bad_mean = MIX_MEANS.copy(); bad_mean[3, 1] = np.nan
    cases = [(MIX_MEANS, bad_cov, MIX_W, "component 2"), (bad_mean, MIX_COVS, MIX_W, "component 3"),
             (MIX_MEANS, MIX_COVS, [1.0, -1.0, 1.0, 1.0], "component 1"), (MIX_MEANS, MIX_COVS, np.zeros(4), "sum"),
             (MIX_MEANS, MIX_COVS, [1.5e308, 1.5e308, 0.0, 0.0], "sum"),
             (np.zeros((4097, 3)), np.zeros((4097, 3, 3)), None, "4096")]
    for means, covs, wts, what in cases:
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_recovery_proposal(means, covs, wts)
        assert ei.value.status == -1 and what in str(ei.value), str(ei.value)
        got = e.recovery_proposal()                              # nothing changed
        assert [int(t) for t in got[0]] == thr and same_bits(got[1], fac)
    many = 4096
    mm = np.tile(MIX_MEANS[0], (many, 1)); mm[:, 0] += np.arange(many)
    e.set_recovery_proposal(mm, np.tile(MIX_COVS[0], (many, 1, 1)))
    got = e.recovery_proposal()
    assert got[0].size == many and [int(t) for t in got[0]] == [(k + 1) << 41 for k in range(many)]
    e.set_recovery_proposal(MIX_MEANS[:1], MIX_COVS[:1])          # a smaller one after a larger one
    assert e.recovery_proposal()[0].tolist() == [2 ** 53]
    e.close()


# ---- 7. a kidnapped robot found again with KLD on: the row profiles/recovery.md marks "not found"
KIDNAP_N = 65536
KIDNAP_A = (0.0, 0.0, 0.0)
KIDNAP_ALPHAS = (0.001, 0.1)
KIDNAP_K = 20
KIDNAP_CONVERGE = 10
KIDNAP_CANDIDATES = [KIDNAP_B, (-46.19, 29.71, 0.1), (-29.91, 35.39, 0.0)]     # the first whose scan the thinned search places
SEARCH = dict(beam_stride=10, stride_cells=4)


def _err(e, truth):
    pose = e.expected_pose()
    return math.hypot(pose[0] - truth[0], pose[1] - truth[1]), abs((pose[2] - truth[2] + math.pi) % (2 * math.pi) - math.pi)


def test_kidnap_with_kld(engine_mod, spielberg):
    """Run A proposes from the scan before every update whose p > 0, run B (the control) injects from free space.  With KLD on the
    converged set is 512 to 768 particles; profiles/recovery.md records 55.3 m for the control."""
    from monte_carlo_localization_amd import synth
    m, n = spielberg, KIDNAP_N
    ang = synth.beam_angles()
    results, used = {}, None
    for propose in (True, False):
        e = make_engine(engine_mod, m, ang, n, seed=SEED)
        scan_a = synth.scan_from_pose(e, m, ang, KIDNAP_A)
        if used is None:
            # precondition (existing code, not the code under test): the thinned search alone places the scan
            for cand in KIDNAP_CANDIDATES:
                scan_b = synth.scan_from_pose(e, m, ang, cand)
                hits, _ = e.global_search_beam(scan_b, max_hits=16, **SEARCH)
                d = np.hypot(hits["pose"][:, 0] - cand[0], hits["pose"][:, 1] - cand[1])
                dth = np.abs((hits["pose"][:, 2] - cand[2] + math.pi) % (2 * math.pi) - math.pi)
                near = np.flatnonzero((d < 0.5) & (dth < 0.2))
                print("candidate", cand, "hit rank", near[:1], "of", hits.size)
                if near.size:
                    used = (cand, scan_b)
                    break
            assert used is not None, "precondition: the thinned search finds none of the candidate poses"
        B, scan_b = used
        e.init_particles_pose(KIDNAP_A, n)
        e.set_kld(min_particles=512, max_particles=n)
        e.set_recovery(alpha_slow=KIDNAP_ALPHAS[0], alpha_fast=KIDNAP_ALPHAS[1])
        for _ in range(KIDNAP_CONVERGE):
            e.update((0.0, 0.0, 0.0), scan_a)
        d, dth = _err(e, KIDNAP_A)
        assert d < 1.0 and dth < math.radians(5), (propose, d, dth)      # (a sanity check: a KLD-sized set is 0.44 m off in the profile)
        injected = proposed = 0
        for k in range(KIDNAP_K):
            if propose and e.recovery_state()[2] > 0:
                e.propose_from_scan(scan_b, **SEARCH)
                proposed += 1
            e.update((0.0, 0.0, 0.0), scan_b)
            injected += e.recovery_state()[3]
        d, dth = _err(e, B)
        results[propose] = (d, dth, injected, proposed)
        print("propose" if propose else "control", "error m / rad", d, dth, "injected", injected, "proposals", proposed, "n", e.n)
        e.close()
    assert results[True][3] > 0 and results[True][2] > 0, results
    assert results[True][0] < 0.25 and results[True][1] < math.radians(5), results
    assert results[False][0] > 10.0, results


# ---- 8. propose_from_scan: the search of the model in use, the forms of its arguments
@pytest.mark.parametrize("lf", [False, True])
def test_propose_from_scan_forms(engine_mod, spielberg, lf):
    from monte_carlo_localization_amd import synth
    m = spielberg
    ang = synth.beam_angles()
    scan = np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)
    e = make_engine(engine_mod, m, ang, 1024, seed=SEED)
    if lf:
        e.set_likelihood_field()
    search, refine = (e.global_search, e.refine_poses) if lf else (e.global_search_beam, e.refine_poses_beam)
    hits = e.propose_from_scan(scan, max_hits=8, **SEARCH)
    want_hits, _ = search(scan, max_hits=8, **SEARCH)
    assert hits.size > 0 and np.array_equal(hits, want_hits)            # the model in use was searched, and not switched
    assert (e.lib.mcl_get_likelihood_table(e._h, None, 0, None) == 0) == lf
    r, _ = refine(hits["pose"], scan)
    thr, fac = e.recovery_proposal()
    want = engine_mod.host_recovery_proposal(r["mean"], r["cov"])
    assert np.array_equal(thr, want[0]) and same_bits(fac, want[1])
    print("nearest component to the pose the golden scan was taken at, m:", np.hypot(fac[:, 0], fac[:, 1]).min())
    # the hit poses with a covariance: the default is one lattice step
    e.propose_from_scan(scan, max_hits=8, refine=False, **SEARCH)
    res = float(np.float32(m.resolution))
    step_cov = np.diag([(4 * res) ** 2, (4 * res) ** 2, (2 * math.pi / 72) ** 2])
    want = engine_mod.host_recovery_proposal(hits["pose"], np.tile(step_cov, (hits.size, 1, 1)))
    got = e.recovery_proposal()
    assert np.array_equal(got[0], want[0]) and same_bits(got[1], want[1])
    e.propose_from_scan(scan, max_hits=8, refine=False, cov=np.diag([0.04, 0.04, 0.01]), **SEARCH)
    assert np.array_equal(e.recovery_proposal()[1][:, 3:], np.tile([0.2, 0.0, 0.2, 0.0, 0.0, 0.1], (hits.size, 1)))
    # seed_counts' shares as weights
    e.propose_from_scan(scan, max_hits=8, weights="likelihood", **SEARCH)
    shares = engine_mod.seed_counts(r["best_log_likelihood"], 1 << 30).astype(np.float64)
    want = engine_mod.host_recovery_proposal(r["mean"], r["cov"], shares)
    assert np.array_equal(e.recovery_proposal()[0], want[0])
    with pytest.raises(ValueError):
        e.propose_from_scan(scan, weights="best")
    # an error of the search propagates
    with pytest.raises(engine_mod.EngineError):
        e.propose_from_scan(scan[:100], **SEARCH)                       # not this engine's beam count
    e.close()
