"""The likelihood-field sensor model on the GPU (mcl_set_likelihood_field) against the numpy restatement
tests/lfield_ref.py: the device field and table exactly; every particle's log-weight bit for bit (an end point within 1e-6 cell of
a cell edge may land on either side) at sizes on both sides of the small-update paths, with scans holding NaN, inf, negative and
max-range readings and particles whose end points leave the map; what resampling, KLD and recovery make of those weights (E6);
switching between the models; the refusals; a global localisation on Spielberg."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lfield_ref as lr
from conftest import GOLDEN, make_engine, tracking_cloud
from test_recovery_host import child_draws, threshold
from whole_set import assert_close, assert_same

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0010 + 4242
ACTION = (0.1, 0.0, 0.02)
MAX_RANGE = 12.0


def _scan(step=1):
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32)


def _angles(step=1):
    from monte_carlo_localization_amd import synth
    return synth.beam_angles(angle_step=step)


def odd_scan(scan):
    """the scan with readings that must not count (NaN, +-inf, negative, max range and beyond) and two that must (0, -0)"""
    s = scan.copy()
    for j, v in ((3, np.nan), (10, np.inf), (11, -np.inf), (17, -0.5), (23, MAX_RANGE), (29, MAX_RANGE + 1.0), (31, 0.0), (37, -0.0)):
        s[j] = v
    return s


def edge_particles(rng, m, n):
    """poses within 2 m of the map's border, inside and outside it: their end points leave the map"""
    H, W = m.data.shape
    res = float(np.float32(m.resolution))
    x0, y0 = m.origin_x, m.origin_y
    x1, y1 = x0 + W * res, y0 + H * res
    side, t, d = rng.integers(0, 4, n), rng.random(n), rng.uniform(-2.0, 2.0, n)
    x = np.where(side == 0, x0 + d, np.where(side == 1, x1 + d, x0 + t * (x1 - x0)))
    y = np.where(side == 2, y0 + d, np.where(side == 3, y1 + d, y0 + t * (y1 - y0)))
    return np.stack([x, y, rng.uniform(-np.pi, np.pi, n)])


@pytest.fixture(scope="module")
def sp_ref(spielberg):
    return dict(D=lr.field(spielberg.data, spielberg.resolution), Lf=lr.table(spielberg.resolution))


class Ambiguity:
    """tally of ambiguous beams over a test, held to the bound of DESIGN.md §4.10 (LF4): at most 1e-5 of all beams, or 2 beams
    where 1e-5 of them is fewer (random poses put an end point within 1e-6 cell of an edge with probability ~4e-6 per beam, so a
    strict 1e-5 at 122 000 beams would hang on whether one or two such beams occur).  Children injected by recovery are not
    counted: they sit on cell corners (mcl_init_global's rule), so their end points lie on cell edges far more often -- their
    log-weights are still checked against every alternative."""

    def __init__(self):
        self.amb = self.beams = 0

    def check(self):
        assert self.amb <= max(1e-5 * self.beams, 2), (self.amb, self.beams)


def check_logw(e, ref, m, ang, scan, tally, sample=None, untallied=None):
    """the engine's log-weights of its current particles against LF5 (of the particles in `sample`, or all; the particles in the
    mask `untallied` stay out of the ambiguity tally); returns them"""
    parts = e.get_particles()
    got = e.log_weights()
    if sample is not None:
        parts, got = np.ascontiguousarray(parts[:, sample]), got[sample]
    want, alts, n_amb = lr.log_weights(parts, ang, scan, ref["D"], ref["Lf"], m.resolution, m.origin_x, m.origin_y, MAX_RANGE)
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    for i in bad:
        assert int(i) in alts and got[i] in alts[int(i)], (int(i), got[i], want[i], alts.get(int(i)))
    counted = np.ones(parts.shape[1], bool) if untallied is None else ~untallied
    tally.amb += int(n_amb[counted].sum())
    tally.beams += int(counted.sum()) * lr.used_beams(ang, scan, MAX_RANGE)[0].size
    return e.log_weights()


# ---- 1. the field and the table
def random_map(seed=3, H=301, W=517):
    return np.random.default_rng(seed).choice(np.array([-1, 0, 100], np.int8), size=(H, W), p=[0.1, 0.87, 0.03])


@pytest.mark.parametrize("which", ["Spielberg_map", "sibal1", "first_map", "random"])
def test_device_field_is_the_restatement(engine_mod, maps_mod, which):
    if which == "random":
        grid, res, ox, oy = random_map(), np.float32(0.05), -3.0, 2.0
    else:
        m = maps_mod.load_npz(os.path.join(GOLDEN, f"map_{which}.npz"))
        grid, res, ox, oy = m.data, m.resolution, m.origin_x, m.origin_y
    e = engine_mod.Engine(max_particles=64)
    e.set_map(grid, res, ox, oy)
    near = 255.5 * float(np.float32(res))                 # K just below the uint16 limit
    for max_occ in (2.0, near):
        e.set_likelihood_field(max_occ_dist_m=max_occ)
        assert lr.K_of(max_occ, res) <= 65535
        got = e.likelihood_field()
        assert np.array_equal(got, lr.field(grid, res, max_occ)), (which, max_occ)
        assert e.likelihood_table().size == lr.K_of(max_occ, res) + 1
    e.close()


def test_field_follows_set_map(engine_mod, spielberg, sibal1):
    e = engine_mod.Engine(max_particles=64)
    e.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    e.set_likelihood_field()
    a = e.likelihood_field()
    e.set_map(sibal1.data, sibal1.resolution, sibal1.origin_x, sibal1.origin_y)           # rebuilt while the model is on
    assert np.array_equal(e.likelihood_field(), lr.field(sibal1.data, sibal1.resolution))
    e.set_likelihood_field(False)
    e.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    with pytest.raises(engine_mod.EngineError) as ei:                                   # off: nothing to read
        e.likelihood_field()
    assert ei.value.status == -2
    e.set_likelihood_field()                                                            # built for the map set before
    assert np.array_equal(e.likelihood_field(), a)
    with pytest.raises(engine_mod.EngineError) as ei:                                   # K = 160000 on a 5 mm map
        e.set_map(np.zeros((64, 64), np.int8), 0.005, 0.0, 0.0)
    assert ei.value.status == -1
    assert np.array_equal(e.likelihood_field(), a)                                      # refused before anything changed
    e.close()


@pytest.mark.parametrize("fields", [dict(), dict(z_rand=0.0, sigma_hit_m=0.01), dict(z_hit=0.9, z_rand=0.1, sigma_hit_m=0.5, max_occ_dist_m=4.0)])
def test_device_table_is_the_restatement(engine_mod, spielberg, fields):
    e = engine_mod.Engine(max_particles=64, max_range_m=20.0, squash_factor=3.0)
    e.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    e.set_likelihood_field(**fields)
    got = e.likelihood_table()
    want = lr.table(spielberg.resolution, max_range_m=20.0, squash_factor=3.0, **fields)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if fields.get("z_rand") == 0.0:
        assert np.isneginf(got).any()
    e.close()


# ---- 2. every particle's log-weight
@pytest.mark.parametrize("n,step", [(2000, 18), (8193, 18), (65536, 1), (262144, 1)])
@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
def test_every_log_weight(engine_mod, spielberg, sp_ref, n, step, mode):
    m, ang = spielberg, _angles(step)
    scan = odd_scan(_scan(step))
    rng = np.random.default_rng(n + mode)
    p0 = tracking_cloud(rng, n)
    k = n // 20
    p0[:, :k] = edge_particles(rng, m, k)
    e = make_engine(engine_mod, m, ang, n, seed=SEED, resample_mode=mode)
    e.set_likelihood_field()
    e.set_particles(p0, np.full(n, 1.0 / n))
    tally = Ambiguity()
    e.sensor_update(scan)                                       # the set as given, edges included
    check_logw(e, sp_ref, m, ang, scan, tally)
    for _ in range(2):                                          # then two full updates (the second one on resampled children)
        e.update(ACTION, scan)
        check_logw(e, sp_ref, m, ang, scan, tally)
        t = e.stage_timings()
        assert t[3] > 0.0 and sum(t[:5]) <= t[5] + 1e-3, t          # the sensor stage is stage 3; the stages fit in the total
    tally.check()
    e.close()


def test_sampled_log_weights_at_4m(engine_mod, spielberg, sp_ref):
    n, m, ang, scan = 1 << 22, spielberg, _angles(), odd_scan(_scan())
    rng = np.random.default_rng(44)
    p0 = tracking_cloud(rng, n)
    p0[:, :n // 50] = edge_particles(rng, m, n // 50)
    e = make_engine(engine_mod, m, ang, n, seed=SEED)
    e.set_likelihood_field()
    e.set_particles(p0, np.full(n, 1.0 / n))
    tally = Ambiguity()
    e.update(ACTION, scan)
    check_logw(e, sp_ref, m, ang, scan, tally, sample=np.sort(rng.choice(n, 65536, replace=False)))
    tally.check()
    e.close()


def test_raw_scan_and_stride(engine_mod, spielberg, sp_ref):
    """mcl_update_scan with angle_step 18 on the raw 1081 ranges (odd readings among the kept ones) is mcl_update on every 18th
    range, bit for bit, and its log-weights are LF5's"""
    n, m, ang = 8192, spielberg, _angles(18)
    raw = odd_scan(_scan(1) * 1.0)
    raw[18 * np.arange(8)] = [np.nan, np.inf, -1.0, MAX_RANGE, 0.0, 3.25, MAX_RANGE + 2.0, -np.inf]
    p0 = tracking_cloud(np.random.default_rng(21), n)
    a, b = (make_engine(engine_mod, m, ang, n, seed=SEED) for _ in range(2))
    for e in (a, b):
        e.set_likelihood_field()
        e.set_particles(p0, np.full(n, 1.0 / n))
    tally = Ambiguity()
    for _ in range(2):
        a.update_scan(ACTION, raw, 18)
        b.update(ACTION, raw[::18].copy())
        assert_same("particles", a.get_particles(), b.get_particles())
        assert_same("log-weights", a.log_weights(), b.log_weights())
        check_logw(a, sp_ref, m, ang, raw[::18].copy(), tally)
    tally.check()
    a.close()
    b.close()


def test_injected_normals_and_uniforms(engine_mod, orc, spielberg, sp_ref):
    """injected draws (the reference-exact hooks): uniform weights and the uniforms (m + 1/2) / N give every child its own
    parent, the injected normals move it as the spec's motion model does, and k_lfield weighs the moved set"""
    n, m, ang, scan = 4096, spielberg, _angles(), _scan()
    rng = np.random.default_rng(23)
    p0 = tracking_cloud(rng, n)
    nrm = rng.normal(size=(n, 3))
    e = make_engine(engine_mod, m, ang, n, seed=SEED)
    e.set_likelihood_field()
    e.set_particles(p0, np.full(n, 1.0 / n))
    e.update(ACTION, scan, normals=nrm, uniforms=(np.arange(n) + 0.5) / n)
    assert np.array_equal(e.resample_indices(), np.arange(n))
    assert_close("children", e.get_particles(), orc.motion_model(p0, ACTION, nrm), 1e-13, 1e-13)
    tally = Ambiguity()
    check_logw(e, sp_ref, m, ang, scan, tally)
    tally.check()
    e.close()


@pytest.mark.parametrize("n", [4096, 65536])
def test_adaptive_resampling_keeps_and_carries(engine_mod, spielberg, sp_ref, n):
    """resample_neff_permille: an update that keeps its particles adds the previous update's logw - max (E9) to k_lfield's sums.
    Every 180th reading of the scan is kept (the rest NaN) and the threshold is N_eff >= N / 10, so that runs of kept updates
    (a carry that is not zero) alternate with resampling ones (a numpy rehearsal of this set gives R K K R K K ...)."""
    m, ang = spielberg, _angles()
    scan = np.full(ang.size, np.nan, np.float32)
    scan[::180] = _scan()[::180]
    e = make_engine(engine_mod, m, ang, n, seed=SEED, resample_neff_permille=100)
    e.set_likelihood_field()
    e.set_particles(tracking_cloud(np.random.default_rng(n + 9), n, sig=(0.05, 0.05, 0.02)), np.full(n, 1.0 / n))
    tally = Ambiguity()
    e.update(ACTION, scan)
    prev = check_logw(e, sp_ref, m, ang, scan, tally)
    kinds = []
    for _ in range(8):
        e.update(ACTION, scan)
        kept = not e.effective_sample_size()[1]
        kinds.append(kept)
        parts, got = e.get_particles(), e.log_weights()
        want, alts, n_amb = lr.log_weights(parts, ang, scan, sp_ref["D"], sp_ref["Lf"], m.resolution, m.origin_x, m.origin_y, MAX_RANGE)
        carry = np.where(prev == -np.inf, -np.inf, prev - prev.max()) if kept else np.zeros(n)
        if kept:
            want = want + carry
        for i in np.flatnonzero(got.view(np.uint64) != want.view(np.uint64)):
            ok = [a + carry[i] for a in alts.get(int(i), [])] if kept else alts.get(int(i), [])
            assert got[i] in ok, (int(i), kept, got[i], want[i])
        tally.amb += int(n_amb.sum())
        tally.beams += n * lr.used_beams(ang, scan, MAX_RANGE)[0].size
        prev = got
    assert True in kinds and False in kinds, kinds
    tally.check()
    e.close()


# ---- 3. what resampling makes of the weights
@pytest.mark.parametrize("mode,kld,rec", [(0, False, False), (1, False, False), (0, True, False), (1, False, True), (0, True, True)],
                         ids=["multinomial", "systematic", "kld", "recovery", "kld+recovery"])
def test_resampling_downstream(engine_mod, orc, spielberg, sp_ref, mode, kld, rec):
    """update 0 forms likelihood-field weights; update 1 must draw from them what the spec's E6 draws (Philox streams 2 / 3), move
    the children as the spec does, and (recovery forced) inject exactly the children whose stream-8 coin is below T"""
    n, m, ang, scan = 65536, spielberg, _angles(), _scan()
    e = make_engine(engine_mod, m, ang, n, seed=SEED, resample_mode=mode)
    e.set_likelihood_field()
    e.set_particles(tracking_cloud(np.random.default_rng(11), n), np.full(n, 1.0 / n))
    if kld:
        e.set_kld(min_particles=256, max_particles=n)
    if rec:
        e.set_recovery()
    tally = Ambiguity()
    e.update(ACTION, scan)
    parents = e.get_particles()
    logw = check_logw(e, sp_ref, m, ang, scan, tally)
    _, q, _ = orc.eng_weights_from_log(logw)
    n1 = e.kld_state()[1]
    if kld:
        assert n1 < n                                           # the draw of update 1 has another size
    T = 0
    if rec:
        e.set_recovery_state(0.0, math.log1p(-0.3))
        T = threshold(e.recovery_state()[2])
        assert T > 0
    e.update(ACTION, scan)
    assert e.n == n1
    if mode == 0:
        want = orc.eng_resample_indices(q, 0, n_children=n1, k53=orc.eng_philox_k53(SEED, 1, 0, n1))
    else:
        want = orc.eng_resample_indices(q, 1, n_children=n1, k0=orc.eng_philox_k0(SEED, 1))
    idx = e.resample_indices()
    inj = np.zeros(n1, bool)
    if rec:
        inj = child_draws(SEED, 1, n1)[0] < np.uint64(T)
        assert inj.any()
        assert np.array_equal(np.flatnonzero(idx == -1), np.flatnonzero(inj))
    assert_same("resample indices", idx[~inj], want[~inj])
    kids = e.get_particles()
    moved = orc.motion_model(parents[:, want], ACTION, orc.eng_philox_normals(SEED, 1, 0, n1))
    assert_close("children", kids[:, ~inj], moved[:, ~inj], 1e-13, 1e-13)
    check_logw(e, sp_ref, m, ang, scan, tally, untallied=inj)   # the new children's log-weights, injected ones included
    tally.check()
    e.close()


# ---- 4. switching between the models
@pytest.mark.parametrize("n", [4096, 65536])
def test_set_and_unset_before_any_update_changes_nothing(engine_mod, spielberg, n):
    m, ang, scan = spielberg, _angles(), _scan()
    p0 = tracking_cloud(np.random.default_rng(5), n)
    never, toggled = (make_engine(engine_mod, m, ang, n, seed=SEED) for _ in range(2))
    for e in (never, toggled):
        e.set_particles(p0, np.full(n, 1.0 / n))
    toggled.set_likelihood_field()
    toggled.set_likelihood_field(False)
    for _ in range(3):
        for e in (never, toggled):
            e.update(ACTION, scan)
        assert_same("particles", toggled.get_particles(), never.get_particles())
        assert_same("resample indices", toggled.resample_indices(), never.resample_indices())
        assert_same("log-weights", toggled.log_weights(), never.log_weights())
        assert toggled.ray_kernel_name() == never.ray_kernel_name()
    never.close()
    toggled.close()


def test_beam_field_beam(engine_mod, orc, spielberg, spielberg_oracle, sp_ref):
    """beam model (the sweep path: its layout, cleared-word cache and far-pass state warm), the likelihood field, the beam model
    again: the last log-weights are the spec oracle's for that particle set"""
    n, m, ang, scan = 65536, spielberg, _angles(), _scan()
    om = spielberg_oracle
    L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
    oi = orc.obs_index(scan, om)
    e = make_engine(engine_mod, m, ang, n, seed=SEED)
    e.set_particles(tracking_cloud(np.random.default_rng(8), n), np.full(n, 1.0 / n))

    def beam_update():
        e.update(ACTION, scan)
        assert e.ray_kernel_name() == "k_rays_sweep"
        want, _, _ = orc.eng_log_weights(om, e.get_particles(), ang, oi, L)
        assert_same("beam-model log-weights", e.log_weights(), want)

    beam_update()
    beam_update()
    e.set_likelihood_field()
    tally = Ambiguity()
    for _ in range(2):
        e.update(ACTION, scan)
        check_logw(e, sp_ref, m, ang, scan, tally)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.ray_kernel_name()
    assert ei.value.status == -5
    e.set_likelihood_field(False)
    beam_update()
    beam_update()
    tally.check()
    e.close()


# ---- 5. refusals
def test_refusals(engine_mod, spielberg):
    m, ang = spielberg, _angles(18)
    obs = _scan(18)
    e = make_engine(engine_mod, m, ang, 1024, seed=3, weight_mode=engine_mod.WEIGHT_PRODUCT, keep_ray_steps=1)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.set_likelihood_field()
    assert ei.value.status == -5
    e.close()
    e = make_engine(engine_mod, m, ang, 1024, seed=3, keep_ray_steps=1)
    bad = [dict(sigma_hit_m=0.0), dict(sigma_hit_m=-1.0), dict(sigma_hit_m=math.nan), dict(max_occ_dist_m=0.0),
           dict(max_occ_dist_m=math.inf), dict(z_hit=-0.5), dict(z_rand=math.nan), dict(z_hit=0.0, z_rand=0.0),
           dict(max_occ_dist_m=16.0), dict(reserved=(0, 1))]           # (16 m: K = 76 204 on this map)
    for b in bad:
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_likelihood_field(**b)
        assert ei.value.status == -1, b
    e.init_particles_pose((0.0, 0.0, 0.0), 1024)
    e.set_likelihood_field()
    lib = e.lib
    assert lib.mcl_stage_rays(e._h, obs.ctypes.data_as(C.c_void_p), C.c_int32(obs.size)) == -5
    act = np.array(ACTION)
    assert lib.mcl_stage_keep(e._h, C.c_int64(0), C.c_int64(1024), act.ctypes.data_as(C.c_void_p)) == -5
    assert lib.mcl_stage_weights(e._h, C.c_double(0.0)) == -5
    assert lib.mcl_stage_finish(e._h, np.zeros(5).ctypes.data_as(C.c_void_p)) == -5
    assert "single-engine" in lib.mcl_last_error(e._h).decode()
    uid = (C.c_ubyte * 128)()
    assert lib.mcl_comm_create(e._h, uid, C.c_int32(1), C.c_int32(0)) == -5
    e.update(ACTION, obs)
    for readback in (e.ray_steps, e.ray_kernel_name, e.ray_kernel_variant):
        with pytest.raises(engine_mod.EngineError) as ei:
            readback()
        assert ei.value.status == -5
    e.set_likelihood_field(False)
    e.update(ACTION, obs)
    assert e.ray_steps().shape == (1024, ang.size)
    e.close()
    g = engine_mod.Group([0], max_particles=1024)
    with pytest.raises(engine_mod.EngineError) as ei:
        g.engine(0).set_likelihood_field()
    assert ei.value.status == -5
    g.close()


# ---- 6. global localisation on Spielberg (the run of profiles/likelihood_field.md, tools/likelihood_field_bench.py global)
LOC_N = 1 << 20
LOC_SEED = 81
LOC_START = (-46.19, 29.66, -3.02)
LOC_ACTION = (0.05, 0.0, 0.01)
LOC_MAX_UPDATES = 5           # fixed from the first run, which needed 2 (profiles/likelihood_field.md)


def test_global_localisation(engine_mod, orc, spielberg, spielberg_oracle):
    """From a uniform 1M cloud, scans cast by the oracle from a robot moving along a short path: the estimate comes within
    0.5 m / 0.1 rad of the truth within LOC_MAX_UPDATES updates"""
    m, ang = spielberg, _angles()
    e = make_engine(engine_mod, m, ang, LOC_N, seed=LOC_SEED)
    e.set_likelihood_field()
    e.init_global(LOC_N)
    truth = np.array(LOC_START, np.float64).reshape(3, 1)
    errs = []
    for _ in range(LOC_MAX_UPDATES):
        truth = orc.motion_model(truth, LOC_ACTION, np.zeros((1, 3)))
        x, y, th = truth[:, 0]
        scan, _ = orc.cast_many(spielberg_oracle, np.full(ang.size, x), np.full(ang.size, y), th + ang.astype(np.float64))
        e.update(LOC_ACTION, scan)
        pose = e.expected_pose()
        d = math.hypot(pose[0] - x, pose[1] - y)
        dth = abs((pose[2] - th + math.pi) % (2 * math.pi) - math.pi)
        errs.append((round(d, 3), round(dth, 4)))
        if d < 0.5 and dth < 0.1:
            break
    assert d < 0.5 and dth < 0.1, errs
    e.close()
