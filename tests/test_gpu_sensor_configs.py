"""Sensor and motion models other than the reference's defaults on the GPU, against the spec oracle given the same parameters
(DESIGN.md §3 E1-E6): log-weights bit for bit on every ray path, -inf entries included; full updates with motion dispersions
of their own; and E5's rule for impossible particles -- logw = -inf => w = q = 0 --, also when every particle of the set is
impossible (z_rand = 0 makes the table hold zeros): then every weight is 0, N_eff is 0, the pose is the reference's
(0, 0, atan2(0, 0)) = (0, 0, 0), and the next draw takes parent 0 for every child (Q = 0, E6)."""
import os
from collections import namedtuple

import numpy as np
import pytest

from conftest import GOLDEN, make_engine, tracking_cloud

pytestmark = pytest.mark.gpu

ACTION = (0.1, 0.0, 0.02)
DEFAULTS = dict(z_hit=0.80, z_short=0.01, z_max=0.07, z_rand=0.12, sigma_hit=8.0, squash_factor=2.2)
CONFIGS = {
    "zrand0_sigma2": dict(z_rand=0.0, sigma_hit=2.0),
    "hit_only_sigma2_squash3.1": dict(z_hit=1.0, z_short=0.0, z_max=0.0, z_rand=0.0, sigma_hit=2.0, squash_factor=3.1),
    "heavy_short_sigma30": dict(z_hit=0.2, z_short=0.6, z_max=0.05, z_rand=0.15, sigma_hit=30.0),
}
TRACK_SIG = (0.2, 0.2, 0.1)        # about half of this cloud sees some beam the zero-z_rand models call impossible
FineMap = namedtuple("FineMap", "data resolution origin_x origin_y")


def sensor_cfg(name_or_dict):
    over = CONFIGS[name_or_dict] if isinstance(name_or_dict, str) else name_or_dict
    return {**DEFAULTS, **over}


def oracle_table(orc, P, k):
    T = orc.sensor_table(P, k["z_hit"], k["z_short"], k["z_max"], k["z_rand"], k["sigma_hit"])
    return orc.eng_log_table(T, 1.0 / k["squash_factor"])


def scan_origin(step=1):
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32).copy()


def long_scan(m, P, n_beams):
    """Every beam reads 3 px short of the maximum range: from inside the track some beam of every particle hits a wall more
    than the Gaussian's reach closer, and with z_rand = 0 nothing else explains the reading (T = 0)."""
    return np.full(n_beams, np.float32((P - 3) * float(m.resolution)), np.float32)


def assert_minus_inf_reached(L, want):
    if (L == -np.inf).any():
        assert np.isneginf(want).any(), "the case reaches no -inf log-weight: it tests nothing of E5"
    else:
        assert np.isfinite(want).all()
    assert not np.isnan(want).any()


def assert_weights(orc, e, logw, parts):
    """The weights, pose and N_eff the engine reports for log-weights `logw` (E5, then the reference's normalisation)."""
    w, _, _ = orc.eng_weights_from_log(logw)
    got = e.get_weights()
    assert not np.isnan(got).any()
    dead = np.isneginf(logw)
    assert (got[dead] == 0.0).all()
    if w.sum() > 0.0:
        np.testing.assert_allclose(got, w / w.sum(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(e.expected_pose(), orc.expected_pose(parts, w / w.sum()), rtol=0, atol=1e-9)
        np.testing.assert_allclose(e.effective_sample_size()[0], w.sum() ** 2 / (w * w).sum(), rtol=1e-9)
    else:
        assert np.array_equal(got, np.zeros(logw.size))
        want_pose = orc.expected_pose(parts, w)
        assert np.array_equal(want_pose, np.zeros(3))
        assert np.array_equal(e.expected_pose(), want_pose)
        assert e.effective_sample_size()[0] == 0.0


# ---------------------------------------------------------------------------------------------- log-weights on every ray path
@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("n,kernel", [(4000, "k_rays_skip"), (65536, "k_rays_sweep")])
def test_log_weights_on_the_short_range_paths(orc, engine_mod, spielberg, spielberg_oracle, name, n, kernel):
    """Spielberg (207 px), 1081 beams: k_rays_skip at 4000 particles, k_rays_sweep in its LDS windows at 65 536 (AUTO)."""
    from monte_carlo_localization_amd import synth
    k = sensor_cfg(name)
    ang = synth.beam_angles()
    e = make_engine(engine_mod, spielberg, ang, n, **k)
    assert e.planned_ray_kernel(n)[0] == kernel
    p = tracking_cloud(np.random.default_rng(n), n, sig=TRACK_SIG)
    e.set_particles(p, np.full(n, 1.0 / n))
    scan = scan_origin()
    e.sensor_update(scan)
    assert e.ray_kernel_name() == kernel
    if kernel == "k_rays_sweep":
        v = e.ray_kernel_variant()
        assert not v["global_fields"] and not v["hybrid"], v
    L = oracle_table(orc, spielberg_oracle.max_range_px, k)
    want, _, _ = orc.eng_log_weights(spielberg_oracle, p, ang, orc.obs_index(scan, spielberg_oracle), L)
    assert_minus_inf_reached(L, want)
    got = e.log_weights()
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {n} log-weights differ"
    assert_weights(orc, e, want, p)
    e.close()


@pytest.mark.parametrize("form", ["global", "hybrid"])
@pytest.mark.parametrize("name", ["zrand0", "zrand0_sigma2"])
def test_log_weights_long_range_global_fields(orc, engine_mod, sibal1, monkeypatch, form, name):
    """sibal1 at 0.025 m (479 px): k_rays_sweep on the wedge fields in global memory, alone or behind the LDS windows."""
    monkeypatch.setenv("MCL_SWEEP_HYBRID", "2" if form == "hybrid" else "0")
    k = sensor_cfg(dict(z_rand=0.0) if name == "zrand0" else CONFIGS[name])
    grid = np.kron(sibal1.data, np.ones((2, 2), np.int8)).astype(np.int8)
    om = orc.OracleMap(grid, 0.025, sibal1.origin_x, sibal1.origin_y)
    assert om.max_range_px == 479
    ang = orc.beam_angles(angle_step=4)
    scan, _ = orc.cast_many(om, np.zeros(ang.size), np.zeros(ang.size), ang.astype(np.float64))
    scan = scan.astype(np.float32)
    n = 3000
    p = tracking_cloud(np.random.default_rng(3), n, sig=(1.0, 1.0, 0.5))
    e = make_engine(engine_mod, FineMap(grid, 0.025, sibal1.origin_x, sibal1.origin_y), ang, n, ray_kernel=engine_mod.RAYS_SWEEP, **k)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(scan)
    assert e.ray_kernel_name() == "k_rays_sweep"
    v = e.ray_kernel_variant()
    assert (v["hybrid"] if form == "hybrid" else v["global_fields"]), v
    L = oracle_table(orc, 479, k)
    want, _, _ = orc.eng_log_weights(om, p, ang, orc.obs_index(scan, om), L)
    assert_minus_inf_reached(L, want)
    assert np.isfinite(want).any()
    got = e.log_weights()
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {n} log-weights differ"
    assert_weights(orc, e, want, p)
    e.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_log_weights_literal_march(orc, engine_mod, spielberg, spielberg_oracle, name):
    from monte_carlo_localization_amd import synth
    k = sensor_cfg(name)
    ang = synth.beam_angles()
    n = 500
    e = make_engine(engine_mod, spielberg, ang, n, ray_kernel=engine_mod.RAYS_MARCH, **k)
    p = tracking_cloud(np.random.default_rng(8), n, sig=TRACK_SIG)
    e.set_particles(p, np.full(n, 1.0 / n))
    scan = scan_origin()
    e.sensor_update(scan)
    assert e.ray_kernel_name() == "k_rays_march"
    L = oracle_table(orc, spielberg_oracle.max_range_px, k)
    want, _, _ = orc.eng_log_weights(spielberg_oracle, p, ang, orc.obs_index(scan, spielberg_oracle), L)
    assert_minus_inf_reached(L, want)
    assert np.array_equal(e.log_weights(), want)
    assert_weights(orc, e, want, p)
    e.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_product_weights_61_beams(orc, engine_mod, spielberg, spielberg_oracle, name):
    """weight_mode PRODUCT (cpp:566-578 literally): the log-weights are still E4's, and the product weights are the reference's
    -- exactly 0 where a table entry is 0."""
    k = sensor_cfg(name)
    ang = orc.beam_angles(angle_step=18)
    assert ang.size == 61
    n = 2000
    e = make_engine(engine_mod, spielberg, ang, n, keep_ray_steps=1, weight_mode=engine_mod.WEIGHT_PRODUCT, **k)
    p = tracking_cloud(np.random.default_rng(9), n, sig=TRACK_SIG)
    e.set_particles(p, np.full(n, 1.0 / n))
    scan = scan_origin(18)
    e.sensor_update(scan)
    P = spielberg_oracle.max_range_px
    L = oracle_table(orc, P, k)
    want, _, _ = orc.eng_log_weights(spielberg_oracle, p, ang, orc.obs_index(scan, spielberg_oracle), L)
    assert_minus_inf_reached(L, want)
    assert np.array_equal(e.log_weights(), want)
    T = orc.sensor_table(P, k["z_hit"], k["z_short"], k["z_max"], k["z_rand"], k["sigma_hit"])
    wref, _, _ = orc.sensor_model(spielberg_oracle, p, ang, scan, T, inv_squash=1.0 / k["squash_factor"])
    got = e.get_weights()
    assert (got[np.isneginf(want)] == 0.0).all() and (wref[np.isneginf(want)] == 0.0).all()
    np.testing.assert_allclose(got, wref / wref.sum(), rtol=1e-12, atol=0)
    e.close()


# ---------------------------------------------------------------------------------------------- whole updates
class Checker:
    """Runs e.update and checks it against the oracle with the engine's sensor and motion parameters (the pattern of
    test_gpu_kld.Checker): resample indices, children, log-weights (with the carry of a kept update), weights, pose, N_eff."""

    def __init__(self, orc, om, e, ang, seed, mode, k, disp):
        self.orc, self.om, self.e, self.ang, self.seed, self.mode, self.disp = orc, om, e, ang, seed, mode, disp
        self.L = oracle_table(orc, om.max_range_px, k)
        self.p = e.get_particles()
        self.q = orc.eng_quantize_weights(e.get_weights())
        self.carry = None
        self.upd = 0
        self.log = []

    def step(self, scan):
        orc, e, n = self.orc, self.e, self.e.n
        e.update(ACTION, scan)
        _, resampled = e.effective_sample_size()
        idx = e.resample_indices()
        if resampled:
            if self.mode == 0:
                want = orc.eng_resample_indices(self.q, 0, n_children=n, k53=orc.eng_philox_k53(self.seed, self.upd, 0, n))
            else:
                want = orc.eng_resample_indices(self.q, 1, n_children=n, k0=orc.eng_philox_k0(self.seed, self.upd))
            assert np.array_equal(idx, want), f"update {self.upd}: {np.count_nonzero(idx != want)} of {n} parents differ"
        else:
            assert np.array_equal(idx, np.arange(n))
        parts = e.get_particles()
        want_parts = orc.motion_model(self.p[:, idx], ACTION, orc.eng_philox_normals(self.seed, self.upd, 0, n), disp=self.disp)
        np.testing.assert_allclose(parts, want_parts, rtol=1e-13, atol=1e-13)
        oi = orc.obs_index(scan, self.om)
        want_logw, _, _ = orc.eng_log_weights(self.om, parts, self.ang, oi, self.L)
        oracle_children, _, _ = orc.eng_log_weights(self.om, want_parts, self.ang, oi, self.L)
        if not resampled:
            want_logw = want_logw + self.carry
            oracle_children = oracle_children + self.carry
        lw = e.log_weights()
        assert np.array_equal(lw, want_logw), f"update {self.upd}: {np.count_nonzero(lw != want_logw)} of {n} log-weights differ"
        assert_weights(orc, e, want_logw, parts)
        _, self.q, mx = orc.eng_weights_from_log(want_logw)
        with np.errstate(invalid="ignore"):
            self.carry = np.where(np.isneginf(want_logw), -np.inf, want_logw - mx)
        t = e.stage_timings()
        path = "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")
        self.log.append((self.upd, e.ray_kernel_name(), bool(resampled), path))
        self.p = parts
        self.upd += 1
        return idx, oracle_children


def _engine_at(engine_mod, spielberg, n, seed, mode, k, disp, **extra):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed, resample_mode=mode, motion_dispersion_x=disp[0],
                    motion_dispersion_y=disp[1], motion_dispersion_theta=disp[2], **k, **extra)
    e.set_particles(tracking_cloud(np.random.default_rng(seed), n, sig=TRACK_SIG), np.full(n, 1.0 / n))
    return e, ang


@pytest.mark.parametrize("disp", [(0.2, 0.01, 0.05), (0.0, 0.0, 0.0)], ids=["disp_wide", "disp_zero"])
@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
def test_three_updates_with_own_sensor_and_motion_models(orc, engine_mod, spielberg, spielberg_oracle, disp, mode):
    """20 000 particles (k_rays_skip; the second and third updates replay the captured graph), z_rand 0 / sigma 2 / squash 3.1
    and dispersions of their own -- (0, 0, 0) makes every child a clone of its parent."""
    k = sensor_cfg(dict(z_rand=0.0, sigma_hit=2.0, squash_factor=3.1))
    n, seed = 20000, 11 + mode
    e, ang = _engine_at(engine_mod, spielberg, n, seed, mode, k, disp)
    c = Checker(orc, spielberg_oracle, e, ang, seed, mode, k, disp)
    scan = scan_origin()
    for _ in range(3):
        c.step(scan)
    assert [r[3] for r in c.log] == ["regular", "graph", "graph"], c.log        # (stage_timings: the graph reports no stage 4)
    if disp == (0.0, 0.0, 0.0):
        assert np.unique(c.p, axis=1).shape[1] < n            # clones
    e.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("n", [2000, 20000, 65536])
def test_all_impossible_update(orc, engine_mod, spielberg, spielberg_oracle, n, mode):
    """An update in which every particle's log-weight is -inf: every weight exactly 0, N_eff 0, the pose (0, 0, 0) exactly,
    and the next update draws parent 0 for every child; the update after that equals the oracle again.  2000 particles take
    the one-workgroup tail (k_tiny_tail), 20 000 the graph replay of k_rays_skip + k_weights, 65 536 k_rays_sweep."""
    k = sensor_cfg("zrand0_sigma2")
    disp = (0.05, 0.025, 0.25)
    seed = 21 + mode
    e, ang = _engine_at(engine_mod, spielberg, n, seed, mode, k, disp)
    c = Checker(orc, spielberg_oracle, e, ang, seed, mode, k, disp)
    scan, dead = scan_origin(), long_scan(spielberg, spielberg_oracle.max_range_px, ang.size)
    c.step(scan)
    _, children = c.step(dead)
    assert np.isneginf(children).all()                         # the precondition, on the oracle's own children
    assert np.isneginf(e.log_weights()).all()
    idx, _ = c.step(scan)
    assert (idx == 0).all()
    c.step(scan)
    paths, kernels = [r[3] for r in c.log], [r[1] for r in c.log]
    if n == 2000:
        assert paths[1:] == ["tiny"] * 3, c.log
    elif n == 20000:
        assert paths == ["regular", "graph", "graph", "graph"], c.log
    else:
        assert set(kernels) == {"k_rays_sweep"}, c.log
    e.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
def test_all_impossible_update_with_adaptive_resampling(orc, engine_mod, spielberg, spielberg_oracle, mode):
    """resample_neff_permille on (k_weights with the carry; no tiny tail, no graph): N_eff 0 after the impossible update forces
    the next draw (every parent 0).  With no motion noise its children are clones, so the next update keeps them (N_eff = N)
    and the one after that, kept as well, drives the clones out of the scan: every log-weight -inf through the carry, max -inf
    in k_weights.  The carry it leaves must be -inf, not NaN; then the next draw is parent 0 again, all equal to the oracle."""
    k = sensor_cfg("zrand0_sigma2")
    disp = (0.0, 0.0, 0.0)
    n, seed = 20000, 31 + mode
    e, ang = _engine_at(engine_mod, spielberg, n, seed, mode, k, disp, resample_neff_permille=500)
    c = Checker(orc, spielberg_oracle, e, ang, seed, mode, k, disp)
    scan, dead = scan_origin(), long_scan(spielberg, spielberg_oracle.max_range_px, ang.size)
    c.step(scan)
    c.step(dead)
    assert np.isneginf(e.log_weights()).all()
    idx, _ = c.step(scan)
    assert c.log[-1][2] and (idx == 0).all(), c.log
    for _ in range(3):
        c.step(scan)
    assert [r[2] for r in c.log] == [True, True, True, False, False, True], c.log
    assert np.isneginf(c.carry).all()                              # after the kept update in which every clone became impossible
    assert (e.resample_indices() == 0).all()
    e.close()


@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
def test_all_impossible_update_two_shard_group(orc, engine_mod, spielberg, spielberg_oracle, mode):
    """A 2-shard group on one device equals one engine through an impossible update and the draw after it."""
    k = sensor_cfg("zrand0_sigma2")
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n, seed = 20000, 41 + mode
    one = make_engine(engine_mod, spielberg, ang, n, seed=seed, resample_mode=mode, **k)
    grp = engine_mod.Group([0, 0], max_particles=n // 2, seed=seed, resample_mode=mode, **k)
    grp.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    grp.set_beam_angles(ang)
    p = tracking_cloud(np.random.default_rng(seed), n, sig=TRACK_SIG)
    one.set_particles(p, np.full(n, 1.0 / n))
    grp.set_particles(p, np.full(n, 1.0 / n))
    scan, dead = scan_origin(), long_scan(spielberg, spielberg_oracle.max_range_px, ang.size)
    for u, obs in enumerate((scan, dead, scan, scan)):
        one.update(ACTION, obs)
        grp.update(ACTION, obs)
        assert np.array_equal(grp.resample_indices(), one.resample_indices()), u
        assert np.array_equal(grp.get_particles(), one.get_particles()), u
        gw, ow = grp.get_weights(), one.get_weights()
        assert not np.isnan(gw).any() and not np.isnan(ow).any()
        if u == 1:
            assert np.array_equal(gw, np.zeros(n)) and np.array_equal(ow, np.zeros(n))
            assert np.array_equal(grp.expected_pose(), np.zeros(3)) and np.array_equal(one.expected_pose(), np.zeros(3))
        else:
            np.testing.assert_allclose(gw, ow, rtol=1e-13, atol=0)
            np.testing.assert_allclose(grp.expected_pose(), one.expected_pose(), rtol=0, atol=1e-12)
        if u == 2:
            assert (one.resample_indices() == 0).all()
    grp.close(); one.close()


@pytest.mark.parametrize("n", [2000, 20000, 65536])
def test_partly_impossible_update(orc, engine_mod, spielberg, spielberg_oracle, n):
    """About half of the cloud sees an impossible reading: the update is bit-exact, those particles carry weight 0, and the
    next draw takes none of them as a parent."""
    k = sensor_cfg("zrand0_sigma2")
    disp = (0.02, 0.01, 0.02)
    seed = 51
    e, ang = _engine_at(engine_mod, spielberg, n, seed, 0, k, disp)
    c = Checker(orc, spielberg_oracle, e, ang, seed, 0, k, disp)
    scan = scan_origin()
    _, children = c.step(scan)
    frac = np.isneginf(children).mean()
    assert 0.4 < frac < 0.7, frac
    lw = e.log_weights()
    dead = np.isneginf(lw)
    assert (e.get_weights()[dead] == 0.0).all() and (e.get_weights()[~dead] > 0.0).any()
    idx, _ = c.step(scan)
    assert not dead[idx].any()
    e.close()
