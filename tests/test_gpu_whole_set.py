"""Every particle of every update against the spec oracle (tests/whole_set.py) at the sizes where the production paths run and
just either side of each path switch: the radix ordering at 4M, BASELINE config #1, the sort switch at 3 000 000, the sweep switch
at 65 536 particles x 2^23 rays, the one-workgroup tail at 8 192, relocalisation clouds (bucket cuts on Spielberg, the far pass of
the long-range hybrid walk), the long-range walk on the 0.025 m map, and an update no particle survives.  Each case asserts the
path it took, so that a moved threshold fails the test instead of quietly testing another path.  Spielberg unless stated, default
configuration through AUTO, no MCL_* switch set."""
import os

import numpy as np
import pytest

import whole_set as ws
from conftest import GOLDEN, make_engine
from test_gpu_sensor_configs import TRACK_SIG, long_scan, oracle_table, sensor_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


def _scan(step=1):
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32).copy()


def _tracking(n, seed, sig=(0.5, 0.5, 0.4)):
    from monte_carlo_localization_amd import synth
    return synth.tracking_cloud(np.random.default_rng(seed), n, sig=sig)


def _from_set(orc, om, e, ang, p, seed, mode=0, L=None):
    """set_particles with uniform weights; the engine must hold exactly the set it was given"""
    n = p.shape[1]
    w = np.full(n, 1.0 / n)
    e.set_particles(p, w)
    ws.assert_same("set_particles", e.get_particles(), p)
    return ws.WholeSet(orc, om, e, ang, seed, p, orc.eng_quantize_weights(w), mode=mode, L=L, rng=np.random.default_rng(seed))


def _kernels(c, name):
    return all(r["kernel"] == name and r["planned"] == name for r in c.log)


def test_headline_4m_radix_ordering(orc, engine_mod, spielberg, spielberg_oracle):
    """4 194 304 x 271 beams: k_rays_sweep with the radix ordering; the second update draws from the compact list."""
    from monte_carlo_localization_amd import synth
    n, seed = 4194304, 7
    assert n >= ws.RADIX_MIN
    ang = synth.beam_angles(angle_step=4)
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed)
    c = _from_set(orc, spielberg_oracle, e, ang, _tracking(n, 1), seed)
    for _ in range(2):
        c.step(_scan(4))
    assert _kernels(c, "k_rays_sweep"), c.log
    assert c.log[1]["compact_used"], c.log
    e.close()


def test_config1_systematic(orc, engine_mod, spielberg, spielberg_oracle):
    """BASELINE config #1: 262 144 x 1081 beams, systematic resampling; k_rays_sweep with the counting sort, the compact list
    from the second update on."""
    from monte_carlo_localization_amd import synth
    n, seed = 262144, 8
    assert n < ws.RADIX_MIN
    ang = synth.beam_angles()
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed, resample_mode=1)
    c = _from_set(orc, spielberg_oracle, e, ang, _tracking(n, 2), seed, mode=1)
    for _ in range(3):
        c.step(_scan())
    assert _kernels(c, "k_rays_sweep"), c.log
    assert all(r["compact_used"] for r in c.log[1:]), c.log
    e.close()


@pytest.mark.parametrize("n", [ws.RADIX_MIN - 1, ws.RADIX_MIN])
def test_sort_switch(orc, engine_mod, spielberg, spielberg_oracle, n):
    """61 beams either side of the counting-sort / radix-sort switch (`n >= 3000000` in mcl_engine.hip)."""
    from monte_carlo_localization_amd import synth
    seed = 9
    ang = synth.beam_angles(angle_step=18)
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed)
    c = _from_set(orc, spielberg_oracle, e, ang, _tracking(n, 3), seed)
    for _ in range(2):
        c.step(_scan(18))
    assert _kernels(c, "k_rays_sweep"), c.log
    e.close()


@pytest.mark.parametrize("n,beams,kernel", [(65535, 128, "k_rays_skip"), (65536, 127, "k_rays_skip"), (65536, 128, "k_rays_sweep"),
                                            (65537, 128, "k_rays_sweep")])
def test_sweep_switch(orc, engine_mod, spielberg, spielberg_oracle, n, beams, kernel):
    """AUTO takes k_rays_sweep from 65 536 particles and 2^23 rays: one particle or one beam short of either stays on k_rays_skip."""
    from monte_carlo_localization_amd import synth
    seed = 10
    assert (n >= ws.SWEEP_MIN_PARTICLES and n * beams >= ws.SWEEP_MIN_RAYS) == (kernel == "k_rays_sweep")
    ang = synth.beam_angles(angle_step=8)[:beams].copy()
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed)
    assert e.planned_ray_kernel(n)[0] == kernel
    c = _from_set(orc, spielberg_oracle, e, ang, _tracking(n, 4), seed)
    for _ in range(2):
        c.step(_scan(8)[:beams].copy())
    assert _kernels(c, kernel), c.log
    e.close()


@pytest.mark.parametrize("n,path", [(ws.TINY_TAIL_MAX, "tiny"), (ws.TINY_TAIL_MAX + 1, "graph")])
def test_tail_switch(orc, engine_mod, spielberg, spielberg_oracle, n, path):
    """From the device's Gaussian initialisation, 61 beams: the one-workgroup tail up to 8 192 particles, the captured graph above,
    from the second update on."""
    from monte_carlo_localization_amd import synth
    seed, pose = 11, (0.0, 0.0, 0.0)
    ang = synth.beam_angles(angle_step=18)
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed)
    e.init_particles_pose(pose, n)
    p0 = e.get_particles()
    ws.assert_close("init_particles_pose", p0, orc.eng_init_pose(seed, 0, pose, 0, n), 1e-13, 1e-13)   # Box-Muller: device libm
    c = ws.WholeSet(orc, spielberg_oracle, e, ang, seed, p0, orc.eng_quantize_weights(np.full(n, 1.0 / n)), rng=np.random.default_rng(seed))
    for _ in range(3):
        c.step(_scan(18))
    assert [r["path"] for r in c.log[1:]] == [path, path], c.log
    assert _kernels(c, "k_rays_skip"), c.log
    e.close()


def test_relocalisation_bucket_cuts(orc, engine_mod, spielberg, spielberg_oracle):
    """1 048 576 particles from the device's global initialisation (free cell corners, cpp:438-439), 61 beams: k_rays_sweep, and on
    Spielberg the spread cloud needs no far pass -- its sorted units are cut at the bucket borders and each fits its LDS window."""
    from monte_carlo_localization_amd import synth
    n, seed = 1 << 20, 12
    ang = synth.beam_angles(angle_step=18)
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed)
    e.init_global(n)
    p0 = e.get_particles()
    ws.assert_same("init_global", p0, orc.eng_init_global(seed, 0, spielberg_oracle, 0, n))
    c = ws.WholeSet(orc, spielberg_oracle, e, ang, seed, p0, orc.eng_quantize_weights(np.full(n, 1.0 / n)), rng=np.random.default_rng(seed))
    for _ in range(2):
        c.step(_scan(18))
    assert _kernels(c, "k_rays_sweep"), c.log
    assert all(r["counters"]["off_window_particles"] == 0 for r in c.log), c.log
    e.close()


def test_relocalisation_long_range_far_pass(orc, engine_mod, maps_mod, spielberg):
    """262 144 particles from the device's global initialisation on the 0.025 m map, 271 beams: the fresh set takes the global-field
    form of k_rays_sweep and hands part of the fresh cloud to the far pass; the next update takes the hybrid walk."""
    from monte_carlo_localization_amd import synth
    fine = maps_mod.synthetic_fine025(spielberg)
    om = orc.OracleMap(fine.data, fine.resolution, fine.origin_x, fine.origin_y)
    n, seed = 262144, 15
    ang = synth.beam_angles(angle_step=4)
    e = make_engine(engine_mod, fine, ang, n, seed=seed)
    scan = synth.scan_from_pose(e, fine, ang, (0.0, 0.0, 0.0))
    e.init_global(n)
    p0 = e.get_particles()
    ws.assert_same("init_global", p0, orc.eng_init_global(seed, 0, om, 0, n))
    c = ws.WholeSet(orc, om, e, ang, seed, p0, orc.eng_quantize_weights(np.full(n, 1.0 / n)), rng=np.random.default_rng(seed))
    for _ in range(2):
        c.step(scan)
    assert _kernels(c, "k_rays_sweep"), c.log
    forms = [("hybrid" if r["variant"]["hybrid"] else "global" if r["variant"]["global_fields"] else "lds") for r in c.log]
    assert forms == ["global", "hybrid"], c.log
    assert c.log[0]["counters"]["off_window_particles"] > 0, c.log
    e.close()


def test_long_range_fine025(orc, engine_mod, maps_mod, spielberg):
    """262 144 x 271 beams on the 0.025 m map (MAX_RANGE_PX 479): the just-loaded set takes the global-field form of k_rays_sweep,
    the updates after it the hybrid walk."""
    from monte_carlo_localization_amd import synth
    fine = maps_mod.synthetic_fine025(spielberg)
    om = orc.OracleMap(fine.data, fine.resolution, fine.origin_x, fine.origin_y)
    assert om.max_range_px == 479
    n, seed = 262144, 13
    ang = synth.beam_angles(angle_step=4)
    e = make_engine(engine_mod, fine, ang, n, seed=seed)
    scan = synth.scan_from_pose(e, fine, ang, (0.0, 0.0, 0.0))
    c = _from_set(orc, om, e, ang, _tracking(n, 5), seed)
    for _ in range(3):
        c.step(scan)
    assert _kernels(c, "k_rays_sweep"), c.log
    forms = [("hybrid" if r["variant"]["hybrid"] else "global" if r["variant"]["global_fields"] else "lds") for r in c.log]
    assert forms == ["global", "hybrid", "hybrid"], c.log
    e.close()


def test_impossible_scan(orc, engine_mod, spielberg, spielberg_oracle):
    """z_rand = 0 (sigma 2) and a scan no particle can explain, 65 536 x 128 beams (k_rays_sweep): every log-weight -inf, Q = 0
    (DESIGN E5), all weights, sums and the pose 0, and every sample_particles draw is particle 0."""
    from monte_carlo_localization_amd import synth
    k = sensor_cfg("zrand0_sigma2")
    n, seed = 65536, 14
    ang = synth.beam_angles(angle_step=8)[:128].copy()
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed, **k)
    L = oracle_table(orc, spielberg_oracle.max_range_px, k)
    c = _from_set(orc, spielberg_oracle, e, ang, _tracking(n, 6, sig=TRACK_SIG), seed, L=L)
    c.step(long_scan(spielberg, spielberg_oracle.max_range_px, ang.size))
    assert np.isneginf(e.log_weights()).all()
    assert c.log[0]["q_total"] == 0
    assert np.array_equal(e.scalars()[[1, 3, 4, 5, 6, 7]], np.zeros(6))
    s = e.sample_particles(ws.SAMPLE_K)
    assert np.array_equal(s, np.repeat(c.p[:, :1], ws.SAMPLE_K, axis=1))
    assert _kernels(c, "k_rays_sweep"), c.log
    e.close()
