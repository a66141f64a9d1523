"""KLD-adaptive particle count on the GPU (mcl_set_kld), through the C ABI on the Spielberg map: every update
of a run whose size the engine chooses is checked against the spec oracle at that size -- the drawn size against
mcl_host_kld_target of the previous count, the count against numpy over the drawn parents, the resample indices, the moved
children and sampled log-weights."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_engine
from test_kld_host import np_bins

pytestmark = pytest.mark.gpu

ACTION = (0.1, 0.0, 0.02)


class Checker:
    """Runs e.update and checks it against the oracle; keeps what the next update's check needs."""

    def __init__(self, orc, om, m, e, ang, scan, seed, mode, kld, rng, full_motion_max=8192):
        self.orc, self.om, self.m, self.e, self.ang, self.scan = orc, om, m, e, ang, scan
        self.seed, self.mode, self.kld, self.rng = seed, mode, kld, rng
        self.L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
        self.oi = orc.obs_index(scan, om)
        self.p = e.get_particles()
        self.q = orc.eng_quantize_weights(e.get_weights())
        self.upd = 0
        self.bins = -1
        self.full_motion_max = full_motion_max
        self.log = []

    def bins_of(self, p):
        m = self.m
        return np_bins(p[0], p[1], p[2], m.data.shape[1], m.data.shape[0], m.resolution, m.origin_x, m.origin_y, self.kld)

    def step(self, expect_kept=None):
        orc, e, n_par = self.orc, self.e, self.e.n
        bins_prev, n_next = e.kld_state()
        assert bins_prev == self.bins
        e.update(ACTION, self.scan)
        _, resampled = e.effective_sample_size()
        n = e.n
        assert n == e.particle_count()
        idx = e.resample_indices()
        if resampled:
            assert n == n_next, (self.upd, n, n_next)
            if self.mode == 0:
                want = orc.eng_resample_indices(self.q, 0, n_children=n, k53=orc.eng_philox_k53(self.seed, self.upd, 0, n))
            else:
                want = orc.eng_resample_indices(self.q, 1, n_children=n, k0=orc.eng_philox_k0(self.seed, self.upd))
            assert np.array_equal(idx, want), f"update {self.upd}: {np.count_nonzero(idx != want)} of {n} parents differ"
            assert idx.max() < n_par
        else:
            assert n == n_par and np.array_equal(idx, np.arange(n))
        bins, n_next_after = e.kld_state()
        assert bins == self.bins_of(self.p[:, idx]), self.upd             # the drawn parents' poses, before the motion model
        if resampled:
            assert n_next_after == self.orc_target(bins, n)
        else:
            assert n_next_after == n_next                                   # a kept update leaves the size alone
        parts = e.get_particles()
        sub = np.arange(n) if n <= self.full_motion_max else np.sort(self.rng.choice(n, 1024, replace=False))
        if sub.size == n:
            nrm = orc.eng_philox_normals(self.seed, self.upd, 0, n)
        else:
            nrm = np.concatenate([orc.eng_philox_normals(self.seed, self.upd, int(i), 1) for i in sub])
        np.testing.assert_allclose(parts[:, sub], orc.motion_model(self.p[:, idx[sub]], ACTION, nrm), rtol=1e-13, atol=1e-13)
        pick = np.arange(n) if n <= self.full_motion_max else np.sort(self.rng.choice(n, 512, replace=False))
        lw = e.log_weights()
        if resampled:
            logw, _, _ = orc.eng_log_weights(self.om, np.ascontiguousarray(parts[:, pick]), self.ang, self.oi, self.L)
            assert np.array_equal(lw[pick], logw), self.upd
        # the weights, the pose and N_eff the engine reports for the new set: the spec's, at the new size
        w, _, _ = orc.eng_weights_from_log(lw)
        np.testing.assert_allclose(e.expected_pose(), orc.expected_pose(parts, w / w.sum()), atol=1e-9)
        np.testing.assert_allclose(e.effective_sample_size()[0], w.sum() ** 2 / (w * w).sum(), rtol=1e-9)
        t = e.stage_timings()
        path = "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")
        self.log.append((self.upd, n_par, n, bins, e.ray_kernel_name(), bool(resampled), path))
        if expect_kept is not None:
            assert (not resampled) == expect_kept
        _, self.q, _ = orc.eng_weights_from_log(lw)
        self.p, self.bins = parts, bins
        self.upd += 1
        return n, bins

    def orc_target(self, bins, n):
        from monte_carlo_localization_amd import engine
        return engine.host_kld_target(self.kld, bins, n)


def _scan(n_beams_step=1):
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::n_beams_step].astype(np.float32)


@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
def test_shrinking_run_from_a_tracking_cloud(orc, engine_mod, spielberg, spielberg_oracle, mode):
    """65 536 particles (k_rays_sweep) shrink to a few thousand (k_rays_skip, then the three-launch path); every update equals
    the oracle at the size the engine chose."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n0, seed = 65536, 31 + mode
    e = make_engine(engine_mod, spielberg, ang, n0, seed=seed, resample_mode=mode)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(5), n0), np.full(n0, 1.0 / n0))
    k = e.set_kld(min_particles=256, max_particles=n0)
    assert e.kld_state() == (-1, n0)
    c = Checker(orc, spielberg_oracle, spielberg, e, ang, _scan(), seed, mode, k, np.random.default_rng(6))
    for _ in range(7):
        c.step()
    ns = [r[2] for r in c.log]
    kernels = [r[4] for r in c.log]
    assert ns[0] == n0 and kernels[0] == "k_rays_sweep", c.log
    assert min(ns) <= 8192 and "k_rays_skip" in kernels, c.log
    assert ns[-1] <= 8192, c.log
    e.close()


def test_growing_run_across_the_sort_switch(orc, engine_mod, spielberg, spielberg_oracle):
    """4096 particles spread over the map with a tight bound: the next draw jumps to 4 194 304 (across 65 536 and the
    counting-sort / rocPRIM switch at 3 000 000), then the peaked weights bring it back below 3M."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    cap, n0, seed = 4194304, 4096, 41
    e = make_engine(engine_mod, spielberg, ang, cap, seed=seed)
    e.set_particles(synth.global_cloud(np.random.default_rng(8), spielberg, n0), np.full(n0, 1.0 / n0))
    k = e.set_kld(min_particles=256, max_particles=cap, err=0.0003)
    c = Checker(orc, spielberg_oracle, spielberg, e, ang, _scan(), seed, 0, k, np.random.default_rng(9))
    for _ in range(3):
        c.step()
    ns = [r[2] for r in c.log]
    assert ns[0] == n0 and ns[1] == cap and ns[2] < 3000000, c.log
    assert c.log[1][4] == "k_rays_sweep"
    e.close()


def test_size_changes_never_replay_a_stale_graph(orc, engine_mod, spielberg, spielberg_oracle):
    """At <= 8192 particles with the default graph_mode, shrink_permille 1000 and round_to 64 change N on most updates: every
    update still equals the oracle (a graph or three-launch path built for another N would not)."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=9)
    n0, seed = 4096, 51
    e = make_engine(engine_mod, spielberg, ang, 8192, seed=seed)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(10), n0, sig=(0.3, 0.3, 0.3)), np.full(n0, 1.0 / n0))
    k = e.set_kld(min_particles=64, max_particles=8192, round_to=64, shrink_permille=1000)
    c = Checker(orc, spielberg_oracle, spielberg, e, ang, _scan(9), seed, 0, k, np.random.default_rng(11))
    for _ in range(12):
        c.step()
    ns = [r[2] for r in c.log]
    changes = sum(a != b for a, b in zip(ns, ns[1:]))
    assert changes >= 4 and len(set(ns)) >= 3, c.log
    assert all(r[4] == "k_rays_skip" for r in c.log)
    e.close()


def test_captured_graph_tail_between_8192_and_65536(orc, engine_mod, spielberg, spielberg_oracle):
    """8192 < N < 65536 on k_rays_skip: with N unchanged the update's tail is a captured graph, replayed with the resampling kernel
    and the clearing kernel launched in front of it (the count reaches word 17 through the graph's copy of the result block).
    First with the size pinned, then free to move inside the range: every update equals the oracle, and the graph path runs."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    n0, seed = 16384, 91
    e = make_engine(engine_mod, spielberg, ang, 65536, seed=seed)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(15), n0), np.full(n0, 1.0 / n0))
    k = e.set_kld(min_particles=n0, max_particles=n0)
    c = Checker(orc, spielberg_oracle, spielberg, e, ang, _scan(18), seed, 0, k, np.random.default_rng(16))
    for _ in range(5):
        c.step()
    c.kld = e.set_kld(min_particles=9216, max_particles=40960, round_to=1024, shrink_permille=500)
    c.bins = -1                                      # (mcl_set_kld: no count yet for the new configuration)
    for _ in range(6):
        c.step()
    assert all(8192 < r[2] < 65536 and r[4] == "k_rays_skip" for r in c.log), c.log
    assert sum(r[6] == "graph" for r in c.log[:5]) >= 3, c.log
    assert sum(r[6] == "graph" for r in c.log[5:]) >= 2, c.log
    e.close()


def test_adaptive_resampling_mixed_in(orc, engine_mod, spielberg, spielberg_oracle):
    """resample_neff_permille with KLD on: kept updates keep N and the size decision, and count the particles' own poses."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    n0, seed = 2048, 61
    e = make_engine(engine_mod, spielberg, ang, n0, seed=seed, resample_neff_permille=1)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(12), n0, sig=(0.2, 0.2, 0.1)), np.full(n0, 1.0 / n0))
    k = e.set_kld(min_particles=256, max_particles=n0, shrink_permille=0)
    c = Checker(orc, spielberg_oracle, spielberg, e, ang, _scan(18), seed, 0, k, np.random.default_rng(13))
    for _ in range(10):
        c.step()
    kinds = [r[5] for r in c.log]
    assert True in kinds and False in kinds, c.log
    e.close()


def _run_plain(engine_mod, spielberg, ang, scan, p0, seed, kld=None, off_after=False, updates=4):
    n0 = p0.shape[1]
    e = make_engine(engine_mod, spielberg, ang, n0, seed=seed)
    e.set_particles(p0, np.full(n0, 1.0 / n0))
    if kld is not None:
        e.set_kld(**kld)
        if off_after:
            e.set_kld(False)
    out = []
    for _ in range(updates):
        e.update(ACTION, scan)
        assert e.n == n0
        out.append((e.get_particles(), e.get_weights(), e.resample_indices(), e.expected_pose(), e.kld_state()))
    e.close()
    return out


@pytest.mark.parametrize("n0", [2000, 100000])
def test_off_means_off(engine_mod, spielberg, n0):
    """KLD never enabled, enabled then disabled, or on with min = max = N: N stays, bins_last is -1 unless counting, and the
    particles, weights, indices and pose are bit-identical to an engine that never heard of KLD."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=4)
    scan = _scan(4)
    p0 = synth.tracking_cloud(np.random.default_rng(14), n0)
    ref = _run_plain(engine_mod, spielberg, ang, scan, p0, 71)
    off = _run_plain(engine_mod, spielberg, ang, scan, p0, 71, kld=dict(max_particles=n0), off_after=True)
    pinned = _run_plain(engine_mod, spielberg, ang, scan, p0, 71, kld=dict(min_particles=n0, max_particles=n0))
    for a, b, c in zip(ref, off, pinned):
        for x, y, z in zip(a[:4], b[:4], c[:4]):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert a[4] == (-1, n0) and b[4] == (-1, n0)
        assert c[4][0] >= 1 and c[4][1] == n0


def test_refusals(engine_mod, spielberg):
    import ctypes as C
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    e = make_engine(engine_mod, spielberg, ang, 1024, seed=3)
    e.init_particles_pose((0.0, 0.0, 0.0), 1024)
    e.set_kld(max_particles=1024)
    obs = _scan(18)
    lib = e.lib
    assert lib.mcl_stage_rays(e._h, obs.ctypes.data_as(C.c_void_p), C.c_int32(obs.size)) == -5
    act = np.array(ACTION)
    assert lib.mcl_stage_keep(e._h, C.c_int64(0), C.c_int64(1024), act.ctypes.data_as(C.c_void_p)) == -5
    assert lib.mcl_stage_weights(e._h, C.c_double(0.0)) == -5
    assert lib.mcl_stage_finish(e._h, np.zeros(5).ctypes.data_as(C.c_void_p)) == -5
    assert "single-engine" in lib.mcl_last_error(e._h).decode()
    uid = (C.c_ubyte * 128)()
    assert lib.mcl_comm_create(e._h, uid, C.c_int32(1), C.c_int32(0)) == -5
    # off again: the update works as before
    e.set_kld(False)
    e.update(ACTION, obs)
    e.close()
    # an engine of a device group refuses KLD
    g = engine_mod.Group([0], max_particles=1024)
    ge = g.engine(0)
    with pytest.raises(engine_mod.EngineError) as ei:
        ge.set_kld(max_particles=1024)
    assert ei.value.status == -5
    g.close()


def test_global_relocalisation_shrinks(engine_mod, spielberg):
    """Global initialisation at 1 048 576 on Spielberg with the default KLD configuration (min_particles 256), a noise-free
    scan from a known pose, the robot standing still: within 30 updates N is at most 1/16 of the start and the expected pose
    within 0.25 m / 5 degrees of the truth.  The pose and seed are ones where the filter without KLD localises from the same
    cloud and scan too (checked first): whether a global initialisation finds the robot is decided by the first draw, with
    KLD as without it."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n0, truth = 1 << 20, np.array([-46.19, 29.66, -3.02])

    def err(e):
        pose = e.expected_pose()
        return np.hypot(*(pose[:2] - truth[:2])), abs((pose[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi)

    plain = make_engine(engine_mod, spielberg, ang, n0, seed=81)
    scan = synth.scan_from_pose(plain, spielberg, ang, truth)
    plain.init_global(n0)
    for _ in range(20):
        plain.update((0.0, 0.0, 0.0), scan)
    d, dth = err(plain)
    assert plain.n == n0 and d < 0.25 and dth < np.radians(5), (d, dth)      # the control: the fixture localises without KLD
    plain.close()
    e = make_engine(engine_mod, spielberg, ang, n0, seed=81)
    e.init_global(n0)
    e.set_kld()
    ns = []
    for _ in range(30):
        e.update((0.0, 0.0, 0.0), scan)
        ns.append(e.n)
        d, dth = err(e)
        if e.n <= n0 // 16 and d < 0.25 and dth < np.radians(5):
            break
    assert e.n <= n0 // 16, ns
    assert d < 0.25 and dth < np.radians(5), (d, dth, ns)
    assert min(ns) <= 1024, ns
    e.close()
