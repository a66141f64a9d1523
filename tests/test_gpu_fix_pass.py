"""k_rays_fix (levels 2 and 3 for the rays the ray kernel lists) in both of its deals (MCL_FIX_DEAL): the flat deal over the
segments' prefix and the deal per segment, each with one add per slot and wave.  debug_force_exact=2 sends EVERY ray of
k_rays_sweep through the fix-up list, so a ray lost at a ragged end, dealt twice, or added to the wrong slot shows up in the
count and in the log-weights, which are exact fp64 sums of fp32 table entries and are compared bit for bit
with the oracle's.  Through the C ABI; the oracle's result of a cloud is computed once and shared by the deals."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_engine, tracking_cloud

pytestmark = pytest.mark.gpu

DEALS = ["flat", "seg"]      # "seg" is what a launch with more segments than the prefix table holds takes
SIG = (0.2, 0.2, 0.4)          # keeps every particle inside its window: off_window_particles == 0, so the ray counts are exact


def scan1081():
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)


_ref = {}


def reference(orc, om, key, p, ang, obs, want_steps=False):
    """(logw, steps) of the oracle for this cloud, once per key"""
    if key not in _ref:
        L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
        logw, steps, _ = orc.eng_log_weights(om, p, ang, orc.obs_index(obs, om), L, want_steps=want_steps)
        _ref[key] = (logw, steps)
    return _ref[key]


def sensor(engine_mod, m, ang, p, obs, kernel=None, **cfg):
    n = p.shape[1]
    e = make_engine(engine_mod, m, ang, n, ray_kernel=engine_mod.RAYS_SWEEP if kernel is None else kernel, **cfg)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(obs)
    return e


def set_deal(monkeypatch, deal):
    monkeypatch.delenv("MCL_FIX_WG", raising=False)
    monkeypatch.setenv("MCL_FIX_DEAL", deal)


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("n", [1, 65, 2047, 2049])
def test_every_ray_through_the_fix_list(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, n, deal):
    """a ragged last wave, segments with no entries (at n = 1 nearly all of them)"""
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=1)
    p = tracking_cloud(np.random.default_rng(40 + n), n, sig=SIG)
    e = sensor(engine_mod, spielberg, ang, p, scan1081(), debug_force_exact=2)
    assert e.ray_kernel_name() == "k_rays_sweep"
    c, got = e.counters(), e.log_weights()
    e.close()
    print(n, deal, c)
    assert c["off_window_particles"] == 0
    assert c["level2_rays"] == n * ang.size
    assert np.array_equal(got, reference(orc, spielberg_oracle, ("all", n), p, ang, scan1081())[0])


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("step,beams", [(18, 61), (4, 271)])
def test_beam_counts_off_the_wave_grid(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, step, beams, deal):
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=step)
    assert ang.size == beams
    n = 2048
    obs = scan1081()[::step].copy()
    p = tracking_cloud(np.random.default_rng(50 + step), n, sig=SIG)
    e = sensor(engine_mod, spielberg, ang, p, obs, debug_force_exact=2)
    c, got = e.counters(), e.log_weights()
    e.close()
    assert c["off_window_particles"] == 0 and c["level2_rays"] == n * beams
    assert np.array_equal(got, reference(orc, spielberg_oracle, ("beams", step), p, ang, obs)[0])


@pytest.mark.parametrize("deal", DEALS)
def test_level_3_beyond_the_exact_list(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, deal):
    """debug_force_exact=1: every ray takes the literal march.  553 472 rays against the 65 536 entries of the exact list: the
    first 65 536 are k_rays_exact's, a wave each, the rest are marched by the lane of k_rays_fix that found them."""
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=1)
    n = 512
    assert n * ang.size > 65536
    p = tracking_cloud(np.random.default_rng(61), n, sig=SIG)
    e = sensor(engine_mod, spielberg, ang, p, scan1081(), debug_force_exact=1)
    c, got = e.counters(), e.log_weights()
    e.close()
    assert c["off_window_particles"] == 0
    assert c["exact_fallback_rays"] == n * ang.size
    assert np.array_equal(got, reference(orc, spielberg_oracle, ("l3", n), p, ang, scan1081())[0])


_nonfinite = {}


@pytest.mark.parametrize("deal", DEALS)
def test_non_finite_particles_among_finite_ones(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, deal):
    """NaN and +-inf in x, y and the heading of one particle in seven: the null wedge field, !sane, the march.  The finite
    particles and those with an infinite position equal the oracle's bit for bit.  A NaN coordinate, or a NaN or infinite
    heading (whose cosine is NaN), reaches the reference's `(int)` conversion of a NaN, which C leaves undefined (x86 gives
    INT_MIN, the device 0: tests/test_gpu_sweep.py leaves such particles out for that reason); those rows are held to one
    value across the deals instead."""
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=1)
    n = 2048
    p = tracking_cloud(np.random.default_rng(71), n, sig=SIG)
    bad = np.arange(3, n, 7)
    vals = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad):
        p[k % 3, i] = vals[(k // 3) % 3]
    has_nan = np.isnan(p).any(axis=0) | ~np.isfinite(p[2])
    e = sensor(engine_mod, spielberg, ang, p, scan1081(), debug_force_exact=2)
    got = e.log_weights()
    e.close()
    want = reference(orc, spielberg_oracle, ("nonfinite", n), p, ang, scan1081())[0]
    print("rows that differ from the oracle:", np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:16], "rows with a NaN in the march:", int(has_nan.sum()))
    assert np.array_equal(got[~has_nan], want[~has_nan])
    first = _nonfinite.setdefault("nan_rows", got[has_nan].copy())
    assert np.array_equal(got[has_nan].view(np.uint64), first.view(np.uint64))


@pytest.mark.parametrize("deal", DEALS)
def test_step_output(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, deal):
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=1)
    n = 512
    p = tracking_cloud(np.random.default_rng(81), n, sig=SIG)
    e = sensor(engine_mod, spielberg, ang, p, scan1081(), debug_force_exact=2, keep_ray_steps=1)
    c, got, steps = e.counters(), e.log_weights(), e.ray_steps()
    e.close()
    want, want_steps = reference(orc, spielberg_oracle, ("steps", n), p, ang, scan1081(), want_steps=True)
    assert c["level2_rays"] == n * ang.size
    assert np.array_equal(steps, want_steps), f"{(steps != want_steps).sum()} of {want_steps.size} ray steps differ"
    assert np.array_equal(got, want)


@pytest.mark.parametrize("deal", DEALS)
def test_two_updates_on_one_engine(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, deal):
    """every ray listed, then the usual few: nothing of the first launch's prefix or counters is left over"""
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=1)
    n = 3800                                  # 4 107 800 rays: the largest launch whose lists have room for every ray
    p = tracking_cloud(np.random.default_rng(91), n, sig=SIG)
    want = reference(orc, spielberg_oracle, ("two", n), p, ang, scan1081())[0]
    e = sensor(engine_mod, spielberg, ang, p, scan1081(), debug_force_exact=2)
    c = e.counters()
    assert c["level2_rays"] == n * ang.size and np.array_equal(e.log_weights(), want)
    e.set_debug_force_exact(0)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(scan1081())
    c, got = e.counters(), e.log_weights()
    e.close()
    print(deal, c)
    assert 0 < c["level2_rays"] < n * ang.size // 100
    assert np.array_equal(got, want)


@pytest.mark.parametrize("deal", DEALS)
@pytest.mark.parametrize("kernel", ["RAYS_CELL", "RAYS_QUAD"])
def test_legacy_library(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, kernel, deal):
    """the predecessors of k_rays_sweep list particle indices and append with memory-side atomics (slot_space == 0)"""
    set_deal(monkeypatch, deal)
    ang = orc.beam_angles(angle_step=1)
    n = 2048
    p = tracking_cloud(np.random.default_rng(101), n, sig=SIG)
    e = sensor(engine_mod, spielberg, ang, p, scan1081(), kernel=getattr(engine_mod, kernel), debug_force_exact=2)
    assert e.ray_kernel_name() == {"RAYS_CELL": "k_rays_cell", "RAYS_QUAD": "k_rays_quad"}[kernel]
    c, got = e.counters(), e.log_weights()
    e.close()
    assert c["level2_rays"] == n * ang.size
    assert np.array_equal(got, reference(orc, spielberg_oracle, ("legacy", n), p, ang, scan1081())[0])


def test_probe_count_is_the_same_for_both_deals(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch):
    ang = orc.beam_angles(angle_step=1)
    n = 512
    p = tracking_cloud(np.random.default_rng(111), n, sig=SIG)
    want = reference(orc, spielberg_oracle, ("probes", n), p, ang, scan1081())[0]
    probes = []
    for deal in DEALS:
        set_deal(monkeypatch, deal)
        e = sensor(engine_mod, spielberg, ang, p, scan1081(), debug_force_exact=2, debug_count_probes=1)
        c = e.counters()
        assert c["level2_rays"] == n * ang.size and np.array_equal(e.log_weights(), want)
        e.close()
        probes.append(c["probes"])
    print(probes)
    assert probes[0] > 0 and probes.count(probes[0]) == len(DEALS)
