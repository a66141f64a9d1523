"""Beam skipping for the likelihood field on the GPU (mcl_set_beam_skip) against the numpy restatements
tests/beam_skip_ref.py and tests/lfield_ref.py: every used beam's agreement count within the ambiguity band of the restatement;
the mask, n_skipped and integrate_all exactly mcl_host_beam_skip_plan of the engine's own counts; every log-weight bit for bit
LF5 on the scan whose skipped beams read NaN; and BS5's identity against a twin engine without beam skipping that is fed that
scan -- through resampling, KLD and recovery.  The scan is the golden Spielberg scan with a sector shortened to 0.4 of its
ranges (an obstacle that is not in the map) plus odd_scan's readings that must not count."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import beam_skip_ref as br
from conftest import make_engine, tracking_cloud
from test_gpu_likelihood_field import ACTION, MAX_RANGE, SEED, Ambiguity, _angles, _scan, check_logw, edge_particles, odd_scan
from test_gpu_likelihood_field import sp_ref  # noqa: F401  (the module's fixture: Spielberg's field and table)
from whole_set import assert_same

pytestmark = pytest.mark.gpu

TIGHT, WIDE = (0.05, 0.05, 0.02), (0.5, 0.5, 0.4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constant(name):
    src = open(os.path.join(ROOT, "monte_carlo_localization_amd", "csrc", "mcl_lfield.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


def shorten(scan, lo=0.28, hi=0.39):
    s = scan.copy()
    s[int(lo * s.size):int(hi * s.size)] *= np.float32(0.4)
    return s


def obstacle_scan(step=1):
    return odd_scan(shorten(_scan(step)))


def used_mask(scan):
    r = np.asarray(scan, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (r >= 0.0) & (r < MAX_RANGE)


def cloud(rng, m, n, sig, edges=True):
    p = tracking_cloud(rng, n, sig=sig)
    k = n // 20 if edges else 0
    if k:
        p[:, :k] = edge_particles(rng, m, k)
    return p


def start(engine_mod, m, ang, p0, skip=True, max_particles=None, **cfg):
    n = p0.shape[1]
    e = make_engine(engine_mod, m, ang, max_particles or n, seed=SEED, **cfg)
    e.set_likelihood_field()
    if skip is not False:
        e.set_beam_skip(**(skip if isinstance(skip, dict) else {}))
    e.set_particles(p0, np.full(n, 1.0 / n))
    return e


def masked(scan, st):
    """the scan whose skipped beams read NaN (BS5)"""
    s = np.asarray(scan, np.float32).copy()
    s[st["kept"] == 2] = np.nan
    return s


def check_counts(engine_mod, e, ref, m, ang, scan, tally, **fields):
    """BS1-BS4 and BS6 after an update of e with `scan`: the counts within the restatement's band, everything else exactly the
    host calls' of the engine's own counts; returns the state"""
    st = e.beam_skip_state()
    parts = e.get_particles()
    n, used = parts.shape[1], used_mask(scan)
    nu = int(used.sum())
    ka, mc, ms = engine_mod.host_beam_skip_thresholds(m.resolution, n, nu, **fields)
    assert ka == br.Ka_of(engine_mod.default_beam_skip_config(**fields).distance_m, m.resolution)
    assert (st["n_particles"], st["n_used"], st["ka"], st["min_count"], st["min_skipped"]) == (n, nu, ka, mc, ms)
    lo, hi, amb = br.counts(parts, ang, scan, ref["D"], ka, m.resolution, m.origin_x, m.origin_y, MAX_RANGE)
    cu = st["counts"][used]
    bad = np.flatnonzero((cu < lo) | (cu > hi))
    assert bad.size == 0, (bad[:5], cu[bad[:5]], lo[bad[:5]], hi[bad[:5]])
    assert not st["counts"][~used].any() and not st["kept"][~used].any()
    tally.amb += amb
    tally.beams += n * nu
    kept, n_skipped, integrate_all = engine_mod.host_beam_skip_plan(cu, n, **fields)
    assert np.array_equal(st["kept"][used], kept)
    assert (st["n_skipped"], st["integrate_all"], st["n_kept"]) == (n_skipped, integrate_all, int((kept == 1).sum()))
    return st


def check_update(engine_mod, e, ref, m, ang, scan, tallies, **fields):
    """check 1: counts, mask and every log-weight (LF5 on the masked scan, the existing bit-for-bit check with alternatives)"""
    st = check_counts(engine_mod, e, ref, m, ang, scan, tallies[0], **fields)
    check_logw(e, ref, m, ang, masked(scan, st), tallies[1])
    return st


def same_filter(a, b, what=""):
    assert a.n == b.n
    assert_same(what + "particles", a.get_particles(), b.get_particles())
    assert_same(what + "log-weights", a.log_weights(), b.log_weights())
    assert_same(what + "weights", a.get_weights(), b.get_weights())
    assert_same(what + "resample indices", a.resample_indices(), b.resample_indices())
    assert_same(what + "expected pose", a.expected_pose(), b.expected_pose())
    assert a.effective_sample_size() == b.effective_sample_size()


# ---- 1. counts, mask, log-weights after sensor_update
@pytest.mark.parametrize("n,step", [(1, 1), (65, 1), (257, 1), (2000, 1), (8193, 1), (65536, 18)])
@pytest.mark.parametrize("sig", [TIGHT, WIDE], ids=["tight", "wide"])
def test_counts_mask_and_log_weights(engine_mod, spielberg, sp_ref, n, step, sig):
    m, ang, scan = spielberg, _angles(step), obstacle_scan(step)
    e = start(engine_mod, m, ang, cloud(np.random.default_rng(n + int(100 * sig[0])), m, n, sig))
    tallies = Ambiguity(), Ambiguity()
    e.sensor_update(scan)
    st = check_update(engine_mod, e, sp_ref, m, ang, scan, tallies)
    if sig == TIGHT and n >= 2000:                     # the obstacle is skipped and nothing else is
        lo, hi = int(0.28 * scan.size), int(0.39 * scan.size)
        sector = np.zeros(scan.size, bool)
        sector[lo:hi] = True
        used = used_mask(scan)
        far = used & (scan > 0.5)                      # (odd_scan's two zero readings end at the particle itself)
        assert (st["kept"][far & sector] == 2).all() and (st["kept"][far & ~sector] == 1).all() and st["integrate_all"] == 0
    for t in tallies:
        t.check()
    e.close()


# ---- 2. full updates: the set that is counted is the resampled, moved one
@pytest.mark.parametrize("n,step,sig", [(2000, 1, TIGHT), (2000, 1, WIDE), (65536, 18, TIGHT)], ids=["2000-tight", "2000-wide", "65536x61"])
@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
def test_full_updates(engine_mod, spielberg, sp_ref, n, step, sig, mode):
    m, ang, scan = spielberg, _angles(step), obstacle_scan(step)
    e = start(engine_mod, m, ang, cloud(np.random.default_rng(7 * n + mode), m, n, sig), resample_mode=mode)
    tallies = Ambiguity(), Ambiguity()
    for _ in range(2):
        e.update(ACTION, scan)
        check_update(engine_mod, e, sp_ref, m, ang, scan, tallies)
        t = e.stage_timings()
        assert t[3] > 0.0 and sum(t[:5]) <= t[5] + 1e-3, t
        assert e.ray_kernel_ms() > 0.0
    for t in tallies:
        t.check()
    e.close()


# ---- 3. the identity (BS5)
def run_identity(engine_mod, m, ang, scans, p0, kld=False, rec=False, sensor_only=False, max_particles=None, **cfg):
    """A with skipping on; B with it off, fed A's scan with A's skipped beams NaN: the same filter after every update.  Returns
    the states of A."""
    a = start(engine_mod, m, ang, p0, max_particles=max_particles, **cfg)
    b = start(engine_mod, m, ang, p0, skip=False, max_particles=max_particles, **cfg)
    for e in (a, b):
        if kld:
            e.set_kld(min_particles=256, max_particles=p0.shape[1])
        if rec:
            e.set_recovery()
    states = []
    for k, scan in enumerate(scans):
        a.sensor_update(scan) if sensor_only else a.update(ACTION, scan)
        st = a.beam_skip_state()
        fed = masked(scan, st)
        b.sensor_update(fed) if sensor_only else b.update(ACTION, fed)
        same_filter(a, b, f"update {k}: ")
        if kld:
            assert a.particle_count() == b.particle_count() and a.kld_state() == b.kld_state()
        if rec:
            ra, rb = a.recovery_state(), b.recovery_state()
            assert_same("recovery averages", np.array(ra[:3]), np.array(rb[:3]))
            assert ra[3] == rb[3]
        states.append(st)
    a.close()
    b.close()
    return states


@pytest.mark.parametrize("kld,rec", [(False, False), (True, False), (False, True)], ids=["plain", "kld", "recovery"])
def test_identity_with_the_masked_scan(engine_mod, spielberg, kld, rec):
    n, m, ang, scan = 8193, spielberg, _angles(), obstacle_scan()
    p0 = cloud(np.random.default_rng(31), m, n, TIGHT)
    states = run_identity(engine_mod, m, ang, [scan] * 3, p0, kld=kld, rec=rec)
    assert all(0 < st["n_kept"] < st["n_used"] for st in states), [(st["n_kept"], st["n_used"]) for st in states]


# ---- 4. nothing skipped, everything integrated, nothing kept
def one_update_each(engine_mod, m, ang, scan, p0, updates=2, **fields):
    """(state of the engine with skipping on) after `updates` updates of it and of a twin with skipping off, which must be the
    same filter; the motion noise is kept small (the reference's 0.25 rad of heading noise would widen the tight cloud)"""
    quiet = dict(motion_dispersion_x=0.01, motion_dispersion_y=0.01, motion_dispersion_theta=0.01)
    a, b = start(engine_mod, m, ang, p0, skip=fields, **quiet), start(engine_mod, m, ang, p0, skip=False, **quiet)
    for k in range(updates):
        for e in (a, b):
            e.update(ACTION, scan)
        same_filter(a, b, f"update {k}: ")
    st = a.beam_skip_state()
    a.close()
    b.close()
    return st


def test_nothing_skipped_is_the_plain_update(engine_mod, spielberg):
    n, m, ang, scan = 8193, spielberg, _angles(), _scan()
    st = one_update_each(engine_mod, m, ang, scan, cloud(np.random.default_rng(41), m, n, TIGHT, edges=False))
    assert st["n_kept"] == st["n_used"] == int(used_mask(scan).sum()) and st["n_skipped"] == 0 and st["integrate_all"] == 0


def test_error_threshold_zero_integrates_all(engine_mod, spielberg):
    n, m, ang, scan = 8193, spielberg, _angles(), obstacle_scan()
    st = one_update_each(engine_mod, m, ang, scan, cloud(np.random.default_rng(42), m, n, TIGHT, edges=False), error_threshold=0.0)
    used = used_mask(scan)
    sector = used.copy()
    sector[:int(0.28 * scan.size)] = sector[int(0.39 * scan.size):] = False
    assert sector.sum() > 100 and (st["counts"][sector] < st["min_count"]).all()          # the sector still disagrees
    assert st["integrate_all"] == 1 and st["min_skipped"] == 0 and st["n_kept"] == st["n_used"] and (st["kept"][used] == 1).all()
    assert st["n_skipped"] >= int(sector.sum())


def test_too_many_skipped_integrates_all(engine_mod, spielberg):
    """95 % of the beams shortened: the default error_threshold 0.9 is reached, every used beam is summed.  (One update: what
    resampling on those weights makes of the set is another scenario.)"""
    n, m, ang = 8193, spielberg, _angles()
    scan = odd_scan(shorten(_scan(), 0.0, 0.95))
    st = one_update_each(engine_mod, m, ang, scan, cloud(np.random.default_rng(43), m, n, TIGHT, edges=False), updates=1)
    assert st["n_skipped"] >= st["min_skipped"] > 0.89 * st["n_used"]
    assert st["integrate_all"] == 1 and st["n_kept"] == st["n_used"]


def test_threshold_one_keeps_nothing(engine_mod, spielberg):
    n, m, ang, scan = 8193, spielberg, _angles(), obstacle_scan()
    e = start(engine_mod, m, ang, cloud(np.random.default_rng(44), m, n, TIGHT), skip=dict(threshold=1.0, error_threshold=2.0))
    e.update(ACTION, scan)
    st = e.beam_skip_state()
    assert st["min_count"] == n + 1 and st["n_kept"] == 0 and st["n_skipped"] == st["n_used"] and st["integrate_all"] == 0
    assert_same("log-weights", e.log_weights(), np.zeros(n))
    w = e.get_weights()
    assert (w == w[0]).all() and abs(w.sum() - 1.0) < 1e-9
    e.close()


# ---- 5. off means off
def test_off_means_off(engine_mod, spielberg):
    n, m, ang, scan = 8193, spielberg, _angles(), obstacle_scan()
    p0 = cloud(np.random.default_rng(51), m, n, TIGHT)
    never, toggled = start(engine_mod, m, ang, p0, skip=False), start(engine_mod, m, ang, p0)
    for e in (never, toggled):
        with pytest.raises(engine_mod.EngineError) as ei:       # off / before the first update
            e.beam_skip_state()
        assert ei.value.status == -2
    toggled.set_beam_skip(False)
    with pytest.raises(engine_mod.EngineError) as ei:
        toggled.beam_skip_state()
    assert ei.value.status == -2
    for k in range(3):
        for e in (never, toggled):
            e.update(ACTION, scan)
        same_filter(toggled, never, f"update {k}: ")
    # on for one update (which `never` follows on the masked scan, BS5), off again: the next updates skip nothing
    toggled.set_beam_skip()
    toggled.update(ACTION, scan)
    st = toggled.beam_skip_state()
    assert st["n_skipped"] > 0 and st["integrate_all"] == 0
    never.update(ACTION, masked(scan, st))
    toggled.set_beam_skip(False)
    with pytest.raises(engine_mod.EngineError) as ei:
        toggled.beam_skip_state()
    assert ei.value.status == -2
    for k in range(3, 6):
        for e in (never, toggled):
            e.update(ACTION, scan)
        same_filter(toggled, never, f"update {k}: ")
    never.close()
    toggled.close()


# ---- 6. the slow counter path: more used beams than the LDS counter row holds
def test_global_counter_path(engine_mod, spielberg, sp_ref):
    m, n = spielberg, 257
    B = kernel_constant("kBsLdsBeams") + 401             # (some 4 % of the beams see nothing within max range)
    ang = np.linspace(-0.75 * np.pi, 0.75 * np.pi, B).astype(np.float32)
    p0 = cloud(np.random.default_rng(61), m, n, TIGHT)
    e = start(engine_mod, m, ang, p0)
    scan = shorten(e.expected_scans((0.0, 0.0, 0.0))[0])
    assert int(used_mask(scan).sum()) > kernel_constant("kBsLdsBeams")
    tallies = Ambiguity(), Ambiguity()
    e.sensor_update(scan)
    st = check_update(engine_mod, e, sp_ref, m, ang, scan, tallies)
    assert 0 < st["n_kept"] < st["n_used"]
    e.update(ACTION, scan)
    check_update(engine_mod, e, sp_ref, m, ang, scan, tallies)
    for t in tallies:
        t.check()
    e.close()
    run_identity(engine_mod, m, ang, [scan] * 3, p0)


# ---- 7. more than one tile per workgroup
def test_persistent_workgroups_walk_several_tiles(engine_mod, spielberg, sp_ref):
    """The counting pass runs min(tiles, CUs * kBsWorkgroupsPerCu) workgroups over tiles of 256 particles.  n = CUs *
    kBsWorkgroupsPerCu * 256 + 513 (524 801 on the 256 CUs of an MI355X): every workgroup has one tile, the first two a second,
    the third a second one of a single particle.  Counts against the restatement; log-weights by the identity against a twin."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * kernel_constant("kBsWorkgroupsPerCu") * 256 + 513
    m, ang, scan = spielberg, _angles(18), obstacle_scan(18)
    p0 = cloud(np.random.default_rng(71), m, n, TIGHT)
    a, b = start(engine_mod, m, ang, p0), start(engine_mod, m, ang, p0, skip=False)
    tally = Ambiguity()
    a.sensor_update(scan)
    st = check_counts(engine_mod, a, sp_ref, m, ang, scan, tally)
    assert 0 < st["n_kept"] < st["n_used"]
    b.sensor_update(masked(scan, st))
    assert_same("log-weights", a.log_weights(), b.log_weights())
    assert_same("weights", a.get_weights(), b.get_weights())
    tally.check()
    a.close()
    b.close()


# ---- 8. update_scan with a stride
def test_update_scan_with_a_stride(engine_mod, spielberg, sp_ref):
    n, m, ang = 8192, spielberg, _angles(18)
    raw = obstacle_scan(1)
    raw[18 * np.arange(8)] = [np.nan, np.inf, -1.0, MAX_RANGE, 0.0, 3.25, MAX_RANGE + 2.0, -np.inf]
    strided = raw[::18].copy()
    p0 = cloud(np.random.default_rng(81), m, n, TIGHT)
    a, b = start(engine_mod, m, ang, p0), start(engine_mod, m, ang, p0)
    tallies = Ambiguity(), Ambiguity()
    for k in range(2):
        a.update_scan(ACTION, raw, 18)
        b.update(ACTION, strided)
        same_filter(a, b, f"update {k}: ")
        sa, sb = a.beam_skip_state(), b.beam_skip_state()
        assert sa["counts"].size == ang.size                    # the engine's beams, not the raw scan's
        for key in sa:
            assert np.array_equal(sa[key], sb[key]), key
        st = check_update(engine_mod, a, sp_ref, m, ang, strided, tallies)
        assert 0 < st["n_kept"] < st["n_used"]
    for t in tallies:
        t.check()
    a.close()
    b.close()


# ---- 9. refusals
def test_refusals(engine_mod, spielberg):
    m, ang = spielberg, _angles(18)
    obs = obstacle_scan(18)
    e = make_engine(engine_mod, m, ang, 1024, seed=3)
    with pytest.raises(engine_mod.EngineError) as ei:           # the field is off
        e.set_beam_skip()
    assert ei.value.status == -2
    e.set_beam_skip(False)                                      # switching it off is always fine
    e.set_likelihood_field()
    bad = [dict(distance_m=0.0), dict(distance_m=-1.0), dict(distance_m=math.nan), dict(distance_m=math.inf), dict(threshold=-0.1),
           dict(threshold=1.5), dict(threshold=math.nan), dict(error_threshold=-0.5), dict(error_threshold=math.nan),
           dict(error_threshold=math.inf), dict(reserved=(0, 1))]
    for b in bad:
        with pytest.raises(engine_mod.EngineError) as ei:
            e.set_beam_skip(**b)
        assert ei.value.status == -1, b
    e.init_particles_pose((0.0, 0.0, 0.0), 1024)
    e.set_beam_skip()
    lib = e.lib
    assert lib.mcl_stage_rays(e._h, obs.ctypes.data_as(C.c_void_p), C.c_int32(obs.size)) == -5
    assert lib.mcl_stage_weights(e._h, C.c_double(0.0)) == -5
    assert lib.mcl_stage_finish(e._h, np.zeros(5).ctypes.data_as(C.c_void_p)) == -5
    e.update(ACTION, obs)
    st = e.beam_skip_state()
    assert st["n_used"] == int(used_mask(obs).sum())
    assert lib.mcl_get_beam_skip_state(e._h, None, None, C.c_size_t(ang.size), None) == 0       # every output may be NULL
    assert lib.mcl_get_beam_skip_state(e._h, None, None, C.c_size_t(ang.size + 1), None) == -1
    e.set_likelihood_field()                                    # re-setting the field keeps beam skipping
    e.update(ACTION, obs)
    assert e.beam_skip_state()["n_used"] == st["n_used"]
    e.set_likelihood_field(False)                               # switching the field off clears it
    with pytest.raises(engine_mod.EngineError) as ei:
        e.beam_skip_state()
    assert ei.value.status == -2
    e.set_likelihood_field()
    e.update(ACTION, obs)
    with pytest.raises(engine_mod.EngineError) as ei:           # still off
        e.beam_skip_state()
    assert ei.value.status == -2
    e.close()
