"""The ordering gather of the radix path reads ONE record per particle: from the second update of a set on the resampling kernel
leaves (heading, 0, pixel x, pixel y) in the constants' buffer instead of (cos, sin, pixel x, pixel y), and k_sort_gather takes the
sincos of the same argument with the same function (csrc/mcl_ray_core.h: particle_heading_record, particle_constants_of).  Nothing
behind the gather may see a difference: log-weights, resample indices and particles are, bit for bit, those of an engine that
orders by the counting sort (MCL_SORT=hist: full-form constants throughout) and the oracle's; the order read back is a permutation
sorted by the host twin's keys; and Engine.sort_record_form says which form each update's gather read -- 'full' on the first
update of a set (k_sort_keys makes its keys) and on an update that injects children (recovery: no keys from the resampling
kernel), 'heading' otherwise.  65 536 particles x 181 beams on the Spielberg fixture with MCL_SORT=radix, the smallest set that
takes k_rays_sweep through the library sort (tests/test_gpu_sort_fine.py); three updates each, so that the heading form runs twice."""
import math

import numpy as np
import pytest

from conftest import make_engine, tracking_cloud
from test_gpu_sort_fine import check_order, scan181

pytestmark = pytest.mark.gpu
N, STEP, SEED = 65536, 6, 12
ACTION = (0.05, 0.0, 0.01)
UPDATES = 3
NAN_ROWS_X, NAN_ROWS_TH = (5, 1024, 40000), (6, 1023, 65535)      # children whose injected normals are NaN (x / heading)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def cloud_of(kind, m):
    from monte_carlo_localization_amd import synth
    n = 66001 if kind == "ragged" else N                  # ragged: the last workgroup of the gather is not full
    if kind in ("tracking", "ragged", "nan"):
        p = tracking_cloud(np.random.default_rng(8), n)
        if kind == "nan":                                  # garbage rows in the set itself: fine bits 0, NaN pixels, the far path
            p[0, 3] = np.nan; p[1, 4] = np.inf; p[2, 7] = np.nan; p[2, 9] = 1e9
        return p
    if kind == "uniform":                                  # runs of length one: whole buckets, units cut at their borders
        p = synth.global_cloud(np.random.default_rng(9), m, n)
        p[:2] += np.random.default_rng(99).uniform(0.1, 0.9, (2, n)) * float(np.float32(m.resolution))
        return p
    assert kind == "one-cell"                              # one quarter cell, one heading bin: one run of equal keys across every block
    res = float(np.float32(m.resolution))
    rng = np.random.default_rng(11)
    cx, cy = math.floor((0.0 - m.origin_x) / res), math.floor((0.0 - m.origin_y) / res)
    p = np.empty((3, n))
    p[0] = m.origin_x + (cx + 0.05 + 0.15 * rng.random(n)) * res
    p[1] = m.origin_y + (cy + 0.05 + 0.15 * rng.random(n)) * res
    p[2] = 1e-3 * rng.random(n)
    return p


def normals_of(kind, u, n):
    """injected normals of update u (None: the engine's own Philox draws).  'nan': NaN rows from the second update on, so that
    the resampling kernel itself makes children with a NaN position or heading and leaves them in the heading form"""
    if kind != "nan" or u == 0:
        return None
    nrm = np.random.default_rng(100 + u).standard_normal((n, 3))
    nrm[list(NAN_ROWS_X), 0] = np.nan
    nrm[list(NAN_ROWS_TH), 2] = np.nan
    return nrm


_runs = {}


def run(engine_mod, m, ang, kind, sort, monkeypatch, tag=None, setup=None, before=None, spread_ok=False, cell=False):
    """[(logw, idx, particles)] and the forms of UPDATES updates from the cloud, the radix order checked after each; once per setting"""
    key = (kind, sort, tag)
    if key in _runs:
        return _runs[key]
    monkeypatch.setenv("MCL_SORT", sort)
    monkeypatch.delenv("MCL_SORT_FINE", raising=False)
    monkeypatch.delenv("MCL_SORT_FINE_SUB", raising=False)
    p0 = cloud_of(kind, m)
    n = p0.shape[1]
    cfg = dict(ray_kernel=engine_mod.RAYS_CELL) if cell else {}        # (k_rays_cell: the legacy build of the library)
    e = make_engine(engine_mod, m, ang, n, seed=SEED, **cfg)
    e.set_particles(p0, np.full(n, 1.0 / n))
    if setup:
        setup(e, n)
    out, forms = [], []
    for u in range(UPDATES):
        if before:
            before(e, u)
        e.update(ACTION, scan181(), normals=normals_of(kind, u, n))
        swept = e.ray_kernel_name() == ("k_rays_cell" if cell else "k_rays_sweep")
        assert swept or spread_ok                           # (children injected all over the map: the engine may run the
        if not swept:                                        #  stage with k_rays_skip, which works from full-form constants)
            forms.append(None)
        elif sort == "radix":
            check_order(engine_mod, e, m, None)              # a permutation, keys non-decreasing and the host twin's
            forms.append(e.sort_record_form())
        else:
            with pytest.raises(engine_mod.EngineError):      # the counting sort: no radix order, full-form constants
                e.sort_record_form()
        out.append((e.log_weights(), e.resample_indices(), e.get_particles()))
    e.close()
    _runs[key] = out, forms
    return _runs[key]


@pytest.mark.parametrize("kind", ["tracking", "one-cell", "uniform", "ragged", "nan"])
def test_results_are_the_counting_sorts(orc, engine_mod, spielberg, monkeypatch, kind):
    ang = orc.beam_angles(angle_step=STEP)
    got, forms = run(engine_mod, spielberg, ang, kind, "radix", monkeypatch)
    want, _ = run(engine_mod, spielberg, ang, kind, "hist", monkeypatch)
    # the first update's keys are k_sort_keys' and its constants k_particle_prep's; then the resampling kernel writes both
    assert forms == ["full"] + ["heading"] * (UPDATES - 1)
    for u in range(UPDATES):
        for a, b, what in zip(got[u], want[u], ("log-weights", "resample indices", "particles")):
            assert same(a, b), (kind, u, what)
    if kind == "nan":
        p = got[1][2]                                        # the children of the second update: NaN where the normals were
        assert np.isnan(p[0, list(NAN_ROWS_X)]).all() and np.isnan(p[2, list(NAN_ROWS_TH)]).all()


def test_results_are_the_oracles(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch):
    """as tests/test_gpu_sort_fine.py holds them: exact fp64 sums bit for bit, the draw of an update from the weights of the one
    before (multinomial, Philox stream of that update) -- here also for the third update, whose parents met the gather in the
    heading form"""
    ang = orc.beam_angles(angle_step=STEP)
    got, _ = run(engine_mod, spielberg, ang, "tracking", "radix", monkeypatch)
    L = orc.eng_log_table(orc.sensor_table(spielberg_oracle.max_range_px))
    oi = orc.obs_index(scan181(), spielberg_oracle)
    logw1, _, p1 = got[0]
    want1, _, _ = orc.eng_log_weights(spielberg_oracle, p1, ang, oi, L)
    assert np.array_equal(logw1, want1)
    prev = want1
    pick = np.random.default_rng(10).choice(N, 6000, replace=False)
    for u in (1, 2):
        logw, idx, p = got[u]
        _, q, _ = orc.eng_weights_from_log(prev)
        assert np.array_equal(idx, orc.eng_resample_indices(q, 0, n_children=N, k53=orc.eng_philox_k53(SEED, u, 0, N)))
        want, _, _ = orc.eng_log_weights(spielberg_oracle, p[:, pick], ang, oi, L)
        assert np.array_equal(logw[pick], want)
        prev = logw
    assert len(np.unique(got[1][1])) < N // 2                # the sets behind the first update are collapsed ones


def test_cell_kernel_keeps_the_full_form(orc, engine_mod, spielberg, monkeypatch):
    """k_rays_cell orders through the same radix path, but its fix-up and far kernels read (cos, sin) from the constants' buffer
    by particle index: it never gets the heading form.  Three updates with MCL_SORT=radix equal the counting sort's, and
    k_rays_sweep's, bit for bit."""
    ang = orc.beam_angles(angle_step=STEP)
    got, forms = run(engine_mod, spielberg, ang, "tracking", "radix", monkeypatch, tag="cell", cell=True)
    want, _ = run(engine_mod, spielberg, ang, "tracking", "hist", monkeypatch, tag="cell", cell=True)
    sweep, _ = run(engine_mod, spielberg, ang, "tracking", "radix", monkeypatch)
    assert forms == ["full"] * UPDATES
    for u in range(UPDATES):
        for a, b, c, what in zip(got[u], want[u], sweep[u], ("log-weights", "resample indices", "particles")):
            assert same(a, b) and same(a, c), (u, what)


def kld_pinned(e, n):
    e.set_kld(min_particles=n, max_particles=n)              # pinned: every update draws n children through k_resample_motion_kld


def recovery_on(e, n):
    e.set_recovery()


def recovery_kld(e, n):
    e.set_recovery()
    e.set_kld(min_particles=n, max_particles=n)


@pytest.mark.parametrize("form", ["kld", "recovery", "mixture", "recovery-kld"])
def test_other_resampling_kernels_leave_the_same_record(orc, engine_mod, spielberg, monkeypatch, form):
    """The KLD instantiation writes the heading form too; an update that injects children (free cells or a pose mixture, with
    and without KLD counting) writes no keys, so its constants keep the full form.  Either way: the counting sort's results."""
    ang = orc.beam_angles(angle_step=STEP)

    def before(e, u):
        if form == "kld" or u == 0:
            return
        if form == "mixture":
            e.set_recovery_proposal(np.array([[0.0, 0.0, 0.0], [0.3, -0.2, 0.1]]),
                                    np.array([np.diag([0.01, 0.01, 0.01]), np.diag([0.02, 0.02, 0.04])]))
        e.set_recovery_state(0.0, math.log1p(-0.3))          # p = 0.3 for this update
        assert abs(e.recovery_state()[2] - 0.3) < 1e-12

    setup = {"kld": kld_pinned, "recovery": recovery_on, "mixture": recovery_on, "recovery-kld": recovery_kld}[form]
    how = dict(tag=form, setup=setup, before=before, spread_ok=form.startswith("recovery"))
    got, forms = run(engine_mod, spielberg, ang, "tracking", "radix", monkeypatch, **how)
    want, _ = run(engine_mod, spielberg, ang, "tracking", "hist", monkeypatch, **how)
    if form == "kld":
        assert forms == ["full", "heading", "heading"]
    else:
        assert forms[0] == "full" and all(f in ("full", None) for f in forms[1:]) and (form != "mixture" or None not in forms)
    for u in range(UPDATES):
        for a, b, what in zip(got[u], want[u], ("log-weights", "resample indices", "particles")):
            assert same(a, b), (form, u, what)
    if form != "kld":
        assert (got[1][1] == -1).sum() > N // 8 and (got[2][1] == -1).sum() > N // 8       # both later updates injected
