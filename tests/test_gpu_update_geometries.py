"""The filter's own stages on the GPU over the geometry family of tests/side_geometries.py (and its 120 x 90 map): whole updates on
each tail and ray-kernel form against the spec oracle on every particle (tests/whole_set.py), the initialisers, the odometry motion
models, the KLD bin count and a free-running KLD run, the pose clusters, recovery from free cells and from a mixture, and the
pruned global search -- each held to its CPU statement (the oracle, numpy, tests/*_ref.py) on maps whose row width, size,
resolution, coordinate magnitude and content the two real maps of the other tests never vary.  tests/test_update_geometries_host.py
holds the statements themselves to the host library on the same maps first.

The only engine-to-engine comparisons are the two the statements leave open: the children an injecting update does not inject
against an engine with recovery off, and the pruned search's hits against mcl_global_search's (held to tests/lfield_ref.py on these
maps by tests/test_gpu_side_geometries.py).

Every comparison is integer-exact or bit-exact but those the project already bounds: whole_set.sum_rel_bound, clusters_ref.chain,
1e-13 for children that went through the device's libm.  One bound is stated here in a form of its own, `held_rel`: see there."""
import math
import os

import numpy as np
import pytest

import clusters_ref as R
import motion_ref as mr
import recovery_mix_ref as mix
import search_pruned_ref as pr
import side_geometries as sg
import whole_set as ws
from conftest import make_engine
from side_geometries import bits
from test_gpu_clusters import check as check_clusters, read_q
from test_gpu_kld import Checker
from test_gpu_motion_model import assert_poses
from test_kld_host import np_bins, np_target
from test_recovery_host import child_draws, free_cells, injected_poses, threshold

pytestmark = pytest.mark.gpu

ALL = sg.NAMES + ("small",)
SEED = 0x5EED_0000_0000_0031 + 2025
N_HEAD = 5
FIRST = 3
RTOL = 1e-13


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


class Case:
    """a geometry, its oracle map, its beams and scans (made once per geometry, left unchanged)"""

    def __init__(self, engine_mod, orc, g):
        self.g, self.orc, self.mod = g, orc, engine_mod
        self.om = g.oracle(orc)
        self.P = self.om.max_range_px
        self.ang = sg.angles(orc, 61)
        self.ang128 = orc.beam_angles(angle_step=8)[:128].copy()                # evenly spaced: the hybrid form needs that
        self.obs = g.scan(orc, self.ang)
        self.odd = sg.odd_scan(self.obs)
        self.obs128 = g.scan(orc, self.ang128)
        self.odd128 = sg.odd_scan(self.obs128)
        self.L = orc.eng_log_table(orc.sensor_table(self.P))
        self.free = free_cells(g.data)
        self.action = (g.res, 0.0, 0.01)
        self.geom = dict(W=g.W, H=g.H, res=g.resolution, ox=g.origin_x, oy=g.origin_y)
        for a in (self.ang, self.ang128, self.obs, self.odd, self.obs128, self.odd128, self.L):
            a.setflags(write=False)

    def logw(self, parts, ang=None, scan=None):
        ang, scan = (self.ang, self.obs) if ang is None else (ang, scan)
        return self.orc.eng_log_weights(self.om, np.ascontiguousarray(parts), ang, self.orc.obs_index(scan, self.om), self.L)[0]

    def np_bins(self, p, k):
        g = self.g
        return np_bins(p[0], p[1], p[2], g.W, g.H, g.resolution, g.origin_x, g.origin_y, k)


_CASES = {}


def case_of(name, engine_mod, orc):
    if name not in _CASES:
        _CASES[name] = Case(engine_mod, orc, sg.small() if name == "small" else sg.family()[name])
    return _CASES[name]


@pytest.fixture(scope="module", params=ALL)
def cx(request, engine_mod, orc):
    return case_of(request.param, engine_mod, orc)


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def form_of(variant):
    return "hybrid" if variant["hybrid"] else "global" if variant["global_fields"] else "lds"


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def held_rel(what, got, want, centre):
    """The initialisers add a draw to a mean: x = mean + L n, one rounding of the sum, with L n through the device's log, sqrt and
    sincos (a few ulp of L n, where numpy's differ).  The project's rule is 1e-13 relative to the coordinate; that form is sound
    while the coordinate is not much smaller than the draw.  Where mean and draw cancel (a cloud of 0.5 m around a pose 0.09 m from
    the map's origin) the coordinate is smaller than the draw's own ulps, and the sound form is relative to the larger operand:
    |got - want| <= 1e-13 max(|want|, |want - mean|).  No absolute term: at (4096.3, -8191.7) this is 4e-10 m, at a coordinate and
    draw of 1 mm it is 1e-16 m.  Headings are compared modulo 2 pi.  Returns how many coordinates the first form alone would
    have failed."""
    got, want = np.asarray(got), np.asarray(want)
    centre = np.asarray(centre, np.float64).reshape(3, -1)
    assert got.shape == want.shape
    d = got - want
    d[2] = (d[2] + math.pi) % (2 * math.pi) - math.pi
    draw = want - centre
    draw[2] = (draw[2] + math.pi) % (2 * math.pi) - math.pi
    scale = np.maximum(np.abs(want), np.abs(draw))
    bad = np.flatnonzero((~(np.abs(d) <= RTOL * scale)).any(axis=0))
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), got[:, bad[:5]].tolist(), want[:, bad[:5]].tolist())
    return int((~(np.abs(d) <= RTOL * np.abs(want))).sum())


# ---- 1. whole-set updates: every particle of every update against the oracle
def whole_set_chain(cx, e, ang, scans, seed, p0, mode=0):
    n = p0.shape[1]
    w = np.full(n, 1.0 / n)
    e.set_particles(p0, w)
    ws.assert_same("set_particles", e.get_particles(), p0)
    c = ws.WholeSet(cx.orc, cx.om, e, ang, seed, p0, cx.orc.eng_quantize_weights(w), mode=mode, L=cx.L, action=cx.action,
                    rng=np.random.default_rng(seed & 0xFFFF), sample_k=min(ws.SAMPLE_K, n // 2))
    for scan in scans:
        c.step(scan)
    return c


def assert_planned(cx, c, what):
    for r in c.log:
        assert r["kernel"] == r["planned"], (what, r)


@pytest.mark.parametrize("n,mode,path", [(2000, 0, "tiny"), (2000, 1, "tiny"), (16384, 0, "graph")])
def test_whole_set_on_the_small_tails(cx, n, mode, path):
    """k_rays_skip with the one-workgroup tail (2000) and the captured graph (16 384), 61 beams, from a cloud of 4 cells around the
    true pose: on tiny and one_free much of it lies in walls and off the map"""
    g = cx.g
    p0 = sg.cloud_around(g, np.random.default_rng(n + mode), n)
    wall, off = sg.cloud_shares(cx.om, p0)
    e = make_engine(cx.mod, g, cx.ang, n, seed=SEED + n + mode, resample_mode=mode)
    c = whole_set_chain(cx, e, cx.ang, (cx.obs, cx.obs, cx.odd), SEED + n + mode, p0, mode)
    print(f"{g.name}: {n} x 61 mode {mode}: start {wall:.3f} in walls, {off:.3f} off the map; paths {[r['path'] for r in c.log]}, kernel {c.log[0]['kernel']}")
    assert_planned(cx, c, "small tails")
    assert all(r["kernel"] == "k_rays_skip" for r in c.log), c.log
    assert [r["path"] for r in c.log[1:]] == [path, path], c.log
    e.close()


def sweep_record(cx, e, c, what):
    g = cx.g
    kernel, why = e.planned_ray_kernel(e.n)
    forms = [form_of(r["variant"]) if r["kernel"] == "k_rays_sweep" else "-" for r in c.log]
    print(f"{g.name}: {what}: P {cx.P}: kernels {[r['kernel'] for r in c.log]}, forms {forms}, paths {[r['path'] for r in c.log]}, "
          f"off-window particles {[r['counters']['off_window_particles'] for r in c.log]}, "
          f"literal-march rays {[r['counters']['exact_fallback_rays'] for r in c.log]}; plan: {why}")
    return forms


def test_whole_set_at_the_sweep_switch(cx):
    """65 536 x 128 evenly spaced beams through AUTO: k_rays_sweep where the plan allows it, in the form the range asks for"""
    g, n = cx.g, 65536
    assert n >= ws.SWEEP_MIN_PARTICLES and n * 128 >= ws.SWEEP_MIN_RAYS
    p0 = sg.cloud_around(g, np.random.default_rng(128), n)
    e = make_engine(cx.mod, g, cx.ang128, n, seed=SEED + 128)
    c = whole_set_chain(cx, e, cx.ang128, (cx.obs128, cx.obs128, cx.odd128), SEED + 128, p0)
    forms = sweep_record(cx, e, c, "65536 x 128 AUTO")
    assert_planned(cx, c, "AUTO")
    kernel = c.log[0]["kernel"]
    assert [r["path"] for r in c.log[1:]] == ["regular" if kernel == "k_rays_sweep" else "graph"] * 2, c.log
    if g.name == "fine":
        assert cx.P == 600 and kernel == "k_rays_sweep" and all(f in ("hybrid", "global") for f in forms), c.log
    if g.name == "coarse":
        assert cx.P == 48 and kernel == "k_rays_sweep" and forms == ["lds"] * 3, c.log
    if cx.P <= 243:
        assert kernel == "k_rays_sweep" and all(f == "lds" for f in forms), c.log
    e.close()


def test_forced_sweep_steps_are_cast_ray(cx):
    """MCL_RAYS_SWEEP with keep_ray_steps at 65 536 x 128: every stored step of the second update is the oracle's cast_ray (the scan
    does not change a ray), and the chain is the oracle's on every particle"""
    g, n = cx.g, 65536
    p0 = sg.cloud_around(g, np.random.default_rng(129), n)
    e = make_engine(cx.mod, g, cx.ang128, n, seed=SEED + 129, ray_kernel=cx.mod.RAYS_SWEEP, keep_ray_steps=1)
    assert e.planned_ray_kernel(n)[0] == "k_rays_sweep", e.planned_ray_kernel(n)
    c = whole_set_chain(cx, e, cx.ang128, (cx.obs128, cx.odd128), SEED + 129, p0)
    sweep_record(cx, e, c, "65536 x 128 forced sweep")
    assert all(r["kernel"] == "k_rays_sweep" for r in c.log), c.log
    parts = e.get_particles()
    a = (parts[2][:, None] + cx.ang128.astype(np.float64)[None, :]).ravel()
    want = cx.orc.cast_many(cx.om, np.repeat(parts[0], 128), np.repeat(parts[1], 128), a, use_omp=True)[1].reshape(n, 128)
    got = e.ray_steps().astype(np.int32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), want[tuple(bad[:5].T)].tolist())
    e.close()


def test_whole_set_from_a_global_start(cx):
    """65 536 x 128 from mcl_init_global: a uniform cloud, every particle on a cell corner, on maps smaller than an LDS window --
    the far pass and the fix-up lists"""
    g, n = cx.g, 65536
    seed = SEED + 130
    e = make_engine(cx.mod, g, cx.ang128, n, seed=seed)
    e.init_global(n)
    p0 = e.get_particles()
    ws.assert_same("init_global", p0, cx.orc.eng_init_global(seed, 0, cx.om, 0, n))
    res = g.res
    assert np.array_equal(p0[0], np.round((p0[0] - g.origin_x) / res) * res + g.origin_x)        # corners: col res + origin
    c = ws.WholeSet(cx.orc, cx.om, e, cx.ang128, seed, p0, cx.orc.eng_quantize_weights(np.full(n, 1.0 / n)), L=cx.L, action=cx.action,
                    rng=np.random.default_rng(130))
    for scan in (cx.obs128, cx.odd128):
        c.step(scan)
    sweep_record(cx, e, c, "65536 x 128 from init_global")
    assert_planned(cx, c, "global start")
    e.close()


# ---- 2. the initialisers
def test_init_global(cx):
    g, n = cx.g, 10000
    seed = SEED + 2
    e = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    e.init_global(n)
    p = e.get_particles()
    ws.assert_same("init_global", p, cx.orc.eng_init_global(seed, 0, cx.om, 0, n))
    assert same_bits(e.get_weights(), np.full(n, 1.0 / n))
    col, row = sg.oracle_cells(cx.om, p[0], p[1])
    assert (g.data[row, col] == 0).all()
    if g.name == "one_free":
        assert np.unique(p[0]).size == 1 and np.unique(p[1]).size == 1 and np.unique(p[2]).size > n // 2
    else:
        assert np.unique(row * g.W + col).size > min(cx.free.size, n) // 4
    # a shard of a second initialisation: rows 2500 .. 7499 of a set of 10 000, drawn with the next init counter
    e.init_global(5000, first_global_index=2500, n_total=n)
    assert e.n == 5000
    ws.assert_same("init_global, sharded", e.get_particles(), cx.orc.eng_init_global(seed, 1, cx.om, 2500, 5000))
    e.close()


def small_cov(g):
    """a full covariance with a spread of half a cell and 0.05 rad"""
    s = 0.5 * g.res
    return np.array([[s * s, 0.3 * s * s, 0.002 * s], [0.3 * s * s, 0.8 * s * s, -0.001 * s], [0.002 * s, -0.001 * s, 0.0025]])


def test_init_pose_gaussian_mixture(cx):
    g, n = cx.g, 4096
    seed = SEED + 3
    e = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    pose = np.array(g.true_pose)
    e.init_particles_pose(pose, n)
    strict = held_rel("init_particles_pose", e.get_particles(), cx.orc.eng_init_pose(seed, 0, pose, 0, n), pose[:, None])
    cov = small_cov(g)
    e.init_particles_gaussian(pose, cov, n)
    strict += held_rel("init_particles_gaussian", e.get_particles(), mr.init_gaussian(seed, 1, pose, cov, 0, n), pose[:, None])
    assert same_bits(e.get_weights(), np.full(n, 1.0 / n))
    # two components: the true pose and its mirror image; rows [0, 1500) are the first's, rows [1500, 4096) the second's
    means = np.array([pose, sg.mirrored_pose(g)])
    covs = np.array([cov, np.diag([(2 * g.res) ** 2, g.res ** 2, 0.0])])         # (the second without heading uncertainty)
    counts = np.array([1500, n - 1500])
    e.init_particles_mixture(means, covs, counts)
    got = e.get_particles()
    want = np.concatenate([mr.init_gaussian(seed, 2, means[0], covs[0], 0, n)[:, :1500], mr.init_gaussian(seed, 2, means[1], covs[1], 0, n)[:, 1500:]], axis=1)
    centre = np.concatenate([np.tile(means[0][:, None], (1, 1500)), np.tile(means[1][:, None], (1, n - 1500))], axis=1)
    strict += held_rel("init_particles_mixture", got, want, centre)
    assert same_bits(got[2, 1500:], np.full(n - 1500, means[1, 2]))
    print(f"{g.name}: initialisers: {strict} of {9 * n} coordinates lie outside 1e-13 of the coordinate alone (cancellation)")
    # an update runs on it
    e.update(cx.action, cx.obs)
    assert np.array_equal(e.log_weights(), cx.logw(e.get_particles()))
    e.close()


# ---- 3. the odometry motion models
@pytest.mark.parametrize("model", ["diff", "omni"])
@pytest.mark.parametrize("name", ["far_origin", "coarse", "tiny"])
def test_motion_models(engine_mod, orc, name, model):
    cx = case_of(name, engine_mod, orc)
    g, n = cx.g, 4096
    seed = SEED + 4
    action = (2 * g.res, 0.0, 0.02) if model == "diff" else (2 * g.res, 0.4 * g.res, 0.02)
    e = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    p0 = sg.cloud_around(g, np.random.default_rng(4), n)
    e.set_particles(p0, np.full(n, 1.0 / n))
    e.set_motion_model(model)
    e.update(action, cx.obs)
    idx = e.resample_indices()
    parts = e.get_particles()
    assert_poses(parts, mr.sample(model, action, p0[:, idx], cx.orc.eng_philox_normals(seed, 0, 0, n)), f"{g.name} {model}")
    assert np.array_equal(e.log_weights(), cx.logw(parts))
    e.close()


# ---- 4. KLD
@pytest.mark.parametrize("form", ["default", "cell"])
@pytest.mark.parametrize("n", [4096, 65536])
def test_kld_bin_count(cx, n, form):
    """min_particles = max_particles = n: the count after an update is np_bins of the drawn parents"""
    g = cx.g
    seed = SEED + 5
    e = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    p0 = sg.cloud_around(g, np.random.default_rng(n), n)
    e.set_particles(p0, np.full(n, 1.0 / n))
    k = e.set_kld(min_particles=n, max_particles=n, **sg.kld_forms(g)[form])
    assert e.kld_state() == (-1, n)
    parents = p0
    for upd in range(2):
        e.update(cx.action, cx.obs)
        idx = e.resample_indices()
        drawn = parents[:, idx]
        want = cx.np_bins(drawn, k)
        got = e.kld_state()
        print(f"{g.name}: n {n}, {form} bins, grid {sg.kld_grid(g, k)}: update {upd} occupies {got[0]} bins")
        assert got == (want, n), (upd, got, want)
        parents = e.get_particles()
    if g.name == "tiny" and form == "default":
        assert sg.kld_grid(g, k) == (1, 1) and got[0] <= 37
    e.close()


class NumpyChecker(Checker):
    def orc_target(self, bins, n):
        return np_target(self.kld, bins, n)


def test_kld_free_running(cx):
    """from 16 384 down: every update's size is np_target of the previous count, and its indices, children and log-weights the
    oracle's at that size"""
    g, n0 = cx.g, 16384
    seed = SEED + 6
    e = make_engine(cx.mod, g, cx.ang, n0, seed=seed)
    e.set_particles(sg.cloud_around(g, np.random.default_rng(6), n0), np.full(n0, 1.0 / n0))
    k = e.set_kld(min_particles=256, max_particles=n0)
    c = NumpyChecker(cx.orc, cx.om, g, e, cx.ang, cx.obs, seed, 0, k, np.random.default_rng(7), full_motion_max=n0)
    for _ in range(4):
        c.step()
    print(f"{g.name}: free-running KLD: (update, parents, n, bins, kernel, resampled, path) {c.log}")
    ns = [r[2] for r in c.log]
    assert ns[0] == n0 and all(256 <= v <= n0 for v in ns)
    e.close()


# ---- 5. clusters
def moment_ratios(e, got, geom, K=16):
    """the worst deviation of the first K clusters' means and covariances in units of test_gpu_clusters.check's bounds"""
    p = e.get_particles()
    q = read_q(e, p.shape[1])
    ref, _, _ = R.clusters(p[0], p[1], p[2], q, geom["W"], geom["H"], geom["res"], geom["ox"], geom["oy"], moments_of=K)
    worst = np.zeros(2)
    for d, c in zip(got, ref):
        W, i = float(np.float64(c["weight_q"])), c["members"]
        h = R.chain(i.size)
        for j in range(2):
            worst[0] = max(worst[0], abs(d["mean"][j] - c["mean"][j]) / ((h + 2) * R.U * c["A1"][j] / W + 4 * R.U * abs(c["mean"][j])))
        S2, A2 = R.second_moments(p[0][i], p[1][i], p[2][i], q[i], d["mean"])
        dev = d["cov"].ravel()[[0, 1, 2, 4, 5, 8]]
        for j in range(6):
            b = (h + 6) * R.U * A2[j] / W + 4 * R.U * abs(S2[j] / W)
            if b > 0:
                worst[1] = max(worst[1], abs(dev[j] - S2[j] / W) / b)
    return worst


def test_pose_clusters(cx):
    g, n = cx.g, 4096
    seed = SEED + 7
    e = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    e.init_global(n)
    got, info, _ = check_clusters(e, cx.geom)
    assert info["n_clusters"] >= 1
    worst = moment_ratios(e, got, cx.geom)
    # two modes: the true pose and its mirror image, a cell of spread each
    rng = np.random.default_rng(8)
    p0 = np.concatenate([sg.cloud_around(g, rng, n // 2, sig_cells=(1.0, 1.0), sig_theta=0.1),
                         sg.cloud_around(g, rng, n // 2, pose=sg.mirrored_pose(g), sig_cells=(1.0, 1.0), sig_theta=0.1)], axis=1)
    e.set_particles(p0, np.full(n, 1.0 / n))
    for _ in range(2):
        e.update(cx.action, cx.obs)
    got, info, labels = check_clusters(e, cx.geom)
    worst = np.maximum(worst, moment_ratios(e, got, cx.geom))
    print(f"{g.name}: clusters after two updates: {info}; worst mean / covariance deviation in units of the bound: {worst}")
    assert worst.max() <= 1.0
    if g.name == "tiny":
        k = cx.mod.default_kld_config()
        assert sg.kld_grid(g, k) == (1, 1)
        assert all(0 <= int(d["first_bin"]) < 36 for d in got)                   # a grid of 1 x 1 x 36
    e.close()


# ---- 6. recovery
def force_p(e, p):
    e.set_recovery_state(0.0, -math.inf if p >= 1.0 else math.log1p(-p))
    return e.recovery_state()[2]


@pytest.mark.parametrize("source", ["free", "mixture"])
@pytest.mark.parametrize("n,path", [(4096, "tiny"), (65536, "graph")])
def test_exact_injection(cx, n, path, source):
    """tests/test_gpu_recovery.py::test_exact_injection (and its mixture twin of test_gpu_recovery_proposal.py) on the geometry, KLD
    counting with the size pinned, p forced to 0.3"""
    exact_injection(cx, n, 0.3, path, source)


@pytest.mark.parametrize("source", ["free", "mixture"])
@pytest.mark.parametrize("name", ["one_free", "open"])
def test_exact_injection_of_every_child(engine_mod, orc, name, source):
    """p = 1 on the map with one free cell (every child at the same x, y) and on the map with nothing but free cells"""
    exact_injection(case_of(name, engine_mod, orc), 4096, 1.0, "tiny", source)


def exact_injection(cx, n, p, path, source):
    g = cx.g
    seed = SEED + 9
    a = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    b = make_engine(cx.mod, g, cx.ang, n, seed=seed)
    p0 = sg.cloud_around(g, np.random.default_rng(n), n)
    for e in (a, b):
        e.set_particles(p0, np.full(n, 1.0 / n))
        kcfg = e.set_kld(min_particles=n, max_particles=n)
    a.set_recovery()
    a.update(cx.action, cx.obs)                              # warm-up: the small-update paths need one regular update first
    b.update(cx.action, cx.obs)
    assert a.recovery_state()[3] == 0
    parents = a.get_particles()
    assert same_bits(parents, b.get_particles())
    if source == "mixture":
        means = g.seeds[:2]
        covs = np.array([small_cov(g), np.diag([(2 * g.res) ** 2, (2 * g.res) ** 2, 0.04])])
        thr, fac = mix.thresholds([1.0, 1.0]), mix.factors(means, covs)
        a.set_recovery_proposal(means, covs)
        dev_thr, dev_fac = a.recovery_proposal()
        assert [int(t) for t in dev_thr] == thr and np.allclose(dev_fac, fac, rtol=1e-15, atol=0)
    T = threshold(force_p(a, p))
    assert T > 0
    a.update(cx.action, cx.obs)
    b.update(cx.action, cx.obs)
    assert path_of(a) == path, (path_of(a), path)
    coin, pick, hb = child_draws(seed, 1, n)
    inj = coin < np.uint64(T)
    if p >= 1.0:
        assert inj.all()
    idx_a, idx_b = a.resample_indices(), b.resample_indices()
    assert np.array_equal(np.flatnonzero(idx_a == -1), np.flatnonzero(inj))
    assert np.array_equal(idx_a[~inj], idx_b[~inj])
    pa, pb = a.get_particles(), b.get_particles()
    if source == "free":
        want_inj = injected_poses(pick[inj], hb[inj], cx.free, g.W, g.resolution, g.origin_x, g.origin_y)
        assert same_bits(pa[:, inj], want_inj), "injected poses differ from the free-cell rule"
        col, row = sg.oracle_cells(cx.om, pa[0, inj], pa[1, inj])
        assert (g.data[row, col] == 0).all()
    else:
        want_inj, comp = mix.injected_poses(seed, 1, np.flatnonzero(inj).astype(np.uint64), pick[inj], thr, fac)
        assert set(np.unique(comp)) == {0, 1}
        assert_poses(pa[:, inj], want_inj, "injected poses differ from the mixture rule")
        assert a.recovery_proposal() is None                 # consumed
        want_inj = pa[:, inj]                                # (for the bin count: the engine's own poses, bin edges cannot differ)
    assert same_bits(pa[:, ~inj], pb[:, ~inj]), "a non-injected child differs from the recovery-off engine's"
    assert np.array_equal(a.log_weights(), cx.logw(pa))
    assert a.recovery_state()[3] == int(inj.sum())
    drawn = parents[:, np.where(inj, 0, idx_b)].copy()
    drawn[:, inj] = want_inj
    assert a.kld_state()[0] == cx.np_bins(drawn, kcfg)
    # the update after the injecting one is the oracle's too
    S, F, p_next, _ = a.recovery_state()
    assert S == F and p_next == 0.0
    a.update(cx.action, cx.obs)
    assert a.recovery_state()[3] == 0 and not (a.resample_indices() == -1).any()
    assert np.array_equal(a.log_weights(), cx.logw(a.get_particles()))
    a.close()
    b.close()


# ---- 7. the pruned search
@pytest.fixture(scope="module")
def lf(cx):
    e = make_engine(cx.mod, cx.g, cx.ang, 64)
    e.set_likelihood_field(True)
    yield e
    e.close()


def test_pruned_search(cx, lf):
    g, e = cx.g, lf
    record = {}
    for stride in g.strides:
        for nms in (0, 1):
            f = dict(stride_cells=stride, n_headings=N_HEAD, nms=nms)
            want, st = e.global_search(cx.obs, max_hits=65536, **f)
            want = want.copy()
            V = e.search_scores(N_HEAD).copy()
            assert st["n_hits"] < 65536 and st["n_poses"] == V.size
            for S in (2, 4, 8):
                ref = pr.blocks(g.data, stride, S)
                best = np.full((N_HEAD, ref["n_blocks"]), -np.inf)
                np.maximum.at(best, (np.arange(N_HEAD)[:, None].repeat(V.shape[1], 1), ref["block_of_pos"][None, :].repeat(N_HEAD, 0)), V)
                for max_hits in (1, 16, 65536):
                    got, ps = e.global_search_pruned(cx.obs, max_hits=max_hits, block=S, first_pairs=FIRST, **f)
                    what = (g.name, stride, nms, S, max_hits)
                    assert ps["n_hits"] == len(got) == min(max_hits, st["n_hits"]), what
                    assert got.dtype == want.dtype and got.tobytes() == want[:len(got)].tobytes(), what
                    assert ps["guard_fallbacks"] == 0, what
                    assert (ps["n_positions"], ps["n_poses"], ps["used_beams"]) == (st["n_positions"], st["n_poses"], st["used_beams"])
                    U = e.search_bounds()
                    assert U.size == ps["pairs"] == N_HEAD * ref["n_blocks"], what
                    assert not np.isnan(U).any() and (U.reshape(N_HEAD, -1) >= best).all(), what          # as doubles, no tolerance
                    r = pr.schedule(U, V, g.data, stride, S, nms, max_hits, FIRST)
                    assert (ps["pairs_scored"], ps["rounds"]) == (r["pairs_scored"], r["rounds"]), (what, ps, r["pairs_scored"], r["rounds"])
                    assert np.array_equal(got["index"], r["hits"]), what
                    record[(stride, nms, S, max_hits)] = (ps["pairs_scored"], ps["pairs"], ps["rounds"])
                    if g.name == "open":
                        assert ps["pairs_scored"] == ps["pairs"]                                         # all ties: nothing is pruned
                    if g.name == "one_free" or (g.name == "tiny" and stride == 3 and S >= 4):
                        assert ps["pairs"] == N_HEAD and ref["n_blocks"] == 1
    print(f"{g.name}: pruned search (stride, nms, block, max_hits) -> (pairs scored, pairs, rounds): {record}")


def test_propose_from_scan_pruned(cx, lf):
    f = dict(stride_cells=cx.g.strides[0], n_headings=N_HEAD)
    want = lf.propose_from_scan(cx.obs, max_hits=8, **f)
    thr, fac = lf.recovery_proposal()
    got = lf.propose_from_scan(cx.obs, max_hits=8, pruned=True, **f)
    thr2, fac2 = lf.recovery_proposal()
    assert len(got) >= 1 and got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert np.array_equal(thr, thr2) and fac.tobytes() == fac2.tobytes()
    lf.set_recovery_proposal(None)
