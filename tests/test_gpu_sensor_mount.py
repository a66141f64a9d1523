"""The sensor mount on the GPU (mcl_set_sensor_mount): the transform against numpy; whole updates on every tail
and ray-kernel form whose children are the oracle's chain (the mount touches neither resampling nor motion) and whose log-weights
are the oracle's AT THE SENSOR POSES the engine reports, bit for bit on every particle; the likelihood field and beam skipping at
those poses; the pose query against an unmounted twin fed the mounted poses; off is off; a mount changed under a captured graph;
a second scan fused into the posterior (mcl_sensor_update_fuse); and a device group of two engines against one mounted engine.

The maps are those of tests/side_geometries.py: the 120 x 90 `small` map everywhere but the long-range forms, which take `fine`
(P = 600).  The clouds start as the geometry tests' do (4 cells of spread), so that part of the set has its sensor in a wall or
off the map while its base is free: each chain prints the shares."""
import math
import os

import numpy as np
import pytest

import beam_skip_ref as br
import lfield_ref as lr
import side_geometries as sg
import whole_set as ws
from conftest import make_engine
from side_geometries import bits

pytestmark = pytest.mark.gpu

MOUNTS = [(0.27, 0.0, 0.0), (-0.4, 0.3, 2.5), (0.0, 0.0, -math.pi)]
FRONT, REAR = MOUNTS[0], MOUNTS[1]
SEED = 0x5EED_0000_0000_0031 + 4025


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


def sm2(m, p):
    """SM2 in numpy, in the rule's order"""
    with np.errstate(invalid="ignore"):
        s, c = np.sin(p[2]), np.cos(p[2])
        return np.stack([p[0] + (c * m[0] - s * m[1]), p[1] + (s * m[0] + c * m[1]), p[2] + m[2]])


class Case:
    """a geometry with its oracle map, beams and table; the scans are cast from the SENSOR at the true pose of each mount"""

    def __init__(self, engine_mod, orc, g):
        self.g, self.orc, self.mod = g, orc, engine_mod
        self.om = g.oracle(orc)
        self.P = self.om.max_range_px
        self.ang = sg.angles(orc, 61)
        self.ang128 = orc.beam_angles(angle_step=8)[:128].copy()
        self.ang40 = (np.linspace(-1.9, 2.1, 40) + 0.013).astype(np.float32)          # the rear unit: other angles, another count
        self.L = orc.eng_log_table(orc.sensor_table(self.P))
        self.action = (g.res, 0.0, 0.01)
        self.scans = {}

    def scan(self, ang, mount):
        key = (ang.size, tuple(mount))
        if key not in self.scans:
            pose = sm2(mount, np.array(self.g.true_pose).reshape(3, 1))[:, 0]
            s = sg.perturbed_scan(self.orc, self.om, ang, pose, seed=self.g.perturb_seed)
            s.setflags(write=False)
            self.scans[key] = s
        return self.scans[key]

    def logw(self, poses, ang, scan):
        return self.orc.eng_log_weights(self.om, np.ascontiguousarray(poses), ang, self.orc.obs_index(scan, self.om), self.L)[0]


_CASES = {}


def case_of(name, engine_mod, orc):
    if name not in _CASES:
        _CASES[name] = Case(engine_mod, orc, sg.small() if name == "small" else sg.family()[name])
    return _CASES[name]


@pytest.fixture(scope="module")
def cx(engine_mod, orc):
    return case_of("small", engine_mod, orc)


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def form_of(variant):
    return "hybrid" if variant["hybrid"] else "global" if variant["global_fields"] else "lds"


def read_q(e):
    import torch
    qt = torch.empty(e.n, dtype=torch.int64, device=torch.device("cuda"))
    e.export_state(0, 0, 0, qt.data_ptr())
    return qt.cpu().numpy().view(np.uint64)


def not_ready(engine_mod, call):
    with pytest.raises(engine_mod.EngineError) as ei:
        call()
    assert "rc=-2" in str(ei.value), str(ei.value)


# ---- 1. the transform
def transform_rows(n, rng):
    p = np.empty((3, n))
    p[0] = rng.uniform(-60.0, 60.0, n)
    p[1] = rng.uniform(-45.0, 45.0, n)
    p[2] = rng.uniform(-np.pi, np.pi, n)
    odd_th = [np.pi, -np.pi, 999999.5, 1e7, np.nan, np.inf, -np.inf]
    for k, v in enumerate(odd_th[:n]):
        p[2, k] = v
    if n > 16:
        p[0, 8], p[1, 9], p[0, 10], p[1, 11] = np.inf, -np.inf, -np.inf, np.inf
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_mount_poses_is_sm2(cx, n):
    """mcl_mount_poses against numpy: the heading one IEEE add (bit-equal); x and y within 2^-49 (|coordinate| + |mx| + |my|) on
    the finite rows, headings of 999 999.5 and 10^7 among them -- three roundings and a device sincos at OpenCL's 4 ulp
    (tests/whole_set.py works with 2 ulp for the same function: no larger bound is known for the device library) --; non-finite
    rows non-finite in the same components; with no mount the input comes back bit for bit"""
    e = make_engine(cx.mod, cx.g, cx.ang, 64)
    p = transform_rows(n, np.random.default_rng(n))
    assert np.array_equal(bits(e.mount_poses(p)), bits(p))
    for m in MOUNTS:
        e.set_sensor_mount(m)
        assert np.array_equal(e.sensor_mount(), np.array(m))
        got, want = e.mount_poses(p), sm2(m, p)
        assert np.array_equal(bits(got[2]), bits(want[2])), m
        fin = np.isfinite(p).all(axis=0)
        for k in (0, 1):
            assert np.array_equal(np.isfinite(got[k]), np.isfinite(want[k])), (m, k)
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (m, k)
            bound = 2.0 ** -49 * (np.abs(want[k][fin]) + abs(m[0]) + abs(m[1]))
            assert (np.abs(got[k][fin] - want[k][fin]) <= bound).all(), (m, k)
            inf = np.isinf(want[k])
            assert np.array_equal(got[k][inf], want[k][inf]), (m, k)
    e.set_sensor_mount(None)
    assert not e.sensor_mount().any()
    assert np.array_equal(bits(e.mount_poses(p)), bits(p))
    for bad in [(np.nan, 0, 0), (0, np.inf, 0), (0, 0, 6.3), (0, 0, -np.inf)]:
        with pytest.raises(cx.mod.EngineError) as ei:
            e.set_sensor_mount(bad)
        assert "rc=-1" in str(ei.value)
    assert not e.sensor_mount().any()
    e.close()


# ---- 2. whole updates: the oracle's chain, the oracle's log-weights at the sensor poses
class MountedSet(ws.WholeSet):
    """whole_set.WholeSet with the log-weights expected at the engine's sensor poses: (a) indices and children as WholeSet holds
    them, (b) sensor_poses() = mount_poses(get_particles()), (c) log_weights() = the oracle's at sensor_poses(), (d) weights,
    q, scalars and readbacks the oracle's weight stage on those log-weights and the BASE poses, sample_particles and particle_mean
    on the base poses (SM4)"""

    def step(self, scan, ang=None):
        orc, e, upd = self.orc, self.e, self.upd
        n = e.n
        e.update(self.action, scan)
        assert e.n == n and e.effective_sample_size()[1]
        tag = f"update {upd}: "
        want_idx = self.expected_indices(n)
        ws.assert_same(tag + "resample indices", e.resample_indices(), want_idx)
        parts = e.get_particles()
        want_parts = orc.motion_model(self.p[:, want_idx], self.action, orc.eng_philox_normals(self.seed, upd, 0, n))
        ws.assert_close(tag + "children", parts, want_parts, 1e-13, 1e-13)
        sp = e.sensor_poses()
        ws.assert_same(tag + "sensor poses", sp, e.mount_poses(parts))
        want_lw, _, _ = orc.eng_log_weights(self.om, sp, self.ang if ang is None else ang, orc.obs_index(scan, self.om), self.L)
        ws.assert_same(tag + "log-weights at the sensor poses", e.log_weights(), want_lw)
        w, q, mx = orc.eng_weights_from_log(want_lw)
        ws.assert_same(tag + "fixed-point weights", self.read_q(n), q)
        sc = e.scalars()
        ws.check_scalars(sc, w, q, mx, parts)
        ws.check_readbacks(e, sc, w)
        ws.check_samples(orc, e, parts, q, self.seed, upd + 1, self.rng, self.sample_k)
        ws.check_particle_mean(e.particle_mean(), parts)
        t = e.stage_timings()
        info = dict(update=upd, n=n, kernel=e.ray_kernel_name(), planned=e.planned_ray_kernel(n)[0], variant=e.ray_kernel_variant(),
                    path="tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular"), counters=e.counters(),
                    differs=int((bits(want_lw) != bits(orc.eng_log_weights(self.om, parts, self.ang if ang is None else ang,
                                                                           orc.obs_index(scan, self.om), self.L)[0])).sum()))
        self.log.append(info)
        self.p, self.q = parts, q
        self.upd += 1
        return info


def mounted_chain(cx, e, ang, mount, seed, n, mode=0, scans=None, what=""):
    g = cx.g
    p0 = sg.cloud_around(g, np.random.default_rng(seed & 0xFFFF), n)
    wall, off = sg.cloud_shares(cx.om, p0)
    swall, soff = sg.cloud_shares(cx.om, sm2(mount, p0))
    w = np.full(n, 1.0 / n)
    e.set_sensor_mount(mount)
    e.set_particles(p0, w)
    not_ready(cx.mod, e.sensor_poses)
    c = MountedSet(cx.orc, cx.om, e, ang, seed, p0, cx.orc.eng_quantize_weights(w), mode=mode, L=cx.L, action=cx.action,
                   rng=np.random.default_rng(seed & 0xFFFF), sample_k=min(ws.SAMPLE_K, n // 2))
    obs = cx.scan(ang, mount)
    for scan in scans or (obs, obs, sg.odd_scan(obs)):
        c.step(scan)
    print(f"{g.name}: {what} {n} x {ang.size}, mount {mount}: bases {wall:.3f} in walls / {off:.3f} off the map, sensors {swall:.3f} / "
          f"{soff:.3f}; paths {[r['path'] for r in c.log]}, kernels {[r['kernel'] for r in c.log]}, log-weights that differ from the "
          f"base poses' {[r['differs'] for r in c.log]} of {n}")
    for r in c.log:
        assert r["kernel"] == r["planned"], r
        assert r["differs"] > n // 2, r                    # (the mount is seen: most log-weights are not those of the base poses)
    return c


@pytest.mark.parametrize("mode,mount", [(0, MOUNTS[0]), (1, MOUNTS[1])])
def test_tiny_tail(cx, mode, mount):
    """2000 x 61: k_rays_skip and the one-workgroup tail, both resample modes"""
    n = 2000
    e = make_engine(cx.mod, cx.g, cx.ang, n, seed=SEED + mode, resample_mode=mode)
    c = mounted_chain(cx, e, cx.ang, mount, SEED + mode, n, mode, what="tiny tail")
    assert all(r["kernel"] == "k_rays_skip" for r in c.log) and [r["path"] for r in c.log[1:]] == ["tiny", "tiny"], c.log
    e.close()


def test_captured_graph(cx):
    """16 384 x 61: k_rays_skip in the captured graph, k_mount_poses inside it"""
    n = 16384
    e = make_engine(cx.mod, cx.g, cx.ang, n, seed=SEED + 2)
    c = mounted_chain(cx, e, cx.ang, MOUNTS[2], SEED + 2, n, what="graph tail")
    assert all(r["kernel"] == "k_rays_skip" for r in c.log) and [r["path"] for r in c.log[1:]] == ["graph", "graph"], c.log
    e.close()


@pytest.mark.parametrize("name,mount", [("small", MOUNTS[1]), ("fine", MOUNTS[0])])
def test_sweep_forms(engine_mod, orc, name, mount):
    """65 536 x 128 evenly spaced beams through AUTO: k_rays_sweep in its LDS form on `small`, in the global-field or hybrid form
    on `fine` (P = 600), with their far, fix and exact passes"""
    cx, n = case_of(name, engine_mod, orc), 65536
    e = make_engine(cx.mod, cx.g, cx.ang128, n, seed=SEED + 3)
    c = mounted_chain(cx, e, cx.ang128, mount, SEED + 3, n, what="AUTO")
    forms = [form_of(r["variant"]) for r in c.log]
    print(f"{name}: P {cx.P}: forms {forms}, off-window particles {[r['counters']['off_window_particles'] for r in c.log]}, "
          f"literal-march rays {[r['counters']['exact_fallback_rays'] for r in c.log]}")
    assert all(r["kernel"] == "k_rays_sweep" and r["path"] == "regular" for r in c.log), c.log
    if name == "fine":
        assert cx.P == 600 and all(f in ("hybrid", "global") for f in forms), forms
    else:
        assert forms == ["lds"] * 3, forms
    e.close()


def test_literal_march_and_stored_steps(cx):
    """ray_kernel = RAYS_MARCH at 4097 x 61 with keep_ray_steps: every stored step is cast_many from the sensor poses"""
    n = 4097
    e = make_engine(cx.mod, cx.g, cx.ang, n, seed=SEED + 4, ray_kernel=cx.mod.RAYS_MARCH, keep_ray_steps=1)
    c = mounted_chain(cx, e, cx.ang, MOUNTS[1], SEED + 4, n, what="literal march")
    assert all(r["kernel"] == "k_rays_march" for r in c.log), c.log
    sp = e.sensor_poses()
    a = (sp[2][:, None] + cx.ang.astype(np.float64)[None, :]).ravel()
    want = cx.orc.cast_many(cx.om, np.repeat(sp[0], 61), np.repeat(sp[1], 61), a)[1].reshape(n, 61)
    got = e.ray_steps().astype(np.int32).reshape(n, 61)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    e.close()


# ---- 3. likelihood field and beam skipping at the sensor poses
def shorten(scan, lo=0.28, hi=0.39):
    s = scan.copy()
    s[int(lo * s.size):int(hi * s.size)] *= np.float32(0.4)
    return s


@pytest.mark.parametrize("mount", MOUNTS[:2])
def test_likelihood_field_and_beam_skip(cx, mount):
    g, n = cx.g, 4097
    D = lr.field(g.data, g.resolution)
    Lf = lr.table(g.resolution, max_range_m=g.max_range_m)
    e = make_engine(cx.mod, g, cx.ang, n, seed=SEED + 5)
    e.set_likelihood_field()
    e.set_sensor_mount(mount)
    p0 = sg.cloud_around(g, np.random.default_rng(5), n, sig_cells=(1.0, 1.0), sig_theta=0.05)
    e.set_particles(p0, np.full(n, 1.0 / n))
    scan = sg.odd_scan(shorten(cx.scan(cx.ang, mount)))

    def check_logw(obs):
        sp = e.sensor_poses()
        ws.assert_same("sensor poses", sp, e.mount_poses(e.get_particles()))
        want, alts, n_amb = lr.log_weights(sp, cx.ang, obs, D, Lf, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
        bad = sg.lf_mismatches(e.log_weights(), want, alts)
        assert not bad, (len(bad), bad[:5])
        assert sg.within_cap(n_amb, n * lr.used_beams(cx.ang, obs, g.max_range_m)[0].size)
        return sp

    for k in range(2):
        e.update(cx.action, scan)
        check_logw(scan)
    # beam skipping: counts and mask are the reference's at the sensor poses
    e.set_beam_skip()
    e.update(cx.action, scan)
    sp = e.sensor_poses()
    st = e.beam_skip_state()
    r = np.asarray(scan, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        used = (r >= 0.0) & (r < g.max_range_m)
    nu = int(used.sum())
    ka, mc, ms = cx.mod.host_beam_skip_thresholds(g.resolution, n, nu)
    lo, hi, amb = br.counts(sp, cx.ang, scan, D, ka, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
    cu = st["counts"][used]
    assert ((cu >= lo) & (cu <= hi)).all(), np.flatnonzero((cu < lo) | (cu > hi))[:5]
    lo_b, hi_b, _ = br.counts(e.get_particles(), cx.ang, scan, D, ka, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
    assert ((cu < lo_b) | (cu > hi_b)).any(), "the counts are also those of the base poses: the mount is not seen"
    kept, n_skipped, integrate_all = cx.mod.host_beam_skip_plan(cu, n)
    assert np.array_equal(st["kept"][used], kept) and (st["n_skipped"], st["integrate_all"]) == (n_skipped, integrate_all)
    print(f"small: likelihood field, mount {mount}: {n_skipped} of {nu} used beams skipped, integrate_all {integrate_all}, {amb} ambiguous")
    masked = np.asarray(scan, np.float32).copy()
    masked[st["kept"] == 2] = np.nan
    check_logw(masked)
    e.close()


# ---- 4. the pose query
@pytest.mark.parametrize("K", [1, 65, 1000])
def test_pose_query_takes_base_poses(cx, K):
    g = cx.g
    rng = np.random.default_rng(K)
    poses = np.concatenate([g.query_poses, g.free_poses(rng, 1000)])[:K]
    obs = cx.scan(cx.ang, FRONT)
    a = make_engine(cx.mod, g, cx.ang, 2000, seed=SEED + 6)
    b = make_engine(cx.mod, g, cx.ang, 2000, seed=SEED + 6)            # never queries
    u = make_engine(cx.mod, g, cx.ang, 64)                             # never hears of a mount
    p0 = sg.cloud_around(g, np.random.default_rng(6), 2000)
    for e in (a, b):
        e.set_sensor_mount(REAR)
        e.set_particles(p0, np.full(2000, 1.0 / 2000))
        e.update(cx.action, obs)
    for lf_on in (False, True):
        for e in (a, b, u):
            e.set_likelihood_field(lf_on)
        sp = a.mount_poses(np.ascontiguousarray(poses.T)).T
        r_a, s_a = a.expected_scans(poses, want_steps=True)
        r_u, s_u = u.expected_scans(sp, want_steps=True)
        assert np.array_equal(r_a.view(np.uint32), r_u.view(np.uint32)) and np.array_equal(s_a, s_u)
        assert a.score_poses(poses, obs).tobytes() == u.score_poses(sp, obs).tobytes()
        if K > 1:
            assert a.score_poses(poses, obs).tobytes() != u.score_poses(poses, obs).tobytes()
    for e in (a, b):
        e.set_likelihood_field(False)
        e.update(cx.action, obs)
    ws.assert_same("particles", a.get_particles(), b.get_particles())
    ws.assert_same("log-weights", a.log_weights(), b.log_weights())
    ws.assert_same("weights", a.get_weights(), b.get_weights())
    ws.assert_same("sensor poses", a.sensor_poses(), b.sensor_poses())
    for e in (a, b, u):
        e.close()


# ---- 5. off is off
@pytest.mark.parametrize("n,B", [(16384, 61), (65536, 128)])
def test_off_is_off(cx, n, B):
    g = cx.g
    ang = cx.ang if B == 61 else cx.ang128
    obs = cx.scan(ang, (0.0, 0.0, 0.0))
    p0 = sg.cloud_around(g, np.random.default_rng(n), n)
    engines = [make_engine(cx.mod, g, ang, n, seed=SEED + 7) for _ in range(4)]
    engines[1].set_sensor_mount((0.0, 0.0, 0.0))
    engines[2].set_sensor_mount((-0.0, 0.0, -0.0))
    engines[3].set_sensor_mount(REAR)
    for e in engines:
        e.set_particles(p0, np.full(n, 1.0 / n))
    # one mounted sensor stage (it reserves the scratch and runs k_mount_poses; no resampling, so the update counter the draws are
    # keyed by stays with the others'), then the mount is cleared and the set started over
    engines[3].sensor_update(obs)
    assert engines[3].sensor_poses().shape == (3, n)
    engines[3].set_sensor_mount(None)
    engines[3].set_particles(p0, np.full(n, 1.0 / n))
    ref = engines[0]
    for k in range(3):
        for e in engines:
            e.update(cx.action, obs if k < 2 else sg.odd_scan(obs))
        want = (ref.ray_kernel_name(), path_of(ref), ref.ray_kernel_variant(), tuple(ref.stage_timings() == 0.0))
        for j, e in enumerate(engines[1:]):
            what = f"update {k}, engine {j + 1}: "
            ws.assert_same(what + "particles", e.get_particles(), ref.get_particles())
            ws.assert_same(what + "weights", e.get_weights(), ref.get_weights())
            ws.assert_same(what + "log-weights", e.log_weights(), ref.log_weights())
            got = (e.ray_kernel_name(), path_of(e), e.ray_kernel_variant(), tuple(e.stage_timings() == 0.0))
            assert got == want, (what, got, want)
        for e in engines:
            not_ready(cx.mod, e.sensor_poses)
    assert path_of(ref) == ("graph" if B == 61 else "regular")
    for e in engines:
        e.close()


# ---- 6. a mount changed under the captured graph
def test_mount_changed_between_graph_updates(cx):
    n = 16384
    e = make_engine(cx.mod, cx.g, cx.ang, n, seed=SEED + 8)
    e.set_sensor_mount(FRONT)
    e.set_particles(sg.cloud_around(cx.g, np.random.default_rng(8), n), np.full(n, 1.0 / n))
    obs = cx.scan(cx.ang, FRONT)
    for k in range(3):
        e.update(cx.action, obs)
    assert path_of(e) == "graph"
    ws.assert_same("log-weights", e.log_weights(), cx.logw(e.sensor_poses(), cx.ang, obs))
    for m in (REAR, FRONT, None, REAR):
        e.set_sensor_mount(m)
        for k in range(3):
            e.update(cx.action, obs)
            if m is None:
                not_ready(cx.mod, e.sensor_poses)
                sp = e.get_particles()
            else:
                sp = e.sensor_poses()
                ws.assert_same("sensor poses", sp, e.mount_poses(e.get_particles()))
                ws.assert_same("sensor poses against numpy's heading", sp[2], e.get_particles()[2] + m[2])
            ws.assert_same(f"mount {m}, update {k}: log-weights", e.log_weights(), cx.logw(sp, cx.ang, obs))
        assert path_of(e) == "graph", (m, path_of(e))
    # a stage without a mount on the SAME particles (no resampling) did not read the scratch: it is no stage's any more
    e.sensor_update(obs)
    assert e.sensor_poses().shape == (3, n)
    e.set_sensor_mount(None)
    e.sensor_update(obs)
    not_ready(cx.mod, e.sensor_poses)
    e.close()


# ---- 7. fusing a second scan
@pytest.mark.parametrize("n", [2000, 4097])
def test_fuse(cx, n):
    g, orc = cx.g, cx.orc
    obs_f, obs_r = cx.scan(cx.ang, FRONT), sg.odd_scan(cx.scan(cx.ang40, REAR))
    a = make_engine(cx.mod, g, cx.ang, n, seed=SEED + 9)
    twin = make_engine(cx.mod, g, cx.ang40, n, seed=SEED + 9)
    p0 = sg.cloud_around(g, np.random.default_rng(9), n)
    a.set_sensor_mount(FRONT)
    a.set_particles(p0, np.full(n, 1.0 / n))
    not_ready(cx.mod, lambda: a.sensor_update_fuse(obs_f))            # no weighting call on this set yet
    for upd in range(2):                                             # (the second update: the tiny tail at 2000)
        a.update(cx.action, obs_f)
        parts = a.get_particles()
        lw_front = a.log_weights()
        ws.assert_same("front log-weights", lw_front, cx.logw(a.sensor_poses(), cx.ang, obs_f))
        a.set_sensor_mount(REAR)
        a.set_beam_angles(cx.ang40)
        a.sensor_update_fuse(obs_r)
        ws.assert_same("particles", a.get_particles(), parts)
        twin.set_sensor_mount(REAR)
        twin.set_particles(parts, np.full(n, 1.0 / n))
        twin.sensor_update(obs_r)
        lw_rear = twin.log_weights()
        ws.assert_same("rear log-weights", lw_rear, cx.logw(a.sensor_poses(), cx.ang40, obs_r))
        ws.assert_same("fused log-weights", a.log_weights(), lw_front + lw_rear)
        w, q, mx = orc.eng_weights_from_log(lw_front + lw_rear)
        ws.assert_same("fused fixed-point weights", read_q(a), q)
        sc = a.scalars()
        ws.check_scalars(sc, w, q, mx, parts)
        ws.check_readbacks(a, sc, w)
        # twice adds twice
        a.sensor_update_fuse(obs_r)
        ws.assert_same("fused twice", a.log_weights(), (lw_front + lw_rear) + lw_rear)
        w, q, mx = orc.eng_weights_from_log((lw_front + lw_rear) + lw_rear)
        ws.assert_same("fixed-point weights, fused twice", read_q(a), q)
        ws.check_scalars(a.scalars(), w, q, mx, parts)
        a.set_sensor_mount(FRONT)
        a.set_beam_angles(cx.ang)
    # a particle the front scan makes impossible stays impossible: z_rand = 0 lets the Gaussian underflow to log 0
    b = make_engine(cx.mod, g, cx.ang, n, seed=SEED + 9, z_rand=0.0, sigma_hit=2.0)
    tb = make_engine(cx.mod, g, cx.ang40, n, seed=SEED + 9, z_rand=0.0, sigma_hit=2.0)
    far = sg.global_cloud(g, np.random.default_rng(10), n)
    far[:, :n // 2] = p0[:, :n // 2]
    b.set_sensor_mount(FRONT)
    b.set_particles(far, np.full(n, 1.0 / n))
    b.sensor_update(obs_f)
    lw_front = b.log_weights()
    dead = np.isneginf(lw_front)
    b.set_sensor_mount(REAR)
    b.set_beam_angles(cx.ang40)
    b.sensor_update_fuse(obs_r)
    tb.set_sensor_mount(REAR)
    tb.set_particles(far, np.full(n, 1.0 / n))
    tb.sensor_update(obs_r)
    with np.errstate(invalid="ignore"):
        want = lw_front + tb.log_weights()
    print(f"small: fuse {n}: {int(dead.sum())} particles impossible under the front scan, {int(np.isneginf(want).sum())} after the rear one")
    assert dead.any() and not np.isnan(want).any()
    ws.assert_same("fused log-weights with -inf", b.log_weights(), want)
    assert (b.get_weights()[dead] == 0.0).all()
    # what voids the state
    b.set_particles(far, np.full(n, 1.0 / n))
    not_ready(cx.mod, lambda: b.sensor_update_fuse(obs_r))
    b.sensor_update(obs_r)
    b.sensor_update_fuse(obs_r)
    b.init_particles_pose(g.true_pose, n)
    not_ready(cx.mod, lambda: b.sensor_update_fuse(obs_r))
    b.sensor_update(obs_r)
    b.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
    not_ready(cx.mod, lambda: b.sensor_update_fuse(obs_r))
    # ... and a bare staged ray stage, which rewrites the log-weights without forming weights
    b.set_particles(far, np.full(n, 1.0 / n))
    b.sensor_update(obs_r)
    b.stage_rays(obs_r)
    not_ready(cx.mod, lambda: b.sensor_update_fuse(obs_r))
    for e in (a, twin, b, tb):
        e.close()


# ---- 8. shards
def test_group_of_two_equals_one_mounted_engine(cx):
    """Two engines on the one device behind mcl_group_set_sensor_mount against one mounted engine: parents and particles bit
    for bit, the single engine's log-weights the oracle's at its sensor poses.  The normalised weights are compared within 1e-13, not bit for bit: w is the same bits, but the group
    divides by a sum reduced per shard and then added (tests/test_gpu_group.py's bound for the same comparison)"""
    g, n = cx.g, 8192
    obs = cx.scan(cx.ang, REAR)
    one = make_engine(cx.mod, g, cx.ang, n, seed=SEED + 11)
    grp = cx.mod.Group([0, 0], max_particles=n // 2, seed=SEED + 11)
    grp.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
    grp.set_beam_angles(cx.ang)
    p0 = sg.cloud_around(g, np.random.default_rng(11), n)
    one.set_sensor_mount(REAR)
    grp.set_sensor_mount(REAR)
    one.set_particles(p0, np.full(n, 1.0 / n))
    grp.set_particles(p0, np.full(n, 1.0 / n))
    for k in range(3):
        one.update(cx.action, obs)
        grp.update(cx.action, obs)
        assert np.array_equal(grp.resample_indices(), one.resample_indices()), k
        ws.assert_same(f"update {k}: particles", grp.get_particles(), one.get_particles())
        # (w is bit-identical; the sum is reduced per shard and then added: tests/test_gpu_group.py's bound)
        np.testing.assert_allclose(grp.get_weights(), one.get_weights(), rtol=1e-13, atol=0)
        ws.assert_same(f"update {k}: log-weights at the sensor poses", one.log_weights(), cx.logw(one.sensor_poses(), cx.ang, obs))
    grp.close()
    one.close()


def test_staged_calls_through_the_communicator_of_one_rank(cx):
    """The staged flow (mcl_stage_rays_async and its siblings, driven by the engine's own communicator with one rank: what dist.py
    runs natively on one device) with a mount: the children of one mounted engine, and the oracle's log-weights at the sensor poses"""
    g, n = cx.g, 8192
    obs = cx.scan(cx.ang, FRONT)
    one = make_engine(cx.mod, g, cx.ang, n, seed=SEED + 12)
    sh = make_engine(cx.mod, g, cx.ang, n, seed=SEED + 12)
    ok, why = sh.comm_available()
    if not ok:
        pytest.skip(f"no RCCL: {why}")
    for e in (one, sh):
        e.set_sensor_mount(FRONT)
        e.init_particles_pose(g.true_pose, n, 0, n)
    sh.comm_create(sh.comm_unique_id(), 1, 0)
    for k in range(3):
        one.update(cx.action, obs)
        pose = sh.comm_update(cx.action, obs)
        ws.assert_same(f"update {k}: particles", sh.get_particles(), one.get_particles())
        ws.assert_same(f"update {k}: sensor poses", sh.sensor_poses(), sh.mount_poses(sh.get_particles()))
        ws.assert_same(f"update {k}: log-weights at the sensor poses", sh.log_weights(), cx.logw(sh.sensor_poses(), cx.ang, obs))
        ws.assert_same(f"update {k}: log-weights", sh.log_weights(), one.log_weights())
        np.testing.assert_allclose(sh.get_weights(), one.get_weights(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(pose, one.expected_pose(), rtol=0, atol=1e-12)
    sh.close()
    one.close()


# ---- 9. the proposal of a search goes to the base frame
def test_propose_from_scan_converts_to_the_base_frame(cx):
    """The searches and refinements ignore the mount (SM4: their poses are sensor poses): with a mount set propose_from_scan finds
    the same hits and sets the proposal of the unmounted means and covariances brought to the base frame by the host functions;
    with none the proposal keeps its bits"""
    g = cx.g
    obs = cx.scan(cx.ang, (0.0, 0.0, 0.0))
    e = make_engine(cx.mod, g, cx.ang, 64)
    e.set_likelihood_field(True)
    f = dict(stride_cells=g.strides[0], n_headings=12)
    hits0 = e.propose_from_scan(obs, max_hits=8, **f)
    thr0, fac0 = e.recovery_proposal()
    r, _ = e.refine_poses(hits0["pose"], obs)
    want0 = cx.mod.host_recovery_proposal(r["mean"], r["cov"])
    assert np.array_equal(thr0, want0[0]) and fac0.tobytes() == want0[1].tobytes()
    e.set_sensor_mount(REAR)
    hits1 = e.propose_from_scan(obs, max_hits=8, **f)
    thr1, fac1 = e.recovery_proposal()
    assert len(hits1) >= 1 and hits1.tobytes() == hits0.tobytes()
    base = cx.mod.host_sensor_unmount(REAR, np.ascontiguousarray(r["mean"].T)).T
    covs = np.stack([cx.mod.host_sensor_mount_cov(REAR, r["mean"][i], r["cov"][i], to_base=True) for i in range(len(base))])
    want1 = cx.mod.host_recovery_proposal(base, covs)
    assert np.array_equal(thr1, want1[0]) and fac1.tobytes() == want1[1].tobytes()
    assert fac1.tobytes() != fac0.tobytes()
    # the round trip: the base means' sensor poses are the refined means
    back = cx.mod.host_sensor_mount(REAR, np.ascontiguousarray(base.T)).T
    assert np.abs(back - r["mean"]).max() <= 1e-12
    e.set_recovery_proposal(None)
    e.close()
