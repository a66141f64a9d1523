"""Scan de-skew on the GPU (mcl_set_beam_offsets): the beam origins against numpy (DS2); every ray of
k_rays_deskew against the oracle's cast_many from the engine's own origins and every log-weight against the table sum in Q3's
order, bit for bit, over the particle and beam counts at which the kernel's loops and marches change (DS3, DS4); a table of zeros
and `off` against twins (DS6); whole updates whose children are the oracle's chain; the likelihood field with DS5's pairs, with and
without beam skipping; two lidars fused; a scan that was really taken on the move; the side calls, which ignore the offsets, and the
refusals.

The maps are those of tests/side_geometries.py: the 120 x 90 `small` map everywhere, `fine` (P = 600, 16-bit steps) once.  The
fixtures and every CPU statement are in tests/deskew_ref.py; tests/test_scan_deskew_host.py checks the fixtures' preconditions."""
import os

import numpy as np
import pytest

import deskew_ref as dr
import lfield_ref as lr
import side_geometries as sg
import whole_set as ws
from conftest import make_engine
from side_geometries import bits

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0031 + 4026
MOUNT = dr.MOUNT
REAR = (-0.4, 0.3, 2.5)
COUNTS = [1, 3, 4, 5, 64, 257, 4097]          # fewer than, equal to and more than the four waves of a workgroup; no multiple of anything


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


class Case:
    def __init__(self, engine_mod, orc, g):
        self.g, self.orc, self.mod = g, orc, engine_mod
        self.om = g.oracle(orc)
        self.P = self.om.max_range_px
        self.L = orc.eng_log_table(orc.sensor_table(self.P))
        self.action = (g.res, 0.0, 0.01)
        self.memo = {}

    def ang(self, B):
        if B not in self.memo:
            self.memo[B] = sg.angles(self.orc, B)
        return self.memo[B]

    def scan(self, B, pose=None):
        key = ("scan", B, pose)
        if key not in self.memo:
            s = sg.perturbed_scan(self.orc, self.om, self.ang(B), pose or self.g.true_pose, seed=self.g.perturb_seed)
            s.setflags(write=False)
            self.memo[key] = s
        return self.memo[key]


_CASES = {}


def case_of(name, engine_mod, orc):
    if name not in _CASES:
        _CASES[name] = Case(engine_mod, orc, sg.small() if name == "small" else sg.family()[name])
    return _CASES[name]


@pytest.fixture(scope="module")
def cx(engine_mod, orc):
    return case_of("small", engine_mod, orc)


def status_of(engine_mod, call):
    with pytest.raises(engine_mod.EngineError) as ei:
        call()
    return ei.value.status


def sensor_poses_of(e, mount):
    """S: SM2's output with a mount, the particles themselves without one"""
    return e.sensor_poses() if mount else e.get_particles()


def check_rays(cx, e, ang, scan, off, mount, what, steps=True):
    """DS3 / DS4 on the state the engine is in: every stored step is cast_many from the engine's own origins at S.theta + a', every
    log-weight the table sum of those steps in Q3's order; the kernel reported is MCL_RAYS_DESKEW"""
    S = sensor_poses_of(e, mount)
    ox, oy = e.beam_origins(S)
    eff = dr.effective_angles(ang, off)
    want_lw, want_st = dr.beam_log_weights(cx.orc, cx.om, cx.L, scan, ox, oy, S[2], eff)
    if steps:
        got = e.ray_steps().astype(np.int64)
        bad = np.argwhere(got != want_st)
        assert bad.size == 0, (what, len(bad), bad[:5].tolist())
    ws.assert_same(what + ": log-weights", e.log_weights(), want_lw)
    assert e.ray_kernel_id() == cx.mod.RAYS_DESKEW and e.ray_kernel_name() == "k_rays_deskew", what
    return S, want_st


# ---- 1. origins
def origin_rows(n, rng):
    p = np.empty((3, n))
    p[0] = rng.uniform(-60.0, 60.0, n)
    p[1] = rng.uniform(-45.0, 45.0, n)
    p[2] = rng.uniform(-np.pi, np.pi, n)
    for k, v in enumerate([np.pi, -np.pi, 999999.5, 1e7, np.nan, np.inf, -np.inf][:n]):
        p[2, k] = v
    if n > 16:
        p[0, 8], p[1, 9], p[0, 10], p[1, 11] = np.inf, -np.inf, -np.inf, np.inf
    return p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_origins_are_ds2(cx, n):
    """mcl_beam_origins against numpy: finite rows within 2^-49 (|coordinate| + |ox| + |oy|) -- three roundings and a device sincos
    at OpenCL's 4 ulp, the bound of test_mount_poses_is_sm2 and for its reason --, non-finite rows non-finite in the same
    components, zero offsets (and offsets off) the input's x and y bit for bit on every row whose heading is finite"""
    p = origin_rows(n, np.random.default_rng(n))
    for B in (1, 61, 65):
        e = make_engine(cx.mod, cx.g, cx.ang(B), 64)
        for table in (None, np.zeros((3, B))):
            e.set_beam_offsets(table)
            x, y = e.beam_origins(p)
            assert x.shape == (n, B)
            # (a heading whose sine and cosine are NaN -- NaN, +-inf -- gives NaN: x + (NaN 0 - NaN 0), what DS2's operations give)
            th_ok = np.isfinite(p[2])
            for got, col in ((x, p[0]), (y, p[1])):
                assert np.array_equal(bits(got[th_ok]), bits(np.repeat(col[th_ok][:, None], B, axis=1))) and np.isnan(got[~th_ok]).all()
        for k in range(2):
            off = dr.table_of(B, k, MOUNT if k else None)
            e.set_beam_offsets(off)
            o, a, on = e.beam_offsets()
            assert on and np.array_equal(bits(o), bits(off)) and np.array_equal(a.view(np.uint32), dr.effective_angles(cx.ang(B), off).view(np.uint32))
            got, want = e.beam_origins(p), dr.origins(p, off)
            fin = np.isfinite(p).all(axis=0)
            for c in (0, 1):
                assert np.array_equal(np.isfinite(got[c]), np.isfinite(want[c])) and np.array_equal(np.isnan(got[c]), np.isnan(want[c])), (B, k, c)
                bound = 2.0 ** -49 * (np.abs(want[c][fin]) + np.abs(off[0])[None, :] + np.abs(off[1])[None, :])
                assert (np.abs(got[c][fin] - want[c][fin]) <= bound).all(), (B, k, c)
                inf = np.isinf(want[c])
                assert np.array_equal(got[c][inf], want[c][inf]), (B, k, c)
        e.close()


# ---- 2. the beam model, every ray
def ray_cloud(cx, n, seed):
    return sg.cloud_around(cx.g, np.random.default_rng(seed), n)


@pytest.mark.parametrize("B", [1, 61, 64, 65, 130])
def test_every_ray(cx, B):
    """sensor_update over the particle counts of COUNTS with one engine per beam count: a mount on every other count, another
    table each time"""
    ang, scan = cx.ang(B), sg.odd_scan(cx.scan(B))
    e = make_engine(cx.mod, cx.g, ang, max(COUNTS), seed=SEED, keep_ray_steps=1)
    for k, n in enumerate(COUNTS):
        mount = MOUNT if k % 2 else None
        off = dr.table_of(B, k, mount)
        assert np.abs(off[:2]).max() > cx.g.res or B == 1                 # (one beam has the stamp 0: no offset where t_ref is 0)
        e.set_sensor_mount(mount)
        e.set_beam_offsets(off)
        e.set_particles(ray_cloud(cx, n, 100 + n), np.full(n, 1.0 / n))
        e.sensor_update(scan)
        check_rays(cx, e, ang, scan, off, mount, f"{n} x {B}")
        assert e.planned_ray_kernel(n)[0] == "k_rays_deskew" and "offsets" in e.planned_ray_kernel(n)[1]
    e.close()


def test_every_ray_of_a_full_scan(cx):
    """64 x 1081: seventeen rounds of the lane-stride loop"""
    B, n = 1081, 64
    ang, scan = cx.ang(B), sg.odd_scan(cx.scan(B))
    e = make_engine(cx.mod, cx.g, ang, n, seed=SEED, keep_ray_steps=1)
    off = dr.table_of(B, 1)
    e.set_beam_offsets(off)
    e.set_particles(ray_cloud(cx, n, 1081), np.full(n, 1.0 / n))
    e.sensor_update(scan)
    check_rays(cx, e, ang, scan, off, None, "64 x 1081")
    e.close()


@pytest.mark.parametrize("level,B", [(1, 61), (1, 1), (2, 61), (1, 130)])
def test_forced_marches(cx, level, B):
    """debug_force_exact 1 sends every ray to the literal march: with 61 or 130 beams every round flags at least kLaneMarchMin lanes
    (each lane marches its own ray; 130 beams end in a round of two flagged lanes, which the wave marches), with one beam the wave
    marches it.  Level 2 forces nothing in a kernel that has no level 1."""
    n = 257
    ang, scan = cx.ang(B), cx.scan(B)
    e = make_engine(cx.mod, cx.g, ang, n, seed=SEED, keep_ray_steps=1, debug_force_exact=level)
    off = dr.table_of(B, 2, MOUNT)
    e.set_sensor_mount(MOUNT)
    e.set_beam_offsets(off)
    e.set_particles(ray_cloud(cx, n, 7 + B), np.full(n, 1.0 / n))
    e.sensor_update(scan)
    check_rays(cx, e, ang, scan, off, MOUNT, f"force {level}, {B} beams")
    marched = e.counters()["exact_fallback_rays"]
    assert marched == n * B if level == 1 else marched < n * B // 4, marched
    e.close()


@pytest.mark.parametrize("zero_beams", [3, 20])
def test_cell_edge_cloud(cx, zero_beams):
    """particles on cell edges: the beams whose offset is zero start on the edge, where the guard flags them by itself -- three of
    them (the wave marches them one after the other) or twenty (each lane marches its own); the others start off the edge and walk"""
    B, n = 61, 257
    g = cx.g
    ang, scan = cx.ang(B), cx.scan(B)
    rng = np.random.default_rng(zero_beams)
    p = np.empty((3, n))
    p[0] = g.origin_x + rng.integers(20, 60, n) * g.res                  # a vertical cell edge
    p[1] = g.origin_y + rng.uniform(12.0, 28.0, n) * g.res
    p[2] = rng.uniform(-np.pi, np.pi, n)
    off = dr.table_of(B, 0)
    off[:2, 5:5 + zero_beams] = 0.0
    e = make_engine(cx.mod, g, ang, n, seed=SEED, keep_ray_steps=1)
    e.set_beam_offsets(off)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(scan)
    check_rays(cx, e, ang, scan, off, None, f"{zero_beams} beams from a cell edge")
    marched = e.counters()["exact_fallback_rays"]
    assert n * zero_beams <= marched < n * (zero_beams + 8), marched
    e.close()


def test_every_ray_on_fine(engine_mod, orc):
    """P = 600: 16-bit steps"""
    fx = case_of("fine", engine_mod, orc)
    B, n = 61, 257
    assert fx.P == 600
    ang, scan = fx.ang(B), sg.odd_scan(fx.scan(B))
    e = make_engine(fx.mod, fx.g, ang, n, seed=SEED, keep_ray_steps=1)
    off = dr.table_of(B, 0, MOUNT)
    e.set_sensor_mount(MOUNT)
    e.set_beam_offsets(off)
    e.set_particles(sg.cloud_around(fx.g, np.random.default_rng(3), n), np.full(n, 1.0 / n))
    e.sensor_update(scan)
    assert e.ray_steps().dtype == np.uint16
    check_rays(fx, e, ang, scan, off, MOUNT, "fine")
    e.close()


# ---- 3. a table of zeros, and off
@pytest.mark.parametrize("lf", [False, True])
def test_zero_table_is_the_plain_update(cx, lf):
    B, n = 61, 4097
    ang, scan = cx.ang(B), sg.odd_scan(cx.scan(B))
    pair = [make_engine(cx.mod, cx.g, ang, n, seed=SEED, keep_ray_steps=1) for _ in range(2)]
    p0 = ray_cloud(cx, n, 31)
    for e in pair:
        e.set_likelihood_field(lf)
        e.set_sensor_mount(MOUNT)
        e.set_particles(p0, np.full(n, 1.0 / n))
    pair[0].set_beam_offsets(np.zeros((3, B)))
    assert pair[0].beam_offsets()[2] and not pair[1].beam_offsets()[2]
    for e in pair:
        e.sensor_update(scan)
    ws.assert_same("log-weights", pair[0].log_weights(), pair[1].log_weights())
    ws.assert_same("weights", pair[0].get_weights(), pair[1].get_weights())
    if not lf:
        assert np.array_equal(pair[0].ray_steps(), pair[1].ray_steps())
        assert pair[0].ray_kernel_name() == "k_rays_deskew" and pair[1].ray_kernel_name() == "k_rays_skip"
    for e in pair:
        e.close()


@pytest.mark.parametrize("n", [2000, 16384])
def test_off_is_off(cx, n):
    """offsets set, used once and cleared: three updates bit-identical to those of a twin that never heard of them, on the tails a
    small set takes (the one-workgroup tail at 2000, the captured graph at 16 384)"""
    B = 61
    ang, scan = cx.ang(B), cx.scan(B)
    a, twin = (make_engine(cx.mod, cx.g, ang, n, seed=SEED + 1) for _ in range(2))
    p0 = ray_cloud(cx, n, n)
    a.set_particles(p0, np.full(n, 1.0 / n))
    twin.set_particles(p0, np.full(n, 1.0 / n))
    a.set_beam_offsets(dr.table_of(B, 0))
    a.sensor_update(scan)                      # (no resampling: the update counter the draws are keyed by stays with the twin's)
    assert a.ray_kernel_id() == cx.mod.RAYS_DESKEW
    a.set_beam_offsets(None)
    assert not a.beam_offsets()[2] and not a.beam_offsets()[0].any()
    a.set_particles(p0, np.full(n, 1.0 / n))
    for k in range(3):
        for e in (a, twin):
            e.update(cx.action, scan if k < 2 else sg.odd_scan(scan))
        ws.assert_same(f"update {k}: particles", a.get_particles(), twin.get_particles())
        ws.assert_same(f"update {k}: weights", a.get_weights(), twin.get_weights())
        ws.assert_same(f"update {k}: log-weights", a.log_weights(), twin.log_weights())
        assert a.ray_kernel_id() == twin.ray_kernel_id() == cx.mod.RAYS_SKIP
        assert tuple(a.stage_timings() == 0.0) == tuple(twin.stage_timings() == 0.0), k
    # set_beam_angles turns the offsets off: the table belonged to the old beams
    a.set_beam_offsets(dr.table_of(B, 1))
    assert a.beam_offsets()[2]
    a.set_beam_angles(ang)
    assert not a.beam_offsets()[2]
    a.update(cx.action, scan)
    twin.update(cx.action, scan)
    ws.assert_same("after set_beam_angles: log-weights", a.log_weights(), twin.log_weights())
    assert a.ray_kernel_id() == cx.mod.RAYS_SKIP
    a.close()
    twin.close()


# ---- 4. whole updates
class DeskewSet(ws.WholeSet):
    """whole_set.WholeSet with a new table before every update and the log-weights expected at the engine's own origins: indices
    and children as WholeSet holds them (resampling and motion are untouched), log_weights() = DS4 at beam_origins(S), then the
    oracle's weight stage on those"""

    def __init__(self, cx, mount, *a, **kw):
        super().__init__(*a, **kw)
        self.cx, self.mount = cx, mount

    def step(self, scan):
        orc, e, upd, cx = self.orc, self.e, self.upd, self.cx
        n = e.n
        off = dr.table_of(self.ang.size, upd, self.mount)
        e.set_beam_offsets(off)
        e.update(self.action, scan)
        assert e.n == n and e.effective_sample_size()[1]
        tag = f"update {upd}: "
        want_idx = self.expected_indices(n)
        ws.assert_same(tag + "resample indices", e.resample_indices(), want_idx)
        parts = e.get_particles()
        want_parts = orc.motion_model(self.p[:, want_idx], self.action, orc.eng_philox_normals(self.seed, upd, 0, n))
        ws.assert_close(tag + "children", parts, want_parts, 1e-13, 1e-13)
        if self.mount:
            ws.assert_same(tag + "sensor poses", e.sensor_poses(), e.mount_poses(parts))
        check_rays(cx, e, self.ang, scan, off, self.mount, tag.strip(": "))
        want_lw = e.log_weights()                                      # (just held to DS4)
        w, q, mx = orc.eng_weights_from_log(want_lw)
        ws.assert_same(tag + "fixed-point weights", self.read_q(n), q)
        sc = e.scalars()
        ws.check_scalars(sc, w, q, mx, parts)
        ws.check_readbacks(e, sc, w)
        ws.check_particle_mean(e.particle_mean(), parts)
        t = e.stage_timings()
        self.log.append(dict(update=upd, path="tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular"),
                             plain=int((bits(want_lw) != bits(orc.eng_log_weights(self.om, sensor_poses_of(e, self.mount), self.ang,
                                                                                  orc.obs_index(scan, self.om), self.L)[0])).sum())))
        self.p, self.q = parts, q
        self.upd += 1


@pytest.mark.parametrize("n,B,mount", [(64, 61, None), (257, 65, MOUNT), (4097, 61, MOUNT), (2000, 61, None)])
def test_whole_updates(cx, n, B, mount):
    ang, scan = cx.ang(B), cx.scan(B)
    e = make_engine(cx.mod, cx.g, ang, n, seed=SEED + 2, keep_ray_steps=1)
    twin = make_engine(cx.mod, cx.g, ang, n, seed=SEED + 2)
    p0 = ray_cloud(cx, n, 40 + n)
    w = np.full(n, 1.0 / n)
    for x in (e, twin):
        x.set_sensor_mount(mount)
        x.set_particles(p0, w)
    c = DeskewSet(cx, mount, cx.orc, cx.om, e, ang, SEED + 2, p0, cx.orc.eng_quantize_weights(w), L=cx.L, action=cx.action)
    c.step(scan)
    # the first update from equal weights: the particles of a twin with offsets off
    twin.update(cx.action, scan)
    ws.assert_same("first update: particles", e.get_particles(), twin.get_particles())
    assert (bits(e.log_weights()) != bits(twin.log_weights())).sum() > n // 2
    c.step(scan)
    c.step(sg.odd_scan(scan))
    print(f"small: {n} x {B}, mount {mount}: paths {[r['path'] for r in c.log]}, log-weights that differ from the plain model's "
          f"{[r['plain'] for r in c.log]} of {n}")
    assert all(r["path"] == "regular" for r in c.log), c.log          # launch by launch: no one-workgroup tail, no captured graph
    assert all(r["plain"] > n // 2 for r in c.log), c.log
    e.close()
    twin.close()


# ---- 5. the likelihood field
@pytest.mark.parametrize("mount", [None, MOUNT])
def test_likelihood_field_and_beam_skip(cx, mount):
    g, B = cx.g, 61
    ang = cx.ang(B)
    D, Lf = lr.field(g.data, g.resolution), lr.table(g.resolution, max_range_m=g.max_range_m)
    p0, scan, off = dr.lf_fixture(sg, cx.orc, g, ang, mount)
    n = dr.LF_N
    eff = dr.effective_angles(ang, off)
    e = make_engine(cx.mod, g, ang, n, seed=SEED + 5)
    e.set_likelihood_field()
    e.set_sensor_mount(mount)
    e.set_beam_offsets(off)
    e.set_particles(p0, np.full(n, 1.0 / n))

    def check_logw(obs, what):
        S = sensor_poses_of(e, mount)
        want, alts, n_amb = dr.lf_log_weights(S, eff, obs, off, D, Lf, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
        bad = sg.lf_mismatches(e.log_weights(), want, alts)
        assert not bad, (what, len(bad), bad[:5])
        if what == "sensor_update":            # (the fixture's poses: the count tests/test_scan_deskew_host.py confirmed)
            assert sg.within_cap(n_amb, n * lr.used_beams(ang, obs, g.max_range_m)[0].size), what
        plain = lr.log_weights(S, ang, obs, D, Lf, g.resolution, g.origin_x, g.origin_y, g.max_range_m)[0]
        assert (bits(want) != bits(plain)).sum() > n // 2, what         # (the offsets are seen)
        return S

    e.sensor_update(scan)                      # the fixture's poses, whose ambiguous beams the CPU file counted
    check_logw(scan, "sensor_update")
    e.update(cx.action, scan)
    check_logw(scan, "update")
    # beam skipping: the counts come from the same end points, and the update is the plain de-skewed one on the masked scan
    e.set_beam_skip()
    e.update(cx.action, scan)
    S = sensor_poses_of(e, mount)
    st = e.beam_skip_state()
    r = np.asarray(scan, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        used = (r >= 0.0) & (r < g.max_range_m)
    ka, mc, ms = cx.mod.host_beam_skip_thresholds(g.resolution, n, int(used.sum()))
    lo, hi, amb = dr.lf_agree_counts(S, eff, scan, off, D, ka, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
    cu = st["counts"][used]
    assert ((cu >= lo) & (cu <= hi)).all(), np.flatnonzero((cu < lo) | (cu > hi))[:5]
    kept, n_skipped, integrate_all = cx.mod.host_beam_skip_plan(cu, n)
    assert np.array_equal(st["kept"][used], kept) and (st["n_skipped"], st["integrate_all"]) == (n_skipped, integrate_all)
    print(f"small: likelihood field, mount {mount}: {n_skipped} of {int(used.sum())} used beams skipped, integrate_all {integrate_all}, {amb} ambiguous")
    masked = np.asarray(scan, np.float32).copy()
    masked[st["kept"] == 2] = np.nan
    check_logw(masked, "beam skipping")
    # ... bit for bit: a twin without beam skipping, at the same particles, on the masked scan
    twin = make_engine(cx.mod, g, ang, n, seed=SEED + 5)
    twin.set_likelihood_field()
    twin.set_sensor_mount(mount)
    twin.set_beam_offsets(off)
    twin.set_particles(e.get_particles(), np.full(n, 1.0 / n))
    twin.sensor_update(masked)
    ws.assert_same("beam skipping against the masked scan", e.log_weights(), twin.log_weights())
    e.close()
    twin.close()


# ---- 6. two lidars
@pytest.mark.parametrize("lf", [False, True])
def test_two_lidars(cx, lf):
    g, n = cx.g, 257
    a_front, a_rear = cx.ang(61), (np.linspace(-1.9, 2.1, 40) + 0.013).astype(np.float32)
    sp_true = lambda m: tuple(dr.sm2(m, np.array(g.true_pose).reshape(3, 1))[:, 0])
    scan_f = sg.perturbed_scan(cx.orc, cx.om, a_front, sp_true(MOUNT), seed=g.perturb_seed)
    scan_r = sg.odd_scan(sg.perturbed_scan(cx.orc, cx.om, a_rear, sp_true(REAR), seed=g.perturb_seed))
    o_front, o_rear = dr.table_of(61, 0, MOUNT), dr.table_of(40, 1, REAR)
    D, Lf = lr.field(g.data, g.resolution), lr.table(g.resolution, max_range_m=g.max_range_m)
    e = make_engine(cx.mod, g, a_front, n, seed=SEED + 6, keep_ray_steps=1)
    e.set_likelihood_field(lf)
    sig = dict(sig_cells=(1.0, 1.0), sig_theta=0.05) if lf else {}
    e.set_particles(sg.cloud_around(g, np.random.default_rng(6), n, **sig), np.full(n, 1.0 / n))

    def term(ang, scan, off, what):
        """this stage's own log-weights, held as tests 2 and 5 hold them"""
        S = e.sensor_poses()
        eff = dr.effective_angles(ang, off)
        if not lf:
            ox, oy = e.beam_origins(S)
            want, st = dr.beam_log_weights(cx.orc, cx.om, cx.L, scan, ox, oy, S[2], eff)
            assert np.array_equal(e.ray_steps().astype(np.int64), st), what
            return want, {}
        want, alts, n_amb = dr.lf_log_weights(S, eff, scan, off, D, Lf, g.resolution, g.origin_x, g.origin_y, g.max_range_m)
        assert sg.within_cap(n_amb, n * lr.used_beams(ang, scan, g.max_range_m)[0].size), what
        return want, alts

    e.set_sensor_mount(MOUNT)
    e.set_beam_offsets(o_front)
    e.update(cx.action, scan_f)
    prev = e.log_weights()
    want, alts = term(a_front, scan_f, o_front, "front")
    assert not sg.lf_mismatches(prev, want, alts)
    e.set_sensor_mount(REAR)
    e.set_beam_angles(a_rear)
    assert not e.beam_offsets()[2]                                      # (the front's table went with the front's beams)
    e.set_beam_offsets(o_rear)
    e.sensor_update_fuse(scan_r)
    new, alts = term(a_rear, scan_r, o_rear, "rear")
    got = e.log_weights()
    # logw = prev + new, one rounded add, prev the left operand; an ambiguous particle may hold any of its alternatives
    bad = [i for i in np.flatnonzero(bits(got) != bits(prev + new)) if not (int(i) in alts and any(got[i] == prev[i] + v for v in alts[int(i)]))]
    assert not bad, bad[:5]
    e.close()


# ---- 7. it matters
def test_a_moving_scan_is_explained_only_with_offsets(cx):
    """the scan of test_moving_scan_differs_from_the_plain_one, cast beam by beam from the engine's own origins of the true pose:
    with offsets on the particle at the true pose casts exactly the scan's rows; with offsets off some beams differ and its
    log-weight is strictly lower"""
    g, B, n = cx.g, 61, 64
    ang = cx.ang(B)
    off = dr.table_of(B, 0)
    truth = np.array(g.true_pose).reshape(3, 1)
    p = ray_cloud(cx, n, 70)
    p[:, 0] = truth[:, 0]
    e = make_engine(cx.mod, g, ang, n, seed=SEED + 7, keep_ray_steps=1)
    e.set_beam_offsets(off)
    ox, oy = e.beam_origins(truth)
    scan, st = dr.moving_scan(cx.orc, cx.om, ang, g.true_pose, off, ox[0], oy[0])
    rows = cx.orc.obs_index(scan, cx.om)
    hit = st < cx.P
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(scan)
    on_steps, on_lw = e.ray_steps().astype(np.int64)[0], e.log_weights()[0]
    assert hit.sum() > 30 and np.array_equal(on_steps[hit], rows[hit])
    e.set_beam_offsets(None)
    e.sensor_update(scan)
    off_steps, off_lw = e.ray_steps().astype(np.int64)[0], e.log_weights()[0]
    differ = int((off_steps[hit] != rows[hit]).sum())
    print(f"small: moving scan: {differ} of {int(hit.sum())} beams in range differ without offsets; log-weight {on_lw:.3f} with, {off_lw:.3f} without")
    assert differ >= 10 and off_lw < on_lw
    e.close()


# ---- 8. side calls and refusals
def test_side_calls_ignore_offsets(cx):
    g, B = cx.g, 61
    ang, scan = cx.ang(B), cx.scan(B)
    a, twin = (make_engine(cx.mod, g, ang, 2000, seed=SEED + 8) for _ in range(2))
    a.set_beam_offsets(dr.table_of(B, 0))
    poses = g.query_poses
    for lf in (False, True):
        for e in (a, twin):
            e.set_likelihood_field(lf)
        r_a, s_a = a.expected_scans(poses, want_steps=True)
        r_t, s_t = twin.expected_scans(poses, want_steps=True)
        assert np.array_equal(r_a.view(np.uint32), r_t.view(np.uint32)) and np.array_equal(s_a, s_t)
        assert a.score_poses(poses, scan).tobytes() == twin.score_poses(poses, scan).tobytes()
    assert a.beam_offsets()[2]
    f = dict(stride_cells=g.strides[0], n_headings=36)
    h_a, h_t = a.global_search_pruned(scan, max_hits=8, **f), twin.global_search_pruned(scan, max_hits=8, **f)
    assert len(h_a[0]) > 0 and h_a[0].tobytes() == h_t[0].tobytes()
    f_a, f_t = a.refine_poses(g.seeds, scan, **g.window_fields), twin.refine_poses(g.seeds, scan, **g.window_fields)
    assert f_a[0].tobytes() == f_t[0].tobytes()
    a.close()
    twin.close()


def test_refusals(cx):
    mod, g, B = cx.mod, cx.g, 61
    ang, scan = cx.ang(B), cx.scan(B)
    off = dr.table_of(B, 0)
    UNSUPPORTED, INVALID, NOT_READY = mod.MCL_ERR_UNSUPPORTED, mod.MCL_ERR_INVALID_ARG, mod.MCL_ERR_NOT_READY
    # before the beam angles exist
    e = mod.Engine(max_particles=64)
    e.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
    assert status_of(mod, lambda: e.set_beam_offsets(off)) == NOT_READY
    e.set_beam_offsets(None)                                           # off is always accepted
    e.set_beam_angles(ang)
    assert status_of(mod, lambda: e.set_beam_offsets(dr.table_of(60, 0))) == INVALID
    bad = off.copy()
    bad[2, 17] = np.nan
    assert status_of(mod, lambda: e.set_beam_offsets(bad)) == INVALID
    bad[2, 17] = np.inf
    assert status_of(mod, lambda: e.set_beam_offsets(bad)) == INVALID
    assert not e.beam_offsets()[2]
    # the staged calls
    e.set_particles(ray_cloud(cx, 64, 9), np.full(64, 1.0 / 64))
    e.set_beam_offsets(off)
    assert status_of(mod, lambda: e.stage_rays(scan)) == UNSUPPORTED
    e.close()
    # PRODUCT mode, a pinned ray kernel
    for cfg in (dict(weight_mode=mod.WEIGHT_PRODUCT, keep_ray_steps=1), dict(ray_kernel=mod.RAYS_SKIP), dict(ray_kernel=mod.RAYS_MARCH)):
        e = make_engine(mod, g, ang, 64, **cfg)
        assert status_of(mod, lambda: e.set_beam_offsets(off)) == UNSUPPORTED, cfg
        assert not e.beam_offsets()[2]
        e.close()
    # a device group of one
    grp = mod.Group([0], max_particles=64)
    grp.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
    grp.set_beam_angles(ang)
    assert status_of(mod, lambda: grp.engine(0).set_beam_offsets(off)) == UNSUPPORTED
    grp.close()
