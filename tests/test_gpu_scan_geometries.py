"""Updates on the GPU over the scan family of tests/scan_geometries.py: every ray kernel, tail and form of k_rays_sweep on beam sets
the Hokuyo grid of the other tests never offers, each held bit for bit to oracle/mcl_oracle.c (oracle_logw of test_gpu_sweep.py,
tests/whole_set.py for indices, children, weights and pose).  No tolerance of this module's own.  The map is the 120 x 90 one of
side_geometries.small() (239 px of range: LDS windows), at 13 m (259 px) for the hybrid form.

Which case crosses which rule of mcl_set_beam_angles / choose_ray_mode / plan_sweep_form, from both sides:

  strictly ascending             hokuyo, ... / descending, repeated        test_engine_state, test_small_paths, test_refusals_*
  less than a turn               turn360 (359 deg), turn720_from_zero / over_turn (399 deg)      the same
  fewer than 16384 beams         b16383 / b16384, b65536                   test_engine_state, test_forced_sweep[b16383], test_refusals_*
  1 .. 65536 beams               b65536 / 0 and 65537                      test_engine_state, test_beam_counts_outside_the_range
  virtual beams: span + wedge    hokuyo, narrow_rear / turn360, turn720_from_zero                test_forced_sweep
  ... 2 beams per wedge          pad_min (2.05) / wedge13 (1.0), coarse30 (0.75), two            test_forced_sweep
  ... 120 beams per wedge        rec1599 (118.4) / fine2701 (225), b16383                        test_forced_sweep
  REC's room, ltd_cols <= 1912   rec1599 (1856) / rec1600 (1920: rec_ok, fetched)                test_forced_sweep, test_engine_state
  the hybrid's room              rec1599, narrow_rear / rec1600            test_hybrid_form_and_its_room
  k_rays_skip<R>, R = 2, 3       four members                              test_skip_rays_per_lane
  AUTO's switch to k_rays_sweep  fine2701, turn360 / coarse30 (rays), every member at 2000      test_auto_at_size, test_small_paths
  (the beam search's B <= M and M % n_headings are crossed by tests/test_gpu_side_scan_geometries.py)"""
import os

import numpy as np
import pytest

import scan_geometries as scg
import side_geometries as sg
import whole_set as ws
from conftest import make_engine
from side_geometries import bits
from test_gpu_group import make_group
from test_gpu_sweep import oracle_logw

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0059
MAX_RAYS = 1 << 23                                  # per oracle comparison (what test_tracking_cloud_1081_beams pays)
BIG = ("b16383", "b16384", "b65536")
QUAD_OK = tuple(n for n in scg.NAMES if n not in ("descending", "repeated", "over_turn", "b16384", "b65536"))
REFUSED = ("descending", "repeated", "over_turn", "b16384")


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


class World:
    """the map, its oracle maps by range, the members' scans from the true pose (made once, left unchanged)"""

    def __init__(self, engine_mod, orc):
        self.mod, self.orc, self.g = engine_mod, orc, sg.small()
        self.om = self.g.oracle(orc)
        self.L = orc.eng_log_table(orc.sensor_table(self.om.max_range_px))
        self.action = (self.g.res, 0.0, 0.01)
        self.pred = {n: scg.predict(a) for n, a in scg.family().items()}
        self.pred["hokuyo18"] = scg.predict(scg.family()["hokuyo"][::18])
        self._scan, self._om13 = {}, None

    def ang(self, name):
        return scg.family()["hokuyo"][::18].copy() if name == "hokuyo18" else scg.family()[name]

    def scan(self, name):
        if name not in self._scan:
            s = scg.scan_for(self.orc, self.om, self.ang(name), self.g.true_pose)
            s.setflags(write=False)
            self._scan[name] = s
        return self._scan[name]

    @property
    def om13(self):
        if self._om13 is None:
            g = self.g
            self._om13 = self.orc.OracleMap(g.data, g.resolution, g.origin_x, g.origin_y, max_range_m=13.0)
        return self._om13

    def tracking(self, n, seed, sig_cells=(4.0, 4.0), sig_theta=0.3):
        return sg.cloud_around(self.g, np.random.default_rng(seed), n, sig_cells=sig_cells, sig_theta=sig_theta)

    def uniform(self, n, seed):
        return sg.global_cloud(self.g, np.random.default_rng(seed), n)

    def held(self, got, p, name, obs=None, om=None, what=""):
        """the log-weights `got` of the particles p are the oracle's, on a fixed sample where n x B exceeds MAX_RAYS"""
        ang, n = self.ang(name), p.shape[1]
        k = min(n, max(64, MAX_RAYS // ang.size))
        sel = np.sort(scg.pick(n, k)) if k < n else np.arange(n)
        want = oracle_logw(self.orc, om or self.om, np.ascontiguousarray(p[:, sel]), ang, self.scan(name) if obs is None else obs)
        ws.assert_same(f"{name}: log-weights {what}", got[sel], want)
        return sel


@pytest.fixture(scope="module")
def W(engine_mod, orc):
    return World(engine_mod, orc)


def form_of(v):
    return {k: v[k] for k in ("global_fields", "hybrid", "turned_directions")}


def sensor(W, name, p, obs=None, **cfg):
    """a fresh engine, the particles p, one sensor update on the member's scan: the engine (the caller closes it)"""
    e = make_engine(W.mod, W.g, W.ang(name), p.shape[1], **cfg)
    e.set_particles(p, np.full(p.shape[1], 1.0 / p.shape[1]))
    e.sensor_update(W.scan(name) if obs is None else obs)
    return e


# ---- 1. what the engine decides for a beam set
@pytest.mark.parametrize("name", scg.NAMES)
def test_engine_state(W, name):
    pred, ang = W.pred[name], W.ang(name)
    e = make_engine(W.mod, W.g, ang, 64)
    assert e.max_range_px == 239
    for n in (65536, 2000):
        assert e.planned_ray_kernel(n) == scg.planned(pred, n), (name, n)
    e.close()
    p = W.tracking(64, 1, sig_cells=(0.5, 0.5))
    e = make_engine(W.mod, W.g, ang, 64, ray_kernel=W.mod.RAYS_SWEEP)
    assert e.planned_ray_kernel(64) == scg.planned(pred, 64, forced_sweep=True)
    if pred["quad_ok"]:
        e.set_particles(p, np.full(64, 1.0 / 64))
        e.sensor_update(W.scan(name))
        table, margin = e.sweep_table()
        print(f"{name}: predicted pad {pred['beam_pad']}, margin {pred['beam_margin']}, columns {pred['ltd_cols']}, REC {pred['rec']}; "
              f"engine: table {table.shape}, margin {margin}, form {e.ray_kernel_variant()}")
        assert (table.shape[1], margin) == (pred["ltd_cols"], pred["beam_margin"])
        assert form_of(e.ray_kernel_variant()) == scg.form(pred)
        assert not table[:, :margin].any() and not table[:, margin + ang.size:].any()           # virtual beams weigh nothing
        W.held(e.log_weights(), p, name)
    e.close()


def test_beam_counts_outside_the_range(W):
    e = make_engine(W.mod, W.g, W.ang("one"), 64)
    for bad in (np.zeros(0, np.float32), np.linspace(-3.0, 3.0, 65537).astype(np.float32)):
        with pytest.raises(W.mod.EngineError) as ei:
            e.set_beam_angles(bad)
        assert ei.value.status == W.mod.MCL_ERR_INVALID_ARG
    e.set_beam_angles(W.ang("b65536"))                       # the largest accepted set
    assert e.planned_ray_kernel(128) == ("k_rays_skip", scg.WHY_SMALL)
    e.close()


# ---- 2. the small paths: every particle of two updates
@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("name", scg.NAMES)
def test_small_paths(W, name, mode):
    """k_rays_skip with the one-workgroup tail: indices, children, log-weights, weights, sums and pose of two updates are the
    oracle's on every particle; launch by launch (graph_mode 1) the same bytes"""
    n = 128 if name in BIG else 2000
    ang, scan = W.ang(name), W.scan(name)
    seed = SEED + 10 * scg.NAMES.index(name) + mode
    p0, w0 = W.tracking(n, 100 + mode), np.full(n, 1.0 / n)
    e = make_engine(W.mod, W.g, ang, n, seed=seed, resample_mode=mode)
    e.set_particles(p0, w0)
    c = ws.WholeSet(W.orc, W.om, e, ang, seed, p0, W.orc.eng_quantize_weights(w0), mode=mode, L=W.L, action=W.action,
                    rng=np.random.default_rng(mode), sample_k=min(ws.SAMPLE_K, n // 2))
    for _ in range(2):
        c.step(scan)
    assert [r["kernel"] for r in c.log] == ["k_rays_skip"] * 2 == [r["planned"] for r in c.log], c.log
    assert c.log[1]["path"] == "tiny", c.log
    b = make_engine(W.mod, W.g, ang, n, seed=seed, resample_mode=mode, graph_mode=1)
    b.set_particles(p0, w0)
    for _ in range(2):
        b.update(W.action, scan)
    assert b.stage_timings()[0] != 0.0                       # not the tiny tail
    for what, x, y in (("particles", e.get_particles(), b.get_particles()), ("log-weights", e.log_weights(), b.log_weights()),
                       ("weights", e.get_weights(), b.get_weights()), ("pose", e.expected_pose(), b.expected_pose())):
        assert np.array_equal(bits(x), bits(y)), (name, what)
    assert np.array_equal(e.resample_indices(), b.resample_indices())
    e.close()
    b.close()


@pytest.mark.parametrize("name", ["fine2701", "turn360", "narrow_rear"])
def test_captured_tail(W, name):
    """16 384 particles: the captured graph tail from the second update on"""
    n = 16384
    e = make_engine(W.mod, W.g, W.ang(name), n, seed=SEED + 3)
    e.set_particles(W.tracking(n, 3), np.full(n, 1.0 / n))
    paths = []
    for k in range(3):
        e.update(W.action, W.scan(name))
        t = e.stage_timings()
        paths.append("tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular"))
        assert e.ray_kernel_name() == "k_rays_skip"
        W.held(e.log_weights(), e.get_particles(), name, what=f"update {k}")
    assert paths[1:] == ["graph", "graph"], paths
    e.close()


# ---- 3. k_rays_skip<R>
@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("name,force", [("hokuyo18", 0), ("wedge13", 0), ("fine2701", 0), ("one", 0), ("hokuyo18", 1), ("hokuyo18", 2)])
def test_skip_rays_per_lane(W, name, R, force):
    """61 beams: fewer than 64 R; 2701: the last group partly padding (2688 + 13 for R = 2, 2688 + 13 of 192 for R = 3)"""
    n, ang = 1500, W.ang(name)
    p = W.tracking(n, 30 + R)
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SKIP, rays_per_lane=R, keep_ray_steps=1, debug_force_exact=force)
    assert e.ray_kernel_name() == "k_rays_skip"
    want, steps, _ = W.orc.eng_log_weights(W.om, p, ang, W.orc.obs_index(W.scan(name), W.om), W.L, want_steps=True)
    ws.assert_same(f"{name} R {R}: log-weights", e.log_weights(), want)
    assert np.array_equal(e.ray_steps(), steps)
    c = e.counters()
    if force:
        assert c["off_window_particles"] == 0 and c["level2_rays"] == n * ang.size, c
    if force == 1:
        assert c["exact_fallback_rays"] == n * ang.size, c
    e.close()


# ---- 4. k_rays_sweep, forced
@pytest.mark.parametrize("name,cloud", [(n, c) for n in QUAD_OK for c in ("tracking", "uniform") if (n, c) != ("b16383", "uniform")])
def test_forced_sweep(W, name, cloud):
    """the LDS-window form on a tracking cloud and on a uniform one (headings everywhere: scan-edge lanes, beamless wedges and the
    far pass take part), in the form `predict` names; b16383: a tracking cloud of 512 only (8.4M rays)"""
    if name == "b16383":
        p = W.tracking(512, 41)
    else:
        p = W.tracking(4096, 41) if cloud == "tracking" else W.uniform(8192, 42)
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SWEEP)
    assert e.ray_kernel_name() == "k_rays_sweep"
    v, c = e.ray_kernel_variant(), e.counters()
    print(f"{name}: {cloud}: form {v}, off-window particles {c['off_window_particles']}, level-2 rays {c['level2_rays']}")
    assert form_of(v) == scg.form(W.pred[name]), (name, v)
    if name == "pad_min":
        assert v["turned_directions"] and e.sweep_table()[1] == 8
    if name in ("fine2701", "b16383", "rec1600"):
        assert not v["turned_directions"]
    W.held(e.log_weights(), p, name, what=cloud)
    e.close()


@pytest.mark.parametrize("cloud", ["tracking", "uniform"])
@pytest.mark.parametrize("name", ["turn360", "fine2701", "rec1600", "narrow_rear", "coarse30"])
def test_forced_sweep_on_the_global_fields(W, name, cloud, monkeypatch):
    monkeypatch.setenv("MCL_SWEEP_GLOBAL", "1")
    monkeypatch.setenv("MCL_SWEEP_HYBRID", "0")
    p = W.tracking(4096, 43) if cloud == "tracking" else W.uniform(8192, 44)
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SWEEP)
    assert e.ray_kernel_name() == "k_rays_sweep"
    assert form_of(e.ray_kernel_variant()) == scg.form(W.pred[name], global_fields=True), (name, e.ray_kernel_variant())
    W.held(e.log_weights(), p, name, what=cloud)
    e.close()


@pytest.mark.parametrize("cloud", ["tracking", "uniform"])
@pytest.mark.parametrize("name", ["narrow_rear", "rec1599", "rec1600"])
def test_hybrid_form_and_its_room(W, name, cloud, monkeypatch):
    """13 m = 259 px, MCL_SWEEP_HYBRID=2 (tools/ray_launch_trace.py's sweep_hybrid): LDS windows as far as they reach, the global
    fields beyond.  rec1600's 1920 table columns leave the beams' offsets no room behind the window: the global-field form, with
    fetched directions, runs in its place"""
    monkeypatch.setenv("MCL_SWEEP_HYBRID", "2")
    om, ang = W.om13, W.ang(name)
    assert om.max_range_px == 259
    obs = scg.scan_for(W.orc, om, ang, W.g.true_pose, max_range_m=13.0)
    p = W.tracking(4096, 45) if cloud == "tracking" else W.uniform(8192, 46)
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SWEEP, max_range_m=13.0, obs=obs)
    assert e.max_range_px == 259 and e.ray_kernel_name() == "k_rays_sweep"
    v = e.ray_kernel_variant()
    assert form_of(v) == scg.form(W.pred[name], hybrid=True), (name, v)
    assert v["hybrid"] == (name != "rec1600") and v["global_fields"] == (name == "rec1600")
    W.held(e.log_weights(), p, name, obs=obs, om=om, what=cloud)
    e.close()


@pytest.mark.parametrize("name", ["narrow_rear", "turn360", "wedge13"])
def test_forced_sweep_steps_are_cast_ray(W, name):
    n, ang = 4096, W.ang(name)
    p = np.concatenate([W.tracking(n // 2, 47), W.uniform(n // 2, 48)], axis=1)
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SWEEP, keep_ray_steps=1)
    assert e.ray_kernel_name() == "k_rays_sweep"
    want, steps, _ = W.orc.eng_log_weights(W.om, p, ang, W.orc.obs_index(W.scan(name), W.om), W.L, want_steps=True)
    a = (p[2][:, None] + ang.astype(np.float64)[None, :]).ravel()
    cast = W.orc.cast_many(W.om, np.repeat(p[0], ang.size), np.repeat(p[1], ang.size), a, use_omp=True)[1].reshape(n, ang.size)
    assert np.array_equal(steps.astype(np.int32), cast)
    got = e.ray_steps().astype(np.int32)
    bad = np.argwhere(got != cast)
    assert bad.size == 0, (len(bad), bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), cast[tuple(bad[:5].T)].tolist())
    ws.assert_same(f"{name}: log-weights", e.log_weights(), want)
    e.close()


@pytest.mark.parametrize("force", [2, 1])
@pytest.mark.parametrize("name", ["narrow_rear", "fine2701"])
def test_forced_sweep_counts_every_ray_once(W, name, force):
    """every ray through the parked-ray overflow into the fix-up list (level 2 / the literal march): the counters equal n x B, so
    virtual beams and beamless wedges add no ray and lose none"""
    n, B = 512, W.ang(name).size
    p = W.tracking(n, 49, sig_cells=(0.5, 0.5), sig_theta=0.4)
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SWEEP, debug_force_exact=force)
    assert e.ray_kernel_name() == "k_rays_sweep"
    c = e.counters()
    assert c["off_window_particles"] == 0, c                 # (off-window pairs go to k_rays_far, which uses no fix-up list)
    W.held(e.log_weights(), p, name)
    assert (c["level2_rays"] if force == 2 else c["exact_fallback_rays"]) == n * B, c
    e.close()


@pytest.mark.parametrize("name", ["narrow_rear", "fine2701"])
def test_three_sweep_updates_each_held_to_the_oracle(W, name):
    """no layout / the stale layout / + the prep fold (tests/test_gpu_sweep.py::test_three_updates_each_checked_against_the_oracle)"""
    n = 4096
    e = make_engine(W.mod, W.g, W.ang(name), n, seed=SEED + 5, ray_kernel=W.mod.RAYS_SWEEP)
    e.set_particles(W.tracking(n, 50), np.full(n, 1.0 / n))
    for k in range(3):
        e.update(W.action, W.scan(name))
        assert e.ray_kernel_name() == "k_rays_sweep"
        assert form_of(e.ray_kernel_variant()) == scg.form(W.pred[name])
        W.held(e.log_weights(), e.get_particles(), name, what=f"update {k}")
    e.close()


# ---- 5. refusals that must stay refusals
@pytest.mark.parametrize("name", REFUSED)
def test_refusals_of_the_forced_sweep(W, name):
    n = 256
    e = make_engine(W.mod, W.g, W.ang(name), n, ray_kernel=W.mod.RAYS_SWEEP)
    assert e.planned_ray_kernel(n) == (None, scg.WHY_NO_WINDOWS)
    e.set_particles(W.tracking(n, 51), np.full(n, 1.0 / n))
    for call in (lambda: e.sensor_update(W.scan(name)), lambda: e.update(W.action, W.scan(name))):
        with pytest.raises(W.mod.EngineError) as ei:
            call()
        assert scg.WHY_NO_WINDOWS in str(ei.value), str(ei.value)
    assert e.ray_kernel_name() == "?"                        # no ray kernel ran
    e.close()


@pytest.mark.parametrize("name", REFUSED)
def test_refused_members_under_auto_at_size(W, name):
    n = 65536
    p = W.tracking(n, 52)
    e = make_engine(W.mod, W.g, W.ang(name), n)
    assert e.planned_ray_kernel(n) == ("k_rays_skip", scg.WHY_NO_WINDOWS)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(W.scan(name))
    assert e.ray_kernel_name() == "k_rays_skip"
    sel = scg.pick(n, 256 if name == "b16384" else 2048)
    ws.assert_same(f"{name}: log-weights", e.log_weights()[sel], oracle_logw(W.orc, W.om, np.ascontiguousarray(p[:, sel]), W.ang(name), W.scan(name)))
    e.close()


# ---- 6. AUTO at size
@pytest.mark.parametrize("name,kernel", [("fine2701", "k_rays_sweep"), ("turn360", "k_rays_sweep"), ("coarse30", "k_rays_skip")])
def test_auto_at_size(W, name, kernel):
    n = 65536
    assert (n * W.ang(name).size >= ws.SWEEP_MIN_RAYS) == (kernel == "k_rays_sweep")
    p = np.concatenate([W.tracking(n // 2, 53), W.uniform(n // 2, 54)], axis=1)
    e = make_engine(W.mod, W.g, W.ang(name), n)
    assert e.planned_ray_kernel(n) == scg.planned(W.pred[name], n)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.sensor_update(W.scan(name))
    assert e.ray_kernel_name() == kernel
    sel = scg.pick(n, 2048)
    ws.assert_same(f"{name}: log-weights", e.log_weights()[sel], oracle_logw(W.orc, W.om, np.ascontiguousarray(p[:, sel]), W.ang(name), W.scan(name)))
    e.close()


# ---- 7. headings on wedge edges
@pytest.mark.parametrize("kernel", ["sweep", "skip"])
@pytest.mark.parametrize("name", ["wedge13", "turn360"])
def test_headings_on_wedge_edges(W, name, kernel):
    """256 headings that are exact multiples of pi / 8, and 256 one ulp to either side of each"""
    p = W.tracking(768, 55, sig_cells=(2.0, 2.0))
    edge = np.pi * np.random.default_rng(56).integers(-8, 9, 256) / 8.0
    p[2] = np.concatenate([edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf)])
    e = sensor(W, name, p, ray_kernel=W.mod.RAYS_SWEEP if kernel == "sweep" else W.mod.RAYS_SKIP)
    assert e.ray_kernel_name() == "k_rays_" + kernel
    W.held(e.log_weights(), p, name, what=kernel)
    e.close()


# ---- 8. a group
@pytest.mark.parametrize("kernel", ["auto", "sweep"])
@pytest.mark.parametrize("name", ["turn360", "narrow_rear"])
def test_group_of_two_shards(W, name, kernel):
    n = 8192
    cfg = dict(seed=SEED + 8, **({"ray_kernel": W.mod.RAYS_SWEEP} if kernel == "sweep" else {}))
    p, w = W.tracking(n, 57), np.full(n, 1.0 / n)
    one = make_engine(W.mod, W.g, W.ang(name), n, **cfg)
    grp = make_group(W.mod, W.g, W.ang(name), n // 2, 2, **cfg)
    one.set_particles(p, w)
    grp.set_particles(p, w)
    for k in range(3):
        one.update(W.action, W.scan(name))
        grp.update(W.action, W.scan(name))
        assert np.array_equal(grp.resample_indices(), one.resample_indices()), k
        parts = grp.get_particles()
        assert np.array_equal(bits(parts), bits(one.get_particles())), k
        logw = np.concatenate([grp.engine(i).log_weights() for i in range(2)])
        assert np.array_equal(bits(logw), bits(one.log_weights())), k
        W.held(logw, parts, name, what=f"update {k}")
    assert grp.engine(1).ray_kernel_name() == one.ray_kernel_name() == ("k_rays_sweep" if kernel == "sweep" else "k_rays_skip")
    grp.close()
    one.close()
