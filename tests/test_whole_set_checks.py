"""The whole-set checker (tests/whole_set.py) sees a single wrong entry.  A stand-in engine answers the engine's readbacks from
the oracle itself -- what a correct engine returns --, so the checker passes it; then one error at a time is planted in one of
its outputs, and the checker must fail and name the entry.  No GPU."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, tracking_cloud
import whole_set as ws

N, SEED = 3000, 77


class OracleEngine:
    """engine.Engine's readbacks after update(), computed by the oracle.  `plant` maps an output name to a function that edits
    that output before it is returned (the planted error)."""

    def __init__(self, orc, om, ang, p, w, seed=SEED):
        self.orc, self.om, self.ang, self.seed = orc, om, np.asarray(ang, np.float32), seed
        self.L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
        self.p = np.array(p, np.float64)
        self.n = self.p.shape[1]
        self.q = orc.eng_quantize_weights(w)
        self.upd = 0
        self.plant = {}

    def _out(self, name, a):
        a = np.array(a, copy=True)
        f = self.plant.get(name)
        return f(a) if f else a

    def update(self, action, scan):
        orc, n = self.orc, self.n
        k53 = orc.eng_philox_k53(self.seed, self.upd, 0, n)
        self.idx = orc.eng_resample_indices(self.q, 0, n_children=n, k53=k53)
        self.p = orc.motion_model(self.p[:, self.idx], action, orc.eng_philox_normals(self.seed, self.upd, 0, n))
        self.logw, _, _ = orc.eng_log_weights(self.om, self.p, self.ang, orc.obs_index(scan, self.om), self.L)
        self.w, self.q, mx = orc.eng_weights_from_log(self.logw)
        s, c = np.sin(self.p[2]), np.cos(self.p[2])
        sc = np.array([mx, math.fsum(self.w), 0.0] + [math.fsum(self.w * t) for t in (self.p[0], self.p[1], s, c, self.w)])
        sc[2:3] = np.array([self.q.sum(dtype=np.uint64)]).view(np.float64)
        self.sc = sc
        self.upd += 1

    def effective_sample_size(self):
        return (self.sc[1] * self.sc[1] / self.sc[7] if self.sc[7] > 0.0 else 0.0), True

    def resample_indices(self):
        return self._out("indices", self.idx)

    def get_particles(self):
        return self._out("particles", self.p)

    def log_weights(self):
        return self._out("logw", self.logw)

    def export_state(self, d_x=0, d_y=0, d_th=0, d_q=0):
        q = self._out("q", self.q)
        np.frombuffer((ctypes.c_uint64 * self.n).from_address(d_q), np.uint64)[:] = q

    def scalars(self):
        return self._out("scalars", self.sc)

    def get_weights(self):
        return self.w / self.sc[1]

    def expected_pose(self):
        k = 1.0 / self.sc[1]
        return np.array([self.sc[3] * k, self.sc[4] * k, math.atan2(self.sc[5] * k, self.sc[6] * k)])

    def sample_particles(self, k, uniforms=None):
        k53 = ws.injected_k53(uniforms) if uniforms is not None else ws.native_sample_k53(self.orc, self.seed, self.upd, k)
        idx = self.orc.eng_resample_indices(self.q, 0, n_children=k, k53=k53)
        return self._out("native_samples" if uniforms is None else "samples", self.p[:, idx])

    def particle_mean(self):
        return np.array([math.fsum(r) / self.n for r in self.p])

    def stage_timings(self):
        return np.ones(6)

    def ray_kernel_name(self):
        return "oracle"

    def planned_ray_kernel(self, n=0):
        return "oracle", ""

    def ray_kernel_variant(self):
        return {}

    def compact_list(self):
        return -1, False

    def counters(self):
        return {}


@pytest.fixture(scope="module")
def setup(orc, spielberg_oracle):
    ang = orc.beam_angles(angle_step=18)
    scan = np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::18].astype(np.float32)
    p0 = tracking_cloud(np.random.default_rng(3), N)
    return ang, scan, p0


def _run(orc, om, setup, plant=None, updates=2):
    """updates through the checker; the planted error (name, function) goes into the last update's outputs"""
    ang, scan, p0 = setup
    w0 = np.full(N, 1.0 / N)
    e = OracleEngine(orc, om, ang, p0, w0)
    c = ws.WholeSet(orc, om, e, ang, SEED, p0, orc.eng_quantize_weights(w0), q_device=None, sample_k=1024)
    for k in range(updates):
        if plant is not None and k == updates - 1:
            e.plant[plant[0]] = plant[1]
        c.step(scan)
    return e, c


def test_clean_run_passes(orc, spielberg_oracle, setup):
    e, c = _run(orc, spielberg_oracle, setup, updates=3)
    assert [r["update"] for r in c.log] == [0, 1, 2]
    assert np.isfinite(e.logw).all() and len(np.unique(e.idx)) < N      # (a real draw: duplicates, finite weights)


def _expect(orc, om, setup, plant, match):
    with pytest.raises(AssertionError, match=match):
        _run(orc, om, setup, plant)


K = 1234        # the entry the errors are planted in


def test_one_log_weight_one_ulp(orc, spielberg_oracle, setup):
    def f(a):
        a[K] = np.nextafter(a[K], np.inf)
        return a
    _expect(orc, spielberg_oracle, setup, ("logw", f), rf"log-weights: 1 of {N} differ; first at \[{K}\]")


def test_one_child_off_by_1e_11(orc, spielberg_oracle, setup):
    def f(a):
        a[1, K] += 1e-11
        return a
    _expect(orc, spielberg_oracle, setup, ("particles", f), rf"children: 1 of {N} differ; first at \[{K}\]")


def test_two_children_swapped(orc, spielberg_oracle, setup):
    j = K + 7
    def f(a):
        a[:, [K, j]] = a[:, [j, K]]
        return a
    _expect(orc, spielberg_oracle, setup, ("particles", f), rf"children: 2 of {N} differ; first at \[{K}, {j}\]")


def test_one_q_off_by_one(orc, spielberg_oracle, setup):
    def f(a):
        a[K] += np.uint64(1)
        return a
    _expect(orc, spielberg_oracle, setup, ("q", f), rf"fixed-point weights: 1 of {N} differ; first at \[{K}\]")


def test_sum_wx_without_the_heaviest_term(orc, spielberg_oracle, setup):
    holder = {}

    def f(a):
        e = holder["e"]
        j = int(np.argmax(e.w))
        a[3] = math.fsum(np.delete(e.w * e.p[0], j))
        return a
    ang, scan, p0 = setup
    w0 = np.full(N, 1.0 / N)
    e = OracleEngine(orc, spielberg_oracle, ang, p0, w0)
    holder["e"] = e
    c = ws.WholeSet(orc, spielberg_oracle, e, ang, SEED, p0, orc.eng_quantize_weights(w0), q_device=None, sample_k=1024)
    c.step(scan)
    e.plant["scalars"] = f
    with pytest.raises(AssertionError, match=r"SCALARS\[3\] \(sum w\*x\)"):
        c.step(scan)
    j = int(np.argmax(e.w))
    assert e.w[j] == 1.0 and abs(e.w[j] * e.p[0, j]) > 1e-6                # the dropped term is no rounding-sized one


def test_native_sample_from_its_neighbour(orc, spielberg_oracle, setup):
    holder = {}
    m = 100

    def f(a):
        e = holder["e"]
        idx = orc.eng_resample_indices(e.q, 0, n_children=a.shape[1], k53=ws.native_sample_k53(orc, SEED, e.upd, a.shape[1]))
        nb = idx[m] + 1 if idx[m] + 1 < N else idx[m] - 1                    # the next particle in CDF (index) order
        a[:, m] = e.p[:, nb]
        return a
    ang, scan, p0 = setup
    w0 = np.full(N, 1.0 / N)
    e = OracleEngine(orc, spielberg_oracle, ang, p0, w0)
    holder["e"] = e
    e.plant["native_samples"] = f
    c = ws.WholeSet(orc, spielberg_oracle, e, ang, SEED, p0, orc.eng_quantize_weights(w0), q_device=None, sample_k=1024)
    with pytest.raises(AssertionError, match=rf"sample_particles \(Philox stream 4\): 1 of 1024 differ; first at \[{m}\]"):
        c.step(scan)


def test_wrong_resample_index(orc, spielberg_oracle, setup):
    def f(a):
        a[K] = (a[K] + 1) % N
        return a
    _expect(orc, spielberg_oracle, setup, ("indices", f), rf"resample indices: 1 of {N} differ; first at \[{K}\]")


def test_sum_bound_is_tight_at_4m():
    n = 4194304
    assert ws.chain_length(n) == 16 + 30
    assert ws.sum_rel_bound(n) < 1e-12
    assert ws.sum_rel_bound(n, trig=True) < 1e-12
    assert ws.sum_rel_bound(33554432, trig=True) < 1e-12
