"""The tight wedge fields on the device (csrc/mcl_wedge.h; k_wedge_field_tight at mcl_set_map) against the Euclidean ones
(MCL_WEDGE_METRIC=0, read at mcl_set_map) and against the oracle: a field only decides how many probes a ray makes, never where
it ends, so log-weights (the hand-written walk: no step output) and ray steps (the per-ray path) are the same bit for bit under
both rules and equal the oracle's, and the probe count under the tight rule is never above the Euclidean rule's."""
import numpy as np
import pytest

import test_gpu_sweep as S
from conftest import tracking_cloud

pytestmark = pytest.mark.gpu


def run_both(engine_mod, monkeypatch, grid, res, ox, oy, ang, p, obs, want_variant=None, **cfg):
    """{metric: (log-weights of the walk, log-weights / steps / probe count of the counting per-ray path)} for "0" and the default."""
    n = p.shape[1]
    out = {}
    for metric in ("0", None):
        if metric is None:
            monkeypatch.delenv("MCL_WEDGE_METRIC", raising=False)
        else:
            monkeypatch.setenv("MCL_WEDGE_METRIC", metric)
        res_m = []
        for keep, count in ((0, 0), (1, 1)):
            e = engine_mod.Engine(max_particles=n, seed=9, keep_ray_steps=keep, debug_count_probes=count,
                                  ray_kernel=engine_mod.RAYS_SWEEP, **cfg)
            e.set_map(grid, res, ox, oy)
            e.set_beam_angles(ang)
            e.set_particles(p, np.full(n, 1.0 / n))
            e.sensor_update(obs)
            assert e.ray_kernel_name() == "k_rays_sweep"
            if want_variant and not keep:
                v = e.ray_kernel_variant()
                assert all(bool(v[k]) == w for k, w in want_variant.items()), v
            res_m.append((e.log_weights(), e.ray_steps().astype(np.int32).ravel() if keep else None, e.counters()["probes"]))
            e.close()
        out[metric] = res_m
    monkeypatch.delenv("MCL_WEDGE_METRIC", raising=False)
    return out


def check(orc, om, ang, p, obs, out, strictly_fewer=False):
    L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
    want_logw, _, _ = orc.eng_log_weights(om, p, ang, orc.obs_index(obs, om), L)
    _, want_steps = orc.cast_many(om, np.repeat(p[0], ang.size), np.repeat(p[1], ang.size),
                                  (p[2][:, None] + ang.astype(np.float64)[None, :]).ravel())
    want_steps = np.asarray(want_steps, np.int32).ravel()
    for metric, ((lw_walk, _, _), (lw_count, steps, probes)) in out.items():
        assert np.array_equal(lw_walk, want_logw), metric
        assert np.array_equal(lw_count, want_logw), metric
        assert np.array_equal(steps, want_steps), metric
        assert probes > 0
    old, new = out["0"][1][2], out[None][1][2]
    print(f"probes: Euclidean rule {old}, tight rule {new} ({new / old:.4f})")
    assert new <= old
    if strictly_fewer:
        assert new < old


@pytest.mark.parametrize("force,n,sig", [(0, 8192, (0.5, 0.5, 0.4)), (2, 2048, (0.2, 0.2, 0.4))])
def test_tracking_cloud_1081_beams_both_rules(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, force, n, sig):
    """The bench's shape in small; force = 2 sends every ray through level 2 (k_rays_fix: fp64 on the wedge field)."""
    ang = orc.beam_angles(angle_step=1)
    p = tracking_cloud(np.random.default_rng(3), n, sig=sig)
    obs = S.scan1081()
    out = run_both(engine_mod, monkeypatch, spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y, ang, p, obs,
                   debug_force_exact=force)
    check(orc, spielberg_oracle, ang, p, obs, out)


def test_scattered_particles_both_rules(orc, engine_mod, sibal1, sibal1_oracle, monkeypatch):
    """Rooms and corridors, 3000 scattered particles x 217 beams: walls beside the rays everywhere -- strictly fewer probes."""
    om = sibal1_oracle
    ang = orc.beam_angles(angle_step=5)
    assert ang.size == 217
    rng = np.random.default_rng(11)
    n = 3000
    p = np.stack([om.origin_x + rng.uniform(-2, 20, n), om.origin_y + rng.uniform(-2, 11, n), rng.uniform(-np.pi, np.pi, n)])
    obs = np.full(ang.size, 3.0, np.float32)
    out = run_both(engine_mod, monkeypatch, sibal1.data, sibal1.resolution, sibal1.origin_x, sibal1.origin_y, ang, p, obs)
    check(orc, om, ang, p, obs, out, strictly_fewer=True)


@pytest.mark.parametrize("form", ["global", "hybrid"])
def test_479_px_map_both_rules(orc, engine_mod, sibal1, monkeypatch, form):
    """The 0.025 m map of tests/test_gpu_sweep_global.py (479 px of range): the global-field form (the ringed, mirrored copies of
    the fields) and the hybrid (LDS windows first, then those copies)."""
    monkeypatch.setenv("MCL_SWEEP_HYBRID", "2" if form == "hybrid" else "0")
    grid = np.kron(sibal1.data, np.ones((2, 2), np.int8)).astype(np.int8)
    res = 0.025
    om = orc.OracleMap(grid, res, sibal1.origin_x, sibal1.origin_y)
    assert om.max_range_px == 479
    ang = orc.beam_angles(angle_step=12)
    rng = np.random.default_rng(41)
    n = 3000
    sx, sy = grid.shape[1] * res, grid.shape[0] * res
    p = np.stack([sibal1.origin_x + rng.uniform(-0.05 * sx, 1.05 * sx, n), sibal1.origin_y + rng.uniform(-0.05 * sy, 1.05 * sy, n),
                  rng.uniform(-np.pi, np.pi, n)])
    p[:, 100:700] = p[:, 100:101] + rng.normal(0, 0.02, (3, 600))                  # full 64-lane groups of near-identical rays
    obs = (rng.uniform(0.3, 13.0, ang.size)).astype(np.float32)
    out = run_both(engine_mod, monkeypatch, grid, res, sibal1.origin_x, sibal1.origin_y, ang, p, obs,
                   want_variant={"hybrid": form == "hybrid", "global_fields": form == "global"})
    check(orc, om, ang, p, obs, out)
