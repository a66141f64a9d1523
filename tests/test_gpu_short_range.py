"""A range shorter than a wave: with MAX_RANGE_PX below 64 the cooperative literal march (wave_march_exact_dir, mcl_ray_core.h)
has one round only, and part of its lanes are masked.  Every caller of the ray functions on one small map with 2 m of range:
the update's stored steps, mcl_query_scans and the beam search's table against the oracle's cast_ray as integers, the beam
refinement's volume against mcl_score_poses as bits -- with debug_force_exact (every ray takes the literal march) and without."""
import numpy as np
import pytest

import beam_search_ref as br
import test_gpu_search_beam as sb
from conftest import make_engine

pytestmark = pytest.mark.gpu

MAX_RANGE = 2.0
N, B = 64, 55
STRIDE, N_HEAD = 3, 8


def poses(m):
    """64 finite poses on the map: free ones, poses on cell corners and edges (the guard sends their rays to the literal march),
    one in the pillar, one a cell off the map"""
    res = float(np.float32(m.resolution))
    rng = np.random.default_rng(7)
    p = np.stack([sb.OX + rng.uniform(0.3, sb.W * res - 0.3, N), sb.OY + rng.uniform(0.3, sb.H * res - 0.3, N),
                  rng.uniform(-np.pi, np.pi, N)], axis=1)
    p[1] = (sb.OX + 50 * res, sb.OY + 15 * res, 0.3)             # a cell corner
    p[2] = (sb.OX + 50 * res, sb.OY + 15.4 * res, 1.0)           # on a vertical cell edge
    p[3] = (sb.OX + 50.3 * res, sb.OY + 16 * res, -1.0)          # on a horizontal one
    p[4] = (sb.OX + 42.5 * res, sb.OY + 57.5 * res, 0.5)         # inside the pillar
    p[5] = (sb.OX - res, sb.OY + 1.0, 0.1)                       # off the map
    return p


class Fixture:
    """the map, the oracle with 2 m of range and what it says (computed once, left unchanged)"""

    def __init__(self, orc, engine_mod):
        self.m = sb.SmallMap(0.05)
        self.om = orc.OracleMap(self.m.data, self.m.resolution, sb.OX, sb.OY, max_range_m=MAX_RANGE)
        self.P = self.om.max_range_px
        self.ang = sb.angles(orc, B)
        self.poses = poses(self.m)
        a = (self.poses[:, 2][:, None] + self.ang.astype(np.float64)[None, :]).ravel()
        self.steps = orc.cast_many(self.om, np.repeat(self.poses[:, 0], B), np.repeat(self.poses[:, 1], B), a)[1].reshape(N, B)
        a0 = self.poses[0, 2] + self.ang.astype(np.float64)
        self.scan = orc.cast_many(self.om, np.full(B, self.poses[0, 0]), np.full(B, self.poses[0, 1]), a0)[0].astype(np.float32)
        self.cells, self.xy = engine_mod.host_search_lattice(self.m.data, self.m.resolution, sb.OX, sb.OY, stride_cells=STRIDE)
        self.g = br.grid(self.ang, N_HEAD)
        self.table = br.table(orc, self.om, self.xy, self.g["phi"])
        for a in (self.steps, self.table):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def fx(orc, engine_mod):
    return Fixture(orc, engine_mod)


def test_the_fixture_has_a_partly_masked_round_hits_and_misses(fx):
    assert 0 < fx.P < 64                                     # one round of the wave's march, lanes P .. 63 masked
    for s in (fx.steps, fx.table):
        assert (s == fx.P).any() and (s < fx.P).any() and (s == 0).any() and (s == fx.P - 1).any()
    assert fx.cells.size > 256 and fx.g["M"] == 72


# ("sweep": the kernels that hand a ray to k_rays_fix and k_rays_exact; AUTO gives so few particles k_rays_skip)
@pytest.mark.parametrize("kernel", ["auto", "sweep"])
@pytest.mark.parametrize("force_exact", [1, 0])
def test_update_steps_are_cast_ray(engine_mod, fx, force_exact, kernel):
    rk = engine_mod.RAYS_SWEEP if kernel == "sweep" else engine_mod.RAYS_AUTO
    e = make_engine(engine_mod, fx.m, fx.ang, N, max_range_m=MAX_RANGE, keep_ray_steps=1, ray_kernel=rk, debug_force_exact=force_exact)
    assert e.max_range_px == fx.P
    e.set_particles(np.ascontiguousarray(fx.poses.T), np.full(N, 1.0 / N))
    e.sensor_update(fx.scan)
    assert np.array_equal(e.ray_steps().astype(np.int64), fx.steps)
    if force_exact:
        assert e.counters()["exact_fallback_rays"] == N * B > 0
    e.close()


@pytest.mark.parametrize("force_exact", [1, 0])
def test_side_calls(engine_mod, fx, force_exact):
    e = make_engine(engine_mod, fx.m, fx.ang, N, max_range_m=MAX_RANGE, debug_force_exact=force_exact)
    assert e.max_range_px == fx.P
    # the query
    _, steps = e.expected_scans(fx.poses, want_steps=True)
    assert np.array_equal(steps.astype(np.int64), fx.steps)
    l3_query = e.query_counters()["level3_rays"]
    # the beam search's table
    _, st = e.global_search_beam(fx.scan, max_hits=0, stride_cells=STRIDE, n_headings=N_HEAD)
    first, R = e.search_beam_table()
    assert st["n_tiles"] == 1 and first == 0 and np.array_equal(R.astype(np.int64), fx.table)
    # the beam refinement's volume is mcl_score_poses on the window, bit for bit
    seed = fx.poses[0]
    f = dict(half_xy=1, half_theta=0)
    _, rst = e.refine_poses_beam(seed, fx.scan, **f)
    got = e.refine_scores()
    want = e.score_poses(engine_mod.host_refine_window(seed, fx.m.resolution, **f), fx.scan)["log_likelihood"]
    assert got.shape == (1, 9) and not np.isnan(got).any()
    assert np.array_equal(sb.bits(got[0]), sb.bits(want))
    assert rst["level3_rays"] == e.query_counters()["level3_rays"]       # (the same rays take the literal march in both routes)
    if force_exact:
        assert l3_query == N * B > 0 and st["level3_rays"] == fx.table.size > 0 and rst["level3_rays"] == rst["rays"] == 9 * B > 0
    e.close()
