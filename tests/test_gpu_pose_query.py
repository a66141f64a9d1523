"""The pose query on the GPU (mcl_query_scans / mcl_score_poses, DESIGN.md §4.12, rules Q1-Q6 of include/mcl_hip_engine.h): the
expected scan and the scan score of poses that are not particles.  The statements it is held to: a twin engine that holds the same
poses as particles (set_particles + sensor_update + ray_steps / log_weights), the CPU oracle (cast_many, eng_log_weights), a numpy
statement of the counts, tests/lfield_ref.py with the likelihood field on; and that an engine which queries runs the same updates,
bit for bit, as one that never does."""
import numpy as np
import pytest

import lfield_ref as lr
import side_geometries as sg
from conftest import make_engine, tracking_cloud

pytestmark = pytest.mark.gpu

RES = np.float32(0.05)
OX, OY = -3.0, -2.25
MAX_RANGE = 12.0


class SmallMap:
    """120 x 90 cells at 0.05 m: an outer wall with two gaps (rays leave the map there), interior walls, a pillar, unknown cells"""

    def __init__(self, W=120, H=90, res=RES, ox=OX, oy=OY, grid=None):
        if grid is not None:
            self.data, self.resolution, self.origin_x, self.origin_y = grid, res, ox, oy
            return
        g = np.zeros((H, W), np.int8)
        g[0, :] = g[-1, :] = 100
        g[:, 0] = g[:, -1] = 100
        g[0, 30:40] = 0
        g[40:50, -1] = 0
        g[30, 20:70] = 100
        g[30:75, 85] = 100
        g[55:60, 40:45] = 100
        g[60:80, 5:15] = -1
        g[10:14, 100:110] = -1
        self.data, self.resolution, self.origin_x, self.origin_y = g, res, ox, oy


@pytest.fixture(scope="module")
def small():
    return SmallMap()


@pytest.fixture(scope="module")
def small_oracle(orc, small):
    return orc.OracleMap(small.data, small.resolution, small.origin_x, small.origin_y)


def angles(orc, B):
    """B beams over the Hokuyo's 270 degrees (B = 1081: the reference's own; B = 1: the first of them)"""
    full = orc.beam_angles()
    return full[np.linspace(0, full.size - 1, B).round().astype(int)].copy() if B > 1 else full[:1].copy()


def special_poses(m):
    """poses on cell corners and edges (the guard sends their rays to level 3), in an occupied cell, off the map on each side,
    and not finite / with a heading beyond 1e6"""
    res = float(np.float32(m.resolution))
    H, W = m.data.shape
    ox, oy = m.origin_x, m.origin_y
    x1, y1 = ox + W * res, oy + H * res
    return np.array([
        [ox + 50 * res, oy + 15 * res, 0.3],            # a cell corner
        [ox + 64 * res, oy + 48 * res, -2.0],           # another
        [ox + 50 * res, oy + 15.4 * res, 1.0],          # on a vertical cell edge
        [ox + 50.3 * res, oy + 16 * res, -1.0],         # on a horizontal one
        [ox + 42.5 * res, oy + 57.5 * res, 0.5],        # inside the pillar
        [ox - 0.4, oy + 1.0, 0.1],                      # off the map, each side
        [x1 + 0.7, oy + 2.0, 3.0],
        [ox + 1.5, oy - 0.3, 1.5],
        [ox + 2.0, y1 + 0.2, -1.5],
        [ox + 2.0, oy + 1.0, np.nan],
        [np.inf, oy + 1.0, 0.0],
        [ox + 2.0, oy + 1.0, 2e6],
    ])


N_FINITE_SPECIAL = 9


def free_poses(rng, m, k):
    """poses drawn inside the map's rectangle (a few land in walls or unknown cells: fine)"""
    res = float(np.float32(m.resolution))
    H, W = m.data.shape
    return np.stack([m.origin_x + rng.uniform(0.3, W * res - 0.3, k), m.origin_y + rng.uniform(0.3, H * res - 0.3, k),
                     rng.uniform(-np.pi, np.pi, k)], axis=1)


def poses_for(m, K, seed=1):
    """K poses: one free pose first, then the special ones as far as K allows, the rest free"""
    rng = np.random.default_rng(seed)
    p = free_poses(rng, m, K)
    p[0] = (m.origin_x + 2.03, m.origin_y + 0.77, 0.4)
    sp = special_poses(m)
    n = min(K - 1, len(sp))
    p[1:1 + n] = sp[:n]
    return p


scan_at = sg.scan_at


def odd_scan(scan, P, res):
    """the scan with readings that are not valid (NaN, +-inf, max range and beyond) and some that are (negative: row 0)"""
    s = sg.odd_scan(scan, MAX_RANGE)
    if 37 < s.size:
        s[37] = P * res
    return s


def twin(engine_mod, m, ang, poses, obs, **cfg):
    """what the parent commit offers: an engine holding the poses as particles -> (steps, log-weights, level-3 rays)"""
    K = len(poses)
    b = make_engine(engine_mod, m, ang, K, keep_ray_steps=1, **cfg)
    return twin_run(b, poses, obs)


def twin_run(b, poses, obs):
    K = len(poses)
    b.set_particles(np.ascontiguousarray(poses.T), np.full(K, 1.0 / K))
    b.sensor_update(obs)
    return b.ray_steps().astype(np.uint16), b.log_weights(), b.counters()["exact_fallback_rays"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def oracle_steps(orc, om, ang, poses):
    a = (poses[:, 2][:, None] + ang.astype(np.float64)[None, :]).ravel()
    r, s = orc.cast_many(om, np.repeat(poses[:, 0], ang.size), np.repeat(poses[:, 1], ang.size), a)
    return r.reshape(len(poses), ang.size), s.reshape(len(poses), ang.size)


# ---- 1. twin-engine equivalence
@pytest.mark.parametrize("force_exact", [0, 1])
@pytest.mark.parametrize("B", [1, 61, 1081])
def test_query_equals_a_twin_engine_holding_the_poses(orc, engine_mod, small, small_oracle, B, force_exact):
    """Engine A holds a tracking set and is queried; engine B gets the same poses as particles.  Steps exactly, log-likelihood bit
    for bit, at K on both sides of a wave and B that is no multiple of 64; A's own particles are untouched."""
    ang = angles(orc, B)
    rng = np.random.default_rng(B)
    a = make_engine(engine_mod, small, ang, 512, seed=5, debug_force_exact=force_exact)
    cloud = tracking_cloud(rng, 512, pose=(OX + 2.0, OY + 0.8, 0.4), sig=(0.1, 0.1, 0.1))
    a.set_particles(cloud, np.full(512, 1.0 / 512))
    b = make_engine(engine_mod, small, ang, 1000, keep_ray_steps=1, debug_force_exact=force_exact)
    P = a.max_range_px
    obs = odd_scan(scan_at(orc, small_oracle, ang, (OX + 2.03, OY + 0.77, 0.4)), P, float(RES))
    for K in (1, 63, 64, 65, 1000):
        poses = poses_for(small, K, seed=K)
        want_steps, want_logw, twin_l3 = twin_run(b, poses, obs)
        ranges, steps = a.expected_scans(poses, want_steps=True)
        l3 = a.query_counters()["level3_rays"]
        sc = a.score_poses(poses, obs)
        assert steps.dtype == np.uint16 and steps.shape == (K, B) and ranges.shape == (K, B)
        assert np.array_equal(steps, want_steps), (K, B, np.argwhere(steps != want_steps)[:5])
        assert np.array_equal(bits(sc["log_likelihood"]), bits(want_logw)), (K, B)
        assert np.array_equal(ranges, np.where(steps >= P, np.float32(MAX_RANGE), (steps.astype(np.float64) * float(RES)).astype(np.float32)))
        if force_exact:
            assert l3 == K * B                              # every ray took the literal march
        elif K >= 63:
            assert l3 >= 4 and twin_l3 >= 1                 # the corner / edge / non-finite poses reached level 3
        assert (sc["n_miss"] == (steps == P).sum(axis=1)).all()
    assert np.array_equal(a.get_particles(), cloud)
    a.close()
    b.close()


# ---- 2. the oracle
@pytest.mark.parametrize("B", [61, 1081])
def test_query_equals_the_oracle(orc, engine_mod, small, small_oracle, B):
    ang = angles(orc, B)
    K = 200
    poses = np.concatenate([poses_for(small, K)[:1 + N_FINITE_SPECIAL], free_poses(np.random.default_rng(3), small, K - 1 - N_FINITE_SPECIAL)])
    assert np.isfinite(poses).all()
    e = make_engine(engine_mod, small, ang, 16)
    P = e.max_range_px
    assert P == small_oracle.max_range_px
    obs = odd_scan(scan_at(orc, small_oracle, ang, poses[0]), P, float(RES))
    L = orc.eng_log_table(orc.sensor_table(P))
    want_logw, want_steps, _ = orc.eng_log_weights(small_oracle, np.ascontiguousarray(poses.T), ang, orc.obs_index(obs, small_oracle), L, want_steps=True)
    want_ranges, cast_steps = oracle_steps(orc, small_oracle, ang, poses)
    assert np.array_equal(cast_steps, want_steps.astype(np.int32))
    ranges, steps = e.expected_scans(poses, want_steps=True)
    sc = e.score_poses(poses, obs)
    assert np.array_equal(steps.astype(np.int32), cast_steps)
    assert np.array_equal(ranges.view(np.uint32), want_ranges.view(np.uint32))
    assert np.array_equal(bits(sc["log_likelihood"]), bits(want_logw))
    one = e.expected_scans(poses[0])                        # a single length-3 pose
    assert one.shape == (1, B) and np.array_equal(one[0], ranges[0])
    e.close()


# ---- 3. ranges beyond 255 px: 16-bit steps
def test_long_range_steps_are_16_bit_and_exact(orc, engine_mod):
    """60 x 400 cells at 0.025 m: 479 px of range on a map narrower than a ray is long"""
    H, W = 400, 60
    rng = np.random.default_rng(8)
    grid = np.zeros((H, W), np.int8)
    grid[rng.random((H, W)) < 0.01] = 100
    grid[0, :] = grid[-1, :] = 100
    m = SmallMap(res=np.float32(0.025), ox=-1.0, oy=-2.0, grid=grid)
    om = orc.OracleMap(grid, m.resolution, m.origin_x, m.origin_y)
    P = om.max_range_px
    assert P == 479
    ang = orc.beam_angles(angle_step=9)
    K = 96
    poses = free_poses(rng, m, K)
    poses[:12] = special_poses(m)
    obs = rng.uniform(0.2, 13.0, ang.size).astype(np.float32)
    e = make_engine(engine_mod, m, ang, 16)
    assert e.max_range_px == P
    ranges, steps = e.expected_scans(poses, want_steps=True)
    sc = e.score_poses(poses, obs)
    t_steps, t_logw, _ = twin(engine_mod, m, ang, poses, obs)
    assert steps.max() > 255
    assert np.array_equal(steps, t_steps)
    assert np.array_equal(bits(sc["log_likelihood"]), bits(t_logw))
    fin = np.isfinite(poses).all(axis=1) & (np.abs(poses[:, 2]) < 1e6)
    want_ranges, want_steps = oracle_steps(orc, om, ang, poses[fin])
    assert np.array_equal(steps[fin].astype(np.int32), want_steps)
    assert np.array_equal(ranges[fin].view(np.uint32), want_ranges.view(np.uint32))
    L = orc.eng_log_table(orc.sensor_table(P))
    want_logw, _, _ = orc.eng_log_weights(om, np.ascontiguousarray(poses[fin].T), ang, orc.obs_index(obs, om), L)
    assert np.array_equal(bits(sc["log_likelihood"][fin]), bits(want_logw))
    e.close()


# ---- 4. the counts
@pytest.mark.parametrize("lf", [False, True])
def test_counts_are_the_numpy_statement(orc, engine_mod, small, small_oracle, lf):
    """n_valid / n_agree / n_miss in integers from the cast steps and the scan's table rows (Q4), under either sensor model"""
    ang = angles(orc, 181)
    K = 100
    poses = poses_for(small, K, seed=4)
    e = make_engine(engine_mod, small, ang, 16)
    if lf:
        e.set_likelihood_field()
    P = e.max_range_px
    obs = odd_scan(scan_at(orc, small_oracle, ang, poses[0]), P, float(RES))
    obs[50:60] += 0.11                                      # two cells off: agree only with a tolerance
    _, steps = e.expected_scans(poses, want_steps=True)
    row = orc.obs_index(obs, small_oracle).astype(np.int64)
    valid = np.isfinite(obs) & (row < P)
    assert 0 < valid.sum() < obs.size and (row[~np.isfinite(obs)] < P).any()
    st = steps.astype(np.int64)
    seen = set()
    for tol in (0, 2, P):
        sc = e.score_poses(poses, obs, tol_steps=tol)
        agree = valid[None, :] & (np.abs(row[None, :] - st) <= tol)
        assert (sc["n_valid"] == valid.sum()).all()
        assert np.array_equal(sc["n_agree"], agree.sum(axis=1))
        assert np.array_equal(sc["n_miss"], (st == P).sum(axis=1))
        assert (sc["reserved"] == 0).all()
        seen.add(int(sc["n_agree"][0]))
    assert len(seen) == 3 and sc["n_agree"][0] == valid.sum()       # the tolerance matters; tol = P: every valid beam agrees
    e.close()


# ---- 5. the likelihood field
def test_likelihood_field_score_equals_twin_and_restatement(orc, engine_mod, small, small_oracle):
    ang = angles(orc, 181)
    K = 300
    poses = poses_for(small, K, seed=6)
    obs = odd_scan(scan_at(orc, small_oracle, ang, poses[0]), small_oracle.max_range_px, float(RES))
    e = make_engine(engine_mod, small, ang, 16)
    e.set_likelihood_field()
    sc = e.score_poses(poses, obs)
    b = make_engine(engine_mod, small, ang, K, keep_ray_steps=1)
    b.set_likelihood_field()
    b.set_particles(np.ascontiguousarray(poses.T), np.full(K, 1.0 / K))
    b.sensor_update(obs)
    assert np.array_equal(bits(sc["log_likelihood"]), bits(b.log_weights()))
    # the restatement, on poses for which it alone stays within the ambiguity cap of DESIGN.md §4.10 (checked here, on the CPU):
    # the free ones -- poses on cell corners put end points on cell edges
    free = np.r_[0, 1 + len(special_poses(small)):K]
    D, Lf = lr.field(small.data, small.resolution), lr.table(small.resolution)
    want, alts, n_amb = lr.log_weights(np.ascontiguousarray(poses[free].T), ang, obs, D, Lf, small.resolution, OX, OY, MAX_RANGE)
    beams = free.size * lr.used_beams(ang, obs, MAX_RANGE)[0].size
    assert n_amb.sum() <= max(1e-5 * beams, 2), (int(n_amb.sum()), beams)
    got = sc["log_likelihood"][free]
    for i in np.flatnonzero(bits(got) != bits(want)):
        assert int(i) in alts and got[i] in alts[int(i)], (int(i), got[i], want[i])
    # the counts still come from cast rays
    _, steps = e.expected_scans(poses, want_steps=True)
    e.set_likelihood_field(False)
    beam = e.score_poses(poses, obs)
    for f in ("n_valid", "n_agree", "n_miss"):
        assert np.array_equal(sc[f], beam[f])
    assert np.array_equal(sc["n_miss"], (steps == e.max_range_px).sum(axis=1))
    assert not np.array_equal(bits(beam["log_likelihood"]), bits(sc["log_likelihood"]))
    e.close()
    b.close()


# ---- 6. read-only
def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


@pytest.mark.parametrize("n,B,path,kld", [(2000, 61, "tiny", False), (2000, 61, "tiny", True), (32768, 61, "graph", False),
                                          (70000, 1081, "regular", False), (70000, 1081, "regular", True)])
def test_queries_leave_every_later_update_bit_identical(orc, engine_mod, small, small_oracle, n, B, path, kld):
    """Two engines with the same seed run 6 updates; one is queried before, between and after them.  Particles, weights, parents
    and the expected pose agree bit for bit after every update, on the three-launch path, the captured graph and a regular
    update (k_rays_sweep), with KLD on and off; the warm paths stay warm."""
    ang = angles(orc, B)
    true = np.array([OX + 2.03, OY + 0.77, 0.4])
    obs = scan_at(orc, small_oracle, ang, true)
    poses = poses_for(small, 64, seed=9)
    cloud = tracking_cloud(np.random.default_rng(n), n, pose=tuple(true), sig=(0.15, 0.15, 0.1))
    engines = []
    for _ in range(2):
        e = make_engine(engine_mod, small, ang, n, seed=77)
        if kld:
            e.set_kld(min_particles=n, max_particles=n)                # (N stays: the warm paths stay in play)
        e.set_particles(cloud, np.full(n, 1.0 / n))
        engines.append(e)
    plain, asked = engines
    assert asked.query_counters()["device_bytes"] == 0                  # nothing allocated before the first query
    first = asked.score_poses(poses, obs)
    for upd in range(6):
        for e in engines:
            e.update((0.02, 0.0, 0.01), obs)
        if upd >= 1:
            assert path_of(asked) == path_of(plain)
            if path != "regular" and not kld:
                assert path_of(asked) == path
        if path == "regular":
            assert asked.ray_kernel_name() == "k_rays_sweep"
        for f in ("get_particles", "get_weights", "resample_indices", "expected_pose"):
            ga, gp = getattr(asked, f)(), getattr(plain, f)()
            assert ga.tobytes() == gp.tobytes(), (f, upd)
        asked.expected_scans(poses[:3 + upd])
        again = asked.score_poses(poses, obs)
        assert again.tobytes() == first.tobytes()                       # and the query does not depend on the filter's state
    assert plain.query_counters()["device_bytes"] == 0
    for e in engines:
        e.close()


# ---- 7. determinism and buffer growth
def test_same_query_same_bits_and_buffers_grow(orc, engine_mod, small, small_oracle):
    ang = angles(orc, 61)
    e = make_engine(engine_mod, small, ang, 16)
    obs = scan_at(orc, small_oracle, ang, (OX + 2.03, OY + 0.77, 0.4))
    big = poses_for(small, 1000, seed=2)
    r1, s1 = e.expected_scans(big[:1], want_steps=True)
    bytes1 = e.query_counters()["device_bytes"]
    rb, sb = e.expected_scans(big, want_steps=True)
    assert e.query_counters()["device_bytes"] > bytes1 > 0
    r1b, s1b = e.expected_scans(big[:1], want_steps=True)
    assert np.array_equal(s1, s1b) and r1.tobytes() == r1b.tobytes()
    assert np.array_equal(sb[0], s1[0]) and rb[0].tobytes() == r1[0].tobytes()
    grown = e.query_counters()["device_bytes"]
    for _ in range(2):
        r2, s2 = e.expected_scans(big, want_steps=True)
        assert r2.tobytes() == rb.tobytes() and np.array_equal(s2, sb)
    a, b = e.score_poses(big[:1], obs), e.score_poses(big, obs)
    c = e.score_poses(big, obs)
    assert b.tobytes() == c.tobytes() and a[0] == b[0]
    assert e.score_poses(big[:1], obs).tobytes() == a.tobytes()
    again = e.query_counters()["device_bytes"]
    e.score_poses(big, obs)
    e.expected_scans(big)
    assert e.query_counters()["device_bytes"] == again >= grown          # nothing grows once the sizes have been seen
    e.close()


# ---- 8. refusals
def test_refusals(orc, engine_mod, small):
    ang = angles(orc, 61)
    pose = np.array([[OX + 2.0, OY + 0.8, 0.0]])
    obs = np.ones(61, np.float32)

    def status(f, *a, **k):
        with pytest.raises(engine_mod.EngineError) as ei:
            f(*a, **k)
        return ei.value.status

    e = engine_mod.Engine(max_particles=16)
    e.n_beams = 61
    assert status(e.expected_scans, pose) == -2 and status(e.score_poses, pose, obs) == -2       # no map
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    assert status(e.expected_scans, pose) == -2 and status(e.score_poses, pose, obs) == -2       # no beams
    e.set_beam_angles(ang)
    assert e.expected_scans(pose).shape == (1, 61)                                               # no particles needed
    assert status(e.expected_scans, np.zeros((0, 3))) == -1
    assert status(e.expected_scans, np.zeros((65537, 3))) == -1
    assert status(e.score_poses, np.zeros((0, 3)), obs) == -1
    assert status(e.score_poses, np.zeros((65537, 3)), obs) == -1
    assert status(e.score_poses, pose, obs[:60]) == -1
    assert status(e.score_poses, pose, obs, tol_steps=-1) == -1
    assert status(e.score_poses, pose, obs, tol_steps=e.max_range_px + 1) == -1
    assert e.lib.mcl_query_scans(e._h, None, 1, None, None) == -1
    assert e.score_poses(pose, obs, tol_steps=e.max_range_px)["n_valid"][0] == 61
    e.close()
    p = make_engine(engine_mod, small, ang, 16, weight_mode=engine_mod.WEIGHT_PRODUCT, keep_ray_steps=1)
    assert status(p.score_poses, pose, obs) == -1
    ranges, steps = p.expected_scans(pose, want_steps=True)
    q = make_engine(engine_mod, small, ang, 16)
    assert np.array_equal(steps, q.expected_scans(pose, want_steps=True)[1])
    p.close()
    q.close()


# ---- 9. ranking the means of pose_clusters
def test_scores_rank_the_cluster_at_the_true_pose_first(orc, engine_mod, small, small_oracle):
    """Two Gaussian clouds, one at the scan's true pose: the scan supports the mean of that cluster, by count and by likelihood.
    (The oracle shows the margin on the CPU first: at the two centres the agreeing beams differ by more than a factor of two.)"""
    ang = angles(orc, 181)
    true = np.array([OX + 2.03, OY + 0.77, 0.4])
    decoy = np.array([OX + 4.6, OY + 3.4, -2.2])
    obs = scan_at(orc, small_oracle, ang, true)
    P = small_oracle.max_range_px
    row = orc.obs_index(obs, small_oracle).astype(np.int64)
    valid = np.isfinite(obs) & (row < P)
    _, st = oracle_steps(orc, small_oracle, ang, np.stack([true, decoy]))
    agree = (valid[None, :] & (np.abs(row[None, :] - st) <= 2)).sum(axis=1)
    assert agree[0] == valid.sum() and agree[0] > 2 * agree[1]
    rng = np.random.default_rng(12)
    n = 600
    cloud = np.concatenate([tracking_cloud(rng, n, tuple(true), sig=(0.02, 0.02, 0.01)),
                            tracking_cloud(rng, n + 200, tuple(decoy), sig=(0.02, 0.02, 0.01))], axis=1)      # the decoy is the heavier mode
    e = make_engine(engine_mod, small, ang, cloud.shape[1])
    e.set_particles(cloud, np.full(cloud.shape[1], 1.0 / cloud.shape[1]))
    clusters, info = e.pose_clusters(8)
    assert info["n_clusters"] >= 2
    means = clusters["mean"]
    sc = e.score_poses(means, obs)
    at_true = int(np.argmin(np.hypot(means[:, 0] - true[0], means[:, 1] - true[1])))
    assert np.hypot(*(means[at_true, :2] - true[:2])) < 0.05 and at_true != 0
    others = np.delete(np.arange(len(means)), at_true)
    assert (sc["n_agree"][at_true] > sc["n_agree"][others]).all()
    assert (sc["log_likelihood"][at_true] > sc["log_likelihood"][others]).all()
    e.close()


# ---- 10. a shard of a device group
def test_query_through_a_group_shard_equals_the_single_engine(orc, engine_mod, small, small_oracle):
    ang = angles(orc, 61)
    poses = poses_for(small, 100, seed=10)
    obs = scan_at(orc, small_oracle, ang, poses[0])
    one = make_engine(engine_mod, small, ang, 16)
    g = engine_mod.Group([0, 0], max_particles=256, seed=3)
    g.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    g.set_beam_angles(ang)
    shard = g.engine(1)
    assert shard.n_beams == 61
    r0, s0 = one.expected_scans(poses, want_steps=True)
    r1, s1 = shard.expected_scans(poses, want_steps=True)
    assert np.array_equal(s0, s1) and r0.tobytes() == r1.tobytes()
    assert one.score_poses(poses, obs).tobytes() == shard.score_poses(poses, obs).tobytes()
    one.close()
    g.close()
