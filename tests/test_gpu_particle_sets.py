"""Updates on the GPU over the particle-set family of tests/particle_sets.py: counts that are no multiple of a wave, a leader group,
the tail's thread count or a scan tile, and start weights whose structure is chosen (all weight on one end, exactly 63 / 64 / 65
particles alive, a list one short of its room, full, and one too long).  Every comparison is one the suite already makes
(tests/whole_set.py: indices, log-weights, fixed-point weights, Q and the maximum bit for bit, children within 1e-13, sums within
sum_rel_bound; the statements of the features in their own reference modules); no tolerance of this module's own.  Spielberg, 61
beams up to 8192 particles and 271 above.

Each case asserts the path it took -- the tail (regular / tiny / graph), the ray kernel, the length of the compact parent list and
whether the draw used it -- so that a moved threshold or a list that silently was not used fails the test.

  a. test_every_member           every (count, pattern), both resampling modes, three updates through WholeSet.step
  b. test_list_off               the same chain with MCL_NO_COMPACT=1: the full CDF (tile_excl / leaders, or the CDF in LDS), bit for bit (a)
  c. test_forced_ray_kernels     k_rays_sweep and k_rays_cell at 1, 65, 257, 1025, 8193 particles: steps are cast_ray's
  d. test_sample_more_rows_than_the_engine_holds, test_product_weights, test_kept_update_carries, test_likelihood_field,
     test_recovery_injection, test_pose_clusters, test_initialisations      the count-dependent features at 1, 65, 1025 and 8193
  e. test_kld_walks_through_ragged_sizes, test_kld_pinned_to_one_particle
  f. test_group_of_ragged_shards, test_group_gathered_weights, test_one_rank_comm_update"""
import os

import numpy as np
import pytest

import motion_ref as mr
import particle_sets as ps
import whole_set as ws
from conftest import GOLDEN, make_engine
from test_gpu_clusters import check as check_clusters, spielberg_geom
from test_gpu_group import make_group
from test_gpu_likelihood_field import Ambiguity, check_logw
from test_gpu_mixture_init import bits
from test_gpu_motion_model import assert_poses
from test_gpu_recovery import force_p
from test_kld_host import np_bins
from test_recovery_host import child_draws, free_cells, injected_poses, threshold

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0062
FEATURE_COUNTS = (1, 65, 1025, 8193)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


class World:
    def __init__(self, engine_mod, orc, m, om):
        self.mod, self.orc, self.m, self.om = engine_mod, orc, m, om
        self.L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
        self._ang, self._scan, self._lf = {}, {}, None

    def ang(self, step):
        if step not in self._ang:
            self._ang[step] = self.orc.beam_angles(angle_step=step)
        return self._ang[step]

    def scan(self, step):
        if step not in self._scan:
            s = np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32).copy()
            s.setflags(write=False)
            self._scan[step] = s
        return self._scan[step]

    def engine(self, n, step, **cfg):
        return make_engine(self.mod, self.m, self.ang(step), n, **cfg)

    def checker(self, e, step, seed, p0, w0, mode=0, rng=0):
        return ws.WholeSet(self.orc, self.om, e, self.ang(step), seed, p0, self.orc.eng_quantize_weights(w0), mode=mode, L=self.L,
                           rng=np.random.default_rng(rng))

    @property
    def lf(self):
        if self._lf is None:
            import lfield_ref as lr
            self._lf = dict(D=lr.field(self.m.data, self.m.resolution), Lf=lr.table(self.m.resolution))
        return self._lf


@pytest.fixture(scope="module")
def W(engine_mod, orc, spielberg, spielberg_oracle):
    return World(engine_mod, orc, spielberg, spielberg_oracle)


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def read_q(e, n):
    """the engine's fixed-point weights"""
    import torch
    qt = torch.empty(n, dtype=torch.int64, device="cuda")
    e.export_state(0, 0, 0, qt.data_ptr())
    return qt.cpu().numpy().view(np.uint64)


def sample_ks(n):
    """sample_particles draws per update: more than n (at most 1025), one, a wave and one"""
    return (min(1025, 3 * n + 1), 1, 65)


def tail_paths(n):
    """a set from outside takes the regular update; after it the one-workgroup tail up to 8192 particles, the captured graph above"""
    return ["regular"] + (["tiny"] if n <= ps.TINY_TAIL_MAX else ["graph"]) * 2


def list_after_update(n, q, no_compact=False):
    """the list an update of n particles leaves: k_tiny_tail (up to 8192 particles, LOG weights, no adaptive resampling) writes none"""
    if no_compact or n <= ps.TINY_TAIL_MAX:
        return -1
    return ps.list_length(np.count_nonzero(q), n)


def start_engine(W, member, mode, seed, **cfg):
    """a fresh engine holding the member's start set, checked: (engine, checker, length of the list set_particles left)"""
    n, pattern = member
    step = ps.beams_step(n)
    p0, w0 = ps.start(n, pattern)
    e = W.engine(n, step, seed=seed, resample_mode=mode, **cfg)
    e.set_particles(p0, w0)
    c = W.checker(e, step, seed, p0, w0, mode=mode, rng=n)
    ws.assert_same("set_particles", e.get_particles(), p0)
    ws.assert_same("set_particles: fixed-point weights", c.read_q(n), c.q)
    assert np.count_nonzero(c.q) == ps.alive(n, pattern)
    return e, c, ps.list_length(ps.alive(n, pattern), n)


# ---- a. every member
@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("member", ps.members(), ids=ps.member_id)
def test_every_member(W, member, mode):
    n, pattern = member
    step = ps.beams_step(n)
    e, c, n_list = start_engine(W, member, mode, SEED + mode)
    assert e.compact_list() == (n_list, False), (e.compact_list(), n_list)        # set_particles scans at every size: a list unless too long
    for k in sample_ks(n):
        c.sample_k = k
        info = c.step(W.scan(step))
        used, n_list = n_list > 0, list_after_update(n, c.q)
        assert e.compact_list() == (n_list, used), (info["update"], e.compact_list(), n_list, used)
    assert [r["path"] for r in c.log] == tail_paths(n), c.log
    assert all(r["kernel"] == "k_rays_skip" == r["planned"] for r in c.log), c.log
    assert all(r["q_total"] > 0 for r in c.log)
    if pattern in ("first", "last"):
        assert c.log[0]["compact_used"]                                   # a list of one entry: no ctop group, a ragged tail of one
    print(f"{ps.member_id(member)} mode {mode}: paths {[r['path'] for r in c.log]}, lists used {[r['compact_used'] for r in c.log]}, "
          f"alive {np.count_nonzero(c.q)}, list {e.compact_list()[0]}")
    e.close()


# ---- b. the list off
OFF_COUNTS = ps.LARGE + (65, 1025)


@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("member", ps.members(OFF_COUNTS), ids=ps.member_id)
def test_list_off(W, monkeypatch, member, mode):
    """MCL_NO_COMPACT=1: every draw searches the full CDF -- all weight on particle n - 1 lands in the ragged last leader group (or the
    last entry of the CDF in LDS), all weight on particle 0 in the first -- and equals the oracle and the engine with the list, bit
    for bit"""
    n, pattern = member
    step = ps.beams_step(n)
    a, _, n_list = start_engine(W, member, mode, SEED + mode)
    monkeypatch.setenv("MCL_NO_COMPACT", "1")
    b, c, _ = start_engine(W, member, mode, SEED + mode)
    monkeypatch.delenv("MCL_NO_COMPACT")
    assert b.compact_list() == (-1, False)
    for u, k in enumerate(sample_ks(n)):
        c.sample_k = k
        a.update(ws.ACTION, W.scan(step))
        c.step(W.scan(step))
        assert b.compact_list() == (-1, False)
        assert a.compact_list()[1] == (n_list > 0), (u, a.compact_list(), n_list)
        n_list = list_after_update(n, c.q)
        idx = b.resample_indices()
        ws.assert_same(f"update {u}: indices, list on / off", a.resample_indices(), idx)
        for what, x, y in (("particles", a.get_particles(), b.get_particles()), ("log-weights", a.log_weights(), b.log_weights()),
                           ("weights", a.get_weights(), b.get_weights()), ("scalars", a.scalars(), b.scalars())):
            ws.assert_same(f"update {u}: {what}, list on / off", x, y)
        if u == 0 and pattern == "last":
            assert (idx == n - 1).all()
        if u == 0 and pattern == "first":
            assert (idx == 0).all()
        if u == 0 and pattern == "ends":
            assert set(np.unique(idx).tolist()) == {0, n - 1}
    assert [r["path"] for r in c.log] == tail_paths(n), c.log
    a.close()
    b.close()


# ---- c. forced ray kernels at ragged counts
@pytest.mark.parametrize("kernel", ["sweep", "cell"])
@pytest.mark.parametrize("n", [1, 65, 257, 1025, 8193])
def test_forced_ray_kernels(W, n, kernel):
    """fewer particles than a chunk, a slice, a wave or a counting-sort bucket row: two updates, every particle through the checker,
    every stored step the oracle's cast_ray"""
    step, name = ps.beams_step(n), "k_rays_" + kernel
    rk = W.mod.RAYS_SWEEP if kernel == "sweep" else W.mod.RAYS_CELL
    e, c, _ = start_engine(W, (n, "flat"), 0, SEED + 2, ray_kernel=rk, keep_ray_steps=1)
    assert e.planned_ray_kernel(n)[0] == name
    ang = W.ang(step)
    for u in range(2):
        c.sample_k = min(65, 3 * n + 1)
        c.step(W.scan(step))
        p = c.p
        _, steps, _ = W.orc.eng_log_weights(W.om, p, ang, W.orc.obs_index(W.scan(step), W.om), W.L, want_steps=True)
        a = (p[2][:, None] + ang.astype(np.float64)[None, :]).ravel()
        cast = W.orc.cast_many(W.om, np.repeat(p[0], ang.size), np.repeat(p[1], ang.size), a, use_omp=True)[1].reshape(n, ang.size)
        assert np.array_equal(steps.astype(np.int32), cast)
        got = e.ray_steps().astype(np.int32)
        bad = np.argwhere(got != cast)
        assert bad.size == 0, (u, len(bad), bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), cast[tuple(bad[:5].T)].tolist())
    assert [r["kernel"] for r in c.log] == [name] * 2, c.log
    assert [r["path"] for r in c.log] == ["regular"] * 2, c.log              # a forced windowed kernel never takes a short tail
    e.close()


# ---- d. count-dependent features
@pytest.mark.parametrize("n", FEATURE_COUNTS)
def test_product_weights(W, n):
    """weight_mode PRODUCT (the reference's product of table entries): steps exactly, weights within the 1e-12 of
    test_weights_match_reference_product, and the next draw is the exact search on the fixed-point weights the engine holds"""
    step, seed = 18, SEED + 3
    orc, ang, scan = W.orc, W.ang(step), W.scan(step)
    p, w0 = ps.start(n, "flat")
    e = W.engine(n, step, seed=seed, keep_ray_steps=1, weight_mode=W.mod.WEIGHT_PRODUCT)
    e.set_particles(p, w0)
    q = orc.eng_quantize_weights(w0)
    table = orc.sensor_table(W.om.max_range_px)
    for u in range(3):
        e.update(ws.ACTION, scan)
        idx = orc.eng_resample_indices(q, 0, n_children=n, k53=orc.eng_philox_k53(seed, u, 0, n))
        ws.assert_same(f"update {u}: resample indices", e.resample_indices(), idx)
        parts = e.get_particles()
        ws.assert_close(f"update {u}: children", parts, orc.motion_model(p[:, idx], ws.ACTION, orc.eng_philox_normals(seed, u, 0, n)), 1e-13, 1e-13)
        w, steps, _ = orc.sensor_model(W.om, parts, ang, scan, table)
        assert np.array_equal(e.ray_steps().astype(np.int32), steps)
        assert w.sum() > 0.0
        np.testing.assert_allclose(e.get_weights(), w / w.sum(), rtol=1e-12, atol=0)
        q = read_q(e, n)
        assert int(q.max()) == 1 << 36                                    # scaled by the heaviest weight; the light ones may round to 0
        p = parts
        assert path_of(e) == "regular"                                   # PRODUCT never takes a short tail
    e.close()


@pytest.mark.parametrize("n", [1, 3, 65])
def test_sample_more_rows_than_the_engine_holds(W, n):
    """mcl_sample_particles takes 1 <= k <= 65536 whatever max_particles is.  (Its rows and uniforms share a scratch of 3 x
    max_particles doubles: an engine of one particle refused every draw, one of 65 every draw of more than 48 rows, until the call
    grew the scratch.)  The exact-CDF search against the oracle, the readbacks that share the scratch afterwards, and the refusals"""
    p, w = ps.start(n, "ends")
    e = W.engine(n, 18, seed=SEED + 14)
    e.set_particles(p, w)
    q = W.orc.eng_quantize_weights(w)
    rng = np.random.default_rng(n)
    for k in (1, n, 4 * n + 1, 4097, 65536):
        u = rng.random(k)
        idx = W.orc.eng_resample_indices(q, 0, n_children=k, k53=ws.injected_k53(u))
        ws.assert_same(f"sample_particles({k})", e.sample_particles(k, u), p[:, idx])
        assert set(np.unique(idx).tolist()) <= {0, n - 1}
        ws.assert_same("get_weights after it", e.get_weights(), w / w.sum())
    idx = W.orc.eng_resample_indices(q, 0, n_children=100, k53=ws.native_sample_k53(W.orc, SEED + 14, 0, 100))
    ws.assert_same("sample_particles (Philox stream 4)", e.sample_particles(100), p[:, idx])
    for bad in (0, 65537):
        with pytest.raises(W.mod.EngineError) as ei:
            e.sample_particles(bad)
        assert ei.value.status == W.mod.MCL_ERR_INVALID_ARG
    e.update(ws.ACTION, W.scan(18))                                       # and the engine goes on
    assert path_of(e) == "regular"
    e.close()


NEFF_PERMILLE = 20         # 121 beams leave N_eff near 0.025 n after a draw and far below 0.02 n after a kept update: the branches alternate


@pytest.mark.parametrize("n", FEATURE_COUNTS)
def test_kept_update_carries(W, n):
    """resample_neff_permille: the scalar restatement of test_adaptive_resampling_neff_option, with this module's comparisons.  A
    kept update reports resampled False and its log-weights add; the one after a collapse resamples.  At n = 1 N_eff is 1 = n:
    every update after the first keeps, whatever the threshold"""
    step, seed, r = 9, SEED + 4, NEFF_PERMILLE
    orc, om, ang, scan = W.orc, W.om, W.ang(step), W.scan(step)
    rng = np.random.default_rng(n)
    p = ps.cloud(rng, n, sig=(0.03, 0.03, 0.01))
    w = np.full(n, 1.0 / n)
    e = W.engine(n, step, seed=seed, resample_neff_permille=r)
    e.set_particles(p, w)
    oi = orc.obs_index(scan, om)
    q, carry, kept = orc.eng_quantize_weights(w), None, []
    for u in range(8):
        neff = w.sum() ** 2 / (w * w).sum()
        keep = carry is not None and neff >= r / 1000.0 * n
        assert carry is None or n == 1 or abs(neff / n - r / 1000.0) > 1e-6       # the input stays away from the threshold
        e.update(ws.ACTION, scan)
        assert e.effective_sample_size()[1] == (not keep), (u, kept, neff)
        idx = np.arange(n) if keep else orc.eng_resample_indices(q, 0, n_children=n, k53=orc.eng_philox_k53(seed, u, 0, n))
        ws.assert_same(f"update {u}: resample indices", e.resample_indices(), idx.astype(np.int32))
        parts = e.get_particles()
        ws.assert_close(f"update {u}: children", parts, orc.motion_model(p[:, idx], ws.ACTION, orc.eng_philox_normals(seed, u, 0, n)), 1e-13, 1e-13)
        logw, _, _ = orc.eng_log_weights(om, parts, ang, oi, W.L)
        if keep:
            logw = logw + carry
        ws.assert_same(f"update {u}: log-weights", e.log_weights(), logw)
        w, q, mx = orc.eng_weights_from_log(logw)
        carry = logw - mx
        ws.assert_same(f"update {u}: fixed-point weights", read_q(e, n), q)
        sc = e.scalars()
        ws.check_scalars(sc, w, q, mx, parts)
        ws.check_readbacks(e, sc, w)
        assert path_of(e) == "regular"                                   # adaptive resampling never takes a short tail
        assert e.compact_list()[0] == ps.list_length(np.count_nonzero(q), n)       # (the regular scan at every size)
        p = parts
        kept.append(keep)
    print(f"n {n}, {r} permille: kept {kept}")
    if n == 1:
        assert kept == [False] + [True] * 7
    else:
        i = kept.index(True)
        assert False in kept[i:], kept                                   # a kept update, and a resampling one after it
    e.close()


@pytest.mark.parametrize("n", FEATURE_COUNTS)
def test_likelihood_field(W, n):
    """k_lfield, one lane per particle, against tests/lfield_ref.py on the set as given and on two updates"""
    step = ps.beams_step(n)
    p0, w0 = ps.start(n, "flat")
    e = W.engine(n, step, seed=SEED + 5)
    e.set_likelihood_field()
    e.set_particles(p0, w0)
    tally = Ambiguity()
    e.sensor_update(W.scan(step))
    lw = check_logw(e, W.lf, W.m, W.ang(step), W.scan(step), tally)
    _, q, _ = W.orc.eng_weights_from_log(lw)                              # (a sensor update weighs the set; it draws nothing)
    for u in range(2):
        parents = e.get_particles()
        e.update(ws.ACTION, W.scan(step))
        idx = W.orc.eng_resample_indices(q, 0, n_children=n, k53=W.orc.eng_philox_k53(SEED + 5, u, 0, n))
        ws.assert_same(f"update {u}: resample indices", e.resample_indices(), idx)
        ws.assert_close(f"update {u}: children", e.get_particles(),
                        W.orc.motion_model(parents[:, idx], ws.ACTION, W.orc.eng_philox_normals(SEED + 5, u, 0, n)), 1e-13, 1e-13)
        lw = check_logw(e, W.lf, W.m, W.ang(step), W.scan(step), tally)
        _, q, _ = W.orc.eng_weights_from_log(lw)
        assert path_of(e) == "regular"                                   # a likelihood-field update never takes a short tail
    tally.check()
    e.close()


@pytest.mark.parametrize("n,p", [(1, 1.0), (1, 0.3), (65, 0.3), (1025, 0.3), (8193, 0.3)])
def test_recovery_injection(W, n, p):
    """the threshold forced through set_recovery_state: the injected set is the stream-8 coins', every injected pose the free-cell
    rule's, every other child the plain draw's (an engine without recovery), the count the coins'"""
    step, seed, m = 18, SEED + 6, W.m
    p0, w0 = ps.start(n, "flat")
    a, b = (W.engine(n, step, seed=seed) for _ in range(2))
    for e in (a, b):
        e.set_particles(p0, w0)
    a.set_recovery()
    for e in (a, b):
        e.update(ws.ACTION, W.scan(step))                                  # (the short tails need one regular update first)
    assert a.recovery_state()[3] == 0
    ws.assert_same("warm-up", a.get_particles(), b.get_particles())
    T = threshold(force_p(a, p))
    assert T > 0
    for e in (a, b):
        e.update(ws.ACTION, W.scan(step))
    assert path_of(a) == path_of(b) == tail_paths(n)[1]
    coin, pick, hb = child_draws(seed, 1, n)
    inj = coin < np.uint64(T)
    if p >= 1.0:
        assert inj.all()
    idx_a, idx_b = a.resample_indices(), b.resample_indices()
    assert np.array_equal(np.flatnonzero(idx_a == -1), np.flatnonzero(inj))
    assert np.array_equal(idx_a[~inj], idx_b[~inj])
    pa, pb = a.get_particles(), b.get_particles()
    want_inj = injected_poses(pick[inj], hb[inj], free_cells(m.data), m.data.shape[1], m.resolution, m.origin_x, m.origin_y)
    ws.assert_same("injected poses", pa[:, inj], want_inj)
    ws.assert_same("non-injected children", pa[:, ~inj], pb[:, ~inj])
    logw, _, _ = W.orc.eng_log_weights(W.om, pa, W.ang(step), W.orc.obs_index(W.scan(step), W.om), W.L)
    ws.assert_same("log-weights", a.log_weights(), logw)
    assert a.recovery_state()[3] == int(inj.sum())
    print(f"n {n}, p {p}: injected {int(inj.sum())}, path {path_of(a)}")
    a.update(ws.ACTION, W.scan(step))                                     # the update after the injecting one
    assert a.recovery_state()[3] == 0
    logw, _, _ = W.orc.eng_log_weights(W.om, a.get_particles(), W.ang(step), W.orc.obs_index(W.scan(step), W.om), W.L)
    ws.assert_same("log-weights after", a.log_weights(), logw)
    a.close()
    b.close()


def lone_cluster(got, info, p):
    """one particle: one cluster with its exact integer weight at the particle's position, no spread in x and y.  Its heading is the
    circular mean atan2(q sin, q cos), which may differ from theta in the last place (the 8 * 2^-53 * pi that
    test_gpu_clusters.check allows the mean); the heading variance is exactly that difference squared"""
    import math
    assert info["n_clusters"] == 1 and int(got[0]["weight_q"]) == 1 << 36 and int(got[0]["n_particles"]) == 1 and got[0]["weight"] == 1.0
    assert np.array_equal(got[0]["mean"][:2], p[:2, 0])
    dt = math.remainder(p[2, 0] - got[0]["mean"][2], 2.0 * math.pi)
    assert abs(dt) <= 8 * ws.U * math.pi
    want = np.zeros((3, 3))
    want[2, 2] = dt * dt
    ws.assert_same("covariance of one particle", got[0]["cov"], want)


@pytest.mark.parametrize("n", FEATURE_COUNTS)
def test_pose_clusters(W, n):
    """mcl_pose_clusters against tests/clusters_ref.py on the set as given (half on each end) and after an update"""
    step = ps.beams_step(n)
    p0, w0 = ps.start(n, "ends")
    e = W.engine(n, step, seed=SEED + 7)
    e.set_particles(p0, w0)
    geom = spielberg_geom(W.m)
    got, info, labels = check_clusters(e, geom)
    assert info["q_total"] == (1 if n == 1 else 2) << 36 and (labels >= 0).sum() == min(n, 2)
    if n == 1:
        lone_cluster(got, info, p0)
    e.update(ws.ACTION, W.scan(step))
    got, info, _ = check_clusters(e, geom)
    assert info["n_clusters"] >= 1
    if n == 1:
        lone_cluster(got, info, e.get_particles())
    e.close()


@pytest.mark.parametrize("n", [1, 65])
def test_initialisations(W, n):
    """the four device initialisations against their CPU statements, and an update from each"""
    step, seed, orc = 18, SEED + 8, W.orc
    pose, mean = (0.0, 0.0, 0.0), (0.3, -0.2, 3.0)
    cov = np.array([[0.30, 0.12, 0.01], [0.12, 0.20, -0.02], [0.01, -0.02, 0.05]])
    flat = np.full(n, 1.0 / n)

    def run(e, p0, upd=0):
        c = W.checker(e, step, seed, p0, flat)
        c.upd, c.sample_k = upd, min(65, 3 * n + 1)
        c.step(W.scan(step))

    e = W.engine(n, step, seed=seed)
    e.init_particles_pose(pose, n)
    p0 = e.get_particles()
    ws.assert_close("init_particles_pose", p0, orc.eng_init_pose(seed, 0, pose, 0, n), 1e-13, 1e-13)
    ws.assert_same("weights", e.get_weights(), flat)
    run(e, p0)
    e.init_global(n)                                                      # the second initialisation of this engine: init index 1
    p0 = e.get_particles()
    ws.assert_same("init_global", p0, orc.eng_init_global(seed, 1, W.om, 0, n))
    run(e, p0, upd=1)
    e.init_particles_gaussian(mean, cov, n)
    p0 = e.get_particles()
    assert_poses(p0, mr.init_gaussian(seed, 2, mean, cov, 0, n), "init_particles_gaussian")
    run(e, p0, upd=2)
    e.close()
    # a mixture with a component that owns no particle: rows of the Gaussian initialisations of the components that do
    means = np.array([mean, (2.0, 1.0, -1.0), (-0.5, 0.25, 0.1)])
    covs = np.array([cov, np.diag([0.25, 0.25, 0.16]), np.diag([0.01, 0.01, 0.0])])
    counts = np.array([0, 0, 1] if n == 1 else [n // 2, 0, n - n // 2], np.int64)
    a = W.engine(n, step, seed=seed)
    a.init_particles_mixture(means, covs, counts)
    got = a.get_particles()
    assert got.shape == (3, n)
    ws.assert_same("mixture weights", a.get_weights(), flat)
    lo = 0
    for comp, k in enumerate(counts):
        if k:
            b = W.engine(n, step, seed=seed)
            b.init_particles_gaussian(means[comp], covs[comp], n)
            assert np.array_equal(bits(got[:, lo:lo + k]), bits(b.get_particles()[:, lo:lo + k])), comp
            b.close()
        lo += int(k)
    run(a, got)
    a.close()


# ---- e. KLD through ragged sizes
def kld_chain(W, e, kld, seed, updates, first_update=0, n_fresh_max=8192):
    """Updates of an engine whose size KLD chooses, with the spec's own normals and uniforms injected (the same draw, through the
    injected-input path): the size drawn is the host rule's from the device's bin count, every child and log-weight the oracle's,
    and an update that changed the size equals a fresh engine pinned to that size and given the same parents, weights, normals and
    uniforms, bit for bit.  first_update: the updates the engine has behind it (the Philox counter).  Returns [(parents, children,
    bins, path)]"""
    orc, m, step = W.orc, W.m, 18
    ang, scan = W.ang(step), W.scan(step)
    oi = orc.obs_index(scan, W.om)
    # the weights as the engine holds them, maximum exactly 1 (flat ones from set_particles quantise to 2^36 each either way)
    w_par = orc.eng_weights_from_log(e.log_weights())[0] if first_update else e.get_weights()
    q = orc.eng_quantize_weights(w_par)
    ws.assert_same("fixed-point weights before the chain", read_q(e, e.n), q)
    log, bins = [], -1
    for u in range(updates):
        n_par = e.n
        bins_prev, n = e.kld_state()
        assert bins_prev == bins
        k53 = orc.eng_philox_k53(seed, first_update + u, 0, n)
        uni = k53.astype(np.float64) / 2.0 ** 53                           # exact: the kernel's floor(u 2^53) is k53 again
        assert np.array_equal(ws.injected_k53(uni), k53)
        nrm = orc.eng_philox_normals(seed, first_update + u, 0, n)
        parents = e.get_particles()
        e.update(ws.ACTION, scan, normals=nrm, uniforms=uni)
        assert e.n == n == e.particle_count() and e.effective_sample_size()[1], (u, e.n, n)
        idx = orc.eng_resample_indices(q, 0, n_children=n, k53=k53)
        ws.assert_same(f"update {u}: resample indices", e.resample_indices(), idx)
        assert idx.max() < n_par
        parts = e.get_particles()
        ws.assert_close(f"update {u}: children", parts, orc.motion_model(parents[:, idx], ws.ACTION, nrm), 1e-13, 1e-13)
        logw, _, _ = orc.eng_log_weights(W.om, parts, ang, oi, W.L)
        ws.assert_same(f"update {u}: log-weights", e.log_weights(), logw)
        bins, n_next = e.kld_state()
        drawn = parents[:, idx]
        assert bins == np_bins(drawn[0], drawn[1], drawn[2], m.data.shape[1], m.data.shape[0], m.resolution, m.origin_x, m.origin_y, kld), u
        assert n_next == W.mod.host_kld_target(kld, bins, n), (u, n_next, bins, n)
        if n != n_par:
            f = W.engine(n_fresh_max, step, seed=seed)
            f.set_particles(parents, w_par)                                # (the maximum is exactly 1: the same fixed-point weights)
            f.set_kld(min_particles=n, max_particles=n)
            assert f.kld_state() == (-1, n)
            f.update(ws.ACTION, scan, normals=nrm, uniforms=uni)
            assert f.n == n
            ws.assert_same(f"update {u}: indices, fresh engine", f.resample_indices(), e.resample_indices())
            for what, x, y in (("particles", f.get_particles(), parts), ("log-weights", f.log_weights(), e.log_weights()),
                               ("weights", f.get_weights(), e.get_weights())):
                ws.assert_same(f"update {u}: {what}, fresh engine", x, y)
            f.close()
        w_par, q, _ = orc.eng_weights_from_log(logw)
        log.append((n_par, n, bins, path_of(e)))
    return log


def test_kld_walks_through_ragged_sizes(W):
    """from a converged set of 4096: round_to 1 and shrink_permille 1000 let every update land on whatever size the bins give"""
    seed, n0 = SEED + 9, 4096
    e = W.engine(8192, 18, seed=seed)
    e.set_particles(ps.cloud(np.random.default_rng(9), n0, sig=(0.3, 0.3, 0.3)), np.full(n0, 1.0 / n0))
    for _ in range(3):
        e.update(ws.ACTION, W.scan(18))                                    # converge
    kld = e.set_kld(min_particles=1, max_particles=8192, round_to=1, shrink_permille=1000)
    assert e.kld_state() == (-1, n0)
    log = kld_chain(W, e, kld, seed, 8, first_update=3)
    ns = [r[1] for r in log]
    print("KLD sizes:", log)
    assert len(set(ns)) >= 4 and any(n % 16 for n in ns) and any(n % 64 for n in ns), log
    assert all(r[3] in ("regular", "tiny") for r in log)
    e.close()


def test_kld_pinned_to_one_particle(W):
    seed, n0 = SEED + 10, 4096
    e = W.engine(8192, 18, seed=seed)
    e.set_particles(ps.cloud(np.random.default_rng(10), n0, sig=(0.3, 0.3, 0.3)), np.full(n0, 1.0 / n0))
    kld = e.set_kld(min_particles=1, max_particles=1)
    assert e.kld_state() == (-1, 1)
    log = kld_chain(W, e, kld, seed, 4)
    assert [r[:2] for r in log] == [(4096, 1), (1, 1), (1, 1), (1, 1)] and all(r[2] == 1 for r in log), log
    assert [r[3] for r in log[2:]] == ["tiny", "tiny"], log
    e.close()


# ---- f. groups of ragged shards on one device
def group_case(W, G, per, kind, mode, updates=4, no_compact=False):
    n, step = G * per, 18
    seed = SEED + 11 + mode
    p, w = ps.group_start(G, per, kind)
    one = W.engine(n, step, seed=seed, resample_mode=mode)
    grp = make_group(W.mod, W.m, W.ang(step), per, G, seed=seed, resample_mode=mode)
    one.set_particles(p, w)
    grp.set_particles(p, w)
    c = W.checker(one, step, seed, p, w, mode=mode, rng=n)
    ws.assert_same("group set_particles", grp.get_particles(), p)
    alive = ps.group_alive(G, per, kind)
    lists = [grp.engine(s).compact_list()[0] for s in range(G)]
    assert lists == ([-1] * G if no_compact else [ps.list_length(k, per) for k in alive]), (lists, alive)
    kinds = []
    for u in range(updates):
        want_lists = all(k >= 0 for k in lists)
        c.sample_k = min(65, 3 * n + 1)
        c.step(W.scan(step))                                              # the one engine, every particle against the oracle
        grp.update(ws.ACTION, W.scan(step))
        idx = grp.resample_indices()
        ws.assert_same(f"update {u}: indices", idx, one.resample_indices())
        ws.assert_same(f"update {u}: particles", grp.get_particles(), one.get_particles())
        logw = np.concatenate([grp.engine(s).log_weights() for s in range(G)])
        ws.assert_same(f"update {u}: log-weights", logw, one.log_weights())
        np.testing.assert_allclose(grp.get_weights(), one.get_weights(), rtol=1e-13, atol=0, err_msg=f"update {u}")
        xb = grp.exchange_bytes()
        assert xb["lists"] == want_lists, (u, xb, lists)
        kinds.append("lists" if xb["lists"] else "dense")
        if u == 0 and kind == "edges":
            got, want = set(np.unique(idx).tolist()), {per - 1, (G - 1) * per}   # r * n_per_rank + local at local = per - 1 and 0
            assert got <= want and (n < 64 or got == want), (got, want)
        lists = [grp.engine(s).compact_list()[0] for s in range(G)]
        q = c.q
        assert lists == [-1 if no_compact else ps.list_length(np.count_nonzero(q[s * per:(s + 1) * per]), per) for s in range(G)], (u, lists)
    grp.close()
    one.close()
    return kinds, alive


@pytest.mark.parametrize("mode", [0, 1], ids=["multinomial", "systematic"])
@pytest.mark.parametrize("kind", ps.GROUP_KINDS)
@pytest.mark.parametrize("G,per", ps.GROUPS)
def test_group_of_ragged_shards(W, G, per, kind, mode):
    """shards of 1, 65, 1025, 2049 and 4099 particles, two to four of them: an empty list (a plateau in the merged CDF), lists of one
    entry at a shard's last and first particle, of 64 and of 65 (chunks of 64 and 128 entries), and lists as long as the shards; 4099
    particles alive outgrow a shard's list (compact_cap 4096): the gathered weights.  Equal to one engine of the whole size, itself
    held to the oracle on every particle"""
    kinds, alive = group_case(W, G, per, kind, mode)
    print(f"G {G} x {per}, {kind}: start lists {alive}, exchanges {kinds}")
    if kind != "flat" or per <= 4096:
        assert kinds[0] == "lists", kinds
    else:
        assert kinds[0] == "dense", kinds


def test_group_gathered_weights(W, monkeypatch):
    """MCL_NO_COMPACT=1 at 3 x 1025: the scan over the 3075 gathered weights, parents read where they live"""
    monkeypatch.setenv("MCL_NO_COMPACT", "1")
    kinds, _ = group_case(W, 3, 1025, "edges", 0, updates=3, no_compact=True)
    assert kinds == ["dense"] * 3


def test_one_rank_comm_update(W):
    """1025 particles through mcl_comm_update with one rank against mcl_update"""
    n, step, seed = 1025, 18, SEED + 13
    ok, why = W.mod.Engine.comm_available()
    if not ok:
        pytest.skip(f"no RCCL: {why}")
    p, w = ps.start(n, "alive65")
    e, one = (W.engine(n, step, seed=seed) for _ in range(2))
    for x in (e, one):
        x.set_particles(p, w)
    e.comm_create(e.comm_unique_id(), 1, 0)
    for k in range(3):
        e.comm_update(ws.ACTION, W.scan(step))
        one.update(ws.ACTION, W.scan(step))
        ws.assert_same(f"update {k}: indices", e.resample_indices(), one.resample_indices())
        ws.assert_same(f"update {k}: particles", e.get_particles(), one.get_particles())
        ws.assert_same(f"update {k}: log-weights", e.log_weights(), one.log_weights())
    e.comm_destroy()
    e.close()
    one.close()
