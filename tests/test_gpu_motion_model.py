"""The odometry motion models and the Gaussian pose initialisation on the GPU (mcl_set_motion_model, mcl_init_particles_gaussian;
DESIGN.md §4.11), through the C ABI on the Spielberg map with the golden scan: every child of every update against
tests/motion_ref.py (the restatement written from the spec) on each update path, off-is-off, the interplay with KLD, recovery
and the likelihood field, sharded sets, the initialisation and a closed tracking loop."""
import math
import os

import numpy as np
import pytest

import motion_ref as mr
from conftest import GOLDEN, make_engine, tracking_cloud
from test_kld_host import np_bins
from test_recovery_host import child_draws, free_cells, injected_poses, threshold

pytestmark = pytest.mark.gpu

SEED = 0x5EED_0000_0000_0020 + 77
ACTIONS = {"diff": (0.1, 0.0, 0.02), "omni": (0.1, 0.02, 0.02)}
TOL = 1e-13


def _scan(step=1):
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32)


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def assert_poses(got, want, msg=""):
    """1e-13 / 1e-13 on every particle, headings modulo 2 pi"""
    np.testing.assert_allclose(got[:2], want[:2], rtol=TOL, atol=TOL, err_msg=msg)
    d = (got[2] - want[2] + math.pi) % (2 * math.pi) - math.pi
    bad = np.abs(d) > TOL + TOL * np.abs(want[2])
    assert not bad.any(), (msg, int(bad.sum()), float(np.abs(d).max()))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


class World:
    def __init__(self, orc, om, step):
        from monte_carlo_localization_amd import synth
        self.orc, self.om = orc, om
        self.ang = synth.beam_angles(angle_step=step)
        self.scan = _scan(step)
        self.L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
        self.oi = orc.obs_index(self.scan, om)

    def check_logw(self, e, parts, rng, k=512):
        n = parts.shape[1]
        pick = np.arange(n) if n <= k else np.sort(rng.choice(n, k, replace=False))
        logw, _, _ = self.orc.eng_log_weights(self.om, np.ascontiguousarray(parts[:, pick]), self.ang, self.oi, self.L)
        assert np.array_equal(e.log_weights()[pick], logw), "log-weights are not those of the moved poses"


def step_and_check(w, e, model, upd, parents, rng, over=None, normals=None, action=None):
    """one update; every child against M5 of its parent; sampled log-weights bit for bit; returns the children"""
    over = over or {}
    action = action or ACTIONS[model]
    al = tuple(over.get(f"alpha{i + 1}", 0.2) for i in range(5))
    fl = (over.get("floor_trans_m", 0.0), over.get("floor_rot_rad", 0.0))
    e.update(action, w.scan, normals=normals)
    n = e.n
    idx = e.resample_indices()
    nrm = normals if normals is not None else w.orc.eng_philox_normals(SEED, upd, 0, n)
    parts = e.get_particles()
    assert_poses(parts, mr.sample(model, action, parents[:, idx], nrm, al, fl), f"{model} update {upd}")
    w.check_logw(e, parts, rng)
    return parts


# ---- 6. per-child parity on every update path
PATHS = [
    # n, beam step, graph_mode, expected path from the second update on, MCL_SORT
    (2000, 18, 0, "tiny", None),
    (32768, 18, 0, "graph", None),
    (65536, 1, 0, None, None),
    (65536, 1, 1, "regular", None),
    (262144, 1, 0, "regular", "radix"),       # k_rays_sweep; the (key, index) pairs of the radix ordering come out of the resampling kernel
]


@pytest.mark.parametrize("model", ["diff", "omni"])
@pytest.mark.parametrize("n,step,graph_mode,path,sort", PATHS)
def test_every_child_on_every_path(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, model, n, step, graph_mode, path, sort):
    if sort:
        monkeypatch.setenv("MCL_SORT", sort)
    w = World(orc, spielberg_oracle, step)
    e = make_engine(engine_mod, spielberg, w.ang, n, seed=SEED, graph_mode=graph_mode)
    p = tracking_cloud(np.random.default_rng(n), n)
    e.set_particles(p, np.full(n, 1.0 / n))
    over = dict(floor_trans_m=0.004) if model == "omni" else {}
    cfg = e.set_motion_model(model, **over)
    got = e.motion_model()
    assert (got.model, got.alpha3, got.floor_trans_m) == (cfg.model, 0.2, over.get("floor_trans_m", 0.0))
    rng = np.random.default_rng(1)
    paths = []
    for upd in range(4):
        p = step_and_check(w, e, model, upd, p, rng, over)
        paths.append(path_of(e))
    if path:
        assert all(q == path for q in paths[1:]), paths
    if n == 262144:
        assert e.ray_kernel_name() == "k_rays_sweep"
    e.close()


@pytest.mark.parametrize("model", ["diff", "omni"])
@pytest.mark.parametrize("n,step", [(2000, 18), (65536, 4)])
def test_injected_normals(orc, engine_mod, spielberg, spielberg_oracle, model, n, step):
    w = World(orc, spielberg_oracle, step)
    e = make_engine(engine_mod, spielberg, w.ang, n, seed=SEED)
    p = tracking_cloud(np.random.default_rng(3), n)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.set_motion_model(model)
    rng = np.random.default_rng(2)
    for upd in range(3):
        p = step_and_check(w, e, model, upd, p, rng, normals=rng.normal(size=(n, 3)))
    e.close()


@pytest.mark.parametrize("model", ["diff", "omni"])
def test_kept_updates_move_every_particle(orc, engine_mod, spielberg, spielberg_oracle, model):
    """Adaptive resampling keeps the set (every particle its own parent): it moves by M5 all the same.  (resample_neff_permille
    = 1 on a tight cloud: kept and resampled updates both occur, as in test_gpu_kld.py; 1000 would keep only a set whose weights
    are all equal.)"""
    w = World(orc, spielberg_oracle, 18)
    n = 2048
    e = make_engine(engine_mod, spielberg, w.ang, n, seed=SEED, resample_neff_permille=1)
    p = tracking_cloud(np.random.default_rng(12), n, sig=(0.2, 0.2, 0.1))
    e.set_particles(p, np.full(n, 1.0 / n))
    e.set_motion_model(model)
    action, kept = ACTIONS[model], []
    for upd in range(8):
        e.update(action, w.scan)
        idx = e.resample_indices()
        kept.append(not e.effective_sample_size()[1])
        if kept[-1]:
            assert np.array_equal(idx, np.arange(n))
        parts = e.get_particles()
        assert_poses(parts, mr.sample(model, action, p[:, idx], orc.eng_philox_normals(SEED, upd, 0, n)), f"update {upd} kept={kept[-1]}")
        p = parts
    assert any(kept) and not all(kept), kept
    e.close()


@pytest.mark.parametrize("model", ["diff", "omni"])
def test_under_the_likelihood_field(orc, engine_mod, spielberg, spielberg_oracle, model):
    import lfield_ref as lr
    from test_gpu_likelihood_field import Ambiguity, check_logw
    w = World(orc, spielberg_oracle, 4)
    n = 16384
    e = make_engine(engine_mod, spielberg, w.ang, n, seed=SEED)
    p = tracking_cloud(np.random.default_rng(5), n)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.set_likelihood_field()
    e.set_motion_model(model)
    ref = dict(D=lr.field(spielberg.data, spielberg.resolution), Lf=lr.table(spielberg.resolution))
    tally, action = Ambiguity(), ACTIONS[model]
    for upd in range(3):
        e.update(action, w.scan)
        idx = e.resample_indices()
        parts = e.get_particles()
        assert_poses(parts, mr.sample(model, action, p[:, idx], orc.eng_philox_normals(SEED, upd, 0, n)), f"update {upd}")
        check_logw(e, ref, spielberg, w.ang, w.scan, tally, sample=np.arange(0, n, 64))
        p = parts
    tally.check()
    e.close()


# ---- 7. off is off
@pytest.mark.parametrize("n", [2000, 100000])
@pytest.mark.parametrize("off", [None, "reference"])
def test_off_is_off(orc, engine_mod, spielberg, spielberg_oracle, n, off):
    w = World(orc, spielberg_oracle, 4)
    p0 = tracking_cloud(np.random.default_rng(14), n)
    action = (0.1, 0.0, 0.02)
    a = make_engine(engine_mod, spielberg, w.ang, n, seed=71)           # never hears of the motion model
    b = make_engine(engine_mod, spielberg, w.ang, n, seed=71)
    for e in (a, b):
        e.set_particles(p0, np.full(n, 1.0 / n))
    b.set_motion_model("diff")
    for _ in range(2):
        a.update(action, w.scan)
        b.update(action, w.scan)
    assert not same_bits(a.get_particles(), b.get_particles())
    for e in (a, b):
        e.set_particles(p0, np.full(n, 1.0 / n))
    b.set_motion_model(off)
    assert b.motion_model().model == engine_mod.MOTION_REFERENCE
    for k in range(5):
        a.update(action, w.scan)
        b.update(action, w.scan)
        assert np.array_equal(a.resample_indices(), b.resample_indices()), k
        assert same_bits(a.get_particles(), b.get_particles()), k
        assert same_bits(a.get_weights(), b.get_weights()), k
        assert path_of(a) == path_of(b)
    a.close(); b.close()


def test_setting_the_model_keeps_graphs_and_recovery_averages(orc, engine_mod, spielberg, spielberg_oracle):
    w = World(orc, spielberg_oracle, 18)
    n = 32768
    e = make_engine(engine_mod, spielberg, w.ang, n, seed=SEED)
    p = tracking_cloud(np.random.default_rng(9), n)
    e.set_particles(p, np.full(n, 1.0 / n))
    e.set_recovery()
    rng = np.random.default_rng(4)
    for _ in range(3):
        e.update(ACTIONS["diff"], w.scan)
    assert path_of(e) == "graph"
    S, F = e.recovery_state()[:2]
    assert not math.isnan(S)
    e.set_motion_model("omni")
    assert e.recovery_state()[:2] == (S, F)
    p = step_and_check(w, e, "omni", 3, e.get_particles(), rng)
    assert path_of(e) == "graph"                     # the captured tail was not dropped
    with pytest.raises(engine_mod.EngineError) as ei:
        e.set_motion_model("diff", alpha2=-1.0)
    assert ei.value.status == -1 and e.motion_model().model == engine_mod.MOTION_OMNI
    e.close()


# ---- 8. interplay with KLD and recovery
@pytest.mark.parametrize("model", ["diff", "omni"])
@pytest.mark.parametrize("n,step", [(4096, 18), (65536, 1)])
def test_with_kld_and_recovery(orc, engine_mod, spielberg, spielberg_oracle, model, n, step):
    w = World(orc, spielberg_oracle, step)
    m = spielberg
    e = make_engine(engine_mod, m, w.ang, n, seed=SEED)
    p = tracking_cloud(np.random.default_rng(21), n)
    e.set_particles(p, np.full(n, 1.0 / n))
    kcfg = e.set_kld(min_particles=n, max_particles=n)
    e.set_recovery()
    e.set_motion_model(model)
    action = ACTIONS[model]
    free = free_cells(m.data)
    rng = np.random.default_rng(6)
    # update 0: KLD alone (recovery's averages are unset: p = 0)
    p1 = step_and_check(w, e, model, 0, p, rng)
    drawn = p[:, e.resample_indices()]
    assert e.kld_state()[0] == np_bins(drawn[0], drawn[1], drawn[2], m.data.shape[1], m.data.shape[0], m.resolution, m.origin_x, m.origin_y, kcfg)
    # update 1: a forced p: injected children are the free-space draws, the others follow M5
    e.set_recovery_state(0.0, math.log1p(-0.3))
    T = threshold(e.recovery_state()[2])
    e.update(action, w.scan)
    coin, pick, hb = child_draws(SEED, 1, n)
    inj = coin < np.uint64(T)
    idx = e.resample_indices()
    assert 0 < inj.sum() < n and np.array_equal(np.flatnonzero(idx == -1), np.flatnonzero(inj))
    parts = e.get_particles()
    want_inj = injected_poses(pick[inj], hb[inj], free, m.data.shape[1], m.resolution, m.origin_x, m.origin_y)
    assert same_bits(parts[:, inj], want_inj), "an injected child went through the motion model"
    nrm = orc.eng_philox_normals(SEED, 1, 0, n)
    assert_poses(parts[:, ~inj], mr.sample(model, action, p1[:, idx[~inj]], nrm[~inj]), "non-injected children")
    drawn = p1[:, np.where(inj, 0, idx)].copy()
    drawn[:, inj] = want_inj
    assert e.kld_state()[0] == np_bins(drawn[0], drawn[1], drawn[2], m.data.shape[1], m.data.shape[0], m.resolution, m.origin_x, m.origin_y, kcfg)
    assert e.recovery_state()[3] == int(inj.sum())
    w.check_logw(e, parts, rng)
    e.close()


# ---- 9. sharded sets
def make_group(engine_mod, m, ang, n_per, shards, **cfg):
    g = engine_mod.Group([0] * shards, max_particles=n_per, **cfg)
    g.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    g.set_beam_angles(ang)
    return g


@pytest.mark.parametrize("model,neff", [("diff", 0), ("omni", 0), ("diff", 20)])
def test_group_equals_one_engine(orc, engine_mod, spielberg, spielberg_oracle, model, neff):
    """Group([0, 0]): lists, the dense exchange of the first update and (neff) mcl_stage_keep, with the model on every shard"""
    w = World(orc, spielberg_oracle, 9)
    n = 8192 if not neff else 3000
    cov = np.array([[0.04, 0.01, 0.0], [0.01, 0.03, 0.002], [0.0, 0.002, 0.01]]) if not neff else np.diag([0.03, 0.03, 0.01]) ** 2
    one = make_engine(engine_mod, spielberg, w.ang, n, seed=7, resample_neff_permille=neff)
    grp = make_group(engine_mod, spielberg, w.ang, n // 2, 2, seed=7, resample_neff_permille=neff)
    one.init_particles_gaussian((0.0, 0.0, 0.0), cov, n)
    grp.init_particles_gaussian((0.0, 0.0, 0.0), cov, n)
    assert same_bits(grp.get_particles(), one.get_particles())
    one.set_motion_model(model)
    grp.set_motion_model(model)
    assert grp.engine(1).motion_model().model == engine_mod.MOTION_MODELS[model]
    p, kept = one.get_particles(), []
    for k in range(3 if not neff else 8):
        one.update(ACTIONS[model], w.scan)
        grp.update(ACTIONS[model], w.scan)
        kept.append(not one.effective_sample_size()[1])
        idx = one.resample_indices()
        assert np.array_equal(grp.resample_indices(), idx), f"update {k}"
        assert same_bits(grp.get_particles(), one.get_particles()), f"update {k}"
        assert_poses(one.get_particles(), mr.sample(model, ACTIONS[model], p[:, idx], orc.eng_philox_normals(7, k, 0, n)), f"update {k}")
        p = one.get_particles()
    if neff:
        assert any(kept), kept
    grp.close(); one.close()


def test_staged_two_shards_equal_one_engine(orc, engine_mod, spielberg, spielberg_oracle):
    """The staged flow (mcl_stage_resample .. mcl_stage_finish, the dense exchange written out by hand) with two shards on one
    device: particles and global parent indices bit-identical to one engine, DIFF, three updates."""
    import torch
    w = World(orc, spielberg_oracle, 9)
    n, S = 4096, 2
    nt = n * S
    p0 = tracking_cloud(np.random.default_rng(31), nt)
    w0 = np.full(nt, 1.0 / nt)
    one = make_engine(engine_mod, spielberg, w.ang, nt, seed=9)
    one.set_particles(p0, w0)
    one.set_motion_model("diff")
    shards = [make_engine(engine_mod, spielberg, w.ang, n, seed=9) for _ in range(S)]
    for s, e in enumerate(shards):
        e.set_particles_shard(p0[:, s * n:(s + 1) * n], w0[s * n:(s + 1) * n], float(w0.max()))
        e.set_motion_model("diff")
    dev = torch.device("cuda:0")
    gx, gy, gth = (torch.empty(nt, dtype=torch.float64, device=dev) for _ in range(3))
    gq, gcdf = (torch.empty(nt, dtype=torch.int64, device=dev) for _ in range(2))
    action = ACTIONS["diff"]
    for k in range(3):
        one.update(action, w.scan)
        for s, e in enumerate(shards):
            e.export_state(gx[s * n:].data_ptr(), gy[s * n:].data_ptr(), gth[s * n:].data_ptr(), gq[s * n:].data_ptr())
        shards[0].scan_weights(gq.data_ptr(), gcdf.data_ptr(), nt)
        torch.cuda.synchronize()
        q_total = int(gcdf[-1].item()) & 0xFFFFFFFFFFFFFFFF
        for s, e in enumerate(shards):
            e.stage_resample(gx.data_ptr(), gy.data_ptr(), gth.data_ptr(), gcdf.data_ptr(), nt, q_total, s * n, nt, action)
        torch.cuda.synchronize()
        for e in shards:
            e.stage_rays(w.scan)
        mx = max(float(e.host_scalars()[0]) for e in shards)
        for e in shards:
            e.stage_weights(mx)
        sc = [e.host_scalars() for e in shards]
        sums = np.sum([[c[1], c[3], c[4], c[5], c[6]] for c in sc], axis=0)
        for e in shards:
            e.stage_finish(sums)
        idx = np.concatenate([e.resample_indices() for e in shards])
        parts = np.concatenate([e.get_particles() for e in shards], axis=1)
        assert np.array_equal(idx, one.resample_indices()), f"update {k}"
        assert same_bits(parts, one.get_particles()), f"update {k}"
    for e in shards:
        e.close()
    one.close()


def test_one_rank_comm_update_equals_one_engine(orc, engine_mod, spielberg, spielberg_oracle):
    w = World(orc, spielberg_oracle, 6)
    n = 65536
    e = make_engine(engine_mod, spielberg, w.ang, n, seed=5)
    ok, why = e.comm_available()
    if not ok:
        pytest.skip(f"no RCCL: {why}")
    one = make_engine(engine_mod, spielberg, w.ang, n, seed=5)
    for x in (e, one):
        x.init_particles_pose((0.0, 0.0, 0.0), n, 0, n)
        x.set_motion_model("diff")
    e.comm_create(e.comm_unique_id(), 1, 0)
    for k in range(3):
        e.comm_update(ACTIONS["diff"], w.scan)
        one.update(ACTIONS["diff"], w.scan)
        assert np.array_equal(e.resample_indices(), one.resample_indices()), k
        assert same_bits(e.get_particles(), one.get_particles()), k
    e.comm_destroy()
    e.close(); one.close()


def _device_count():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif(_device_count() < 2, reason="needs two GPUs: the group's peer copies between DISTINCT devices")
def test_group_on_two_distinct_devices(orc, engine_mod, spielberg, spielberg_oracle):
    w = World(orc, spielberg_oracle, 4)
    n = 262144
    one = make_engine(engine_mod, spielberg, w.ang, n, seed=7)
    one.init_particles_pose((0.0, 0.0, 0.0), n)
    grp = engine_mod.Group([0, 1], max_particles=n // 2, seed=7)
    grp.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    grp.set_beam_angles(w.ang)
    grp.init_particles_pose((0.0, 0.0, 0.0), n)
    one.set_motion_model("diff"); grp.set_motion_model("diff")
    for k in range(3):
        one.update(ACTIONS["diff"], w.scan)
        grp.update(ACTIONS["diff"], w.scan)
        assert np.array_equal(grp.resample_indices(), one.resample_indices()), f"update {k}"
        assert same_bits(grp.get_particles(), one.get_particles()), f"update {k}"
    grp.close(); one.close()


# ---- 10. Gaussian initialisation
def test_gaussian_init_every_particle(orc, engine_mod, spielberg):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    n, seed = 100000, 1234
    e = make_engine(engine_mod, spielberg, ang, n, seed=seed)
    mean = (1.5, -0.7, 3.0)                                   # (a heading near pi: part of the cloud wraps)
    cov = np.array([[0.30, 0.12, 0.01], [0.12, 0.20, -0.02], [0.01, -0.02, 0.05]])
    e.init_particles_gaussian(mean, cov, n)
    assert_poses(e.get_particles(), mr.init_gaussian(seed, 0, mean, cov, 0, n), "init 0")
    np.testing.assert_allclose(e.get_weights(), np.full(n, 1.0 / n), rtol=1e-12, atol=0)
    # the second initialisation of the engine draws with the next init counter; diag(0.25, 0.25, 0.16) is the pose cloud
    e.init_particles_gaussian(mean, np.diag([0.25, 0.25, 0.16]), n)
    assert_poses(e.get_particles(), orc.eng_init_pose(seed, 1, mean, 0, n), "pose cloud")
    # zero heading variance: one heading
    flat = np.array([[0.09, 0.03, 0.0], [0.03, 0.04, 0.0], [0.0, 0.0, 0.0]])
    e.init_particles_gaussian((0.0, 0.0, 0.7), flat, n)
    got = e.get_particles()
    assert (got[2] == 0.7).all()
    assert_poses(got, mr.init_gaussian(seed, 2, (0.0, 0.0, 0.7), flat, 0, n), "flat")
    # sharded offsets: two halves of a set of n, each with its first global index, are the one call's particles
    whole = mr.init_gaussian(seed, 3, mean, cov, 0, n)
    e.init_particles_gaussian(mean, cov, n // 2, first_global_index=n // 2, n_total=n)
    assert e.n == n // 2
    assert_poses(e.get_particles(), whole[:, n // 2:], "second shard")
    # refusals: nothing changes
    before = e.get_particles()
    for bad in (np.diag([0.25, -0.25, 0.1]), np.array([[1.0, 0.1, 0.0], [0.2, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.diag([1.0, float("nan"), 1.0])):
        with pytest.raises(engine_mod.EngineError) as ei:
            e.init_particles_gaussian(mean, bad, n)
        assert ei.value.status == -1
    assert same_bits(e.get_particles(), before)
    # an update after it runs (layouts, KLD, recovery were reset as by mcl_init_particles_pose)
    e.init_particles_gaussian((0.0, 0.0, 0.0), np.diag([0.04, 0.04, 0.01]), n)
    e.update((0.1, 0.0, 0.0), _scan(18))
    e.close()


def test_gaussian_init_sample_covariance(engine_mod, spielberg):
    """n = 2^20, a full covariance (correlated x-y, a heading variance small enough that nothing wraps): every entry of the sample
    covariance within 6 sqrt((Sii Sjj + Sij^2) / n) of Sij -- the 6-sigma band of the estimator.  The numpy restatement passes
    the same assertion with the same seed (tests/test_motion_host.py::test_init_restatement)."""
    from monte_carlo_localization_amd import synth
    n, pose = 1 << 20, (0.3, -1.2, 0.5)
    cov = np.array([[0.30, 0.12, 0.004], [0.12, 0.20, -0.003], [0.004, -0.003, 0.0025]])
    e = make_engine(engine_mod, spielberg, synth.beam_angles(angle_step=18), n, seed=2024)
    e.init_particles_gaussian(pose, cov, n)
    ok, worst = mr.cov_band_ok(e.get_particles(), pose, cov)
    print("worst |S_ij - Sigma_ij| / band:", worst)
    assert ok, worst
    e.close()


# ---- 11. closed loop
def trajectory(lateral=0.0):
    """60 steps of 0.1 m: a left curve, a right curve, a tighter left curve (the track bends left there)"""
    return [(0.1, lateral, 0.015 if k < 20 else (-0.015 if k < 40 else 0.02)) for k in range(60)]


def run_loop(orc, engine_mod, m, om, model, acts, n=65536, seed=11):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    e = make_engine(engine_mod, m, ang, n, seed=seed)
    truth = np.array([[0.0], [0.0], [0.0]])
    e.init_particles_gaussian(truth[:, 0], np.diag([0.25, 0.25, 0.16]), n)
    if model != "reference":
        e.set_motion_model(model)
    a64 = ang.astype(np.float64)
    errs = []
    for act in acts:
        truth = mr.compose(act, truth)
        x, y, th = truth[:, 0]
        scan, _ = orc.cast_many(om, np.full(a64.size, x), np.full(a64.size, y), th + a64)
        e.update((act[0], 0.0, act[2]) if model == "reference" else act, np.asarray(scan, np.float32))
        pose = e.expected_pose()
        errs.append((math.hypot(pose[0] - x, pose[1] - y), abs((pose[2] - th + math.pi) % (2 * math.pi) - math.pi)))
    e.close()
    return errs


@pytest.mark.parametrize("leg", ["curves", "slip"])
def test_closed_loop_tracks(orc, engine_mod, spielberg, spielberg_oracle, leg):
    """Truth advanced without noise by the restatement, scans cast from it by the oracle, 65 536 particles, AMCL's default alphas:
    the final pose within 0.25 m / 5 degrees (the bound test_gpu_kld.py uses for "localised").  "curves": DIFF, with the REFERENCE
    model as control (it must localise too).  "slip": 2 cm of lateral displacement per step under OMNI."""
    if leg == "curves":
        runs = {mdl: run_loop(orc, engine_mod, spielberg, spielberg_oracle, mdl, trajectory()) for mdl in ("reference", "diff")}
    else:
        runs = {"omni": run_loop(orc, engine_mod, spielberg, spielberg_oracle, "omni", trajectory(lateral=0.02))}
    for mdl, errs in runs.items():
        print(mdl, "final error (m, rad):", errs[-1], "worst (m):", max(d for d, _ in errs))
    for mdl, errs in runs.items():
        d, dth = errs[-1]
        assert d < 0.25 and dth < math.radians(5), (mdl, d, dth)
