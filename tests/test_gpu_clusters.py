"""Pose clustering on the GPU (mcl_pose_clusters) against the numpy restatement (tests/clusters_ref.py): every
label, weight_q, count, first_bin and the order exactly; every fp64 sum within (h + 2) * 2^-53 * sum|t| of math.fsum, h being
the longest addition chain of the device's fixed reduction (clusters_ref.chain), plus a few ulp for sin / cos.  Also: the same
state gives the same bytes, clustering between updates changes nothing the updates compute, and the refusals."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import clusters_ref as R
from conftest import GOLDEN, make_engine

pytestmark = pytest.mark.gpu

ACTION = (0.1, 0.0, 0.02)


def _scan(step=1):
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32)


def read_q(e, n):
    q = np.empty(n, np.uint64)
    e.export_state(0, 0, 0, q.ctypes.data)
    return q


def check(e, geom, K=16, **cfg):
    """Clusters the engine's set and compares everything with the restatement; returns (clusters, info, labels)."""
    got, info = e.pose_clusters(K, **cfg)
    labels = e.cluster_labels()
    p = e.get_particles()
    n = p.shape[1]
    q = read_q(e, n)
    bx, by, nth = cfg.get("bin_x_m", 0.5), cfg.get("bin_y_m", 0.5), cfg.get("n_theta_bins", 36)
    ref, ref_labels, tot = R.clusters(p[0], p[1], p[2], q, geom["W"], geom["H"], geom["res"], geom["ox"], geom["oy"], bx, by, nth,
                                      moments_of=K)
    assert info == dict(n_clusters=len(ref), **tot)
    assert np.array_equal(labels, ref_labels)
    assert got.size == min(K, len(ref))
    for r, (d, c) in enumerate(zip(got, ref)):
        assert (int(d["weight_q"]), int(d["n_particles"]), int(d["n_bins"]), int(d["first_bin"])) == \
            (c["weight_q"], c["n_particles"], c["n_bins"], c["first_bin"]), r
        assert d["weight"] == c["weight"], r
        W = float(np.float64(c["weight_q"]))
        i = c["members"]
        h = R.chain(i.size)
        sq = math.fsum(q[i].astype(np.float64).tolist())
        for j in range(2):                                    # x, y: S / W
            b = (h + 2) * R.U * c["A1"][j] / W + 4 * R.U * abs(c["mean"][j])
            assert abs(d["mean"][j] - c["mean"][j]) <= b, (r, j, d["mean"][j], c["mean"][j], b)
        dS = (h + 2) * R.U * c["A1"][2] + 4 * R.U * sq
        dC = (h + 2) * R.U * c["A1"][3] + 4 * R.U * sq
        Rr = math.hypot(c["S1"][2], c["S1"][3])
        if Rr > 100 * (dS + dC):                              # (a heading spread over the whole turn has no stable mean)
            dth = math.remainder(d["mean"][2] - c["mean"][2], 2 * math.pi)
            assert abs(dth) <= 1.02 * (dS + dC) / Rr + 8 * R.U * math.pi, (r, dth)
        # the covariance about the device's own mean: the terms are formed exactly as on the device
        S2, A2 = R.second_moments(p[0][i], p[1][i], p[2][i], q[i], d["mean"])
        dev = d["cov"].ravel()[[0, 1, 2, 4, 5, 8]]
        for j in range(6):
            b = (h + 6) * R.U * A2[j] / W + 4 * R.U * abs(S2[j] / W)
            assert abs(dev[j] - S2[j] / W) <= b, (r, j, dev[j], S2[j] / W, b)
        assert np.array_equal(d["cov"], d["cov"].T)
    return got, info, labels


def spielberg_geom(m):
    return dict(W=m.data.shape[1], H=m.data.shape[0], res=m.resolution, ox=m.origin_x, oy=m.origin_y)


@pytest.mark.parametrize("name", list(R.hand_sets()))
def test_hand_built_sets(engine_mod, name):
    p, w, nth, want = R.hand_sets()[name]
    g = R.HAND_MAP
    e = engine_mod.Engine(max_particles=64)
    e.set_map(np.zeros((g["H"], g["W"]), np.int8), g["res"], g["ox"], g["oy"])
    e.set_particles(p, w)
    got, info, labels = check(e, g, n_theta_bins=nth)
    assert info["n_clusters"] == want
    e.close()


@pytest.mark.parametrize("n", [262144, 4194304])
def test_tracking_cloud_after_updates(engine_mod, spielberg, n):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    e = make_engine(engine_mod, spielberg, ang, n, seed=5)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(5), n), np.full(n, 1.0 / n))
    scan, geom = _scan(), spielberg_geom(spielberg)
    e.update(ACTION, scan)
    check(e, geom)
    e.update(ACTION, scan)
    e.update(ACTION, scan)
    got, info, _ = check(e, geom)
    assert info["n_clusters"] >= 1 and got[0]["weight"] > 0.5
    e.close()


def test_uniform_4m_after_init_global(engine_mod, spielberg):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n = 4194304
    e = make_engine(engine_mod, spielberg, ang, n, seed=7)
    e.init_global(n)
    geom = spielberg_geom(spielberg)
    got, info, _ = check(e, geom)
    assert info["n_clusters"] >= 1 and got[0]["n_bins"] > 100000
    e.update((0.0, 0.0, 0.0), _scan())
    check(e, geom)
    e.close()


def test_stock_size_five_updates_from_global(engine_mod, spielberg):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    n = 2000
    e = make_engine(engine_mod, spielberg, ang, n, seed=11)
    e.init_global(n)
    geom, scan = spielberg_geom(spielberg), _scan(18)
    counts = []
    for _ in range(5):
        e.update((0.0, 0.0, 0.0), scan)
        counts.append(check(e, geom)[1]["n_clusters"])
    assert max(counts) > 1, counts
    e.close()


def test_no_weight_gives_no_clusters(engine_mod, spielberg):
    """An all-impossible update (z_rand = 0, every beam reads long): Q = 0, no clusters, every label -1."""
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n = 20000
    e = make_engine(engine_mod, spielberg, ang, n, seed=21, z_rand=0.0, sigma_hit=2.0)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(21), n, sig=(0.2, 0.2, 0.1)), np.full(n, 1.0 / n))
    e.update(ACTION, _scan())
    dead = np.full(ang.size, np.float32((e.max_range_px - 3) * float(spielberg.resolution)), np.float32)
    e.update(ACTION, dead)
    assert np.isneginf(e.log_weights()).all()
    got, info, labels = check(e, spielberg_geom(spielberg))
    assert info["n_clusters"] == 0 and info["q_total"] == 0 and got.size == 0 and (labels == -1).all()
    e.close()


def test_kld_across_a_size_change(engine_mod, spielberg):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n0 = 65536
    e = make_engine(engine_mod, spielberg, ang, n0, seed=31)
    e.set_particles(synth.tracking_cloud(np.random.default_rng(5), n0), np.full(n0, 1.0 / n0))
    e.set_kld(min_particles=256, max_particles=n0)
    geom, scan = spielberg_geom(spielberg), _scan()
    sizes = []
    for _ in range(4):
        e.update(ACTION, scan)
        sizes.append(e.particle_count())
        _, _, labels = check(e, geom)
        assert labels.size == sizes[-1]
    assert len(set(sizes)) > 1, sizes
    e.close()


def test_same_state_same_bytes(engine_mod, spielberg):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    n = 1048576
    e = make_engine(engine_mod, spielberg, ang, n, seed=9)
    e.init_global(n)
    e.update((0.0, 0.0, 0.0), _scan())
    a, ia = e.pose_clusters(64)
    la = e.cluster_labels()
    b, ib = e.pose_clusters(64)
    lb = e.cluster_labels()
    assert a.tobytes() == b.tobytes() and ia == ib and np.array_equal(la, lb)
    e.close()


@pytest.mark.parametrize("n,kld", [(20000, False), (65536, True)], ids=["graph_path", "kld"])
def test_clustering_changes_no_update(engine_mod, spielberg, n, kld):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles()
    p = synth.tracking_cloud(np.random.default_rng(3), n)
    es = []
    for _ in range(2):
        e = make_engine(engine_mod, spielberg, ang, n, seed=13)
        e.set_particles(p, np.full(n, 1.0 / n))
        if kld:
            e.set_kld(min_particles=256, max_particles=n)
        es.append(e)
    plain, clus = es
    scan = _scan()
    for u in range(5):
        clus.pose_clusters(8)
        plain.update(ACTION, scan)
        clus.update(ACTION, scan)
        with pytest.raises(engine_mod.EngineError) as ei:          # the labels of the clustering before the update are void
            clus.cluster_labels()
        assert ei.value.status == -2
        assert np.array_equal(plain.get_particles(), clus.get_particles()), u
        assert np.array_equal(plain.log_weights(), clus.log_weights()), u
        assert np.array_equal(plain.resample_indices(), clus.resample_indices()), u
        assert plain.kld_state() == clus.kld_state(), u
    plain.close()
    clus.close()


def test_refusals(engine_mod, spielberg):
    from monte_carlo_localization_amd import synth
    ang = synth.beam_angles(angle_step=18)
    e = engine_mod.Engine(max_particles=1024)
    lib = e.lib
    c = engine_mod.default_cluster_config()
    for f in [dict(bin_x_m=0.0), dict(bin_y_m=-1.0), dict(bin_x_m=float("nan")), dict(bin_y_m=float("inf")), dict(n_theta_bins=0),
              dict(reserved=1)]:
        bad = engine_mod.default_cluster_config(**f)
        assert lib.mcl_pose_clusters(e._h, C.byref(bad), 0, None, None, None) == -1, f
    for k in (-1, 65537):
        assert lib.mcl_pose_clusters(e._h, C.byref(c), k, None, None, None) == -1
    assert lib.mcl_pose_clusters(e._h, C.byref(c), 0, None, None, None) == -2           # no map, no particles
    assert lib.mcl_get_cluster_labels(e._h, None, 0) == -2
    e.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    e.set_beam_angles(ang)
    e.init_global(1024)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.pose_clusters(4, bin_x_m=0.001, bin_y_m=0.001)                                 # a grid of more than 2^31 bits
    assert ei.value.status == -1
    got, info = e.pose_clusters(0)
    assert got.size == 0 and info["n_clusters"] >= 1 and e.cluster_labels().size == 1024
    uid = e.comm_unique_id()
    e.comm_create(uid, 1, 0)                                                             # a 1-rank communicator
    with pytest.raises(engine_mod.EngineError) as ei:
        e.pose_clusters(4)
    assert ei.value.status == -5
    e.close()
    g = engine_mod.Group([0, 0], max_particles=1024)                                     # one device, two shards
    g.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    g.set_beam_angles(ang)
    g.init_global(2048)
    with pytest.raises(engine_mod.EngineError) as ei:
        g.engine(0).pose_clusters(4)
    assert ei.value.status == -5
    g.close()
