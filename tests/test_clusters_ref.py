"""Pose clustering, host side (no GPU): the numpy restatement (tests/clusters_ref.py) against a brute-force BFS on small random
sets and on hand-built cases, and the library's new C ABI: the symbols, the defaults, and the calls it refuses."""
import ctypes as C

import numpy as np
import pytest

import clusters_ref as R


def _ref(p, q, nth=36):
    m = R.HAND_MAP
    return R.clusters(p[0], p[1], p[2], q, m["W"], m["H"], m["res"], m["ox"], m["oy"], nth=nth)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("nth", [1, 2, 3, 36])
def test_restatement_against_brute_force(seed, nth):
    rng = np.random.default_rng(seed)
    n = 300
    p = np.vstack([rng.uniform(-5.5, 5.5, n), rng.uniform(-5.5, 5.5, n), rng.uniform(-np.pi, np.pi, n)])
    q = rng.integers(0, 4, n).astype(np.uint64) << np.uint64(30)          # a quarter weigh nothing
    m = R.HAND_MAP
    cl, labels, tot = _ref(p, q, nth)
    b, nx, ny, outside = R.particle_bins(p[0], p[1], p[2], m["W"], m["H"], m["res"], m["ox"], m["oy"], 0.5, 0.5, nth)
    member = (b != outside) & (q != 0)
    first = R.brute_force_labels(b, member, nx, ny, nth)
    got_first = np.array([cl[v]["first_bin"] if v >= 0 else -1 for v in labels])
    assert np.array_equal(got_first, first)
    assert len(cl) == np.unique(first[first >= 0]).size
    w = [c["weight_q"] for c in cl]
    assert all((w[i], -cl[i]["first_bin"]) >= (w[i + 1], -cl[i + 1]["first_bin"]) for i in range(len(cl) - 1))
    assert sum(w) + tot["q_outside"] + 0 == tot["q_total"] - int(q[(b != outside) & (q == 0)].sum())
    assert tot["n_outside"] == int((b == outside).sum())


def test_bins_agree_with_np_bins(engine_mod):
    from test_kld_host import np_bins
    rng = np.random.default_rng(3)
    p = np.vstack([rng.uniform(-6, 6, 2000), rng.uniform(-6, 6, 2000), rng.uniform(-4, 4, 2000)])
    m = R.HAND_MAP
    k = engine_mod.default_kld_config()
    b, *_ = R.particle_bins(p[0], p[1], p[2], m["W"], m["H"], m["res"], m["ox"], m["oy"], k.bin_x_m, k.bin_y_m, k.n_theta_bins)
    assert np.unique(b).size == np_bins(p[0], p[1], p[2], m["W"], m["H"], m["res"], m["ox"], m["oy"], k)


@pytest.mark.parametrize("name", list(R.hand_sets()))
def test_hand_built(name):
    p, w, nth, want = R.hand_sets()[name]
    q = (w * 2 ** 30).astype(np.uint64)
    cl, labels, tot = _ref(p, q, nth)
    assert len(cl) == want
    if name == "two_blobs_heavier_first":
        assert cl[0]["n_particles"] == 30 and cl[1]["n_particles"] == 10
        assert abs(cl[0]["mean"][0] - (-5 + 4.5 * 0.5)) < 0.1
    if name == "equal_weights_by_first_bin":
        assert cl[0]["weight_q"] == cl[1]["weight_q"] and cl[0]["first_bin"] < cl[1]["first_bin"]
    if name == "zero_weight_does_not_bridge":
        assert (labels[5:10] == -1).all()
    if name == "outside_nan_huge_heading_excluded":
        assert tot["n_outside"] == 4 and tot["q_outside"] == 4 * 2 ** 30 and (labels[-4:] == -1).all()
    if name == "heading_wrap_joins":
        assert abs(abs(cl[0]["mean"][2]) - np.pi) < 0.2 and cl[0]["cov"][2, 2] < 0.05     # the wrap: no spread of 2 pi
    for c in cl:
        assert np.allclose(c["cov"], c["cov"].T) and (np.linalg.eigvalsh(c["cov"]) > -1e-12).all()


def test_no_weight_gives_no_clusters():
    p, w, nth, _ = R.hand_sets()["two_blobs_heavier_first"]
    cl, labels, tot = _ref(p, np.zeros(p.shape[1], np.uint64))
    assert cl == [] and (labels == -1).all() and tot["q_total"] == 0


# ---- the C ABI (fails on a library without the feature)
def test_abi_symbols_and_defaults(engine_mod):
    lib = engine_mod.load_library()
    for s in ("mcl_default_cluster_config", "mcl_pose_clusters", "mcl_get_cluster_labels"):
        assert hasattr(lib, s), s
    c = engine_mod.default_cluster_config()
    assert (c.bin_x_m, c.bin_y_m, c.n_theta_bins, c.reserved) == (0.5, 0.5, 36, 0)
    assert C.sizeof(engine_mod.Cluster) == 8 * 17 and engine_mod.CLUSTER_DTYPE.itemsize == 136
    with pytest.raises(AttributeError):
        engine_mod.default_cluster_config(bin_z_m=1.0)


def test_abi_refusals_without_an_engine(engine_mod):
    lib = engine_mod.load_library()
    c = engine_mod.default_cluster_config()
    n = C.c_int64(-1)
    tot = (C.c_uint64 * 3)()
    assert lib.mcl_pose_clusters(None, C.byref(c), 0, None, C.byref(n), tot) == -1
    assert lib.mcl_get_cluster_labels(None, None, 0) == -1
    assert n.value == -1

