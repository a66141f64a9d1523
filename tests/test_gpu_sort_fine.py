"""Fine key bits on the radix ordering path (MCL_SORT_FINE, csrc/mcl_sort_key.h): the order of an update's ray stage, read back
(Engine.sort_order), is a permutation sorted over all 22 + F key bits whose keys are the host twin's (host_sort_key) for the
particle in every slot under the layout read back with them -- and the order still decides nothing: log-weights and resample
indices are the same doubles and integers with 0, 2 and 6 fine bits and with the default (two bits, both sub-cell bits: quarter
cells), and the oracle's.  65 536 particles x 181 beams on the
Spielberg fixture, the smallest set that takes k_rays_sweep; MCL_SORT=radix sends it through the library sort.  Each cloud is
followed over two updates: the first orders by keys k_sort_keys makes from this update's layout, the second (the set collapsed by
the resampling) by keys the resampling kernel writes from the previous update's layout."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_engine, tracking_cloud

pytestmark = pytest.mark.gpu
N, STEP, SEED = 65536, 6, 12
ACTION = (0.05, 0.0, 0.01)
FINES = (0, 2, 6, None)          # MCL_SORT_FINE; None: unset, the default form


def scan181():
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"].astype(np.float32)[::STEP].copy()


def cloud_of(kind, m):
    from monte_carlo_localization_amd import synth
    if kind == "tracking":
        return tracking_cloud(np.random.default_rng(8), N)
    p = synth.global_cloud(np.random.default_rng(9), m, N)            # sparse: whole buckets, units cut at their borders
    p[:2] += np.random.default_rng(99).uniform(0.1, 0.9, (2, N)) * float(np.float32(m.resolution))    # off the cell corners
    return p


def pixels(e, m, p):
    """pixel coordinates as the engine forms them (particle_constants): NaN where the heading is unusable"""
    ok = np.isfinite(p[2]) & (np.abs(p[2]) < 1e6)
    px = np.where(ok, (p[0] - np.float64(m.origin_x)) / np.float64(np.float32(m.resolution)), np.nan)
    py = np.where(ok, (p[1] - np.float64(m.origin_y)) / np.float64(np.float32(m.resolution)), np.nan)
    return px, py


def check_order(engine_mod, e, m, fine):
    o = e.sort_order()
    p = e.get_particles()
    n = p.shape[1]
    if fine is None:
        assert (o["fine"], o["fine_sub"]) == (2, 1)                                              # the default: quarter cells
    else:
        assert (o["fine"], o["fine_sub"]) == (fine, None)
    fine = o["fine"]
    assert o["n"] == n
    assert np.array_equal(np.sort(o["perm"]), np.arange(n, dtype=np.uint32))                    # a permutation
    k = o["keys"].astype(np.uint64)
    assert np.all(k[1:] >= k[:-1])                                                               # sorted over all 22 + F bits
    assert int(k.max()) < 1 << (engine_mod.SORT_KEY_LOG2 + fine)
    H, W = m.data.shape
    px, py = pixels(e, m, p)
    twin = engine_mod.host_sort_key(o["bbox"], o["tilemap"], W, H, px, py, p[2], fine=fine, n_layout=n, fine_sub=o["fine_sub"])
    assert np.array_equal(o["keys"], twin[o["perm"]])
    if fine:
        assert np.any(k & np.uint64((1 << fine) - 1))                                            # (and the fine bits are in use)
    return o


_runs = {}


def two_updates(engine_mod, m, ang, kind, fine, monkeypatch):
    """(logw, idx, particles) after each of two updates from the cloud, with the order checked after both; once per setting"""
    if (kind, fine) in _runs:
        return _runs[kind, fine]
    monkeypatch.setenv("MCL_SORT", "radix")
    if fine is None:
        monkeypatch.delenv("MCL_SORT_FINE", raising=False)
    else:
        monkeypatch.setenv("MCL_SORT_FINE", str(fine))
    e = make_engine(engine_mod, m, ang, N, seed=SEED)
    e.set_particles(cloud_of(kind, m), np.full(N, 1.0 / N))
    out = []
    coarse = []
    for _ in range(2):
        e.update(ACTION, scan181())
        assert e.ray_kernel_name() == "k_rays_sweep"
        o = check_order(engine_mod, e, m, fine)
        coarse.append(o["keys"] >> o["fine"])
        out.append((e.log_weights(), e.resample_indices(), e.get_particles()))
    e.close()
    _runs[kind, fine] = out, coarse
    return _runs[kind, fine]


@pytest.mark.parametrize("kind", ["tracking", "global"])
def test_order_is_the_twins_and_results_are_the_oracles(orc, engine_mod, spielberg, spielberg_oracle, monkeypatch, kind):
    ang = orc.beam_angles(angle_step=STEP)
    assert ang.size == 181
    runs = {F: two_updates(engine_mod, spielberg, ang, kind, F, monkeypatch) for F in FINES}
    (base, coarse0) = runs[0]
    for F in FINES[1:]:
        got, coarse = runs[F]
        for u in range(2):
            for a, b, what in zip(got[u], base[u], ("log-weights", "resample indices", "particles")):
                assert np.array_equal(a, b), (F, u, what)
            # the sorted coarse keys are the same multiset: units, cuts and windows see what they saw
            assert np.array_equal(coarse[u], coarse0[u]), (F, u)
    # ... and the oracle's, as tests/test_gpu_sweep.py holds them: exact fp64 sums, bit for bit; the draw of the second update from
    # the first update's weights (multinomial, Philox stream of update 1)
    T = orc.sensor_table(spielberg_oracle.max_range_px)
    L = orc.eng_log_table(T)
    oi = orc.obs_index(scan181(), spielberg_oracle)
    logw1, idx1, p1 = base[0]
    want1, _, _ = orc.eng_log_weights(spielberg_oracle, p1, ang, oi, L)
    assert np.array_equal(logw1, want1)
    _, q, _ = orc.eng_weights_from_log(want1)
    logw2, idx2, p2 = base[1]
    assert np.array_equal(idx2, orc.eng_resample_indices(q, 0, n_children=N, k53=orc.eng_philox_k53(SEED, 1, 0, N)))
    assert len(np.unique(idx2)) < N // 2                                # the second set is a collapsed one
    pick = np.random.default_rng(10).choice(N, 6000, replace=False)
    want2, _, _ = orc.eng_log_weights(spielberg_oracle, p2[:, pick], ang, oi, L)
    assert np.array_equal(logw2[pick], want2)


@pytest.mark.parametrize("form", ["one-rank-group", "kld"])
def test_other_resampling_kernels_write_the_same_keys(orc, engine_mod, spielberg, monkeypatch, form):
    """The sharded resampling (a group of one shard) and the KLD instantiations write the keys too: three updates with six fine bits
    give what they give with none."""
    ang = orc.beam_angles(angle_step=STEP)
    res = {}
    for F in (0, 6):
        monkeypatch.setenv("MCL_SORT", "radix")
        monkeypatch.setenv("MCL_SORT_FINE", str(F))
        if form == "kld":
            e = make_engine(engine_mod, spielberg, ang, N, seed=SEED)
        else:
            e = engine_mod.Group([0], max_particles=N, seed=SEED)
            e.set_map(spielberg.data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
            e.set_beam_angles(ang)
        e.set_particles(tracking_cloud(np.random.default_rng(8), N), np.full(N, 1.0 / N))
        if form == "kld":
            e.set_kld(min_particles=N, max_particles=N)      # pinned: every update draws N children through k_resample_motion_kld
        seen = []
        for _ in range(3):
            e.update(ACTION, scan181())
            seen.append((e.get_particles(), e.get_weights(), e.resample_indices()))
        if form == "kld":
            assert e.ray_kernel_name() == "k_rays_sweep" and e.sort_order()["fine"] == F
        e.close()
        res[F] = seen
    for u in range(3):
        for a, b in zip(res[0][u], res[6][u]):
            assert np.array_equal(a, b), u
