"""The buffers the engine, the clustering, the communicator and the group keep between calls (csrc/mcl_buffers.h): one long-lived
engine walks through steps that make every buffer grow, shrink in demand and grow again -- particle counts on every update path,
beam sets, maps, KLD, the likelihood field, recovery, clusterings, the staged calls, a refused call in the middle -- and after
each step its outputs are, byte for byte, those of a fresh engine that made only that step.  Randomness is injected (normals and
uniforms), so the update counter of the Philox streams does not enter.  A second engine in the same process, after the first was
closed, repeats the first; a one-device group and a one-rank communicator are created and closed twice."""
import types

import numpy as np
import pytest

from test_gpu_search_streamed import MAX_RANGE, TRUE_POSE, SmallMap, scan_at

pytestmark = pytest.mark.gpu

CAP = 131072
ACTION = (0.05, 0.0, 0.02)
MCL_ERR_UNSUPPORTED = -5                                                   # (include/mcl_hip_engine.h)


def cloud(n, sig=(0.15, 0.15, 0.2)):
    rng = np.random.default_rng(n)
    p = np.asarray(TRUE_POSE)[:, None] + rng.normal(0.0, sig, (n, 3)).T
    return np.ascontiguousarray(p), np.full(n, 1.0 / n)


def path_of(e):
    t = e.stage_timings()
    return "tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular")


def state(e, idx=True, steps=True):
    out = [e.get_particles().tobytes(), e.get_weights().tobytes(), e.log_weights().tobytes(), e.expected_pose().tobytes()]
    if idx:
        out.append(e.resample_indices().tobytes())
    if steps:
        out.append(e.ray_steps().tobytes())
    return b"".join(out)


def updates(n, B, k, expect=None, kernel=None, steps=True):
    """set n particles, k updates with injected normals and uniforms; the path of every update is part of the result"""
    def call(e, w):
        e.set_particles(*cloud(n))
        rng = np.random.default_rng(n + B)
        out, paths = [], []
        for _ in range(k):
            rows = e.kld_state()[1]
            e.update(ACTION, w.scan[B], normals=rng.normal(size=(rows, 3)), uniforms=rng.random(rows))
            paths.append(path_of(e))
            out.append(state(e, steps=steps))
        if expect:
            assert paths == expect, (n, B, paths)
        if kernel:
            assert e.ray_kernel_name() == kernel
        return b"".join(out) + repr((paths, e.kld_state(), e.particle_count())).encode()
    return call


def sensor(n, B, steps=True):
    def call(e, w):
        e.set_particles(*cloud(n))
        e.sensor_update(w.scan[B])
        return state(e, idx=False, steps=steps)
    return call


def clusters(n, K):
    def call(e, w):
        e.set_particles(*cloud(n, (1.0, 1.0, 1.0)))                        # (spread: many occupied bins, many components)
        e.sensor_update(w.scan[61])
        cl, info = e.pose_clusters(max_clusters=K, bin_x_m=0.1, bin_y_m=0.1, n_theta_bins=12)
        assert info["n_clusters"] >= 1 and len(cl) == min(K, info["n_clusters"])
        return cl.tobytes() + repr(sorted(info.items())).encode() + e.cluster_labels().tobytes()
    return call


def feature(name, n, B=61, **fields):
    """KLD / the likelihood field / recovery on, two updates and a weighting (with the field: its field and table too), off again"""
    def call(e, w):
        lf = name == "likelihood_field"
        getattr(e, "set_" + name)(True, **fields)
        out = updates(n, B, 2, steps=not lf)(e, w) + sensor(n // 2, B, steps=not lf)(e, w)
        if lf:
            out += e.likelihood_field().tobytes() + e.likelihood_table().tobytes()
        if name == "recovery":
            out += repr(e.recovery_state()).encode()
        getattr(e, "set_" + name)(False)
        return out
    return call


def distinct_parents(n_children, n_total):
    def call(e, w):
        import torch
        dev = torch.device("cuda:0")
        rng = np.random.default_rng(n_total)
        parent = torch.from_numpy(rng.integers(0, n_total, n_children).astype(np.int32)).to(dev)
        distinct = torch.zeros(n_children, dtype=torch.int64, device=dev)
        slot = torch.zeros(n_children, dtype=torch.int32, device=dev)
        cnt = e.stage_distinct_parents(parent.data_ptr(), n_children, n_total, distinct.data_ptr(), slot.data_ptr())
        torch.cuda.synchronize()
        assert 0 < cnt <= n_children
        return distinct[:cnt].cpu().numpy().tobytes() + slot.cpu().numpy().tobytes()
    return call


def long_scan(n):
    """mcl_scan_weights over an array longer than max_particles (the scan's spine grows), then an ordinary update"""
    def call(e, w):
        import torch
        dev = torch.device("cuda:0")
        q = torch.from_numpy(np.random.default_rng(n).integers(0, 1 << 20, n).astype(np.int64)).to(dev)
        cdf = torch.zeros(n, dtype=torch.int64, device=dev)
        e.scan_weights(q.data_ptr(), cdf.data_ptr(), n)
        torch.cuda.synchronize()
        got = cdf.cpu().numpy()
        assert np.array_equal(got, np.cumsum(q.cpu().numpy()))
        return got.tobytes() + updates(16384, 61, 2)(e, w)
    return call


def refused_map(e, w):
    """a range beyond 2047 px: refused, and nothing of the engine is lost"""
    from monte_carlo_localization_amd.engine import EngineError
    m = w.maps["small"]
    with pytest.raises(EngineError) as ei:
        e.set_map(m.data, MAX_RANGE / 2100.0, m.origin_x, m.origin_y)
    assert ei.value.status == MCL_ERR_UNSUPPORTED and "2047" in str(ei.value)
    return sensor(2048, 61)(e, w)


# (name, map, beams, call): the sizes of every buffer grow, shrink and grow again; the features interleaved
STEPS = [
    ("tiny 2048", "small", 61, updates(2048, 61, 3, ["regular", "tiny", "tiny"])),
    ("graph 16384", "small", 61, updates(16384, 61, 3, ["regular", "graph", "graph"])),
    ("sweep 65536 x 181", "small", 181, updates(65536, 181, 2, kernel="k_rays_sweep")),
    ("sensor 4096 x 61", "small", 61, sensor(4096, 61)),
    ("clusters 4", "small", 61, clusters(8192, 4)),
    ("kld", "small", 61, feature("kld", 16384, max_particles=32768, min_particles=1024)),
    ("cropped map", "cropped", 61, updates(16384, 61, 2)),
    ("clusters 64", "cropped", 61, clusters(65536, 64)),
    ("kld, cropped map", "cropped", 61, feature("kld", 4096, min_particles=512)),
    ("refused map", "small", 61, refused_map),
    ("field", "small", 61, feature("likelihood_field", 16384)),
    ("field, 181 beams", "small", 181, feature("likelihood_field", 32768, B=181, max_occ_dist_m=1.0)),
    ("distinct parents", "small", 61, distinct_parents(50000, 4 * CAP)),
    ("recovery", "small", 61, feature("recovery", 16384)),
    ("long scan", "small", 61, long_scan(3 * CAP + 5)),
    ("distinct parents, more", "small", 61, distinct_parents(CAP, 1 << 26)),
    ("sweep 131072 x 181", "small", 181, updates(131072, 181, 2, kernel="k_rays_sweep")),
    ("kld again", "small", 61, feature("kld", 16384, max_particles=CAP, min_particles=1024, bin_x_m=0.25, bin_y_m=0.25)),
    ("field, 61 beams again", "cropped", 61, feature("likelihood_field", 2048)),
    ("clusters 4 again", "small", 61, clusters(2048, 4)),
    ("tiny 2048 again", "small", 61, updates(2048, 61, 3, ["regular", "tiny", "tiny"])),
]
RADIX_STEPS = [STEPS[2], STEPS[16], ("sweep 65536 x 181 again", "small", 181, updates(65536, 181, 2, kernel="k_rays_sweep"))]


@pytest.fixture(scope="module")
def world(orc):
    m = SmallMap()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    cropped = types.SimpleNamespace(data=np.ascontiguousarray(m.data[:80, :100]), resolution=m.resolution, origin_x=m.origin_x,
                                    origin_y=m.origin_y)
    ang = {B: orc.beam_angles(angle_step=1080 // (B - 1)) for B in (61, 181)}
    assert all(a.size == B for B, a in ang.items())
    scan = {B: scan_at(orc, om, a, TRUE_POSE) for B, a in ang.items()}
    return types.SimpleNamespace(maps=dict(small=m, cropped=cropped), ang=ang, scan=scan)


def place(e, w, map_name, B, have):
    """the step's map and beam set, set when they are not the engine's current ones"""
    if have.get("map") != map_name:
        m = w.maps[map_name]
        e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
    if have.get("B") != B:
        e.set_beam_angles(w.ang[B])
    have.update(map=map_name, B=B)


def run_steps(engine_mod, w, steps, fresh):
    e = engine_mod.Engine(max_particles=CAP, keep_ray_steps=1, seed=3)
    have, out = {}, []
    for name, map_name, B, call in steps:
        place(e, w, map_name, B, have)
        got = call(e, w)
        if fresh is not None:
            assert got == fresh(name, map_name, B, call), name
        out.append(got)
    e.close()
    return out


@pytest.fixture(scope="module")
def fresh(engine_mod, world):
    """the bytes of a step on an engine that makes no other step (made once per step)"""
    seen = {}

    def get(name, map_name, B, call):
        if name not in seen:
            e = engine_mod.Engine(max_particles=CAP, keep_ray_steps=1, seed=3)
            place(e, world, map_name, B, {})
            seen[name] = call(e, world)
            e.close()
        return seen[name]
    return get


def test_every_step_equals_a_fresh_engine(engine_mod, world, fresh):
    run_steps(engine_mod, world, STEPS, fresh)


def test_radix_ordering_buffers(engine_mod, world, monkeypatch):
    """MCL_SORT=radix (read at mcl_create): the second key / index arrays and rocPRIM's scratch, grown and reused"""
    monkeypatch.setenv("MCL_SORT", "radix")
    seen = {}

    def fresh_radix(name, map_name, B, call):
        if name not in seen:
            seen[name] = run_steps(engine_mod, world, [(name, map_name, B, call)], None)[0]
        return seen[name]
    got = run_steps(engine_mod, world, RADIX_STEPS, fresh_radix)
    monkeypatch.delenv("MCL_SORT")
    hist = run_steps(engine_mod, world, RADIX_STEPS[:1], None)
    assert got[0] == hist[0]                                               # (the ordering never changes a result)


def test_create_use_close_twice_in_one_process(engine_mod, world):
    first = run_steps(engine_mod, world, STEPS[:6], None)
    assert run_steps(engine_mod, world, STEPS[:6], None) == first


def test_group_and_communicator_twice(engine_mod, world):
    m, ang, scan = world.maps["small"], world.ang[61], world.scan[61]
    n = 16384
    rounds = []
    for _ in range(2):
        g = engine_mod.Group([0], max_particles=n, seed=5)
        g.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        g.set_beam_angles(ang)
        g.set_particles(*cloud(n))
        out = []
        for _ in range(3):
            g.update(ACTION, scan)
            out.append(g.get_particles().tobytes() + g.get_weights().tobytes() + g.resample_indices().tobytes())
        g.close()
        e = engine_mod.Engine(max_particles=n, seed=5)
        e.set_map(m.data, m.resolution, m.origin_x, m.origin_y)
        e.set_beam_angles(ang)
        e.set_particles(*cloud(n))
        if e.comm_available()[0]:
            for _ in range(2):                                             # (and a second communicator on the same engine)
                e.comm_create(e.comm_unique_id(), 1, 0)
                e.comm_selftest()
                e.comm_update(ACTION, scan)
                out.append(e.get_particles().tobytes() + e.resample_indices().tobytes())
                e.comm_destroy()
        e.close()
        rounds.append(out)
    assert rounds[0] == rounds[1]
