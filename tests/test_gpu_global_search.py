"""The global search on the GPU (mcl_global_search, DESIGN.md §4.13, rules S1-S8 of include/mcl_hip_engine.h): the score volume
against mcl_score_poses bit for bit and against the numpy statement tests/lfield_ref.py; the hits against a numpy restatement of
S5; that it finds a known pose; that an engine which searches runs the same updates, bit for bit, as one that never does; the
refusals."""
import ctypes as C

import numpy as np
import pytest

import lfield_ref as lr
import side_geometries as sg
from conftest import make_engine, tracking_cloud
from side_geometries import lattice, odd_scan, scan_at  # noqa: F401  (the helpers these tests defined, now by geometry)

pytestmark = pytest.mark.gpu

RES = np.float32(0.05)
OX, OY = -3.0, -2.25
MAX_RANGE = 12.0
W, H = 120, 90


class SmallMap:
    """120 x 90 cells at 0.05 m: an outer wall with two gaps (beams leave the map there), interior walls, a pillar, a post of one
    cell (on the lattice of stride 3, whose position count is then no multiple of 64), unknown cells"""

    def __init__(self, grid=None):
        if grid is None:
            g = np.zeros((H, W), np.int8)
            g[0, :] = g[-1, :] = 100
            g[:, 0] = g[:, -1] = 100
            g[0, 30:40] = 0
            g[40:50, -1] = 0
            g[30, 20:70] = 100
            g[30:75, 85] = 100
            g[55:60, 40:45] = 100
            g[64, 64] = 100
            g[60:80, 5:15] = -1
            g[10:14, 100:110] = -1
            grid = g
        self.data, self.resolution, self.origin_x, self.origin_y = grid, RES, OX, OY


@pytest.fixture(scope="module")
def small():
    return SmallMap()


@pytest.fixture(scope="module")
def small_oracle(orc, small):
    return orc.OracleMap(small.data, small.resolution, small.origin_x, small.origin_y)


def angles(orc, B):
    """B beams over the Hokuyo's 270 degrees (B = 1: the first of them)"""
    full = orc.beam_angles()
    return full[np.linspace(0, full.size - 1, B).round().astype(int)].copy() if B > 1 else full[:1].copy()


def lf_engine(engine_mod, m, ang, n=64, **lf_fields):
    e = make_engine(engine_mod, m, ang, n)
    e.set_likelihood_field(True, **lf_fields)
    return e


def score_all(e, poses, obs):
    """mcl_score_poses over all poses, in chunks of at most 65536"""
    return np.concatenate([e.score_poses(poses[s:s + 65536], obs)["log_likelihood"] for s in range(0, len(poses), 65536)])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


TRUE_POSE = (OX + 25.5 * 0.05, OY + 15.5 * 0.05, 0.4)


# ---- 1. the volume is mcl_score_poses, bit for bit
@pytest.mark.parametrize("stride,n_head,B,beam_stride,lf_fields", [
    (2, 5, 61, 1, {}),
    (3, 1, 61, 1, {}),
    (2, 5, 1, 1, {}),
    (3, 1, 1, 1, {}),
    (2, 5, 61, 3, {}),
    (3, 1, 61, 1, dict(max_occ_dist_m=4.6)),         # K = 8464 >= 8192: the table is read from global memory
])
def test_volume_is_score_poses(engine_mod, orc, small, small_oracle, stride, n_head, B, beam_stride, lf_fields):
    ang = angles(orc, B)
    e = lf_engine(engine_mod, small, ang, **lf_fields)
    if lf_fields:
        assert e.likelihood_table().size - 1 >= 8192
    obs = odd_scan(scan_at(orc, small_oracle, ang, TRUE_POSE))
    cells, xy, theta, poses = lattice(engine_mod, small, stride, n_head)
    if stride == 3:
        assert cells.size % 64 != 0 and cells.size > 256
    _, st = e.global_search(obs, max_hits=0, stride_cells=stride, n_headings=n_head, beam_stride=beam_stride)
    assert st["n_positions"] == cells.size and st["n_poses"] == len(poses)
    masked = obs.copy()
    masked[np.arange(B) % beam_stride != 0] = np.nan
    assert st["used_beams"] == lr.used_beams(ang, masked, MAX_RANGE)[0].size
    got = e.search_scores()
    want = score_all(e, poses, masked)
    assert got.shape == want.shape
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    if B > 1:
        assert np.unique(got).size > 100                   # (a volume, not a constant)


# ---- 2. the volume against the independent statement
def perturbed_scan(orc, om, ang):
    """ranges cast by the oracle from a known pose, moved by about a millimetre (fixed seed): end points off the cell edges"""
    return sg.perturbed_scan(orc, om, ang, TRUE_POSE)


def test_volume_is_the_restatement(engine_mod, orc, small, small_oracle):
    ang = angles(orc, 61)
    obs = perturbed_scan(orc, small_oracle, ang)
    cells, xy, theta, poses = lattice(engine_mod, small, 2, 5)
    D, Lf = lr.field(small.data, small.resolution), lr.table(small.resolution)
    want, alts, n_amb = lr.log_weights(np.ascontiguousarray(poses.T), ang, obs, D, Lf, small.resolution, OX, OY, MAX_RANGE)
    # LF4's cap, confirmed on the CPU statement alone before the device is held to it: ambiguous beams at most 1e-5 of all beams,
    # or 2 beams where that is fewer than one
    beams = len(poses) * lr.used_beams(ang, obs, MAX_RANGE)[0].size
    assert beams > 0 and int(n_amb.sum()) <= max(1e-5 * beams, 2), (int(n_amb.sum()), beams)
    e = lf_engine(engine_mod, small, ang)
    e.global_search(obs, max_hits=0, stride_cells=2, n_headings=5)
    got = e.search_scores()
    for i in np.flatnonzero(bits(got) != bits(want)):
        assert int(i) in alts and got[i] in alts[int(i)], (int(i), got[i], want[i], alts.get(int(i)))


# ---- 3. the hits are S5
def hits_ref(V, cells, stride, nms):
    """S5 restated on the 120 x 90 lattice of these tests: the candidates' pose indices, best first.  V: (n_head, n_pos)"""
    return sg.hits_ref(SmallMap(), V, cells, stride, nms)


def check_hits(engine_mod, e, small, obs, stride, n_head, nms, max_hits, beam_stride=1):
    cells, xy, theta, _ = lattice(engine_mod, small, stride, n_head)
    hits, st = e.global_search(obs, max_hits=max_hits, stride_cells=stride, n_headings=n_head, nms=nms, beam_stride=beam_stride)
    V = e.search_scores(n_head)
    want = hits_ref(V, cells, stride, nms)
    assert st["n_hits"] == want.size
    m = min(max_hits, want.size)
    assert len(hits) == m
    assert np.array_equal(hits["index"], want[:m])
    k, p = want[:m] // cells.size, want[:m] % cells.size
    assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
    assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p]))
    assert np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
    return hits, st, want


@pytest.mark.parametrize("stride,n_head", [(2, 5), (3, 1), (3, 2)])
@pytest.mark.parametrize("nms", [0, 1])
def test_hits_are_s5(engine_mod, orc, small, small_oracle, stride, n_head, nms):
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    obs = odd_scan(scan_at(orc, small_oracle, ang, TRUE_POSE))
    hits, st, want = check_hits(engine_mod, e, small, obs, stride, n_head, nms, max_hits=4096)
    assert want.size > 5
    if nms == 0:
        assert st["n_hits"] == st["n_poses"]                            # (no -inf in this table: every pose is a candidate)
    else:
        # no two neighbours are both candidates: at most one per 2 x 2 x 2 block of the lattice
        h0 = stride // 2
        nx, ny = (W - 1 - h0) // stride + 1, (H - 1 - h0) // stride + 1
        assert st["n_hits"] <= ((nx + 1) // 2) * ((ny + 1) // 2) * ((n_head + 1) // 2)
    # fewer hits asked for than there are: the same list, cut
    few, st2, _ = check_hits(engine_mod, e, small, obs, stride, n_head, nms, max_hits=5)
    assert st2["n_hits"] == st["n_hits"] and np.array_equal(few["index"], hits["index"][:5])
    # max_hits = 0 with a null hits: the count alone
    none, st3 = e.global_search(obs, max_hits=0, stride_cells=stride, n_headings=n_head, nms=nms)
    assert len(none) == 0 and st3["n_hits"] == st["n_hits"]


@pytest.mark.parametrize("nms", [0, 1])
def test_hits_of_a_scan_without_a_usable_beam(engine_mod, orc, small, nms):
    """every score is 0.0: the tie rule (the lower index is better) decides"""
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    obs = np.full(61, np.nan, np.float32)
    obs[5], obs[9] = MAX_RANGE, -1.0
    hits, st, want = check_hits(engine_mod, e, small, obs, 2, 5, nms, max_hits=65536)
    assert st["used_beams"] == 0
    assert np.array_equal(bits(e.search_scores()), np.zeros(st["n_poses"], np.uint64))
    assert hits["index"][0] == 0 and np.all(np.diff(hits["index"]) > 0)
    assert st["n_hits"] == (st["n_poses"] if nms == 0 else want.size)


# ---- 4. it localises
def test_search_finds_a_lattice_pose(engine_mod, orc, small):
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    stride, n_head = 2, 72
    cells, xy, theta, _ = lattice(engine_mod, small, stride, n_head)
    p = int(np.flatnonzero(cells == 15 * W + 25)[0])          # the lattice cell (col 25, row 15): free, in the asymmetric lower left
    k = 50
    truth = np.array([xy[p, 0], xy[p, 1], theta[k]])
    obs = e.expected_scans(truth)[0]                          # noise-free
    hits, st = e.global_search(obs, max_hits=8, stride_cells=stride, n_headings=n_head)
    assert st["n_hits"] >= 1
    best = hits[0]["pose"]
    step = stride * float(RES)
    assert abs(best[0] - truth[0]) <= step * (1 + 1e-9) and abs(best[1] - truth[1]) <= step * (1 + 1e-9)
    dth = abs((best[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi)
    assert dth <= 2 * np.pi / n_head * (1 + 1e-9)
    # ... and seeding from the hits gives a cloud around it
    counts = engine_mod.seed_counts(hits["log_likelihood"], 64)
    assert counts.sum() == 64 and counts[0] == counts.max()
    e.init_particles_mixture(hits["pose"], np.diag([0.01, 0.01, 0.01]), counts)
    assert e.particle_count() == 64


# ---- 5. read-only
def test_search_leaves_the_updates_alone(engine_mod, orc, small, small_oracle):
    ang = angles(orc, 61)
    n = 2000
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=TRUE_POSE, sig=(0.2, 0.2, 0.2))
    scans = [scan_at(orc, small_oracle, ang, (TRUE_POSE[0] + 0.05 * t, TRUE_POSE[1], TRUE_POSE[2])) for t in range(1, 4)]
    a, b = lf_engine(engine_mod, small, ang, n), lf_engine(engine_mod, small, ang, n)
    assert a.search_bytes() == 0 and b.search_bytes() == 0
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    hits0, _ = b.global_search(scans[0], max_hits=4)
    for t, scan in enumerate(scans):
        for e in (a, b):
            e.update((0.05, 0.0, 0.0), scan)
        hits, st = b.global_search(scan, max_hits=4, stride_cells=2 + t % 2, n_headings=8)
        assert st["device_bytes"] == b.search_bytes() > 0
    assert a.search_bytes() == 0
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))


# ---- 6. the refusals
def expect(engine_mod, status, fn, *args, **kw):
    with pytest.raises(engine_mod.EngineError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    return str(ei.value)


def test_refusals(engine_mod, orc, small):
    INVALID, NOT_READY = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY
    ang = angles(orc, 61)
    obs = np.full(61, 1.0, np.float32)
    # not ready: no map, no beams, the field off -- the message says which
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.global_search, obs)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    assert "beam" in expect(engine_mod, NOT_READY, e.global_search, obs)
    e.set_beam_angles(ang)
    assert "likelihood-field" in expect(engine_mod, NOT_READY, e.global_search, obs)
    expect(engine_mod, NOT_READY, e.search_scores)                     # before any search
    e.set_likelihood_field(True)
    # refused arguments
    for fields in (dict(stride_cells=0), dict(n_headings=0), dict(beam_stride=0), dict(nms=2), dict(reserved=(0, 0, 0, 1))):
        expect(engine_mod, INVALID, e.global_search, obs, **fields)
    expect(engine_mod, INVALID, e.global_search, obs[:60])             # n_beams != B
    expect(engine_mod, INVALID, e.global_search, obs, max_hits=65537)
    n, st = C.c_int64(), np.zeros(4, np.uint64)
    cfg = engine_mod.default_search_config()
    assert e.lib.mcl_global_search(e._h, C.byref(cfg), None, 61, 0, None, C.byref(n), st.ctypes.data_as(C.c_void_p)) == INVALID   # null obs
    assert e.lib.mcl_global_search(e._h, C.byref(cfg), obs.ctypes.data_as(C.c_void_p), 61, -1, None, C.byref(n), None) == INVALID
    assert e.lib.mcl_global_search(e._h, C.byref(cfg), obs.ctypes.data_as(C.c_void_p), 61, 4, None, C.byref(n), None) == INVALID  # null hits
    expect(engine_mod, INVALID, e.global_search, obs, stride_cells=1, n_headings=20000)     # ~10 000 positions x 20 000 >= 2^27
    assert e.search_bytes() < 1 << 22                                  # ... refused before the volume was asked for
    # a search, then a new map: the volume is gone until the next search
    hits, st = e.global_search(obs, max_hits=2, n_headings=3)
    assert e.search_scores().size == st["n_poses"]
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    expect(engine_mod, NOT_READY, e.search_scores)
    e.global_search(obs, max_hits=2, n_headings=3)
    assert e.search_scores().size == st["n_poses"]
    # a lattice without a free position
    full = np.full((H, W), 100, np.int8)
    full[0, 0] = 0                                                     # free, but on no lattice of stride 2
    e.set_map(full, small.resolution, small.origin_x, small.origin_y)
    assert "position" in expect(engine_mod, NOT_READY, e.global_search, obs)
    # the field off again: refused again
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    e.set_likelihood_field(False)
    expect(engine_mod, NOT_READY, e.global_search, obs)
