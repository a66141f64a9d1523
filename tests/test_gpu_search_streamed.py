"""The global search in heading slabs on the GPU (mcl_global_search_streamed, DESIGN.md §4.16, rules ST1-ST6 of
include/mcl_hip_engine.h): the hits and their count against mcl_global_search and mcl_global_search_sequence byte for byte, for
every slab size; ties across slab boundaries; a lattice beyond 2^27 poses, checked against mcl_score_poses; that an engine which
searches runs the same updates, bit for bit, as one that never does; the refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_engine, tracking_cloud
from side_geometries import compose, odd_scan, scan_at  # noqa: F401  (imported from here by other tests too)

pytestmark = pytest.mark.gpu

RES = np.float32(0.05)
OX, OY = -3.0, -2.25
MAX_RANGE = 12.0
W, H = 120, 90
MIB = 1 << 20


class SmallMap:
    """120 x 90 cells at 0.05 m: an outer wall with two gaps (beams leave the map there), interior walls, a pillar, a post of one
    cell (on the lattice of stride 3, whose position count is then no multiple of 64), unknown cells"""

    def __init__(self):
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
        self.data, self.resolution, self.origin_x, self.origin_y = g, RES, OX, OY


@pytest.fixture(scope="module")
def small():
    return SmallMap()


@pytest.fixture(scope="module")
def small_oracle(orc, small):
    return orc.OracleMap(small.data, small.resolution, small.origin_x, small.origin_y)


def angles(orc, B):
    full = orc.beam_angles()
    return full[np.linspace(0, full.size - 1, B).round().astype(int)].copy()


def lf_engine(engine_mod, m, ang, n=64):
    e = make_engine(engine_mod, m, ang, n)
    e.set_likelihood_field(True)
    return e


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


TRUE_POSE = (OX + 25.5 * 0.05, OY + 15.5 * 0.05, 0.4)


def same(a, b):
    """two results (hits, stats): the hits byte for byte, and their count"""
    return a[0].tobytes() == b[0].tobytes() and len(a[0]) == len(b[0]) and a[1]["n_hits"] == b[1]["n_hits"]


def check_stats(st, n, G):
    assert st["slab_headings"] == min(G, n) and st["n_slabs"] == -(-n // min(G, n))
    assert st["headings_scored"] <= n + 2
    if G >= n:
        assert st["n_slabs"] == 1 and st["headings_scored"] == n


# ---- 1. identity with mcl_global_search
@pytest.mark.parametrize("stride,n_head", [(2, 5), (3, 1), (3, 2), (3, 7)])
@pytest.mark.parametrize("nms", [0, 1])
def test_hits_are_those_of_the_unstreamed_search(engine_mod, orc, small, small_oracle, stride, n_head, nms):
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    obs = odd_scan(scan_at(orc, small_oracle, ang, TRUE_POSE))
    f = dict(stride_cells=stride, n_headings=n_head, nms=nms)
    for max_hits in (0, 16, 65536):
        want = e.global_search(obs, max_hits=max_hits, **f)
        assert want[1]["n_hits"] > 5
        if stride == 3:
            assert want[1]["n_positions"] % 64 != 0
        for G in sorted({1, 2, 3, n_head, n_head + 1}):
            got = e.global_search_streamed(obs, max_hits=max_hits, slab_headings=G, **f)
            assert same(got, want), (max_hits, G)
            check_stats(got[1], n_head, G)
            assert got[1]["n_positions"] == want[1]["n_positions"] and got[1]["n_poses"] == want[1]["n_poses"]
            assert got[1]["used_beams"] == want[1]["used_beams"]
            if max_hits == 0:
                assert got[1]["candidates_compacted"] == 0
            else:
                assert min(max_hits, got[1]["n_hits"]) <= got[1]["candidates_compacted"] <= got[1]["n_hits"]
        # the default plan (the budget holds every heading), and a zero rel in the place of none
        assert same(e.global_search_streamed(obs, max_hits=max_hits, **f), want)
        assert same(e.global_search_streamed(obs, rel=np.zeros(3), max_hits=max_hits, slab_headings=2, **f), want)


# ---- 2. ties across slab boundaries
@pytest.mark.parametrize("nms", [0, 1])
def test_ties_come_out_in_index_order(engine_mod, orc, small, nms):
    """a scan without a usable beam: every score is +0.0, and the lower index is the better pose, across slabs too"""
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    obs = np.full(61, np.nan, np.float32)
    obs[5], obs[9] = MAX_RANGE, -1.0
    f = dict(stride_cells=2, n_headings=5, nms=nms)
    want = e.global_search(obs, max_hits=65536, **f)
    assert want[1]["used_beams"] == 0 and np.all(want[0]["log_likelihood"] == 0.0)
    assert len(want[0]) > 5 if nms == 0 else len(want[0]) >= 1           # (among equal neighbours only the lowest index is a maximum)
    assert np.all(np.diff(want[0]["index"]) > 0)
    if nms == 0:
        assert want[1]["n_hits"] == want[1]["n_poses"]
    for G in (1, 2):
        got = e.global_search_streamed(obs, max_hits=65536, slab_headings=G, **f)
        assert same(got, want), G
    # fewer hits than candidates: the list is full after the first slab, and later ties must lose
    few = e.global_search_streamed(obs, max_hits=7, slab_headings=1, **f)
    assert same(few, e.global_search(obs, max_hits=7, **f))


# ---- 3. identity with mcl_global_search_sequence
@pytest.mark.parametrize("stride,n_head", [(2, 5), (3, 7)])
def test_hits_are_those_of_the_sequence_search(engine_mod, orc, small, small_oracle, stride, n_head):
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    rel = np.array([[-0.5, 0.0, 0.1], [0.0, 0.0, 0.0]])
    scans = np.stack([scan_at(orc, small_oracle, ang, compose(TRUE_POSE, r)) for r in rel])
    scans[1] = odd_scan(scans[1])
    for nms in (0, 1):
        f = dict(stride_cells=stride, n_headings=n_head, nms=nms)
        want = e.global_search_sequence(scans, rel, max_hits=4096, **f)
        assert want[1]["n_hits"] > 5
        for G in (1, 3):
            got = e.global_search_streamed(scans, rel, max_hits=4096, slab_headings=G, **f)
            assert same(got, want), (nms, G)
            check_stats(got[1], n_head, G)
            assert got[1]["used_beams"] == want[1]["used_beams"]


# ---- 4. beyond the old limit
def neighbours(idx, n_pos, n_head, pmap, ix, iy):
    """the indices of the up to 26 lattice neighbours of pose idx (S5)"""
    k, p = divmod(int(idx), n_pos)
    out = set()
    for dk in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = pmap[iy[p] + 1 + dy, ix[p] + 1 + dx]
                if q >= 0:
                    out.add(((k + dk) % n_head) * n_pos + int(q))
    out.discard(int(idx))
    return sorted(out)


def test_a_lattice_beyond_the_old_limit(engine_mod, orc, small, small_oracle):
    ang = angles(orc, 3)
    e = lf_engine(engine_mod, small, ang)
    obs = scan_at(orc, small_oracle, ang, TRUE_POSE)
    cells, xy = engine_mod.host_search_lattice(small.data, small.resolution, small.origin_x, small.origin_y, stride_cells=1)
    n_pos, n = cells.size, 16384
    while n_pos * n < 1 << 27:
        n *= 2
    theta = engine_mod.host_search_headings(n_headings=n)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.global_search(obs, max_hits=64, stride_cells=1, n_headings=n)
    assert ei.value.status == engine_mod.MCL_ERR_INVALID_ARG
    before = e.search_bytes()
    f = dict(stride_cells=1, n_headings=n, budget_bytes=64 * MIB)
    hits, st = e.global_search_streamed(obs, max_hits=64, nms=1, **f)
    assert st["n_positions"] == n_pos and st["n_poses"] == n_pos * n and 1 <= len(hits) == min(64, st["n_hits"])
    # the budget: the slab buffers are the plan's, within 64 MiB; the rest is what the lattice, the headings and the scan take
    G, slabs, plan_bytes = engine_mod.host_search_slabs(n_pos, stride_cells=1, n_headings=n, budget_bytes=64 * MIB)
    assert (st["slab_headings"], st["n_slabs"]) == (G, slabs) and slabs > 1 and plan_bytes <= 64 * MIB
    assert st["headings_scored"] == n + 2
    assert st["device_bytes"] == e.search_bytes()
    rest = st["device_bytes"] - before - plan_bytes
    assert 0 <= rest <= n_pos * 24 + W * H * 4 + n * 8 + 3 * 16 + 4096
    # every hit is the lattice pose of its index, scored as mcl_score_poses scores it, in S5's order
    idx = hits["index"]
    k, p = idx // n_pos, idx % n_pos
    assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p])) and np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
    ll = hits["log_likelihood"]
    assert np.array_equal(bits(ll), bits(e.score_poses(hits["pose"], obs)["log_likelihood"]))
    assert all(ll[i] > ll[i + 1] or (ll[i] == ll[i + 1] and idx[i] < idx[i + 1]) for i in range(len(hits) - 1))
    # ... and better than each of its up to 26 neighbours
    ix, iy = (cells.astype(np.int64) % W), (cells.astype(np.int64) // W)
    pmap = np.full((H + 2, W + 2), -1, np.int64)
    pmap[iy + 1, ix + 1] = np.arange(n_pos)
    for h in hits:
        nb = np.array(neighbours(h["index"], n_pos, n, pmap, ix, iy), np.int64)
        assert 7 <= nb.size <= 26
        poses = np.column_stack([xy[nb % n_pos], theta[nb // n_pos]])
        t = e.score_poses(poses, obs)["log_likelihood"]
        assert np.all((h["log_likelihood"] > t) | ((h["log_likelihood"] == t) & (h["index"] < nb)))
    # completeness, spot-checked: the headings of n = 64 are headings of this lattice, so its best pose is a pose of this one
    step = n // 64
    assert np.array_equal(bits(engine_mod.host_search_headings(n_headings=64)), bits(theta[::step]))
    coarse, _ = e.global_search(obs, max_hits=1, stride_cells=1, n_headings=64, nms=0)
    best, st0 = e.global_search_streamed(obs, max_hits=1, nms=0, **f)
    assert len(coarse) == 1 and len(best) == 1 and st0["n_slabs"] > 1
    assert not (coarse[0]["log_likelihood"] > best[0]["log_likelihood"])
    assert best[0]["log_likelihood"] >= hits[0]["log_likelihood"]


# ---- 5. read-only
def test_streamed_search_leaves_the_updates_alone(engine_mod, orc, small, small_oracle):
    ang = angles(orc, 61)
    n = 2000
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=TRUE_POSE, sig=(0.2, 0.2, 0.2))
    scans = [scan_at(orc, small_oracle, ang, (TRUE_POSE[0] + 0.05 * t, TRUE_POSE[1], TRUE_POSE[2])) for t in range(1, 4)]
    a, b = lf_engine(engine_mod, small, ang, n), lf_engine(engine_mod, small, ang, n)
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    b.global_search_streamed(scans[0], max_hits=4)
    idx = []
    for t, scan in enumerate(scans):
        for e in (a, b):
            e.update((0.05, 0.0, 0.0), scan)
        idx.append((a.resample_indices(), b.resample_indices()))
        hits, st = b.global_search_streamed(scan, max_hits=4, slab_headings=1 + t, stride_cells=2 + t % 2, n_headings=8)
        assert len(hits) == 4 and st["device_bytes"] == b.search_bytes() > 0
    assert a.search_bytes() == 0
    assert all(np.array_equal(x, y) for x, y in idx)
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))
    # no volume is kept, until an unstreamed search runs
    with pytest.raises(engine_mod.EngineError) as ei:
        b.search_scores()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    _, st = b.global_search(scans[0], max_hits=0, n_headings=3)
    assert b.search_scores().size == st["n_poses"]
    b.global_search_streamed(scans[0], max_hits=0, n_headings=3)
    with pytest.raises(engine_mod.EngineError) as ei:
        b.search_scores()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY


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
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.global_search_streamed, obs)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    e.set_beam_angles(ang)
    assert "likelihood-field" in expect(engine_mod, NOT_READY, e.global_search_streamed, obs)
    e.set_likelihood_field(True)
    assert "n_beams" in expect(engine_mod, INVALID, e.global_search_streamed, obs[:60])
    n, st = C.c_int64(), np.zeros(8, np.uint64)
    cfg, sc = engine_mod.default_search_config(), engine_mod.search_stream_config()
    p = obs.ctypes.data_as(C.c_void_p)
    assert e.lib.mcl_global_search_streamed(e._h, C.byref(cfg), C.byref(sc), p, None, 1, 61, 4, None, C.byref(n), None) == INVALID
    assert "hits is null" in e.lib.mcl_last_error(e._h).decode()
    two = np.full((2, 61), 1.0, np.float32)
    assert "n_scans" in expect(engine_mod, INVALID, e.global_search_streamed, np.full((17, 61), 1.0, np.float32), np.zeros((17, 3)))
    assert e.lib.mcl_global_search_streamed(e._h, C.byref(cfg), C.byref(sc), p, None, 0, 61, 0, None, C.byref(n), None) == INVALID
    assert "n_scans" in e.lib.mcl_last_error(e._h).decode()
    assert "rel is null" in expect(engine_mod, INVALID, e.global_search_streamed, two)                 # NULL only with one scan
    assert "finite" in expect(engine_mod, INVALID, e.global_search_streamed, two, np.array([[0, 0, 0], [0, np.inf, 0]]))
    assert "reserved" in expect(engine_mod, INVALID, e.global_search_streamed, obs, stream_reserved=(0, 0, 1, 0, 0))
    assert "slab_headings" in expect(engine_mod, INVALID, e.global_search_streamed, obs, slab_headings=-1)
    assert e.search_bytes() == 0
    # a budget too small for G = 1: the message names the bytes needed, nothing is allocated, an earlier volume stays
    _, st1 = e.global_search(obs, max_hits=0, n_headings=3)
    held = e.search_bytes()
    need = engine_mod.host_search_slabs(st1["n_positions"], n_headings=3, slab_headings=1)[2]
    msg = expect(engine_mod, INVALID, e.global_search_streamed, obs, n_headings=3, budget_bytes=need - 1)
    assert str(need) in msg and "bytes" in msg
    assert e.search_bytes() == held and e.search_scores().size == st1["n_poses"]
    hits, st2 = e.global_search_streamed(obs, n_headings=3, budget_bytes=need)
    assert st2["slab_headings"] == 1 and st2["n_slabs"] == 3 and e.search_bytes() == held + need
