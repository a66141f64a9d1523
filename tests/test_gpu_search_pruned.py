"""The global search with exact pruning on the GPU (mcl_global_search_pruned, DESIGN.md §4.20, rules P1 - P6 of
include/mcl_hip_engine.h).  The yardstick is mcl_global_search in the same process: the hits byte for byte; the bounds against the
exhaustive volume with no tolerance; the rounds against tests/search_pruned_ref.py; that an engine which calls it runs the same
updates and searches as one that never does; the refusals."""
import numpy as np
import pytest

import search_pruned_ref as pr
from conftest import make_engine, tracking_cloud
from side_geometries import angles, odd_scan, scan_at

pytestmark = pytest.mark.gpu

RES = np.float32(0.05)
OX, OY = -2.4, -1.8
W, H = 97, 71                                   # no multiple of block * stride for any block and stride used here
N_HEAD = 8
FIRST = 24                                      # a small first round, so that calls run several rounds


class Room:
    """97 x 71 cells at 0.05 m: an outer wall with a gap in the bottom wall (beams leave the map there), two inner walls, a pillar,
    unknown cells; at stride 1 and 8 headings the volume stays below 65536 poses, so max_hits can exceed the candidates"""

    def __init__(self, empty=False):
        g = np.zeros((H, W), np.int8)
        if not empty:
            g[0, :] = g[-1, :] = 100
            g[:, 0] = g[:, -1] = 100
            g[0, 20:28] = 0
            g[25, 15:60] = 100
            g[25:60, 70] = 100
            g[45:49, 30:34] = 100
            g[55:65, 5:12] = -1
        self.data, self.resolution, self.origin_x, self.origin_y = g, RES, OX, OY


TRUE_POSE = (OX + 40.5 * 0.05, OY + 12.5 * 0.05, 0.4)


@pytest.fixture(scope="module")
def room():
    return Room()


@pytest.fixture(scope="module")
def ang(orc):
    return angles(orc, 61)


@pytest.fixture(scope="module")
def scans(orc, room, ang):
    om = orc.OracleMap(room.data, room.resolution, room.origin_x, room.origin_y)
    inside = scan_at(orc, om, ang, TRUE_POSE)
    off = inside.copy()
    off[::3] = 9.0                              # longer than the map: these end points are off the map from every pose
    return dict(inside=inside, off_map=off, odd=odd_scan(inside))


@pytest.fixture(scope="module")
def eng(engine_mod, room, ang):
    e = make_engine(engine_mod, room, ang, 64)
    e.set_likelihood_field(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def exhaustive(eng, scans):
    """mcl_global_search once per (scan, stride, nms): its hits with the largest max_hits, its candidate count, its volume"""
    memo = {}

    def get(scan, stride, nms, n_head=N_HEAD):
        key = (scan, stride, nms, n_head)
        if key not in memo:
            hits, st = eng.global_search(scans[scan], max_hits=65536, stride_cells=stride, n_headings=n_head, nms=nms)
            V = eng.search_scores().reshape(n_head, -1)
            V.setflags(write=False)
            memo[key] = (hits.copy(), st, V)
        return memo[key]
    return get


def same_hits(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


# ---- 1. the hits are mcl_global_search's, byte for byte
@pytest.mark.parametrize("scan", ["inside", "off_map", "odd"])
@pytest.mark.parametrize("max_hits", [1, 16, 65536])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("nms", [0, 1])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_hits_identical(eng, scans, exhaustive, block, nms, stride, max_hits, scan):
    want, st, V = exhaustive(scan, stride, nms)
    assert st["n_hits"] < 65536 and st["n_poses"] == V.size                 # 65536 is more than there are candidates
    got, ps = eng.global_search_pruned(scans[scan], max_hits=max_hits, block=block, first_pairs=FIRST, stride_cells=stride,
                                       n_headings=N_HEAD, nms=nms)
    print("pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"])
    assert ps["n_hits"] == len(got) == min(max_hits, st["n_hits"])
    assert same_hits(got, want[:len(got)])
    assert ps["guard_fallbacks"] == 0
    assert (ps["n_positions"], ps["n_poses"], ps["used_beams"]) == (st["n_positions"], st["n_poses"], st["used_beams"])
    assert 1 <= ps["pairs_scored"] <= ps["pairs"] and ps["rounds"] >= 1


def test_hits_identical_with_the_defaults(eng, scans, exhaustive):
    """the default block and first round, 72 headings, every beam and every tenth"""
    for beam_stride in (1, 10):
        want, st = eng.global_search(scans["inside"], max_hits=16, beam_stride=beam_stride)
        got, ps = eng.global_search_pruned(scans["inside"], max_hits=16, beam_stride=beam_stride)
        print("beam_stride", beam_stride, "pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"])
        assert same_hits(got, want) and ps["guard_fallbacks"] == 0 and ps["used_beams"] == st["used_beams"]


# ---- 2. a map without obstacles: every score is equal, and the strict stop rule scores everything
@pytest.mark.parametrize("nms", [0, 1])
def test_map_without_obstacles(engine_mod, ang, scans, nms):
    e = make_engine(engine_mod, Room(empty=True), ang, 64)
    e.set_likelihood_field(True)
    want, st = e.global_search(scans["inside"], max_hits=16, n_headings=N_HEAD, nms=nms)
    V = e.search_scores()
    assert np.unique(V).size == 1 and np.isfinite(V[0])
    got, ps = e.global_search_pruned(scans["inside"], max_hits=16, first_pairs=FIRST, n_headings=N_HEAD, nms=nms)
    assert ps["pairs_scored"] == ps["pairs"]
    assert same_hits(got, want[:len(got)]) and len(got) == min(16, st["n_hits"])
    U = e.search_bounds()
    assert (U == V[0]).all()
    e.close()


# ---- 3. the bound holds as bits
@pytest.mark.parametrize("scan", ["inside", "off_map", "odd"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_bounds_dominate_every_score(engine_mod, eng, room, scans, exhaustive, block, stride, scan):
    _, _, V = exhaustive(scan, stride, 1)
    _, ps = eng.global_search_pruned(scans[scan], max_hits=1, block=block, first_pairs=FIRST, stride_cells=stride, n_headings=N_HEAD)
    U = eng.search_bounds()
    plan = engine_mod.host_search_blocks(room.data, block=block, stride_cells=stride)
    ref = pr.blocks(room.data, stride, block)
    assert plan["n_blocks"] == ref["n_blocks"] and U.size == ps["pairs"] == N_HEAD * plan["n_blocks"]
    best = np.full((N_HEAD, plan["n_blocks"]), -np.inf)
    np.maximum.at(best, (np.arange(N_HEAD)[:, None].repeat(V.shape[1], 1), ref["block_of_pos"][None, :].repeat(N_HEAD, 0)), V)
    U = U.reshape(N_HEAD, -1)
    assert not np.isnan(U).any()
    assert (U >= best).all()                                    # as doubles, no tolerance
    assert ps["guard_fallbacks"] == 0
    finite = np.isfinite(best)
    print("block", block, "stride", stride, scan, "median slack of U over the block's best score:", np.median(U[finite] - best[finite]))


# ---- 4. pairs scored and rounds are what the schedule gives for the device's own U and the exhaustive volume
@pytest.mark.parametrize("block,nms,stride,max_hits,first,scan", [
    (8, 1, 2, 16, FIRST, "inside"), (4, 1, 2, 16, FIRST, "inside"), (2, 1, 2, 16, FIRST, "inside"), (2, 1, 1, 1, FIRST, "inside"),
    (4, 0, 2, 16, FIRST, "off_map"), (8, 1, 1, 65536, FIRST, "odd"), (2, 0, 1, 16, 3, "odd"), (4, 1, 1, 16, 0, "off_map"),
    (2, 1, 2, 4, 1, "inside"),
])
def test_stats_agree_with_the_schedule(eng, room, scans, exhaustive, block, nms, stride, max_hits, first, scan):
    want, _, V = exhaustive(scan, stride, nms)
    got, ps = eng.global_search_pruned(scans[scan], max_hits=max_hits, block=block, first_pairs=first, stride_cells=stride,
                                       n_headings=N_HEAD, nms=nms)
    r = pr.schedule(eng.search_bounds(), V, room.data, stride, block, nms, max_hits, first)
    print("pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"], "ref", r["pairs_scored"], r["rounds"])
    assert (ps["pairs_scored"], ps["rounds"]) == (r["pairs_scored"], r["rounds"])
    assert np.array_equal(got["index"], r["hits"]) and same_hits(got, want[:len(got)])


# ---- 5. pruning happens
def test_pruning_happens(eng, scans):
    """Asserted for block 2 at stride 2: its window w = 4 cells = 0.2 m is sigma_hit, far below the 1.5 m between this room's walls,
    so a block's bound is near its best score.  The windows of block 4 (0.4 m) and 8 (0.8 m) approach the room's structure; their
    shares are printed, not asserted."""
    shares = {}
    for block in (2, 4, 8):
        _, ps = eng.global_search_pruned(scans["inside"], max_hits=16, block=block, first_pairs=FIRST, n_headings=N_HEAD)
        shares[block] = (ps["pairs_scored"], ps["pairs"], ps["rounds"])
    print("pairs scored, pairs, rounds by block:", shares)
    assert shares[2][0] < shares[2][1]


# ---- 6. nothing else changes
def test_later_behaviour_is_unchanged(engine_mod, room, ang, scans):
    rng = np.random.default_rng(3)
    p = tracking_cloud(rng, 512, TRUE_POSE, (0.2, 0.2, 0.2))
    w = np.full(512, 1.0 / 512)
    out = []
    for prune in (False, True):
        e = make_engine(engine_mod, room, ang, 512, seed=11)
        e.set_likelihood_field(True)
        e.set_particles(p, w)
        e.global_search(scans["inside"], max_hits=16)
        volume = e.search_scores().copy()
        if prune:
            before = e.search_bytes()
            e.global_search_pruned(scans["inside"], max_hits=16, first_pairs=FIRST)
            e.global_search_pruned(scans["odd"], max_hits=4, block=4, stride_cells=1)
            assert e.search_bytes() > before > 0
            assert e.search_scores().tobytes() == volume.tobytes()          # the volume of the earlier search stays
        e.update((0.05, 0.0, 0.01), scans["inside"])
        e.update((0.05, 0.0, 0.01), scans["odd"])
        hits, st = e.global_search(scans["off_map"], max_hits=16)
        out.append((e.get_particles().copy(), e.get_weights().copy(), hits.copy(), st["n_hits"], e.search_scores().copy(), volume))
        e.close()
    a, b = out
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert same_hits(a[2], b[2]) and a[3] == b[3]
    assert a[4].tobytes() == b[4].tobytes() and a[5].tobytes() == b[5].tobytes()


# ---- 7. the opt-in of propose_from_scan
def test_propose_from_scan_pruned(engine_mod, room, ang, scans):
    e = make_engine(engine_mod, room, ang, 64)
    e.set_likelihood_field(True)
    want = e.propose_from_scan(scans["inside"], max_hits=8)
    thr, fac = e.recovery_proposal()
    got = e.propose_from_scan(scans["inside"], max_hits=8, pruned=True)
    thr2, fac2 = e.recovery_proposal()
    assert len(got) == 8 and same_hits(got, want)
    assert np.array_equal(thr, thr2) and fac.tobytes() == fac2.tobytes()
    e.set_likelihood_field(False)
    with pytest.raises(engine_mod.EngineError):
        e.propose_from_scan(scans["inside"], max_hits=8, pruned=True)
    e.close()


# ---- 8. the refusals, and when the bounds can be read
def test_refusals(engine_mod, room, ang, scans):
    e = make_engine(engine_mod, room, ang, 64)
    scan = scans["inside"]
    with pytest.raises(engine_mod.EngineError) as err:                       # the field is off
        e.global_search_pruned(scan)
    assert err.value.status == engine_mod.MCL_ERR_NOT_READY
    e.set_likelihood_field(True)
    with pytest.raises(engine_mod.EngineError) as err:                       # before any call
        e.search_bounds()
    assert err.value.status == engine_mod.MCL_ERR_NOT_READY
    for kw in (dict(max_hits=0), dict(block=3), dict(block=16), dict(block=1), dict(first_pairs=-1), dict(prune_reserved=(0, 0, 1, 0, 0, 0)),
               dict(max_hits=65537), dict(stride_cells=0), dict(nms=2)):
        with pytest.raises(engine_mod.EngineError) as err:
            e.global_search_pruned(scan, **kw)
        assert err.value.status == engine_mod.MCL_ERR_INVALID_ARG, kw
    with pytest.raises(engine_mod.EngineError):
        e.global_search_pruned(scan[:10])
    assert e.search_bytes() == 0                                             # a refused call allocates nothing
    hits, ps = e.global_search_pruned(scan, max_hits=4)
    assert len(hits) == 4 and e.search_bounds().size == ps["pairs"]
    assert e.search_bytes() >= ps["device_bytes"] > 0
    with pytest.raises(engine_mod.EngineError):                              # no volume: the call keeps none
        e.search_scores()
    e.set_map(room.data, room.resolution, room.origin_x, room.origin_y)
    with pytest.raises(engine_mod.EngineError) as err:                       # after mcl_set_map
        e.search_bounds()
    assert err.value.status == engine_mod.MCL_ERR_NOT_READY
    hits2, _ = e.global_search_pruned(scan, max_hits=4)                      # the new map's field is pooled again
    assert same_hits(hits, hits2)
    e.close()
