"""The pruned search over a scan sequence on the GPU (mcl_global_search_sequence_pruned, DESIGN.md §4.21, rules PS1 - PS5 of
include/mcl_hip_engine.h).  The yardstick is mcl_global_search_sequence in the same process: the hits byte for byte; the bounds
against the exhaustive summed volume with no tolerance; that the bound is the stated one (the single search's for one scan, the
in-order fold of the per-scan bounds otherwise); the rounds against tests/search_pruned_ref.py; that two scans still tell the
congruent corridors apart; that an engine which calls it runs the same updates and searches as one that never does; the refusals.
The room is that of tests/test_gpu_search_pruned.py."""
import ctypes as C

import numpy as np
import pytest

import search_pruned_ref as pr
from conftest import make_engine, tracking_cloud
from search_sequence_pruned_ref import bits, fold
from side_geometries import angles, compose, scan_at
from test_gpu_search_sequence import NHEAD5, REL5, STRIDE5, twin_case

pytestmark = pytest.mark.gpu

RES = np.float32(0.05)
OX, OY = -2.4, -1.8
W, H = 97, 71                                   # no multiple of block * stride for any block and stride used here
N_HEAD = 8
FIRST = 24                                      # a small first round, so that calls run several rounds
MAX_RANGE = 12.0


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

# the rel sets: rows of (dx, dy, dtheta), the pose at scan s in the anchor's frame; the last scan is the anchor's
REL = dict(
    a=np.zeros((1, 3)),                                                         # one scan at the anchor
    b=np.array([[-0.33, 0.12, 0.2], [0.0, 0.0, 0.0]]),                          # a rotation, a translation of 6.6 and 2.4 cells
    c=np.array([[8.0, 0.0, 0.0], [-0.21, 0.04, -0.1], [0.0, 0.0, 0.0]]),        # 8 m: off the 4.85 m x 3.55 m map from every pose
    d=np.zeros((3, 3)),                                                         # three identical scans
)


@pytest.fixture(scope="module")
def room():
    return Room()


@pytest.fixture(scope="module")
def ang(orc):
    return angles(orc, 61)


@pytest.fixture(scope="module")
def scans(orc, room, ang):
    """per rel set the scans a robot takes along the path whose pose at the anchor is TRUE_POSE.  Set c: scan 0 is taken from the
    anchor and scored from 8 m away, scan 1 has no usable beam (NaN, max range, a negative reading)"""
    om = orc.OracleMap(room.data, room.resolution, room.origin_x, room.origin_y)
    out = {k: np.stack([scan_at(orc, om, ang, compose(TRUE_POSE, r)) for r in rel]) for k, rel in REL.items()}
    out["c"][0] = out["a"][0]
    out["c"][1] = np.nan
    out["c"][1, 5], out["c"][1, 9] = MAX_RANGE, -1.0
    assert np.array_equal(out["d"][0], out["d"][2]) and np.array_equal(out["d"][0], out["a"][0])
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def eng(engine_mod, room, ang):
    e = make_engine(engine_mod, room, ang, 64)
    e.set_likelihood_field(True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def exhaustive(eng, scans):
    """mcl_global_search_sequence once per (rel set, stride, nms): its hits with the largest max_hits, its stats, its volume"""
    memo = {}

    def get(case, stride, nms):
        key = (case, stride, nms)
        if key not in memo:
            hits, st = eng.global_search_sequence(scans[case], REL[case], max_hits=65536, stride_cells=stride, n_headings=N_HEAD, nms=nms)
            V = eng.search_scores().reshape(N_HEAD, -1)
            V.setflags(write=False)
            memo[key] = (hits.copy(), st, V)
        return memo[key]
    return get


def same_hits(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


def pruned(e, scans, case, **kw):
    kw.setdefault("n_headings", N_HEAD)
    kw.setdefault("first_pairs", FIRST)
    return e.global_search_sequence_pruned(scans[case], REL[case], **kw)


# ---- 1. the hits are mcl_global_search_sequence's, byte for byte
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("max_hits", [1, 16, 65536])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("nms", [0, 1])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_hits_identical(eng, scans, exhaustive, block, nms, stride, max_hits, case):
    want, st, V = exhaustive(case, stride, nms)
    assert st["n_hits"] < 65536 and st["n_poses"] == V.size                 # 65536 is more than there are candidates
    got, ps = pruned(eng, scans, case, max_hits=max_hits, block=block, stride_cells=stride, nms=nms)
    print("pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"])
    assert ps["n_hits"] == len(got) == min(max_hits, st["n_hits"])
    assert same_hits(got, want[:len(got)])
    assert ps["guard_fallbacks"] == 0
    assert (ps["n_positions"], ps["n_poses"], ps["used_beams"], ps["n_scans"]) == (st["n_positions"], st["n_poses"], st["used_beams"], st["n_scans"])
    assert ps["n_scans"] == len(REL[case])
    assert 1 <= ps["pairs_scored"] <= ps["pairs"] and ps["rounds"] >= 1


def test_the_odd_scans_are_what_they_should_be(engine_mod, eng, scans, exhaustive):
    """set c: scan 1 contributes no beam, and scan 0's pose is off the map from every lattice pose"""
    _, st, _ = exhaustive("c", 2, 1)
    _, one = eng.global_search_sequence(scans["c"][1:2], REL["c"][1:2], max_hits=0, n_headings=N_HEAD)
    assert one["used_beams"] == 0 and st["used_beams"] > 61
    off = engine_mod.host_search_sequence_offsets(REL["c"], n_headings=N_HEAD)
    assert (np.hypot(off[:, 0, 0], off[:, 0, 1]) > np.hypot(W, H) * float(RES)).all()       # further than the map's diagonal


# ---- 2. the bound holds as bits
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_bounds_dominate_every_summed_score(engine_mod, eng, room, scans, exhaustive, block, stride, case):
    _, _, V = exhaustive(case, stride, 1)
    _, ps = pruned(eng, scans, case, max_hits=1, block=block, stride_cells=stride)
    U = eng.search_bounds()
    plan = engine_mod.host_search_blocks(room.data, block=block, stride_cells=stride)
    ref = pr.blocks(room.data, stride, block)
    assert plan["n_blocks"] == ref["n_blocks"] and U.size == ps["pairs"] == N_HEAD * plan["n_blocks"]
    assert np.array_equal(plan["blocks"], ref["blocks"])
    best = np.full((N_HEAD, plan["n_blocks"]), -np.inf)
    np.maximum.at(best, (np.arange(N_HEAD)[:, None].repeat(V.shape[1], 1), ref["block_of_pos"][None, :].repeat(N_HEAD, 0)), V)
    U = U.reshape(N_HEAD, -1)
    assert not np.isnan(U).any()
    assert (U >= best).all()                                    # as doubles, no tolerance
    assert ps["guard_fallbacks"] == 0
    finite = np.isfinite(best)
    print("block", block, "stride", stride, case, "median slack of U over the block's best summed score:", np.median(U[finite] - best[finite]))


def test_bounds_dominate_with_a_table_that_ends_in_minus_infinity(engine_mod, room, ang, scans):
    """z_rand = 0 and a narrow sigma: far from an obstacle and off the map a beam's term is -inf, so summed scores and bounds are
    -inf for many blocks (most of all where a scan is scored from 8 m away); the comparison includes them"""
    e = make_engine(engine_mod, room, ang, 64)
    e.set_likelihood_field(True, z_rand=0.0, sigma_hit_m=0.05)
    ref = pr.blocks(room.data, 2, 4)
    minus_inf = finite = False
    for case in ("b", "c"):
        want, st = e.global_search_sequence(scans[case], REL[case], max_hits=16, n_headings=N_HEAD)
        V = e.search_scores().reshape(N_HEAD, -1)
        got, ps = pruned(e, scans, case, max_hits=16, block=4)
        U = e.search_bounds().reshape(N_HEAD, -1)
        best = np.full(U.shape, -np.inf)
        np.maximum.at(best, (np.arange(N_HEAD)[:, None].repeat(V.shape[1], 1), ref["block_of_pos"][None, :].repeat(N_HEAD, 0)), V)
        assert not np.isnan(U).any() and not np.isnan(V).any()
        assert (U >= best).all()
        assert same_hits(got, want[:len(got)]) and len(got) == min(16, st["n_hits"])
        minus_inf, finite = minus_inf or bool(np.isneginf(U).any()), finite or bool(np.isfinite(U).any())
        print(case, "bounds of -inf:", int(np.isneginf(U).sum()), "of", U.size, "hits", len(got))
    assert minus_inf and finite
    e.close()


# ---- 3. the bound is the stated one, not a looser one
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_one_scan_at_the_anchor_is_the_single_pruned_search(eng, scans, block, stride):
    """(i) PS5: hits, U and stats[0 .. 8) are mcl_global_search_pruned's"""
    kw = dict(max_hits=16, block=block, first_pairs=FIRST, stride_cells=stride, n_headings=N_HEAD)
    h1, s1 = eng.global_search_pruned(scans["a"][0], **kw)
    U1 = eng.search_bounds()
    h2, s2 = eng.global_search_sequence_pruned(scans["a"], REL["a"], **kw)
    U2 = eng.search_bounds()
    h3, s3 = eng.global_search_pruned(scans["a"][0], **kw)
    U3 = eng.search_bounds()
    assert np.array_equal(bits(U1), bits(U2)) and np.array_equal(bits(U1), bits(U3))
    assert same_hits(h1, h2) and same_hits(h1, h3) and len(h1) == 16
    assert s2.pop("n_scans") == 1
    assert s1 == s2 == s3                                       # the eight, device_bytes included: no buffer of the pruned search grew


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_bound_of_two_scans_is_the_fold_of_the_scans_bounds(eng, scans, block, stride):
    """(ii) PS3: U = (0.0 + Ua) + Ub, Ua and Ub from one-scan calls with their own rel rows"""
    kw = dict(max_hits=1, block=block, stride_cells=stride)
    parts = []
    for s in range(2):
        e_scans, e_rel = scans["b"][s:s + 1], REL["b"][s:s + 1]
        eng.global_search_sequence_pruned(e_scans, e_rel, n_headings=N_HEAD, first_pairs=FIRST, **kw)
        parts.append(eng.search_bounds())
    pruned(eng, scans, "b", **kw)
    U = eng.search_bounds()
    assert np.array_equal(bits(U), bits((0.0 + parts[0]) + parts[1]))
    assert np.array_equal(bits(U), bits(fold(parts)))
    assert not np.array_equal(bits(parts[0]), bits(parts[1]))   # (two different scans from two different places)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("block", [2, 4, 8])
def test_bound_of_three_identical_scans_is_the_threefold_sum(eng, scans, block, stride):
    """(iii) PS3: U = ((0.0 + U1) + U1) + U1, U1 the single scan's bound"""
    kw = dict(max_hits=1, block=block, stride_cells=stride)
    pruned(eng, scans, "a", **kw)
    U1 = eng.search_bounds()
    pruned(eng, scans, "d", **kw)
    U = eng.search_bounds()
    assert np.array_equal(bits(U), bits(fold([U1, U1, U1])))


# ---- 4. pairs scored and rounds are what the schedule gives for the device's own U and the exhaustive summed volume
@pytest.mark.parametrize("block,nms,stride,max_hits,first,case", [
    (8, 1, 2, 16, FIRST, "b"), (4, 1, 2, 16, FIRST, "b"), (2, 1, 2, 16, FIRST, "b"), (2, 1, 1, 1, FIRST, "a"),
    (4, 0, 2, 16, FIRST, "c"), (8, 1, 1, 65536, FIRST, "c"), (2, 0, 1, 16, 3, "d"), (4, 1, 1, 16, 0, "b"),
    (2, 1, 2, 4, 1, "d"),
])
def test_stats_agree_with_the_schedule(eng, room, scans, exhaustive, block, nms, stride, max_hits, first, case):
    want, _, V = exhaustive(case, stride, nms)
    got, ps = pruned(eng, scans, case, max_hits=max_hits, block=block, first_pairs=first, stride_cells=stride, nms=nms)
    r = pr.schedule(eng.search_bounds(), V, room.data, stride, block, nms, max_hits, first)
    print("pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"], "ref", r["pairs_scored"], r["rounds"])
    assert (ps["pairs_scored"], ps["rounds"]) == (r["pairs_scored"], r["rounds"])
    assert np.array_equal(got["index"], r["hits"]) and same_hits(got, want[:len(got)])


# ---- 5. a map without obstacles: every summed score is equal, and the strict stop rule scores everything
@pytest.mark.parametrize("nms", [0, 1])
def test_map_without_obstacles(engine_mod, ang, scans, nms):
    e = make_engine(engine_mod, Room(empty=True), ang, 64)
    e.set_likelihood_field(True)
    want, st = e.global_search_sequence(scans["b"], REL["b"], max_hits=16, n_headings=N_HEAD, nms=nms)
    V = e.search_scores()
    assert np.unique(V).size == 1 and np.isfinite(V[0])
    got, ps = pruned(e, scans, "b", max_hits=16, nms=nms)
    assert ps["pairs_scored"] == ps["pairs"]
    assert same_hits(got, want[:len(got)]) and len(got) == min(16, st["n_hits"])
    U = e.search_bounds()
    assert (U == V[0]).all()
    e.close()


# ---- 6. the congruent corridors
def test_two_scans_resolve_congruent_corridors_pruned(engine_mod, orc):
    m, ang5, scans5, i_true, i_twin, n_pos = twin_case(engine_mod, orc)
    e = make_engine(engine_mod, m, ang5, 64)
    e.set_likelihood_field(True)
    fields = dict(stride_cells=STRIDE5, n_headings=NHEAD5)
    want, st = e.global_search_sequence(scans5, REL5, max_hits=64, **fields)
    assert want["index"][0] == i_true                                        # the right corridor
    for block in (2, 4, 8):
        got, ps = e.global_search_sequence_pruned(scans5, REL5, max_hits=64, block=block, first_pairs=FIRST, **fields)
        print("block", block, "pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"])
        assert got["index"][0] == i_true and same_hits(got, want[:len(got)]) and len(got) == min(64, st["n_hits"])
        assert ps["n_scans"] == 2 and ps["n_positions"] == n_pos and ps["guard_fallbacks"] == 0
    got, ps = e.global_search_sequence_pruned(scans5, REL5, max_hits=1, block=2, first_pairs=FIRST, **fields)
    print("one hit, block 2: pairs scored", ps["pairs_scored"], "of", ps["pairs"], "rounds", ps["rounds"])
    assert got["index"][0] == i_true and same_hits(got, want[:1])
    assert ps["pairs_scored"] < ps["pairs"]                                  # pruning happens on this input
    e.close()


# ---- 7. nothing else changes
def test_later_behaviour_is_unchanged(engine_mod, room, ang, scans):
    rng = np.random.default_rng(3)
    p = tracking_cloud(rng, 512, TRUE_POSE, (0.2, 0.2, 0.2))
    w = np.full(512, 1.0 / 512)
    out = []
    for prune in (False, True):
        e = make_engine(engine_mod, room, ang, 512, seed=11)
        e.set_likelihood_field(True)
        e.set_particles(p, w)
        for t, case in enumerate(("b", "c", "d")):
            if prune:
                pruned(e, scans, case, max_hits=16, block=(8, 4, 2)[t], stride_cells=1 + t % 2)
            e.update((0.05, 0.0, 0.01), scans[case][-1])
        out.append((e.get_particles().copy(), e.get_weights().copy()))
        e.close()
    a, b = out
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_the_other_searches_are_left_alone(eng, scans):
    # the volume of an earlier sequence search stays
    eng.global_search_sequence(scans["b"], REL["b"], max_hits=4, n_headings=N_HEAD)
    volume = eng.search_scores().copy()
    # what the single pruned search returns before ...
    kw = dict(max_hits=16, block=4, first_pairs=FIRST, n_headings=N_HEAD)
    h1, s1 = eng.global_search_pruned(scans["a"][0], **kw)
    U1 = eng.search_bounds().copy()
    pruned(eng, scans, "c", max_hits=16, block=4)
    pruned(eng, scans, "b", max_hits=3, block=2, stride_cells=1)
    assert eng.search_scores().tobytes() == volume.tobytes()
    assert eng.search_bounds().size > U1.size                   # (the bounds are now the sequence call's: smaller blocks, a finer lattice)
    # ... and after
    h2, s2 = eng.global_search_pruned(scans["a"][0], **kw)
    assert same_hits(h1, h2) and np.array_equal(bits(eng.search_bounds()), bits(U1))
    s1.pop("device_bytes"), s2.pop("device_bytes")              # (block 2 at stride 1 in between: its tables asked for more)
    assert s1 == s2
    assert eng.search_scores().tobytes() == volume.tobytes()


# ---- 8. the refusals
def expect(engine_mod, status, fn, *args, **kw):
    with pytest.raises(engine_mod.EngineError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    return str(ei.value)


def test_refusals(engine_mod, room, ang, scans):
    INVALID, NOT_READY, UNSUPPORTED = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY, -5     # (MCL_ERR_UNSUPPORTED)
    sc, rel = scans["b"], REL["b"]
    want = None

    def valid(e):
        """after a refusal a valid call still gives the right hits"""
        got, ps = e.global_search_sequence_pruned(sc, rel, max_hits=4, n_headings=N_HEAD)
        assert same_hits(got, want) and ps["n_scans"] == 2

    # not ready: no map, no beams, the field off -- the message says which
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.global_search_sequence_pruned, sc, rel)
    e.set_map(room.data, room.resolution, room.origin_x, room.origin_y)
    assert "beam" in expect(engine_mod, NOT_READY, e.global_search_sequence_pruned, sc, rel)
    e.set_beam_angles(ang)
    assert "likelihood-field" in expect(engine_mod, NOT_READY, e.global_search_sequence_pruned, sc, rel)
    e.set_likelihood_field(True)
    expect(engine_mod, NOT_READY, e.search_bounds)                           # before any call

    def raw(scans_p, rel_p, S, n_beams=61, max_hits=1, hits_p=True, n_p=True):
        n, cfg, pc = C.c_int64(), engine_mod.default_search_config(n_headings=N_HEAD), engine_mod.search_prune_config()
        hits = np.zeros(max(max_hits, 1), engine_mod.SEARCH_HIT_DTYPE)
        rc = e.lib.mcl_global_search_sequence_pruned(e._h, C.byref(cfg), C.byref(pc), scans_p, rel_p, S, n_beams, max_hits,
                                                     hits.ctypes.data_as(C.c_void_p) if hits_p else None, C.byref(n) if n_p else None, None)
        return rc, e.lib.mcl_last_error(e._h).decode()

    s2, r2 = np.ascontiguousarray(sc), np.ascontiguousarray(rel)
    sp, rp = s2.ctypes.data_as(C.c_void_p), r2.ctypes.data_as(C.c_void_p)
    # the sequence's own: the number of scans, null scans or rel, a rel that is not finite, n_beams
    for S in (0, -1, engine_mod.MAX_SEARCH_SCANS + 1):
        rc, why = raw(sp, rp, S)
        assert rc == INVALID and "n_scans" in why
    many = np.full((engine_mod.MAX_SEARCH_SCANS + 1, 61), 1.0, np.float32)
    assert "n_scans" in expect(engine_mod, INVALID, e.global_search_sequence_pruned, many, np.zeros((len(many), 3)))
    rc, why = raw(None, rp, 2)
    assert rc == INVALID and "scans is null" in why
    rc, why = raw(sp, None, 2)
    assert rc == INVALID and "rel is null" in why
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            r = rel.copy()
            r[0, col] = bad
            assert "not finite" in expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc, r)
    assert "n_beams" in expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc[:, :60], rel)
    # the pruned search's own
    for kw in (dict(max_hits=0), dict(block=3), dict(block=16), dict(block=1), dict(first_pairs=-1), dict(prune_reserved=(0, 0, 1, 0, 0, 0)),
               dict(max_hits=65537), dict(stride_cells=0), dict(n_headings=0), dict(beam_stride=0), dict(nms=2), dict(reserved=(0, 0, 0, 1))):
        expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc, rel, **kw)
    rc, why = raw(sp, rp, 2, hits_p=False)
    assert rc == INVALID and "hits is null" in why
    rc, why = raw(sp, rp, 2, n_p=False)
    assert rc == INVALID
    assert e.search_bytes() == 0                                             # a refused call allocates nothing
    expect(engine_mod, NOT_READY, e.search_bounds)                           # ... and leaves no bounds
    # the Python layer
    with pytest.raises(ValueError):
        e.global_search_sequence_pruned(sc, np.zeros((3, 3)))
    with pytest.raises(ValueError):
        e.global_search_sequence_pruned(sc[0], rel)
    # a valid call; null config, prune config and stats are the defaults
    want, st = e.global_search_sequence(sc, rel, max_hits=4, n_headings=N_HEAD)
    want = want.copy()
    valid(e)
    assert e.search_bounds().size > 0
    n, hits = C.c_int64(), np.zeros(4, engine_mod.SEARCH_HIT_DTYPE)
    assert e.lib.mcl_global_search_sequence_pruned(e._h, None, None, sp, rp, 2, 61, 4, hits.ctypes.data_as(C.c_void_p), C.byref(n), None) == engine_mod.MCL_OK
    d, _ = e.global_search_sequence(sc, rel, max_hits=4)
    assert n.value == 4 and same_hits(hits, d)
    for kw in (dict(max_hits=0), dict(block=3)):
        expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc, rel, **kw)
        valid(e)
    r = rel.copy()
    r[1, 2] = np.nan
    expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc, r)
    valid(e)
    # pairs * S * S >= 2^31 with fewer than 2^27 poses: one free cell per 8 x 8 block, so a pair holds one pose in its 64 slots
    sparse = np.full((H, W), 100, np.int8)
    sparse[::8, ::8] = 0
    n_free = int((sparse == 0).sum())
    n_head = (1 << 31) // (n_free * 64) + 1
    assert n_free * n_head < 1 << 27
    e.set_map(sparse, room.resolution, room.origin_x, room.origin_y)
    expect(engine_mod, NOT_READY, e.search_bounds)                           # after mcl_set_map
    assert "2^31" in expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc, rel, stride_cells=1, n_headings=n_head, block=8)
    assert "2^27" in expect(engine_mod, INVALID, e.global_search_sequence_pruned, sc, rel, stride_cells=1, n_headings=(1 << 27) // n_free + 1)
    # a lattice without a free position
    full = np.full((H, W), 100, np.int8)
    e.set_map(full, room.resolution, room.origin_x, room.origin_y)
    assert "position" in expect(engine_mod, NOT_READY, e.global_search_sequence_pruned, sc, rel)
    e.set_map(room.data, room.resolution, room.origin_x, room.origin_y)
    valid(e)                                                                 # the new map's field is pooled again
    e.set_likelihood_field(False)
    expect(engine_mod, NOT_READY, e.global_search_sequence_pruned, sc, rel)
    e.close()
    # an engine of a device group
    g = engine_mod.Group([0], max_particles=1024)
    g.set_map(room.data, room.resolution, room.origin_x, room.origin_y)
    g.set_beam_angles(ang)
    assert "single-engine" in expect(engine_mod, UNSUPPORTED, g.engine(0).global_search_sequence_pruned, sc, rel)
    g.close()
