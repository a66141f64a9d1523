"""The global search over a scan sequence on the GPU (mcl_global_search_sequence, DESIGN.md §4.15, rules SQ1-SQ7 of
include/mcl_hip_engine.h): the summed volume against mcl_score_poses bit for bit and against the numpy statement
tests/lfield_ref.py; the hits against the numpy restatement of S5; the identity with mcl_global_search for one scan at the anchor;
that two scans tell apart two places one scan cannot; that an engine which searches runs the same updates, bit for bit, as one that
never does; the refusals.  The map, the scans and the helpers are those of tests/test_gpu_global_search.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lfield_ref as lr
from conftest import tracking_cloud
from side_geometries import compose, masked, scan_poses
from test_gpu_global_search import (H, MAX_RANGE, OX, OY, RES, TRUE_POSE, W, SmallMap, angles, bits, expect, hits_ref, lattice, lf_engine,
                                    odd_scan, scan_at, score_all, small, small_oracle)  # noqa: F401  (small, small_oracle: fixtures)

pytestmark = pytest.mark.gpu


def fold(accs):
    """SQ4: ((+0.0 + acc_0) + acc_1) + ... in scan order"""
    total = np.zeros_like(accs[0])
    for a in accs:
        total = total + a
    return total


REL3 = np.array([[-0.5, 0.0, 0.0], [0.2, -0.1, 0.3], [0.0, 0.0, 0.0]])
REL2 = np.array([[-0.35, 0.1, 0.2], [0.0, 0.0, 0.0]])
REL_OFF = np.array([[-1.0, 0.5, 0.1], [0.0, 0.0, 0.0]])          # scan 0 from a metre behind: off the map for poses near its edges


def scans_for(orc, om, ang, rel, at=TRUE_POSE):
    """the scans a robot would take whose pose at the anchor is `at`"""
    return np.stack([scan_at(orc, om, ang, compose(at, r)) for r in rel])


# ---- 1. the summed volume is mcl_score_poses, bit for bit
@pytest.mark.parametrize("stride,n_head,B,beam_stride,lf_fields,rel,special", [
    (2, 5, 61, 1, {}, REL3, "odd"),                  # one scan without a usable beam, one with the odd readings
    (3, 1, 61, 1, {}, REL_OFF, "off"),               # the position count is no multiple of 64 and over 256; scan poses off the map
    (2, 5, 1, 1, {}, REL2, None),
    (2, 5, 61, 3, {}, REL2, None),
    (3, 1, 61, 1, dict(max_occ_dist_m=4.6), REL2, None),          # K = 8464 >= 8192: the table is read from global memory
    (2, 5, 61, 1, dict(z_rand=0.0, sigma_hit_m=0.05), REL_OFF, "inf"),   # a table that ends in -inf: off the map is -inf
])
def test_volume_is_the_sum_of_score_poses(engine_mod, orc, small, small_oracle, stride, n_head, B, beam_stride, lf_fields, rel, special):
    ang = angles(orc, B)
    e = lf_engine(engine_mod, small, ang, **lf_fields)
    K = e.likelihood_table().size - 1
    assert (K >= 8192) == ("max_occ_dist_m" in lf_fields)
    # (the -inf table: the scans of a robot ON the lattice, so that at least its pose keeps every end point on the map)
    at = (TRUE_POSE[0], TRUE_POSE[1], engine_mod.host_search_headings(n_headings=n_head)[3]) if special == "inf" else TRUE_POSE
    scans = scans_for(orc, small_oracle, ang, rel, at)
    if special == "inf":
        scans[scans > 2.0] = np.nan                      # (... the beams that leave through the wall's gaps dropped with the long ones)
    if special == "odd":
        scans[0] = odd_scan(scans[0])
        scans[1] = np.nan
        scans[1, 5], scans[1, 9] = MAX_RANGE, -1.0
    S = len(rel)
    poses = scan_poses(engine_mod, small, rel, stride, n_head)
    n_pos = poses.shape[1] // n_head
    if stride == 3:
        assert n_pos % 64 != 0 and n_pos > 256
    _, st = e.global_search_sequence(scans, rel, max_hits=0, stride_cells=stride, n_headings=n_head, beam_stride=beam_stride)
    assert st["n_scans"] == S and st["n_positions"] == n_pos and st["n_poses"] == poses.shape[1]
    used = [lr.used_beams(ang, masked(scans[s], beam_stride), MAX_RANGE)[0].size for s in range(S)]
    assert st["used_beams"] == sum(used)
    if special == "odd":
        assert used[1] == 0 and used[0] > 0 and used[2] > 0
    if special in ("off", "inf"):
        x, y = poses[0, :, 0], poses[0, :, 1]
        out = (x < OX) | (x >= OX + W * float(RES)) | (y < OY) | (y >= OY + H * float(RES))
        assert 0 < out.sum() < out.size
    got = e.search_scores()
    want = fold([score_all(e, poses[s], masked(scans[s], beam_stride)) for s in range(S)])
    assert got.shape == want.shape
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    if special == "inf":
        assert np.isneginf(got).any() and np.isfinite(got).any()
    else:
        assert np.isfinite(got).all()
    if B > 1:
        assert np.unique(got).size > 100                   # (a volume, not a constant)


# ---- 2. the summed volume against the independent statement
def perturbed(scans):
    """the ranges moved by about a millimetre (fixed seed): end points off the cell edges"""
    return (scans + np.random.default_rng(7).uniform(0.0005, 0.0015, scans.shape).astype(np.float32)).astype(np.float32)


def restatement(m, poses, ang, scans, **lf_fields):
    """per scan (log-weights, alternatives, ambiguous beams) of tests/lfield_ref.py at the poses of SQ2"""
    D, Lf = lr.field(m.data, m.resolution), lr.table(m.resolution, **lf_fields)
    return [lr.log_weights(np.ascontiguousarray(poses[s].T), ang, scans[s], D, Lf, m.resolution, m.origin_x, m.origin_y, MAX_RANGE)
            for s in range(len(scans))]


def test_volume_is_the_restatement(engine_mod, orc, small, small_oracle):
    ang = angles(orc, 61)
    scans = perturbed(scans_for(orc, small_oracle, ang, REL2))
    poses = scan_poses(engine_mod, small, REL2, 2, 5)
    ref = restatement(small, poses, ang, scans)
    # the cap of the single-scan test, confirmed on the CPU statement alone before the device is held to it: ambiguous beams at most
    # 1e-5 of all beams, or 2 beams where that is fewer than one
    beams = poses.shape[1] * sum(lr.used_beams(ang, s, MAX_RANGE)[0].size for s in scans)
    n_amb = sum(int(r[2].sum()) for r in ref)
    assert beams > 0 and n_amb <= max(1e-5 * beams, 2), (n_amb, beams)
    want = fold([r[0] for r in ref])
    e = lf_engine(engine_mod, small, ang)
    e.global_search_sequence(scans, REL2, max_hits=0, stride_cells=2, n_headings=5)
    got = e.search_scores()
    assert got.shape == want.shape
    for i in np.flatnonzero(bits(got) != bits(want)):
        i = int(i)
        assert any(i in r[1] for r in ref), (i, got[i], want[i])
        sums = {float(fold([np.float64(v) for v in pick])) for pick in itertools.product(*[r[1].get(i, [r[0][i]]) for r in ref])}
        assert got[i] in sums, (i, got[i], want[i], sorted(sums))


# ---- 3. the hits are S5 on the summed volume
@pytest.mark.parametrize("stride,n_head", [(2, 5), (3, 2)])
@pytest.mark.parametrize("nms", [0, 1])
def test_hits_are_s5(engine_mod, orc, small, small_oracle, stride, n_head, nms):
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    scans = scans_for(orc, small_oracle, ang, REL2)
    cells, xy, theta, _ = lattice(engine_mod, small, stride, n_head)
    counts = set()
    for max_hits in (0, 1, 65536):
        hits, st = e.global_search_sequence(scans, REL2, max_hits=max_hits, stride_cells=stride, n_headings=n_head, nms=nms)
        V = e.search_scores(n_head)
        want = hits_ref(V, cells, stride, nms)
        assert 5 < want.size < 65536 and st["n_hits"] == want.size           # (65536 is more than there are)
        m = min(max_hits, want.size)
        assert len(hits) == m
        assert np.array_equal(hits["index"], want[:m])
        k, p = want[:m] // cells.size, want[:m] % cells.size
        assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
        assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p]))        # the lattice pose: the anchor
        assert np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
        counts.add(st["n_hits"])
    assert len(counts) == 1
    if nms == 0:
        assert counts == {V.size}


# ---- 4. SQ7: one scan at the anchor is mcl_global_search
@pytest.mark.parametrize("stride,n_head,beam_stride", [(2, 5, 1), (3, 2, 3), (2, 72, 1)])
def test_one_scan_at_the_anchor_is_the_single_search(engine_mod, orc, small, small_oracle, stride, n_head, beam_stride):
    ang = angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    obs = odd_scan(scan_at(orc, small_oracle, ang, TRUE_POSE))
    fields = dict(stride_cells=stride, n_headings=n_head, beam_stride=beam_stride)
    h1, st1 = e.global_search(obs, max_hits=4096, **fields)
    v1 = e.search_scores()
    h2, st2 = e.global_search_sequence(obs[None], np.zeros((1, 3)), max_hits=4096, **fields)
    v2 = e.search_scores()
    assert np.array_equal(bits(v1), bits(v2))
    assert h1.tobytes() == h2.tobytes() and len(h1) > 0
    assert st2.pop("n_scans") == 1
    st1.pop("device_bytes"), st2.pop("device_bytes")        # (the sequence search has two small buffers more)
    assert st1 == st2


# ---- 5. two scans tell apart what one cannot
STRIDE5, NHEAD5, K0 = 2, 8, 4                               # theta_4 of 8 headings is exactly 0
SHIFT = 40                                                  # rows from corridor A to corridor B: 20 lattice steps


def twin_map():
    """120 x 90 cells.  Two congruent dead-end corridors, 6 cells wide and 50 long, closed at their right end and open to one room
    at their left: A (rows 20-25) and B = A moved down by SHIFT rows.  The room differs around the mouths: a block faces A's,
    nothing faces B's; the outer wall is 19 rows from A's upper side and 22 from B's lower."""
    g = np.zeros((H, W), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    for r0 in (20, 20 + SHIFT):
        g[r0 - 1, 60:112] = 100
        g[r0 + 6, 60:112] = 100
        g[r0 - 1:r0 + 7, 111] = 100
    g[12:34, 36:40] = 100                                   # the block in front of A's mouth
    g[75:80, 20:30] = 100                                   # something else, below B's
    return SmallMap(g)


def exact_scan(m, ang, pose, step=0.02):
    """ranges to the first occupied cell along each beam, marched in steps of `step` cells and so exact to a millimetre: the
    oracle's cast, quantised to whole steps of the map's resolution as the reference's is, makes a pose two cells off fit a scan
    slightly better than the pose it was taken at; with this one the truth is a local maximum.  The end point lies just inside
    the occupied cell, off every cell edge."""
    res = float(m.resolution)
    a = float(pose[2]) + ang.astype(np.float64)
    px, py, dx, dy = (pose[0] - m.origin_x) / res, (pose[1] - m.origin_y) / res, np.cos(a), np.sin(a)
    r = np.full(a.size, MAX_RANGE, np.float64)
    alive = np.ones(a.size, bool)
    for i in range(int(np.hypot(W, H) / step) + 1):
        t = i * step + 0.007
        cx, cy = np.floor(px + t * dx).astype(int), np.floor(py + t * dy).astype(int)
        inside = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H)
        hit = alive & inside & (m.data[np.where(inside, cy, 0), np.where(inside, cx, 0)] > 50)
        r[hit] = t * res
        alive &= inside & ~hit
        if not alive.any():
            break
    return r.astype(np.float32)


def cell_pose(col, row, theta=0.0):
    return (OX + (col + 0.5) * float(RES), OY + (row + 0.5) * float(RES), theta)


TRUTH_CELL, EARLIER_COL = (101, 23 + SHIFT), 49             # deep in B facing its dead end; earlier: outside B's mouth (col 60)
TWIN_CELL = (101, 23)
REL5 = np.array([[(EARLIER_COL - TRUTH_CELL[0]) * 0.05, 0.0, 0.0], [0.0, 0.0, 0.0]])


def twin_case(engine_mod, orc):
    """(map, angles, scans, index of the truth, index of the twin, n_pos)"""
    m = twin_map()
    ang = angles(orc, 61)
    truth = cell_pose(*TRUTH_CELL)
    scans = np.stack([exact_scan(m, ang, cell_pose(EARLIER_COL, TRUTH_CELL[1])), exact_scan(m, ang, truth)])
    cells, xy, theta, _ = lattice(engine_mod, m, STRIDE5, NHEAD5)
    assert theta[K0] == 0.0
    p_true = int(np.flatnonzero(cells == TRUTH_CELL[1] * W + TRUTH_CELL[0])[0])
    p_twin = int(np.flatnonzero(cells == TWIN_CELL[1] * W + TWIN_CELL[0])[0])
    assert p_true > p_twin                                   # a tie broken by index would pick the twin
    return m, ang, scans, K0 * cells.size + p_true, K0 * cells.size + p_twin, cells.size


def test_two_scans_resolve_congruent_corridors(engine_mod, orc):
    m, ang, scans, i_true, i_twin, n_pos = twin_case(engine_mod, orc)
    # the statement on the CPU first: one scan cannot tell the corridors apart, two can, and nothing beats the truth
    poses = scan_poses(engine_mod, m, REL5, STRIDE5, NHEAD5)
    ref = restatement(m, poses, ang, scans)
    assert all(not r[1] for r in ref)                                        # (no end point near a cell edge: the statement is unique)
    ref_one, ref_seq = ref[1][0], fold([r[0] for r in ref])
    margin_one, margin_seq = ref_one[i_true] - ref_one[i_twin], ref_seq[i_true] - ref_seq[i_twin]
    assert abs(margin_one) < margin_seq and margin_seq > 0
    assert int(np.argmax(ref_seq)) == i_true and np.sum(ref_seq == ref_seq[i_true]) == 1
    # the device
    e = lf_engine(engine_mod, m, ang)
    fields = dict(stride_cells=STRIDE5, n_headings=NHEAD5)
    one, st1 = e.global_search(scans[1], max_hits=64, **fields)
    assert i_true in one["index"] and i_twin in one["index"]
    ll = dict(zip(one["index"].tolist(), one["log_likelihood"].tolist()))
    assert ll[i_true] - ll[i_twin] == margin_one
    seq, st2 = e.global_search_sequence(scans, REL5, max_hits=64, **fields)
    assert st2["n_scans"] == 2 and st2["n_positions"] == n_pos
    assert seq["index"][0] == i_true
    assert np.array_equal(bits(seq["pose"][0]), bits(np.array([poses[1, i_true, 0], poses[1, i_true, 1], 0.0])))
    V = e.search_scores()
    assert V[i_true] - V[i_twin] == margin_seq
    assert abs(ll[i_true] - ll[i_twin]) < V[i_true] - V[i_twin]
    if i_twin in seq["index"]:
        assert list(seq["index"]).index(i_twin) > 0


# ---- 6. read-only
def test_sequence_search_leaves_the_updates_alone(engine_mod, orc, small, small_oracle):
    ang = angles(orc, 61)
    n = 2000
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=TRUE_POSE, sig=(0.2, 0.2, 0.2))
    scans = [scan_at(orc, small_oracle, ang, (TRUE_POSE[0] + 0.05 * t, TRUE_POSE[1], TRUE_POSE[2])) for t in range(1, 4)]
    a, b = lf_engine(engine_mod, small, ang, n), lf_engine(engine_mod, small, ang, n)
    assert a.search_bytes() == 0 and b.search_bytes() == 0
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    b.global_search_sequence(scans[:1], np.zeros((1, 3)), max_hits=4)
    grown = b.search_bytes()
    assert grown > 0
    for t, scan in enumerate(scans):
        for e in (a, b):
            e.update((0.05, 0.0, 0.0), scan)
        rel = engine_mod.relative_poses([(0.05 * u, 0.0, 0.0) for u in range(t + 1)])
        hits, st = b.global_search_sequence(scans[:t + 1], rel, max_hits=4, stride_cells=2 + t % 2, n_headings=8)
        assert st["n_scans"] == t + 1 and st["device_bytes"] == b.search_bytes() >= grown
    assert b.search_bytes() > grown                                            # (more scans, more headings: the buffers grew)
    assert a.search_bytes() == 0
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))


# ---- 7. the refusals
def test_refusals(engine_mod, orc, small):
    INVALID, NOT_READY = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY
    ang = angles(orc, 61)
    scans, rel = np.full((2, 61), 1.0, np.float32), np.zeros((2, 3))
    # not ready: no map, no beams, the field off -- the message says which
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.global_search_sequence, scans, rel)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    assert "beam" in expect(engine_mod, NOT_READY, e.global_search_sequence, scans, rel)
    e.set_beam_angles(ang)
    assert "likelihood-field" in expect(engine_mod, NOT_READY, e.global_search_sequence, scans, rel)
    e.set_likelihood_field(True)
    assert e.search_bytes() == 0

    def raw(scans_p, rel_p, S, n_beams=61, max_hits=0, hits_p=None):
        n, cfg = C.c_int64(), engine_mod.default_search_config()
        rc = e.lib.mcl_global_search_sequence(e._h, C.byref(cfg), scans_p, rel_p, S, n_beams, max_hits, hits_p, C.byref(n), None)
        return rc, e.lib.mcl_last_error(e._h).decode()

    sp, rp = scans.ctypes.data_as(C.c_void_p), rel.ctypes.data_as(C.c_void_p)
    # the sequence's own: the number of scans, null scans or rel, a rel that is not finite, n_beams
    for S in (0, -1, engine_mod.MAX_SEARCH_SCANS + 1):
        rc, why = raw(sp, rp, S)
        assert rc == INVALID and "n_scans" in why
    many = np.full((engine_mod.MAX_SEARCH_SCANS + 1, 61), 1.0, np.float32)
    assert "n_scans" in expect(engine_mod, INVALID, e.global_search_sequence, many, np.zeros((len(many), 3)))
    rc, why = raw(None, rp, 2)
    assert rc == INVALID and "scans is null" in why
    rc, why = raw(sp, None, 2)
    assert rc == INVALID and "rel is null" in why
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            r = rel.copy()
            r[1, col] = bad
            assert "not finite" in expect(engine_mod, INVALID, e.global_search_sequence, scans, r)
    assert "n_beams" in expect(engine_mod, INVALID, e.global_search_sequence, scans[:, :60], rel)
    # what the single search refuses
    for fields in (dict(stride_cells=0), dict(n_headings=0), dict(beam_stride=0), dict(nms=2), dict(reserved=(0, 0, 0, 1))):
        expect(engine_mod, INVALID, e.global_search_sequence, scans, rel, **fields)
    assert "max_hits" in expect(engine_mod, INVALID, e.global_search_sequence, scans, rel, max_hits=65537)
    rc, why = raw(sp, rp, 2, max_hits=4)
    assert rc == INVALID and "hits is null" in why
    n = C.c_int64()
    cfg = engine_mod.default_search_config()
    assert e.lib.mcl_global_search_sequence(e._h, C.byref(cfg), sp, rp, 2, 61, 0, None, None, None) == INVALID            # null n_hits
    assert "2^27" in expect(engine_mod, INVALID, e.global_search_sequence, scans, rel, stride_cells=1, n_headings=20000)
    assert e.search_bytes() < 1 << 22                                  # ... refused before the volume was asked for
    expect(engine_mod, NOT_READY, e.search_scores)                     # no refused call left a volume
    # the Python layer: one row of rel per scan
    with pytest.raises(ValueError):
        e.global_search_sequence(scans, np.zeros((3, 3)))
    # a search, then a new map: the volume is gone until the next search
    hits, st = e.global_search_sequence(scans, rel, max_hits=2, n_headings=3)
    assert e.search_scores().size == st["n_poses"]
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    expect(engine_mod, NOT_READY, e.search_scores)
    # a lattice without a free position; the field off again
    full = np.full((H, W), 100, np.int8)
    full[0, 0] = 0
    e.set_map(full, small.resolution, small.origin_x, small.origin_y)
    assert "position" in expect(engine_mod, NOT_READY, e.global_search_sequence, scans, rel)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    e.set_likelihood_field(False)
    expect(engine_mod, NOT_READY, e.global_search_sequence, scans, rel)
