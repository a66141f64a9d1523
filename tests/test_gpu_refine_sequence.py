"""The pose refinement over a scan sequence on the GPU (mcl_refine_poses_sequence, DESIGN.md §4.23, rules RS1-RS7 of
include/mcl_hip_engine.h): the summed volume against the fold of mcl_score_poses at RS2's poses bit for bit and against the numpy
statement tests/lfield_ref.py; the records against mcl_host_refine_reduce; the identity with mcl_refine_poses for one scan at the
anchor; that the sequence ranks two places the anchor scan cannot; that an engine which refines runs the same updates, bit for
bit, as one that never does; the buffers it shares with the other refinements; propose_from_scans; the refusals.  The fixtures
are those of tests/refine_ref.py and tests/refine_sequence_ref.py, decided on the CPU by tests/test_refine_sequence_host.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import lfield_ref as lr
import refine_ref as rr
import refine_sequence_ref as rs
from conftest import make_engine, tracking_cloud
from side_geometries import compose, masked
from test_gpu_refine import bits, expect, lf_engine, small, small_oracle  # noqa: F401  (small, small_oracle: fixtures)

pytestmark = pytest.mark.gpu

SMALL_WINDOW = dict(half_xy=1, half_theta=1)                    # 27 poses: a wave holds lanes of three seeds and nine headings


def scans_for(orc, om, ang, rel, at=rr.P_STAR):
    """the scans a robot would take whose pose at the anchor is `at`"""
    return np.stack([rr.scan_at(orc, om, ang, compose(at, r)) for r in rel])


def folded_scores(engine_mod, e, seeds, scans, rel, beam_stride=1, **fields):
    """RS4 from mcl_score_poses: (M, n_win), the poses of RS2 formed in numpy from the two host tables"""
    seeds = np.atleast_2d(seeds)
    off = engine_mod.host_refine_sequence_offsets(seeds, rel, **fields)
    out = []
    for m, seed in enumerate(seeds):
        poses = rs.scan_poses(engine_mod.host_refine_window(seed, rr.RES, **fields), off[m], **fields)
        out.append(rs.fold([e.score_poses(poses[s], masked(scans[s], beam_stride))["log_likelihood"] for s in range(len(scans))]))
    return np.stack(out)


def check_records(engine_mod, r, seeds, want, **fields):
    tol_mean, tol_cov, tol_s = rr.tolerances(rr.RES, **fields)
    for m in range(len(seeds)):
        h = engine_mod.host_refine_reduce(seeds[m], rr.RES, want[m], **fields)
        for name in ("best", "best_log_likelihood", "seed_log_likelihood"):
            assert np.array_equal(bits(r[m][name]), bits(h[name])), (m, name)
        assert int(r[m]["best_index"]) == int(h["best_index"]) == rr.best(want[m], **fields)
        err = (np.abs(r[m]["mean"] - h["mean"]) / tol_mean).max(), (np.abs(r[m]["cov"] - h["cov"]) / tol_cov).max(), \
            abs(float(r[m]["weight_sum"]) - float(h["weight_sum"])) / tol_s
        print("seed", m, "mean / cov / weight_sum error in tolerances:", err)
        assert max(err) <= 1.0
        assert np.array_equal(r[m]["cov"], r[m]["cov"].T)


# ---- 1. the summed volume is the fold of mcl_score_poses, bit for bit; the records are the host restatement's
@pytest.mark.parametrize("M,fields,B,beam_stride,lf_fields,rel,special", [
    (3, SMALL_WINDOW, 61, 1, {}, rs.REL3, "odd"),              # one scan without a usable beam, one with the odd readings
    (3, rr.FIXTURE_WINDOW, 61, 1, {}, rs.REL_OFF, None),       # 1701 lanes: seeds change inside a workgroup; a scan pose off the map
    (1, {}, 61, 1, {}, rs.REL3, None),                         # the default window
    (3, SMALL_WINDOW, 61, 1, {}, rs.REL16, None),              # S = 16
    (3, SMALL_WINDOW, 1, 1, {}, rs.REL2, None),
    (3, rr.FIXTURE_WINDOW, 61, 3, {}, rs.REL2, None),
    (3, SMALL_WINDOW, 61, 1, dict(max_occ_dist_m=4.6), rs.REL3, None),      # K = 8464 >= 8192: the table is read from global memory
    (3, SMALL_WINDOW, 61, 1, dict(z_rand=0.0, sigma_hit_m=0.05), rs.REL2, "inf"),   # a table that ends in -inf: off the map is -inf
], ids=["odd", "off", "default", "S16", "B1", "stride3", "global-table", "inf"])
def test_volume_is_the_fold_of_score_poses(engine_mod, orc, small, small_oracle, M, fields, B, beam_stride, lf_fields, rel, special):
    ang = rr.angles(orc, B)
    e = lf_engine(engine_mod, small, ang, **lf_fields)
    assert (e.likelihood_table().size - 1 >= 8192) == ("max_occ_dist_m" in lf_fields)
    scans = scans_for(orc, small_oracle, ang, rel)
    if special == "inf":
        assert np.isinf(e.likelihood_table()[-1])
        scans[scans > 2.0] = np.nan                      # (the beams that leave through the wall's gaps dropped with the long ones)
    if special == "odd":
        scans[0] = rr.odd_scan(scans[0])
        scans[1] = np.nan
        scans[1, 5], scans[1, 9] = rr.MAX_RANGE, -1.0
    seeds = rr.SEEDS[:M]
    S = len(rel)
    r, st = e.refine_poses_sequence(seeds, scans, rel, beam_stride=beam_stride, **fields)
    n_win = rr.offsets(**fields).shape[0]
    assert st["n_win"] == n_win and st["n_poses"] == M * n_win and st["n_scans"] == S and st["device_bytes"] == e.refine_bytes() > 0
    used = [lr.used_beams(ang, masked(scans[s], beam_stride), rr.MAX_RANGE)[0].size for s in range(S)]
    assert st["used_beams"] == sum(used)
    if special == "odd":
        assert used[1] == 0 and used[0] > 0 and used[2] > 0
    got = e.refine_scores()
    want = folded_scores(engine_mod, e, seeds, scans, rel, beam_stride, **fields)
    assert got.shape == want.shape == (M, n_win)
    assert not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    if special == "inf":
        assert np.isneginf(got).any() and np.isfinite(got).any()
    else:
        assert np.isfinite(got).all()
    if B > 1 and n_win > 100:
        assert np.unique(got).size > 100                   # (a volume, not a constant)
    check_records(engine_mod, r, seeds, want, **fields)
    r2, _ = e.refine_poses_sequence(seeds, scans, rel, beam_stride=beam_stride, **fields)      # the same state, the same bytes
    assert r.tobytes() == r2.tobytes() and np.array_equal(bits(e.refine_scores()), bits(got))


# ---- 2. RS6: one scan at the anchor is mcl_refine_poses
@pytest.mark.parametrize("fields", [SMALL_WINDOW, rr.FIXTURE_WINDOW], ids=["27", "567"])
def test_one_scan_at_the_anchor_is_the_single_refinement(engine_mod, orc, small, small_oracle, fields):
    ang = rr.angles(orc, 61)
    e = lf_engine(engine_mod, small, ang)
    obs = rr.odd_scan(rr.scan_at(orc, small_oracle, ang, rr.P_STAR))
    r1, st1 = e.refine_poses(rr.SEEDS, obs, **fields)
    v1 = e.refine_scores()
    r2, st2 = e.refine_poses_sequence(rr.SEEDS, obs[None], np.zeros((1, 3)), **fields)
    v2 = e.refine_scores()
    assert np.array_equal(bits(v1), bits(v2)) and np.unique(v1).size > 10
    assert r1.tobytes() == r2.tobytes()
    assert st2.pop("n_scans") == 1
    st1.pop("device_bytes"), st2.pop("device_bytes")        # (the sequence has the table and the offsets more)
    assert st1 == st2


# ---- 3. the summed volume against the independent statement
def test_volume_is_the_restatement(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    F = rr.FIXTURE_WINDOW
    scans = rs.perturbed(scans_for(orc, small_oracle, ang, rs.REL2))
    (want, ref), = rs.statement(lr, small, ang, scans, rr.SEEDS[:1], rs.REL2, rr.MAX_RANGE, **F)
    # the cap, confirmed on the CPU statement alone before the device is held to it (tests/test_refine_sequence_host.py too)
    beams = want.size * sum(lr.used_beams(ang, s, rr.MAX_RANGE)[0].size for s in scans)
    n_amb = sum(int(r[2].sum()) for r in ref)
    assert beams > 0 and n_amb <= max(1e-5 * beams, 2), (n_amb, beams)
    e = lf_engine(engine_mod, small, ang)
    e.refine_poses_sequence(rr.SEEDS[0], scans, rs.REL2, **F)
    got = e.refine_scores()[0]
    assert got.shape == want.shape
    for i in np.flatnonzero(bits(got) != bits(want)):
        i = int(i)
        assert any(i in r[1] for r in ref), (i, got[i], want[i])
        sums = {float(rs.fold([np.float64(v) for v in pick])) for pick in itertools.product(*[r[1].get(i, [r[0][i]]) for r in ref])}
        assert got[i] in sums, (i, got[i], want[i], sorted(sums))


# ---- 4. the twin corridors: the anchor scan cannot rank them, the sequence can
def test_sequence_ranks_the_twin_corridors(engine_mod, orc):
    m = rs.twin_map()
    ang = rr.angles(orc, 61)
    scans, seeds, W = rs.twin_scans(m, ang), rs.twin_seeds(), rs.TWIN_WINDOW
    seq = rs.statement(lr, m, ang, scans, seeds, rs.REL5, rr.MAX_RANGE, **W)
    assert all(int(r[2].sum()) == 0 and not r[1] for _, ref in seq for r in ref)     # the statement is unique there
    e = lf_engine(engine_mod, m, ang, n=1000)
    one, _ = e.refine_poses(seeds, scans[1], **W)
    assert bits(one["best_log_likelihood"][0]) == bits(one["best_log_likelihood"][1])
    assert engine_mod.seed_counts(one["best_log_likelihood"], 1000).tolist() == [500, 500]
    r, st = e.refine_poses_sequence(seeds, scans, rs.REL5, **W)
    assert st["n_scans"] == 2 and st["n_win"] == 45
    assert np.array_equal(bits(e.refine_scores()), bits(np.stack([vol for vol, _ in seq])))
    assert np.array_equal(bits(r["best_log_likelihood"]), bits(np.array([vol.max() for vol, _ in seq])))
    assert r["best_log_likelihood"][1] - r["best_log_likelihood"][0] > 40.0
    counts = engine_mod.seed_counts(r["best_log_likelihood"], 1000)
    assert counts.tolist() == [0, 1000]
    e.init_particles_mixture(r["mean"], r["cov"], counts)
    p = e.get_particles()
    rows = (p[1] - m.origin_y) / float(m.resolution)
    assert p.shape[1] == 1000 and np.all((rows >= rs.TRUTH_CELL[1] - 3) & (rows < rs.TRUTH_CELL[1] + 3))


# ---- 5. read-only
def test_sequence_refinement_leaves_the_updates_alone(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    n = 2000
    pose = rr.P_STAR
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=pose, sig=(0.2, 0.2, 0.2))
    scans = [rr.scan_at(orc, small_oracle, ang, (pose[0] + 0.02 * t, pose[1], pose[2])) for t in range(1, 4)]
    a, b = lf_engine(engine_mod, small, ang, n), lf_engine(engine_mod, small, ang, n)
    assert a.refine_bytes() == 0 and b.refine_bytes() == 0
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    grown = []
    for t, scan in enumerate(scans):
        rel = engine_mod.relative_poses([(0.02 * u, 0.0, 0.0) for u in range(t + 1)])
        r, st = b.refine_poses_sequence(rr.SEEDS[:1 + t], scans[:t + 1], rel, half_xy=1 + t, half_theta=2 * t)
        assert st["n_scans"] == t + 1 and st["device_bytes"] == b.refine_bytes() > 0
        grown.append(b.refine_bytes())
        for e in (a, b):
            e.update((0.02, 0.0, 0.0), scan)
        assert np.array_equal(bits(a.get_particles()), bits(b.get_particles())), t
        assert np.array_equal(bits(a.get_weights()), bits(b.get_weights())), t
    assert grown[0] < grown[1] < grown[2]
    assert a.refine_bytes() == 0
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))


# ---- 6. the buffers the refinements share
def test_shared_buffers_hold_nothing_stale(engine_mod, orc, small, small_oracle):
    ang = rr.angles(orc, 61)
    scans = scans_for(orc, small_oracle, ang, rs.REL3)
    scans[0] = rr.odd_scan(scans[0])
    F, G = rr.FIXTURE_WINDOW, SMALL_WINDOW
    calls = [lambda e: e.refine_poses(rr.SEEDS, scans[2], **F),
             lambda e: e.refine_poses_sequence(rr.SEEDS, scans, rs.REL3, **F),
             lambda e: e.refine_poses_beam(rr.SEEDS[:2], scans[0], **G),
             lambda e: e.refine_poses(rr.SEEDS[:1], scans[0], **G),
             lambda e: e.refine_poses_sequence(rr.SEEDS[:2], scans[:2], rs.REL_OFF, **G)]
    e = lf_engine(engine_mod, small, ang)
    for call in calls:
        r, _ = call(e)
        v = e.refine_scores()
        fresh = lf_engine(engine_mod, small, ang)
        r0, _ = call(fresh)
        assert r.tobytes() == r0.tobytes()
        assert v.shape == fresh.refine_scores().shape and np.array_equal(bits(v), bits(fresh.refine_scores()))
        fresh.close()
    assert e.refine_scores().shape == (2, 27)                       # the last call's volume
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    expect(engine_mod, engine_mod.MCL_ERR_NOT_READY, e.refine_scores)


# ---- 7. propose_from_scans
def test_propose_from_scans(engine_mod, orc):
    m = rs.twin_map()
    ang = rr.angles(orc, 61)
    scans, W = rs.twin_scans(m, ang), rs.TWIN_WINDOW
    SEARCH = dict(stride_cells=2, n_headings=8)
    e = lf_engine(engine_mod, m, ang)
    for pruned, search in ((True, e.global_search_sequence_pruned), (False, e.global_search_sequence)):
        hits = e.propose_from_scans(scans, rs.REL5, max_hits=8, refine_fields=W, pruned=pruned, **SEARCH)
        want_hits, _ = search(scans, rs.REL5, max_hits=8, **SEARCH)
        assert hits.size > 1 and np.array_equal(hits, want_hits) and np.isfinite(hits["log_likelihood"]).all()
        r, _ = e.refine_poses_sequence(hits["pose"], scans, rs.REL5, **W)
        thr, fac = e.recovery_proposal()
        want = engine_mod.host_recovery_proposal(r["mean"], r["cov"])
        assert thr.size == hits.size and np.array_equal(thr, want[0]) and np.array_equal(bits(fac), bits(want[1]))
    # seed_counts' shares of the summed scores as weights.  Without nms every lattice pose is a candidate and the twin's lattice
    # pose is the 1049th best of 20008 by the CPU statement (unique there), so among 2048 hits it is a finite one: its
    # component of the proposal gets nothing
    seeds = rs.twin_seeds()
    hits = e.propose_from_scans(scans, rs.REL5, max_hits=2048, weights="likelihood", refine_fields=W, pruned=False, nms=0, **SEARCH)
    assert hits.size == 2048 and np.isfinite(hits["log_likelihood"]).all()
    r, _ = e.refine_poses_sequence(hits["pose"], scans, rs.REL5, **W)
    shares = engine_mod.seed_counts(r["best_log_likelihood"], 1 << 30).astype(np.float64)
    thr, fac = e.recovery_proposal()
    assert thr.size == hits.size and np.array_equal(thr, engine_mod.host_recovery_proposal(r["mean"], r["cov"], shares)[0])
    twin = np.flatnonzero((np.abs(hits["pose"][:, :2] - seeds[0, :2]).max(axis=1) < 1e-9) & (np.abs(hits["pose"][:, 2]) < 1e-9))
    truth = np.flatnonzero((np.abs(hits["pose"][:, :2] - seeds[1, :2]).max(axis=1) < 1e-9) & (np.abs(hits["pose"][:, 2]) < 1e-9))
    assert twin.size == 1 and truth.tolist() == [0]
    share = np.diff(np.concatenate([[0], thr.astype(object)]))
    print("the twin is hit", twin.tolist(), "of", hits.size, "with threshold share", int(share[twin[0]]), "; nonzero shares", int((share > 0).sum()))
    assert np.isfinite(r["best_log_likelihood"][twin[0]]) and int(share[twin[0]]) == 0
    assert int(share[0]) > 0 and int(np.argmax(share)) == int(np.argmax(r["best_log_likelihood"]))
    # every hit dropped: the proposal is cleared
    assert e.recovery_proposal() is not None
    assert e.propose_from_scans(scans, rs.REL5, max_hits=0, pruned=False, **SEARCH).size == 0      # (the pruned search refuses max_hits = 0)
    assert e.recovery_proposal() is None
    with pytest.raises(ValueError):
        e.propose_from_scans(scans, rs.REL5, weights="best")
    # the field off: refused, the model is not switched
    e.set_likelihood_field(False)
    expect(engine_mod, engine_mod.MCL_ERR_NOT_READY, e.propose_from_scans, scans, rs.REL5, **SEARCH)
    assert e.lib.mcl_get_likelihood_table(e._h, None, 0, None) != 0


# ---- 8. the refusals
def test_refusals(engine_mod, orc, small):
    INVALID, NOT_READY = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY
    ang = rr.angles(orc, 61)
    scans, rel, seeds = np.full((2, 61), 1.0, np.float32), np.zeros((2, 3)), rr.SEEDS
    f = lambda e: e.refine_poses_sequence
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, f(e), seeds, scans, rel)
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    assert "beam" in expect(engine_mod, NOT_READY, f(e), seeds, scans, rel)
    e.set_beam_angles(ang)
    assert "likelihood-field" in expect(engine_mod, NOT_READY, f(e), seeds, scans, rel)
    e.set_likelihood_field(True)
    assert e.refine_bytes() == 0

    def raw(seeds_p, scans_p, rel_p, S, M=3, n_beams=61, out_p=True):
        cfg, out = engine_mod.default_refine_config(), np.zeros(3, engine_mod.REFINE_DTYPE)
        rc = e.lib.mcl_refine_poses_sequence(e._h, C.byref(cfg), seeds_p, M, scans_p, rel_p, S, n_beams,
                                             out.ctypes.data_as(C.c_void_p) if out_p else None, None)
        return rc, e.lib.mcl_last_error(e._h).decode()

    s = np.ascontiguousarray(seeds.T)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for S in (0, -1, engine_mod.MAX_SEARCH_SCANS + 1):
        rc, why = raw(vp(s), vp(scans), vp(rel), S)
        assert rc == INVALID and "n_scans" in why
    many = np.full((engine_mod.MAX_SEARCH_SCANS + 1, 61), 1.0, np.float32)
    assert "n_scans" in expect(engine_mod, INVALID, f(e), seeds, many, np.zeros((len(many), 3)))
    rc, why = raw(vp(s), None, vp(rel), 2)
    assert rc == INVALID and "scans is null" in why
    rc, why = raw(vp(s), vp(scans), None, 2)
    assert rc == INVALID and "rel is null" in why
    rc, why = raw(None, vp(scans), vp(rel), 2)
    assert rc == INVALID and "null" in why
    rc, why = raw(vp(s), vp(scans), vp(rel), 2, out_p=False)
    assert rc == INVALID and "null" in why
    for bad in (np.nan, np.inf, -np.inf):
        for col in range(3):
            r = rel.copy()
            r[0, col] = bad
            assert "not finite" in expect(engine_mod, INVALID, f(e), seeds, scans, r)
            p = seeds.copy()
            p[1, col] = bad
            assert "non-finite" in expect(engine_mod, INVALID, f(e), p, scans, rel)
    assert "n_beams" in expect(engine_mod, INVALID, f(e), seeds, scans[:, :60], rel)
    # what R7 refuses of the config and of M
    for fields in (dict(half_xy=-1), dict(half_theta=-1), dict(step_xy_cells=0.0), dict(step_theta_rad=np.nan), dict(beam_stride=0),
                   dict(reserved=(0, 0, 1)), dict(half_xy=90, half_theta=1), dict(half_xy=0, half_theta=16384)):
        expect(engine_mod, INVALID, f(e), seeds, scans, rel, **fields)
    expect(engine_mod, INVALID, f(e), np.zeros((0, 3)), scans, rel)
    expect(engine_mod, INVALID, f(e), np.zeros((4097, 3)), scans, rel, half_xy=0, half_theta=0)
    # the row cap: 9 seeds x 32767 headings x 16 scans = 4 718 448 rows (M n_win stays below 2^27)
    why = expect(engine_mod, INVALID, f(e), np.zeros((9, 3)), np.full((16, 61), 1.0, np.float32), np.zeros((16, 3)), half_xy=0, half_theta=16383)
    assert "MCL_REFINE_SEQ_MAX_ROWS" in why and str(1 << 21) in why and "9 seeds" in why and "32767" in why and "16 scans" in why
    assert e.refine_bytes() == 0                                        # ... all refused before anything was asked for
    expect(engine_mod, NOT_READY, e.refine_scores)
    with pytest.raises(ValueError):
        e.refine_poses_sequence(seeds, scans, np.zeros((3, 3)))         # the Python layer: one row of rel per scan
    # a null config and null stats are the defaults; then a new map: the volume is gone
    out = np.zeros(3, engine_mod.REFINE_DTYPE)
    assert e.lib.mcl_refine_poses_sequence(e._h, None, vp(s), 3, vp(scans), vp(rel), 2, 61, vp(out), None) == engine_mod.MCL_OK
    r, st = e.refine_poses_sequence(seeds, scans, rel)
    assert r.tobytes() == out.tobytes() and st["n_win"] == 1701 and e.refine_scores().shape == (3, 1701)
    before = e.refine_bytes()
    expect(engine_mod, INVALID, f(e), seeds, scans, rel, half_theta=-1)
    assert e.refine_bytes() == before
    e.set_map(small.data, small.resolution, small.origin_x, small.origin_y)
    expect(engine_mod, NOT_READY, e.refine_scores)
    e.set_likelihood_field(False)
    expect(engine_mod, NOT_READY, f(e), seeds, scans, rel)
