"""The side calls on the GPU over the scan family of tests/scan_geometries.py, on the 120 x 90 map of side_geometries.small():
mcl_query_scans and mcl_score_poses, the likelihood-field update, mcl_global_search and its streamed, beam, pruned and
sequence-pruned forms, mcl_refine_poses and mcl_refine_poses_beam, each held to its CPU statement (the oracle's cast_ray,
tests/lfield_ref.py, beam_search_ref.py, refine_beam_ref.py, refine_ref.py) or -- the pruned searches -- to the unpruned call, on
beam sets the Hokuyo grid of tests/test_gpu_side_geometries.py never offers: full turns, angles up to 2 pi, a descending scan, more
than a turn, 2701 beams, 45 degrees, one beam per wedge, one beam.  Every comparison is integer-exact or bit-exact but the two the
project defines: LF4's ambiguity band, whose cap tests/test_scan_geometries_host.py confirms on the CPU for every set of poses used
here, and refine_ref.tolerances for the moments.  The beam search's rules B <= M and M % n_headings == 0 are crossed here: B == M
on turn360 and turn720_from_zero, B > M on over_turn."""
import os

import numpy as np
import pytest

import beam_search_ref as br
import refine_beam_ref as rb
import refine_ref as rr
import scan_geometries as scg
import side_geometries as sg
from conftest import make_engine, tracking_cloud
from side_geometries import bits
from test_gpu_side_geometries import held_to_lf
from test_scan_geometries_host import LF_STRIDE, N_HEAD, lf_scan

pytestmark = pytest.mark.gpu

# n_headings of the beam search (they divide M), and the lattice: stride 4 keeps fine2701's table of 3600 angles small
BEAM_HEADS = dict(turn360=(72, 360), turn720_from_zero=(72,), fine2701=(72,), narrow_rear=(72,), coarse30=(12,), wedge13=(16, 8), one=(8,))
BEAM_STRIDE = dict(fine2701=4)
BEAM_REFUSED = dict(descending=scg.NO_ASCEND, over_turn=scg.NO_TURN)
REL3 = np.array([[-4.0, 1.0, 0.15], [-2.0, 0.5, 0.05], [0.0, 0.0, 0.0]])       # in cells (x, y) and radians: three scans along a path
FIRST = 3


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


class Case:
    """a member of the scan family on the map, its scans and one engine per sensor model (made once per member)"""

    def __init__(self, engine_mod, orc, name):
        self.name, self.orc, self.mod = name, orc, engine_mod
        self.g = sg.small()
        self.om = self.g.oracle(orc)
        self.P = self.om.max_range_px
        self.ang = scg.family()[name]
        self.B = self.ang.size
        self.obs = lf_scan(orc, self.g, name)                                    # the field calls: no reading of 0
        self.odd = scg.scan_for(orc, self.om, self.ang, self.g.true_pose)         # the beam calls: every odd reading
        self.seeds = scg.seeds(self.g)
        self.rel = REL3 * np.array([self.g.res, self.g.res, 1.0])
        seed = scg.PERTURB_SEED.get(name, 7)
        self.scans3 = np.stack([scg.scan_for(orc, self.om, self.ang, sg.compose(self.g.true_pose, r), seed=seed + s, zero=False)
                                for s, r in enumerate(self.rel)])
        self.beam = make_engine(engine_mod, self.g, self.ang, 4096)
        self.lf = make_engine(engine_mod, self.g, self.ang, 4096)
        self.lf.set_likelihood_field(True)
        assert self.beam.max_range_px == self.P

    def close(self):
        self.beam.close()
        self.lf.close()

    def oracle_scans(self, poses):
        a = (poses[:, 2][:, None] + self.ang.astype(np.float64)[None, :]).ravel()
        r, s = self.orc.cast_many(self.om, np.repeat(poses[:, 0], self.B), np.repeat(poses[:, 1], self.B), a)
        return r.reshape(len(poses), self.B), s.reshape(len(poses), self.B)


@pytest.fixture(scope="module", params=scg.SIDE)
def cx(request, engine_mod, orc):
    c = Case(engine_mod, orc, request.param)
    yield c
    c.close()


def members(*names):
    """a test of some members only: the fixture's parameters, overridden"""
    return pytest.mark.parametrize("cx", names, indirect=True)


# ---- 1. the pose query
@pytest.mark.parametrize("force_exact", [0, 1, 2])
def test_query_steps_are_cast_ray(cx, force_exact):
    q = cx.g.query_poses
    e = cx.beam if not force_exact else make_engine(cx.mod, cx.g, cx.ang, 64, debug_force_exact=force_exact)
    want_ranges, want_steps = cx.oracle_scans(q)
    ranges, steps = e.expected_scans(q, want_steps=True)
    l3 = e.query_counters()["level3_rays"]
    print(f"{cx.name}: level-3 rays of the 64 query poses: {l3} of {steps.size} (force_exact={force_exact})")
    assert steps.dtype == np.uint16 and steps.shape == (64, cx.B)
    assert np.array_equal(steps.astype(np.int32), want_steps), np.argwhere(steps != want_steps)[:5]
    assert np.array_equal(ranges.view(np.uint32), want_ranges.view(np.uint32))
    if force_exact == 1:
        assert l3 == steps.size
    if force_exact:
        e.close()


# ---- 2. the scores
def test_beam_scores_and_counts(cx):
    q = cx.g.query_poses
    want = rb.scores(cx.orc, cx.om, q, cx.ang, cx.odd)
    _, steps = cx.oracle_scans(q)
    for tol in (0, 2):
        sc = cx.beam.score_poses(q, cx.odd, tol_steps=tol)
        assert np.array_equal(bits(sc["log_likelihood"]), bits(want))
        n_valid, n_agree, n_miss = sg.counts_ref(cx.orc, cx.om, steps, cx.odd, tol)
        assert (sc["n_valid"] == n_valid).all() and 0 < n_valid <= cx.B
        assert np.array_equal(sc["n_agree"], n_agree) and np.array_equal(sc["n_miss"], n_miss)
        assert (sc["reserved"] == 0).all()
    assert sc["n_agree"][0] > 0                                 # the true pose agrees with its own scan


def test_field_scores_and_update(cx):
    g, q = cx.g, cx.g.query_poses
    want, alts, n_amb, beams = sg.lf_statement(g, q, cx.ang, cx.obs)
    sc = cx.lf.score_poses(q, cx.obs)
    held_to_lf(sc["log_likelihood"], want, alts, n_amb, beams, "score_poses")
    _, steps = cx.oracle_scans(q)
    n_valid, n_agree, n_miss = sg.counts_ref(cx.orc, cx.om, steps, cx.obs, 2)                 # the counts still come from cast rays
    assert (sc["n_valid"] == n_valid).all() and np.array_equal(sc["n_agree"], n_agree) and np.array_equal(sc["n_miss"], n_miss)
    p = g.particles
    want, alts, n_amb, beams = sg.lf_statement(g, p.T, cx.ang, cx.obs)
    cx.lf.set_particles(p, np.full(4096, 1.0 / 4096))
    cx.lf.sensor_update(cx.obs)
    held_to_lf(cx.lf.log_weights(), want, alts, n_amb, beams, "sensor_update")


# ---- 3. the global search under the likelihood field, whole and streamed
def test_global_search(cx):
    g, e = cx.g, cx.lf
    cells, xy, theta, poses = sg.lattice(cx.mod, g, LF_STRIDE, N_HEAD)
    f = dict(stride_cells=LF_STRIDE, n_headings=N_HEAD)
    want, alts, n_amb, beams = sg.lf_statement(g, poses, cx.ang, cx.obs)
    _, st = e.global_search(cx.obs, max_hits=0, **f)
    assert st["n_positions"] == cells.size and st["n_poses"] == len(poses)
    held_to_lf(e.search_scores(), want, alts, n_amb, beams, "search volume")
    V = e.search_scores(N_HEAD)
    for nms in (0, 1):
        fn = dict(nms=nms, **f)
        want_hits = sg.hits_ref(g, V, cells, LF_STRIDE, nms)
        assert want_hits.size >= 1
        for max_hits in (want_hits.size // 2, 65536):
            hits, st = e.global_search(cx.obs, max_hits=max_hits, **fn)
            m = min(max_hits, want_hits.size)
            assert st["n_hits"] == want_hits.size and len(hits) == m and np.array_equal(hits["index"], want_hits[:m])
            k, p = want_hits[:m] // cells.size, want_hits[:m] % cells.size
            assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
            assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p])) and np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
            for G in (1, 2):
                s_hits, s_st = e.global_search_streamed(cx.obs, max_hits=max_hits, slab_headings=G, **fn)
                assert s_hits.tobytes() == hits.tobytes() and len(s_hits) == len(hits) and s_st["n_hits"] == st["n_hits"], (nms, max_hits, G)


# ---- 4. the global search under the beam model
def test_beam_search(cx):
    g, e = cx.g, cx.beam
    if cx.name in BEAM_REFUSED:
        for n_head in (8, 72):
            with pytest.raises(cx.mod.EngineError) as ei:
                e.global_search_beam(cx.odd, max_hits=4, stride_cells=3, n_headings=n_head)
            assert ei.value.status == cx.mod.MCL_ERR_INVALID_ARG and BEAM_REFUSED[cx.name] in str(ei.value), str(ei.value)
        return
    stride = BEAM_STRIDE.get(cx.name, 3)
    for n_head in BEAM_HEADS[cx.name]:
        grid = br.grid(cx.ang, n_head)
        pred = scg.beam_grid(cx.ang, n_head)
        assert pred["refusal"] is None and (grid["M"], grid["heading_step"]) == (pred["M"], pred["heading_step"])
        M = grid["M"]
        if cx.name in ("turn360", "turn720_from_zero"):
            assert M == cx.B                                    # B == M: the scan is the whole grid
        cells, xy, theta, _ = sg.lattice(cx.mod, g, stride, n_head)
        n_pos = cells.size
        S = br.table(cx.orc, cx.om, xy, grid["phi"])
        want = br.volume(cx.orc, cx.om, S, cx.odd, n_head, grid["heading_step"])
        _, st = e.global_search_beam(cx.odd, max_hits=0, stride_cells=stride, n_headings=n_head)
        assert st["n_positions"] == n_pos and st["n_poses"] == n_pos * n_head and st["used_beams"] == cx.B and st["grid_angles"] == M
        first, R = e.search_beam_table()
        assert first == (st["n_tiles"] - 1) * st["tile_positions"] and R.shape == (n_pos - first, M)
        assert np.array_equal(R.astype(np.int64), S[first:])
        V = e.search_scores(n_head)
        assert not np.isnan(V).any() and np.array_equal(bits(V), bits(want))
        print(f"{cx.name}: beam search, {n_head} headings, M {M}: {n_pos} positions, level-3 rays {st['level3_rays']} of {S.size}")
        for nms in (0, 1):
            want_hits = br.hits(V, cells, stride, nms, g.W, g.H)
            hits, st = e.global_search_beam(cx.odd, max_hits=65536, nms=nms, stride_cells=stride, n_headings=n_head)
            m = min(65536, want_hits.size)
            assert st["n_hits"] == want_hits.size and len(hits) == m and np.array_equal(hits["index"], want_hits[:m])
            k, p = want_hits[:m] // n_pos, want_hits[:m] % n_pos
            assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
            assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p])) and np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
    # a heading count that does not divide the grid is refused with the grid's size
    if cx.B >= 2:
        bad = next(h for h in (7, 11, 13) if M % h)
        with pytest.raises(cx.mod.EngineError) as ei:
            e.global_search_beam(cx.odd, max_hits=4, stride_cells=stride, n_headings=bad)
        assert f"n_headings must divide the angle grid M = {M}" in str(ei.value)


# ---- 5. the pruned searches: the hits of the unpruned calls
@members("turn360", "narrow_rear", "fine2701")
def test_pruned_searches(cx):
    e = cx.lf
    for nms in (0, 1):
        f = dict(stride_cells=LF_STRIDE, n_headings=N_HEAD, nms=nms)
        want, st = e.global_search(cx.obs, max_hits=65536, **f)
        want = want.copy()
        want_seq, st_seq = e.global_search_sequence(cx.scans3, cx.rel, max_hits=65536, **f)
        want_seq = want_seq.copy()
        assert 1 <= st["n_hits"] < 65536 and 1 <= st_seq["n_hits"] < 65536 and st_seq["n_scans"] == 3
        for block in (2, 4):
            for max_hits in (1, 16, 65536):
                got, ps = e.global_search_pruned(cx.obs, max_hits=max_hits, block=block, first_pairs=FIRST, **f)
                what = (cx.name, nms, block, max_hits)
                assert ps["n_hits"] == len(got) == min(max_hits, st["n_hits"]), what
                assert got.dtype == want.dtype and got.tobytes() == want[:len(got)].tobytes(), what
                assert ps["guard_fallbacks"] == 0 and 1 <= ps["pairs_scored"] <= ps["pairs"], (what, ps)
                got, ps = e.global_search_sequence_pruned(cx.scans3, cx.rel, max_hits=max_hits, block=block, first_pairs=FIRST, **f)
                assert ps["n_hits"] == len(got) == min(max_hits, st_seq["n_hits"]) and ps["n_scans"] == 3, what
                assert got.tobytes() == want_seq[:len(got)].tobytes(), what
                assert ps["guard_fallbacks"] == 0, (what, ps)


# ---- 6. the refinements
def check_records(cx, e, r, V, fields):
    """best pose, mean and covariance against refine_ref.best / moments within refine_ref.tolerances"""
    g = cx.g
    tol_mean, tol_cov, tol_s = rr.tolerances(g.resolution, **fields)
    for m, seed in enumerate(cx.seeds):
        wb = rr.best(V[m], **fields)
        b, mean, cov, S = rr.moments(seed, g.resolution, V[m], **fields)
        assert int(r[m]["best_index"]) == wb
        assert np.array_equal(bits(r[m]["best"]), bits(b))
        assert np.array_equal(bits(r[m]["best_log_likelihood"]), bits(V[m, wb]))
        assert np.array_equal(bits(r[m]["seed_log_likelihood"]), bits(V[m, V.shape[1] // 2]))
        err = np.array([(np.abs(r[m]["mean"] - mean) / tol_mean).max(), (np.abs(r[m]["cov"] - cov) / tol_cov).max(),
                        abs(float(r[m]["weight_sum"]) - S) / tol_s])
        print(f"{cx.name}: seed {m}: mean / cov / weight_sum error in tolerances: {err}")
        assert err.max() <= 1.0, (m, err)
        assert np.array_equal(r[m]["cov"], r[m]["cov"].T)


@members("turn360", "narrow_rear", "fine2701", "descending")
def test_refinements(cx):
    g, F = cx.g, cx.g.window_fields
    win = np.concatenate([rr.window(s, g.resolution, **F) for s in cx.seeds])
    n_win = win.shape[0] // 3
    # under the likelihood field
    want, alts, n_amb, beams = sg.lf_statement(g, win, cx.ang, cx.obs)
    r, st = cx.lf.refine_poses(cx.seeds, cx.obs, **F)
    assert st["n_win"] == n_win and st["n_poses"] == 3 * n_win
    got = cx.lf.refine_scores()
    assert got.shape == (3, n_win)
    held_to_lf(got.ravel(), want, alts, n_amb, beams, "refine volume")
    check_records(cx, cx.lf, r, got, F)
    # under the beam model
    want = rb.scores(cx.orc, cx.om, win, cx.ang, cx.odd).reshape(3, -1)
    r, st = cx.beam.refine_poses_beam(cx.seeds, cx.odd, **F)
    assert st["n_win"] == n_win and st["rays"] == want.size * cx.B and st["used_beams"] == cx.B
    print(f"{cx.name}: beam refinement: level-3 rays {st['level3_rays']} of {st['rays']}")
    got = cx.beam.refine_scores()
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    check_records(cx, cx.beam, r, want, F)


# ---- 7. read-only
@pytest.mark.parametrize("field", [False, True], ids=["beam", "field"])
def test_an_update_after_every_side_call_is_that_of_a_fresh_engine(cx, field):
    g, n = cx.g, 2000
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=g.true_pose, sig=(2 * g.res, 2 * g.res, 0.2))
    a, b = make_engine(cx.mod, g, cx.ang, n), make_engine(cx.mod, g, cx.ang, n)
    for e in (a, b):
        if field:
            e.set_likelihood_field(True)
        e.set_particles(cloud, np.full(n, 1.0 / n))
    f = dict(stride_cells=LF_STRIDE, n_headings=N_HEAD)
    a.expected_scans(g.query_poses)
    a.score_poses(g.query_poses, cx.odd)
    if cx.name in BEAM_HEADS:
        a.global_search_beam(cx.odd, max_hits=4, stride_cells=BEAM_STRIDE.get(cx.name, 3), n_headings=BEAM_HEADS[cx.name][-1])
    a.refine_poses_beam(cx.seeds, cx.odd, **g.window_fields)
    if field:
        a.global_search(cx.obs, max_hits=4, **f)
        a.global_search_sequence(cx.scans3, cx.rel, max_hits=4, **f)
        a.global_search_streamed(cx.obs, max_hits=4, slab_headings=2, **f)
        a.global_search_pruned(cx.obs, max_hits=4, block=4, first_pairs=FIRST, **f)
        a.global_search_sequence_pruned(cx.scans3, cx.rel, max_hits=4, block=4, first_pairs=FIRST, **f)
        a.refine_poses(cx.seeds, cx.obs, **g.window_fields)
    for e in (a, b):
        e.update((g.res, 0.0, 0.01), cx.obs)
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))
    assert np.array_equal(a.resample_indices(), b.resample_indices())
    a.close()
    b.close()


# ---- 8. the query's beam limit
def test_query_serves_65535_beams_and_refuses_65536(engine_mod, orc):
    g = sg.small()
    om = g.oracle(orc)
    ang = scg.family()["b65536"]
    q = g.query_poses[:8]
    e = make_engine(engine_mod, g, ang, 64)
    for call in (lambda: e.expected_scans(q), lambda: e.score_poses(q, np.full(ang.size, 3.0, np.float32))):
        with pytest.raises(engine_mod.EngineError) as ei:
            call()
        assert ei.value.status == -5 and scg.NO_QUERY in str(ei.value), str(ei.value)               # MCL_ERR_UNSUPPORTED
    e.set_beam_angles(ang[:65535])
    ranges, steps = e.expected_scans(q, want_steps=True)
    a = (q[:, 2][:, None] + ang[:65535].astype(np.float64)[None, :]).ravel()
    want_r, want_s = orc.cast_many(om, np.repeat(q[:, 0], 65535), np.repeat(q[:, 1], 65535), a, use_omp=True)
    assert np.array_equal(steps.astype(np.int32).ravel(), want_s) and np.array_equal(ranges.view(np.uint32).ravel(), want_r.view(np.uint32))
    e.close()
