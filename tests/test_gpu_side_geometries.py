"""The side calls on the GPU over the geometry family of tests/side_geometries.py: mcl_query_scans and mcl_score_poses, the
likelihood-field update, mcl_global_search and its sequence, streamed and beam forms, mcl_refine_poses and mcl_refine_poses_beam,
each held to its CPU statement (the oracle's cast_ray, tests/lfield_ref.py, beam_search_ref.py, refine_beam_ref.py, refine_ref.py)
and not to another device call, on maps whose row width, lattice size, resolution, coordinate magnitude and content the
120 x 90 map of the other side-call tests never varies.  Every comparison is integer-exact or bit-exact but the two the project
defines: LF4's ambiguity band, whose cap tests/test_side_geometries_host.py confirms on the CPU for every set of poses used
here, and refine_ref.tolerances for the moments."""
import itertools

import numpy as np
import pytest

import beam_search_ref as br
import refine_beam_ref as rb
import refine_ref as rr
import side_geometries as sg
from conftest import make_engine, tracking_cloud
from side_geometries import bits

pytestmark = pytest.mark.gpu

N_HEAD, N_HEAD_BEAM = 5, 8
REL = np.array([[-3.0, 1.0, 0.1], [0.0, 0.0, 0.0]])            # in cells (x, y) and radians: scaled by the resolution


class Case:
    """a geometry, its scans and one engine per sensor model (made once per geometry)"""

    def __init__(self, engine_mod, orc, g):
        self.g, self.orc, self.mod = g, orc, engine_mod
        self.om = g.oracle(orc)
        self.P = self.om.max_range_px
        self.ang, self.ang55 = sg.angles(orc, 61), sg.even_angles(orc, 55)
        self.obs = g.scan(orc, self.ang)                                        # about a millimetre off the cast ranges
        self.odd = sg.odd_scan(sg.scan_at(orc, self.om, self.ang, g.true_pose))
        self.odd55 = sg.odd_scan(sg.scan_at(orc, self.om, self.ang55, g.true_pose))
        self.rel = REL * np.array([g.res, g.res, 1.0])
        self.earlier = sg.perturbed_scan(orc, self.om, self.ang, sg.compose(g.true_pose, self.rel[0]), seed=g.perturb_seed + 1)
        self.beam = make_engine(engine_mod, g, self.ang, 4096)
        self.lf = make_engine(engine_mod, g, self.ang, 4096)
        self.lf.set_likelihood_field(True)
        self.beam55 = make_engine(engine_mod, g, self.ang55, 64)
        assert self.beam.max_range_px == self.P
        self.worst = np.zeros(3)                                                # moment deviations in refine_ref.tolerances

    def close(self):
        for e in (self.beam, self.lf, self.beam55):
            e.close()

    def oracle_scans(self, poses, ang):
        a = (poses[:, 2][:, None] + ang.astype(np.float64)[None, :]).ravel()
        r, s = self.orc.cast_many(self.om, np.repeat(poses[:, 0], ang.size), np.repeat(poses[:, 1], ang.size), a)
        return r.reshape(len(poses), ang.size), s.reshape(len(poses), ang.size)


@pytest.fixture(scope="module", params=sg.NAMES)
def cx(request, engine_mod, orc):
    c = Case(engine_mod, orc, sg.family()[request.param])
    yield c
    c.close()


def held_to_lf(got, want, alts, n_amb, beams, what):
    """LF4: bit for bit the statement's value, or one of the listed sums of a pose with an end point in the ambiguity band --
    after the cap on such end points has been confirmed on the statement alone"""
    assert beams > 0 and sg.within_cap(n_amb, beams), (what, int(np.sum(n_amb)), beams)
    assert got.shape == want.shape and not np.isnan(got).any()
    bad = sg.lf_mismatches(got, want, alts)
    assert not bad, (what, len(bad), bad[:5])


# ---- 1. the pose query
@pytest.mark.parametrize("force_exact", [0, 1])
def test_query_steps_are_cast_ray(cx, force_exact):
    q = cx.g.query_poses
    e = cx.beam if not force_exact else make_engine(cx.mod, cx.g, cx.ang, 64, debug_force_exact=1)
    want_ranges, want_steps = cx.oracle_scans(q, cx.ang)
    ranges, steps = e.expected_scans(q, want_steps=True)
    l3 = e.query_counters()["level3_rays"]
    print(f"{cx.g.name}: level-3 rays of the 64 query poses: {l3} of {steps.size} (force_exact={force_exact})")
    assert steps.dtype == np.uint16 and steps.shape == (64, 61)
    assert np.array_equal(steps.astype(np.int32), want_steps), np.argwhere(steps != want_steps)[:5]
    assert np.array_equal(ranges.view(np.uint32), want_ranges.view(np.uint32))
    if force_exact:
        assert l3 == steps.size
        e.close()
    if cx.g.name == "fine":
        assert cx.P > 255                                       # 16-bit steps
    if cx.g.name == "open":
        assert not (cx.g.data > 50).any() and (steps < cx.P).any()              # nothing to hit: the map's border ends the rays
    if cx.g.name not in sg.DEGENERATE:
        assert (steps == 0).any() and ((steps > 0) & (steps < cx.P)).any()


# ---- 2. the scores
def test_beam_scores_and_counts(cx):
    q = cx.g.query_poses
    want = rb.scores(cx.orc, cx.om, q, cx.ang, cx.odd)
    _, steps = cx.oracle_scans(q, cx.ang)
    for tol in (0, 2):
        sc = cx.beam.score_poses(q, cx.odd, tol_steps=tol)
        assert np.array_equal(bits(sc["log_likelihood"]), bits(want))
        n_valid, n_agree, n_miss = sg.counts_ref(cx.orc, cx.om, steps, cx.odd, tol)
        assert (sc["n_valid"] == n_valid).all() and 0 < n_valid < 61
        assert np.array_equal(sc["n_agree"], n_agree) and np.array_equal(sc["n_miss"], n_miss)
        assert (sc["reserved"] == 0).all()
    assert sc["n_agree"][0] > 0                                 # the true pose agrees with its own scan


def test_field_scores_and_update(cx):
    g, q = cx.g, cx.g.query_poses
    want, alts, n_amb, beams = sg.lf_statement(g, q, cx.ang, cx.obs)
    sc = cx.lf.score_poses(q, cx.obs)
    held_to_lf(sc["log_likelihood"], want, alts, n_amb, beams, "score_poses")
    _, steps = cx.oracle_scans(q, cx.ang)
    n_valid, n_agree, n_miss = sg.counts_ref(cx.orc, cx.om, steps, cx.obs, 2)                 # the counts still come from cast rays
    assert (sc["n_valid"] == n_valid).all() and np.array_equal(sc["n_agree"], n_agree) and np.array_equal(sc["n_miss"], n_miss)
    # an update of 4096 particles
    p = g.particles
    want, alts, n_amb, beams = sg.lf_statement(g, p.T, cx.ang, cx.obs)
    cx.lf.set_particles(p, np.full(4096, 1.0 / 4096))
    cx.lf.sensor_update(cx.obs)
    held_to_lf(cx.lf.log_weights(), want, alts, n_amb, beams, "sensor_update")
    if g.name == "open":
        K = cx.lf.likelihood_table().size - 1
        assert (cx.lf.likelihood_field() == K).all()
        assert np.unique(want).size == 1                        # every end point reads K


# ---- 3. the global search under the likelihood field
def check_hits(cx, search, V, cells, xy, theta, stride, nms, max_hits):
    hits, st = search(max_hits)
    want = sg.hits_ref(cx.g, V, cells, stride, nms)
    assert st["n_hits"] == want.size and st["n_positions"] == cells.size and st["n_poses"] == V.size
    m = min(max_hits, want.size)
    assert len(hits) == m
    assert np.array_equal(hits["index"], want[:m])
    k, p = want[:m] // cells.size, want[:m] % cells.size
    assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
    assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p]))
    assert np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
    return hits, st, want


def fold(accs):
    """SQ4: ((+0.0 + acc_0) + acc_1) + ... in scan order"""
    total = np.zeros_like(accs[0])
    for a in accs:
        total = total + a
    return total


def test_global_search(cx):
    g, e = cx.g, cx.lf
    for stride in g.strides:
        cells, xy, theta, poses = sg.lattice(cx.mod, g, stride, N_HEAD)
        ref_cells, ref_xy = sg.lattice_ref(g, stride)
        assert np.array_equal(cells, ref_cells) and np.array_equal(bits(xy), bits(ref_xy))
        f = dict(stride_cells=stride, n_headings=N_HEAD)
        # the volume
        want, alts, n_amb, beams = sg.lf_statement(g, poses, cx.ang, cx.obs)
        _, st = e.global_search(cx.obs, max_hits=0, **f)
        assert st["n_positions"] == cells.size and st["n_poses"] == len(poses)
        held_to_lf(e.search_scores(), want, alts, n_amb, beams, f"search volume, stride {stride}")
        V = e.search_scores(N_HEAD)
        # the hits, for fewer and for more than there are candidates; the streamed search gives the same
        for nms in (0, 1):
            fn = dict(nms=nms, **f)
            n_cand = sg.hits_ref(g, V, cells, stride, nms).size
            assert n_cand >= 1
            for max_hits in (n_cand // 2, 65536):
                hits, st, want_hits = check_hits(cx, lambda mh: e.global_search(cx.obs, max_hits=mh, **fn), V, cells, xy, theta, stride, nms, max_hits)
                for G in (1, 2):
                    s_hits, s_st = e.global_search_streamed(cx.obs, max_hits=max_hits, slab_headings=G, **fn)
                    assert s_hits.tobytes() == hits.tobytes() and len(s_hits) == len(hits) and s_st["n_hits"] == st["n_hits"], (stride, nms, max_hits, G)
            if g.name == "open":
                # every score of a heading is equal (every end point reads K): ties come out in index order
                assert np.unique(V).size == 1
                if nms == 0:
                    assert np.array_equal(want_hits, np.arange(V.size))
            if g.name == "one_free":
                assert st["n_positions"] == 1
                order = np.lexsort((np.arange(N_HEAD), -V[:, 0]))
                if nms == 0:
                    assert np.array_equal(want_hits, order)
                else:
                    assert want_hits[0] == order[0]
        # a sequence of two scans joined by a displacement of a few cells; one scan at the anchor is the single search
        scans = np.stack([cx.earlier, cx.obs])
        sp = sg.scan_poses(cx.mod, g, cx.rel, stride, N_HEAD)
        ref = [sg.lf_statement(g, sp[s], cx.ang, scans[s]) for s in range(2)]
        assert all(sg.within_cap(r[2], r[3]) for r in ref)
        want = fold([r[0] for r in ref])
        _, st = e.global_search_sequence(scans, cx.rel, max_hits=0, **f)
        assert st["n_scans"] == 2 and st["n_poses"] == want.size
        got = e.search_scores()
        assert got.shape == want.shape and not np.isnan(got).any()
        for i in np.flatnonzero(bits(got) != bits(want)):
            i = int(i)
            assert any(i in r[1] for r in ref), (i, got[i], want[i])
            sums = {float(fold([np.float64(v) for v in pick])) for pick in itertools.product(*[r[1].get(i, [r[0][i]]) for r in ref])}
            assert got[i] in sums, (i, got[i], want[i], sorted(sums))
        Vs = e.search_scores(N_HEAD)
        check_hits(cx, lambda mh: e.global_search_sequence(scans, cx.rel, max_hits=mh, nms=1, **f), Vs, cells, xy, theta, stride, 1, 65536)
        h1, st1 = e.global_search(cx.obs, max_hits=4096, **f)
        v1 = e.search_scores()
        h2, st2 = e.global_search_sequence(cx.obs[None], np.zeros((1, 3)), max_hits=4096, **f)
        assert np.array_equal(bits(v1), bits(e.search_scores())) and h1.tobytes() == h2.tobytes() and st1["n_hits"] == st2["n_hits"]


# ---- 4. the global search under the beam model
def test_beam_search(cx):
    g, e = cx.g, cx.beam55
    grid = br.grid(cx.ang55, N_HEAD_BEAM)
    assert grid["M"] == 72
    L3 = {}
    for stride in g.strides:
        cells, xy, theta, _ = sg.lattice(cx.mod, g, stride, N_HEAD_BEAM)
        n_pos = cells.size
        S = br.table(cx.orc, cx.om, xy, grid["phi"])
        want = br.volume(cx.orc, cx.om, S, cx.odd55, N_HEAD_BEAM, grid["heading_step"])
        width = 1 if cx.P <= 255 else 2
        f = dict(stride_cells=stride, n_headings=N_HEAD_BEAM)
        for budget in (0, 256 * 72 * width):                    # one tile; tiles of 256 positions
            T, tiles = sg.tile_plan(n_pos, 72, cx.P, budget)
            _, st = e.global_search_beam(cx.odd55, max_hits=0, table_budget_bytes=budget, **f)
            assert st["n_positions"] == n_pos and st["n_poses"] == n_pos * N_HEAD_BEAM and st["used_beams"] == 55
            assert (st["grid_angles"], st["tile_positions"], st["n_tiles"]) == (72, T, tiles)
            if budget and n_pos > 256:
                assert tiles >= 2
            first, R = e.search_beam_table()
            assert first == (tiles - 1) * T and R.shape == (n_pos - first, 72)
            assert np.array_equal(R.astype(np.int64), S[first:])
            V = e.search_scores(N_HEAD_BEAM)
            assert not np.isnan(V).any() and np.array_equal(bits(V), bits(want))
            L3[(stride, budget)] = st["level3_rays"]
        assert L3[(stride, 0)] == L3[(stride, 256 * 72 * width)]
        print(f"{g.name}: beam search, stride {stride}: {n_pos} positions, level-3 rays {st['level3_rays']} of {S.size}")
        for nms in (0, 1):
            want_hits = br.hits(V, cells, stride, nms, g.W, g.H)
            assert want_hits.size >= 1
            for max_hits in (want_hits.size // 2, 65536):
                hits, st = e.global_search_beam(cx.odd55, max_hits=max_hits, nms=nms, **f)
                m = min(max_hits, want_hits.size)
                assert st["n_hits"] == want_hits.size and len(hits) == m and np.array_equal(hits["index"], want_hits[:m])
                k, p = want_hits[:m] // n_pos, want_hits[:m] % n_pos
                assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
                assert np.array_equal(bits(hits["pose"][:, :2]), bits(xy[p])) and np.array_equal(bits(hits["pose"][:, 2]), bits(theta[k]))
        if g.name == "one_free":
            assert n_pos == 1


# ---- 5. the refinements
def check_records(cx, e, r, V, fields):
    """best pose, mean and covariance against refine_ref.best / moments within refine_ref.tolerances at the geometry's
    resolution; the covariance seeds a cloud"""
    g = cx.g
    tol_mean, tol_cov, tol_s = rr.tolerances(g.resolution, **fields)
    for m, seed in enumerate(g.seeds):
        wb = rr.best(V[m], **fields)
        b, mean, cov, S = rr.moments(seed, g.resolution, V[m], **fields)
        assert int(r[m]["best_index"]) == wb
        assert np.array_equal(bits(r[m]["best"]), bits(b))
        assert np.array_equal(bits(r[m]["best_log_likelihood"]), bits(V[m, wb]))
        assert np.array_equal(bits(r[m]["seed_log_likelihood"]), bits(V[m, V.shape[1] // 2]))
        err = np.array([(np.abs(r[m]["mean"] - mean) / tol_mean).max(), (np.abs(r[m]["cov"] - cov) / tol_cov).max(),
                        abs(float(r[m]["weight_sum"]) - S) / tol_s])
        print(f"{g.name}: seed {m}: mean / cov / weight_sum error in tolerances: {err}")
        cx.worst = np.maximum(cx.worst, err)
        assert err.max() <= 1.0, (m, err)
        assert np.array_equal(r[m]["cov"], r[m]["cov"].T)
        e.init_particles_gaussian(r[m]["mean"], r[m]["cov"], 64)
        assert e.particle_count() == 64 and np.isfinite(e.get_particles()).all()


def test_refine_field(cx):
    g, e, F = cx.g, cx.lf, cx.g.window_fields
    win = np.concatenate([rr.window(s, g.resolution, **F) for s in g.seeds])
    want, alts, n_amb, beams = sg.lf_statement(g, win, cx.ang, cx.obs)
    r, st = e.refine_poses(g.seeds, cx.obs, **F)
    n_win = win.shape[0] // 3
    assert st["n_win"] == n_win and st["n_poses"] == 3 * n_win
    got = e.refine_scores()
    assert got.shape == (3, n_win)
    held_to_lf(got.ravel(), want, alts, n_amb, beams, "refine volume")
    check_records(cx, e, r, got, F)


def test_refine_beam(cx):
    g, e, F = cx.g, cx.beam, cx.g.window_fields
    win = np.concatenate([rr.window(s, g.resolution, **F) for s in g.seeds])
    want = rb.scores(cx.orc, cx.om, win, cx.ang, cx.odd).reshape(3, -1)
    r, st = e.refine_poses_beam(g.seeds, cx.odd, **F)
    assert st["n_win"] == want.shape[1] and st["rays"] == want.size * 61 and st["used_beams"] == 61
    print(f"{g.name}: beam refinement: level-3 rays {st['level3_rays']} of {st['rays']}")
    got = e.refine_scores()
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(bits(got), bits(want))
    check_records(cx, e, r, want, F)
    # a second, smaller window with the other step: half a cell on tiny, two cells elsewhere (the third seed's reaches well off the map)
    F2 = dict(half_xy=1, half_theta=1, step_xy_cells=0.5 if g.name == "tiny" else 2.0)
    win = np.concatenate([rr.window(s, g.resolution, **F2) for s in g.seeds])
    e.refine_poses_beam(g.seeds, cx.odd, **F2)
    assert np.array_equal(bits(e.refine_scores().ravel()), bits(rb.scores(cx.orc, cx.om, win, cx.ang, cx.odd)))


# ---- 7. read-only
@pytest.mark.parametrize("field", [False, True], ids=["beam", "field"])
def test_an_update_after_every_side_call_is_that_of_a_fresh_engine(cx, field):
    g = cx.g
    n = 2000
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=g.true_pose, sig=(2 * g.res, 2 * g.res, 0.2))
    scan = sg.scan_at(cx.orc, cx.om, cx.ang, g.true_pose)
    a, b = make_engine(cx.mod, g, cx.ang, n), make_engine(cx.mod, g, cx.ang, n)
    for e in (a, b):
        if field:
            e.set_likelihood_field(True)
        e.set_particles(cloud, np.full(n, 1.0 / n))
    stride = g.strides[0]
    f = dict(stride_cells=stride, n_headings=N_HEAD)
    a.expected_scans(g.query_poses)
    a.score_poses(g.query_poses, cx.odd)
    a.global_search_beam(cx.odd, max_hits=4, stride_cells=stride, n_headings=N_HEAD_BEAM)     # (61 beams 4.5 degrees apart: M = 80)
    a.refine_poses_beam(g.seeds, cx.odd, **g.window_fields)
    if field:
        a.global_search(cx.obs, max_hits=4, **f)
        a.global_search_sequence(np.stack([cx.earlier, cx.obs]), cx.rel, max_hits=4, **f)
        a.global_search_streamed(cx.obs, max_hits=4, slab_headings=2, **f)
        a.global_search_pruned(cx.obs, max_hits=4, block=4, first_pairs=3, **f)
        a.refine_poses(g.seeds, cx.obs, **g.window_fields)
    for e in (a, b):
        e.update((g.res, 0.0, 0.01), scan)
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))
    assert np.array_equal(a.resample_indices(), b.resample_indices())
    a.close()
    b.close()
