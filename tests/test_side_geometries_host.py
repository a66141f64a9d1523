"""The host half of the geometry family of tests/side_geometries.py, without a device: the lattice, the likelihood field and its
table, the refinement window and records and the beam search's grid on every member against their numpy statements; and the
conditions tests/test_gpu_side_geometries.py rests on, decided by the statements alone -- that few enough beam end points lie
within lfield_ref.AMBIG of a cell edge for LF4's cap to hide nothing, and that the fixtures exercise what they are meant to."""
import numpy as np
import pytest

import beam_search_ref as br
import lfield_ref as lr
import refine_ref as rr
import side_geometries as sg

N_HEAD, N_HEAD_BEAM = 5, 8
REL = np.array([[-3.0, 1.0, 0.1], [0.0, 0.0, 0.0]])            # in cells (x, y) and radians: scaled by the resolution


@pytest.fixture(params=sg.NAMES)
def geo(request):
    return sg.family()[request.param]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def test_the_family_is_what_the_table_says():
    want = dict(narrow=(37, 301, 0.05, -1.0, -7.0), wide=(517, 23, 0.05, -12.0, -0.5), coarse=(64, 48, 0.25, -8.0, -6.0),
                fine=(150, 110, 0.02, -1.5, -1.1), spielberg_res=(120, 90, 0.05796, -3.37, 1.91), far_origin=(120, 90, 0.05, 4096.3, -8191.7),
                tiny=(9, 7, 0.05, 0.0, 0.0), open=(80, 60, 0.05, -2.0, -1.5), one_free=(40, 30, 0.05, -1.0, -0.75))
    fam = sg.family()
    assert tuple(fam) == sg.NAMES == tuple(want)
    for name, (W, H, res, ox, oy) in want.items():
        g = fam[name]
        assert (g.W, g.H, g.origin_x, g.origin_y, g.max_range_m) == (W, H, ox, oy, 12.0) and g.resolution == np.float32(res)
        assert g.resolution.dtype == np.float32
    assert not (fam["open"].data != 0).any()
    assert (fam["one_free"].data == 0).sum() == 1
    for name in ("narrow", "wide"):
        assert fam[name].W % 8 != 0 and fam[name].W % 2 == 1
    # the same grid twice: the generator is deterministic
    again = sg._build()
    assert all(np.array_equal(again[n].data, fam[n].data) for n in sg.NAMES)


def test_ranges_and_tables(orc, geo):
    """P and K as the issue's table has them"""
    P, K = geo.oracle(orc).max_range_px, lr.K_of(2.0, geo.resolution)
    # (fine: float32(0.02) lies below 0.02, so (2.0 / res)^2 lies above 10 000 and its ceiling is 10 001)
    want = dict(coarse=(48, 64), fine=(600, 10001)).get(geo.name)
    if want:
        assert (P, K) == want
    if geo.name == "fine":
        assert P > 255 and K >= 8192                            # 16-bit steps together with the table from global memory
    if geo.name == "coarse":
        assert P < 64 and 0.2 / geo.res < 1.0                   # one masked round of the wave march; sigma_hit below one cell


# ---- S1
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_lattice_is_s1(engine_mod, geo, stride):
    want_cells, want_xy = sg.lattice_ref(geo, stride)
    if want_cells.size == 0:
        cells, xy = engine_mod.host_search_lattice(geo.data, geo.resolution, geo.origin_x, geo.origin_y, stride_cells=stride)
        assert cells.size == 0
        return
    cells, xy = engine_mod.host_search_lattice(geo.data, geo.resolution, geo.origin_x, geo.origin_y, stride_cells=stride)
    assert cells.dtype == np.uint32 and np.array_equal(cells, want_cells)
    assert np.array_equal(bits(xy), bits(want_xy))
    assert np.all(np.diff(cells.astype(np.int64)) > 0)          # row-major order
    if stride in geo.strides:
        c, r = geo.true_cell
        assert r * geo.W + c in cells                           # the true cell is a position of the lattices in use
        assert np.array_equal(bits(xy[np.flatnonzero(cells == r * geo.W + c)[0]]), bits(geo.lattice_pose[:2]))


def test_lattice_sizes(engine_mod, geo):
    n = {s: sg.lattice_ref(geo, s)[0].size for s in (1, 2, 3)}
    assert n[3] % 64 != 0                                       # a last workgroup that is not full
    if geo.name == "tiny":
        assert 0 < n[3] < n[1] < 64
    if geo.name == "one_free":
        assert n == {1: 1, 2: 1, 3: 1}
    if geo.name in ("narrow", "wide"):
        assert min(geo.W, geo.H) // 3 <= 12                     # a handful of lattice columns (rows)


# ---- LF: field and table
def test_field_and_table_are_the_statement(engine_mod, geo):
    D = engine_mod.host_likelihood_field(geo.data, geo.resolution)
    want = lr.field(geo.data, geo.resolution)
    assert D.dtype == np.uint16 and D.shape == (geo.H, geo.W) and np.array_equal(D, want)
    Lf = engine_mod.host_likelihood_table(geo.resolution)
    want_lf = lr.table(geo.resolution)
    assert Lf.size == lr.K_of(2.0, geo.resolution) + 1
    assert np.array_equal(Lf.view(np.uint32), want_lf.view(np.uint32))
    if geo.name == "open":
        assert (D == Lf.size - 1).all()                         # no occupied cell: K everywhere


# ---- R1, R3, R4
def test_window_is_r1(engine_mod, geo):
    for seed in geo.seeds:
        got = engine_mod.host_refine_window(seed, geo.resolution, **geo.window_fields)
        want = rr.window(seed, geo.resolution, **geo.window_fields)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    # the third seed's window reaches off the map, the first's (but on the map smaller than a window) stays on it
    w = rr.window(geo.seeds[2], geo.resolution, **geo.window_fields)
    assert (w[:, 0] < geo.origin_x).any() and (w[:, 0] >= geo.origin_x).any()
    if geo.name == "tiny":
        ext = (2 * geo.window_fields["half_xy"]) * geo.window_fields["step_xy_cells"]
        assert ext >= geo.H                                     # a map smaller than one window


def window_volumes(orc, geo):
    """the statement's field-model volume of the three seeds' windows: ((3, n_win) scores, alternatives, ambiguous beams, beams)"""
    if "window_volumes" not in geo.memo:
        ang = sg.angles(orc, 61)
        obs = geo.scan(orc, ang)
        win = np.concatenate([rr.window(s, geo.resolution, **geo.window_fields) for s in geo.seeds])
        want, alts, n_amb, beams = sg.lf_statement(geo, win, ang, obs)
        geo.memo["window_volumes"] = (want.reshape(3, -1), alts, n_amb, beams)
    return geo.memo["window_volumes"]


def test_records_are_r3_r4(engine_mod, orc, geo):
    """mcl_host_refine_reduce against refine_ref.best / moments within refine_ref.tolerances at the geometry's resolution"""
    V = window_volumes(orc, geo)[0]
    tol_mean, tol_cov, tol_s = rr.tolerances(geo.resolution, **geo.window_fields)
    worst = np.zeros(3)
    for m, seed in enumerate(geo.seeds):
        h = engine_mod.host_refine_reduce(seed, geo.resolution, V[m], **geo.window_fields)
        b, mean, cov, S = rr.moments(seed, geo.resolution, V[m], **geo.window_fields)
        assert int(h["best_index"]) == rr.best(V[m], **geo.window_fields)
        assert np.array_equal(bits(h["best"]), bits(b))
        err = np.array([(np.abs(h["mean"] - mean) / tol_mean).max(), (np.abs(h["cov"] - cov) / tol_cov).max(), abs(float(h["weight_sum"]) - S) / tol_s])
        worst = np.maximum(worst, err)
    print(geo.name, "host records, mean / cov / weight_sum error in tolerances:", worst)
    assert worst.max() <= 1.0


# ---- B1, B5
def test_beam_grid_and_tile_plan(engine_mod, orc, geo):
    ang = sg.even_angles(orc, 55)
    got, want = engine_mod.host_search_beam_grid(ang, N_HEAD_BEAM), br.grid(ang, N_HEAD_BEAM)
    assert got["M"] == want["M"] == 72 and got["heading_step"] == want["heading_step"] == 9
    assert got["delta"] == want["delta"] and got["max_dev"] == want["max_dev"] and np.array_equal(bits(got["phi"]), bits(want["phi"]))
    P = geo.oracle(orc).max_range_px
    width = 1 if P <= 255 else 2
    for stride in geo.strides:
        n_pos = sg.lattice_ref(geo, stride)[0].size
        T, tiles = sg.tile_plan(n_pos, 72, P)
        assert tiles == 1 and T == -(-n_pos // 256) * 256
        T, tiles = sg.tile_plan(n_pos, 72, P, 256 * 72 * width)
        assert T == 256 and tiles == -(-n_pos // 256)
    if geo.name not in ("tiny", "one_free"):
        assert sg.tile_plan(sg.lattice_ref(geo, geo.strides[0])[0].size, 72, P, 256 * 72 * width)[1] >= 2


# ---- the ambiguity cap, from the statement alone
def pose_sets(engine_mod, orc, geo):
    """name -> (poses (n, 3), scan): every set of poses the GPU tests hold to tests/lfield_ref.py under LF4's ambiguity rule"""
    ang = sg.angles(orc, 61)
    obs = geo.scan(orc, ang)
    sets = {}
    for stride in geo.strides:
        sets[f"lattice, stride {stride}"] = (sg.lattice(engine_mod, geo, stride, N_HEAD)[3], obs)
    stride = geo.strides[0]
    rel = REL * np.array([geo.res, geo.res, 1.0])
    sp = sg.scan_poses(engine_mod, geo, rel, stride, N_HEAD)
    earlier = sg.perturbed_scan(orc, geo.oracle(orc), ang, sg.compose(geo.true_pose, rel[0]), seed=geo.perturb_seed + 1)
    sets["sequence, earlier scan"] = (sp[0], earlier)
    sets["sequence, anchor scan"] = (sp[1], obs)
    sets["window"] = (np.concatenate([rr.window(s, geo.resolution, **geo.window_fields) for s in geo.seeds]), obs)
    sets["query"] = (geo.query_poses, obs)
    sets["particles"] = (geo.particles.T, obs)
    return sets


def test_ambiguous_beams_stay_within_the_cap(engine_mod, orc, geo):
    for name, (poses, obs) in pose_sets(engine_mod, orc, geo).items():
        _, alts, n_amb, beams = sg.lf_statement(geo, poses, sg.angles(orc, 61), obs)
        print(f"{geo.name}: {name}: {int(n_amb.sum())} ambiguous of {beams} beams")
        assert beams > 0 and sg.within_cap(n_amb, beams), (geo.name, name, int(n_amb.sum()), beams)


# ---- a useful fixture
def test_the_fixture_is_useful(engine_mod, orc, geo):
    om = geo.oracle(orc)
    P = om.max_range_px
    ang = sg.angles(orc, 61)
    q = geo.query_poses
    assert q.shape == (64, 3) and np.isfinite(q).all() and q[6, 2] == np.pi
    res = geo.res
    cx, cy = (q[:, 0] - geo.origin_x) / res, (q[:, 1] - geo.origin_y) / res
    assert abs(cx[1] - round(cx[1])) < 1e-6 and abs(cy[1] - round(cy[1])) < 1e-6          # the corner
    assert abs(cx[2] - round(cx[2])) < 1e-6 and abs(cy[3] - round(cy[3])) < 1e-6          # the two edges
    assert cx[5] < 0.0                                                                       # off the map
    col, row = int(np.floor(cx[0])), int(np.floor(cy[0]))
    assert (col, row) == geo.true_cell and geo.data[row, col] == 0
    assert min(cx[0] - col, col + 1 - cx[0], cy[0] - row, row + 1 - cy[0]) > 0.05          # the true pose: off the cell's edges
    a = (q[:, 2][:, None] + ang.astype(np.float64)[None, :]).ravel()
    steps = orc.cast_many(om, np.repeat(q[:, 0], ang.size), np.repeat(q[:, 1], ang.size), a)[1]
    # the reference's ray ends where it leaves the map (at that step, not at P): a miss needs P free cells in a line inside the map
    can_miss = max(geo.W, geo.H) > P
    if geo.name == "open":
        assert (steps < P).any()                                # nothing is hit: a ray ends at the map's border
        assert can_miss is False
    elif geo.name == "one_free":
        assert (steps < P).all() and (steps == 0).any()
    else:
        assert (steps == 0).any() and ((steps > 0) & (steps < P)).any()
        assert (steps == P).any() == can_miss, (geo.name, P)
        assert can_miss == (geo.name in ("narrow", "wide", "coarse"))
        obs = geo.scan(orc, ang)
        assert lr.used_beams(ang, obs, geo.max_range_m)[0].size >= 20                       # a scan that sees walls
        if geo.name == "fine":
            assert P > 255 > steps.max()                        # 16-bit entries by P; the map itself is shorter than 256 cells


# ---- the arithmetic the ambiguity band rests on
def test_cell_coordinates_stay_far_inside_the_ambiguity_band(orc, geo):
    """DESIGN.md §4.10 puts the device's end points "within ~1e-12 cell of the real value" and the tests' band at 1e-6 cell.  The
    device's arithmetic -- lf_cell_coord, the host's beam pairs, the two fmas of lf_beam_value -- is restated here in exact
    rationals (an fma is one rounding of the exact value) for the 64 query poses and every used beam, and compared, like the
    numpy statement's end point, with the real value (x + r cos(theta + a) - origin) / res.  The real value is formed in exact
    rationals from fp64 cosines and one fp64 add of the angles, which puts it within about 2e-16 (r / res + 1) cell of the
    truth: 2e-13 cell at 600 cells of range.  The rule of LF4 is sound iff both deviations together stay inside the band: then
    whenever the device and the statement disagree on a cell, the statement lists the end point as ambiguous.  The pose's own
    coordinate takes three roundings (the difference, 1 / res, the product): at most 4 * 2^-53 of its value.  (The host's sine and
    cosine stand in for the device's, an ulp or two apart: 1e-16 of the beam's length in cells.)"""
    from fractions import Fraction as Fr
    ang = sg.angles(orc, 61)
    a, r = lr.used_beams(ang, geo.scan(orc, ang), geo.max_range_m)
    res = geo.res
    inv_res = 1.0 / res
    u, v = r * np.cos(a) * inv_res, r * np.sin(a) * inv_res                  # the host's beam pairs (lf_used_beams)
    worst = dict(pose=0.0, device=0.0, statement=0.0)
    for x, y, th in geo.query_poses:
        s, c = np.sin(th), np.cos(th)
        for p, o, rot in ((x, geo.origin_x, (c, -s)), (y, geo.origin_y, (s, c))):
            cell = (p - o) * inv_res                                         # lf_cell_coord
            exact = (Fr(p) - Fr(o)) / Fr(res)
            assert abs(Fr(cell) - exact) <= 4 * Fr(2) ** -53 * abs(exact)
            worst["pose"] = max(worst["pose"], float(abs(Fr(cell) - exact)))
            trig = np.cos(th + a) if rot[0] is c else np.sin(th + a)
            stated = (p + r * trig - o) / res                                # tests/lfield_ref.py
            for j in range(a.size):
                inner = float(Fr(rot[1]) * Fr(v[j]) + Fr(cell))              # fma(-s, b.y, px) / fma(c, b.y, py)
                dev = float(Fr(rot[0]) * Fr(u[j]) + Fr(inner))               # fma(c, b.x, .) / fma(s, b.x, .)
                real = (Fr(p) + Fr(r[j]) * Fr(trig[j]) - Fr(o)) / Fr(res)
                worst["device"] = max(worst["device"], float(abs(Fr(dev) - real)))
                worst["statement"] = max(worst["statement"], float(abs(Fr(stated[j]) - real)))
    print(f"{geo.name}: worst deviation in cells: pose coordinate {worst['pose']:.2e}, device end point {worst['device']:.2e}, "
          f"statement end point {worst['statement']:.2e}")
    assert worst["device"] + worst["statement"] < lr.AMBIG
