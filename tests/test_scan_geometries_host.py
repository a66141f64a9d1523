"""The host half of the scan family of tests/scan_geometries.py, without a device: that `predict` -- the rules of
mcl_set_beam_angles and plan_sweep_form restated from their comments -- gives what the family's table says and flips at the exact
boundaries; that mcl_host_search_beam_grid gives the grid or the refusal `beam_grid` states for every member; and the conditions
tests/test_gpu_side_scan_geometries.py rests on, decided by the statements alone: few enough end points within lfield_ref.AMBIG of
a cell edge for LF4's cap to hide nothing, and scans with readings that count and readings that do not."""
import numpy as np
import pytest

import lfield_ref as lr
import refine_ref as rr
import scan_geometries as scg
import side_geometries as sg

N_HEAD = 5
LF_STRIDE = 3
WEDGE = 2.0 * np.pi / 16

# name: (B, quad_ok, beam_pad, beam_margin, ltd_cols, rec_ok, rec, M, refusal); None: the table leaves it open
TABLE = dict(
    hokuyo=(1081, True, 90, 96, 1280, True, True, 1440, None),
    turn360=(360, True, 0, 0, 384, False, False, 360, None),
    turn720_from_zero=(720, True, 0, 0, 768, False, False, 720, None),
    descending=(271, False, 0, 0, 320, False, False, None, scg.NO_ASCEND),
    repeated=(271, False, 0, 0, None, False, False, 360, scg.NO_EVEN),
    over_turn=(400, False, 0, 0, 448, False, False, 360, scg.NO_TURN),
    fine2701=(2701, True, 0, 0, 2752, False, False, 3600, None),
    rec1599=(1599, True, 119, 128, 1856, True, True, 1895, scg.NO_EVEN),
    rec1600=(1600, True, 119, 128, 1920, True, False, 1895, scg.NO_EVEN),
    pad_min=(25, True, 3, 8, 64, True, True, 33, scg.NO_EVEN),
    wedge13=(13, True, 0, 0, 64, False, False, 16, None),
    coarse30=(10, True, 0, 0, 64, False, False, 12, None),
    narrow_rear=(91, True, 45, 48, 192, True, True, 720, None),
    one=(1, True, 0, 0, 64, False, False, None, None),
    two=(2, True, 0, 0, 64, False, False, 11, scg.NO_EVEN),
    b16383=(16383, True, 0, 0, 16384, False, False, None, scg.NO_GRID),
    b16384=(16384, False, 0, 0, None, False, False, None, scg.NO_GRID),
    b65536=(65536, False, 0, 0, None, False, False, None, scg.NO_GRID),
)


@pytest.fixture(params=scg.NAMES)
def member(request):
    return request.param, scg.family()[request.param]


def test_the_family_is_what_the_table_says(orc):
    fam = scg.family()
    assert tuple(fam) == scg.NAMES == tuple(TABLE)
    assert np.array_equal(fam["hokuyo"], orc.beam_angles())
    assert np.array_equal(fam["descending"], orc.beam_angles(angle_step=4)[::-1])
    rep = fam["repeated"]
    assert rep[100] == rep[99] and np.array_equal(np.delete(rep, 100), np.delete(orc.beam_angles(angle_step=4), 100))
    for name, a in fam.items():
        assert a.dtype == np.float32 and not a.flags.writeable and np.isfinite(a).all()
    assert fam["narrow_rear"][0] == np.float32(2.0) and fam["turn720_from_zero"][0] == 0.0
    assert float(fam["turn720_from_zero"][-1]) > 2.0 * np.pi - 0.01             # angles up to 2 pi
    assert float(fam["over_turn"][-1]) - float(fam["over_turn"][0]) > 2.0 * np.pi
    assert all(np.array_equal(again, fam[n]) for n, again in scg._build().items())


def test_predict_gives_the_table(member):
    name, ang = member
    B, quad_ok, pad, margin, cols, rec_ok, rec, M, refusal = TABLE[name]
    p = scg.predict(ang)
    assert p["accepted"] and p["B"] == B == ang.size
    assert (p["quad_ok"], p["beam_pad"], p["beam_margin"], p["rec_ok"], p["rec"]) == (quad_ok, pad, margin, rec_ok, rec), p
    if cols is not None:
        assert p["ltd_cols"] == cols
    assert (p["M"], p["refusal"]) == (M, refusal)
    assert p["rec_room"] == (p["ltd_cols"] <= 1912)


def test_what_the_members_are_there_for():
    P = {n: scg.predict(a) for n, a in scg.family().items()}
    assert P["rec1599"]["rec_ok"] and P["rec1599"]["rec_room"] and P["rec1600"]["rec_ok"] and not P["rec1600"]["rec_room"]
    assert [n for n in scg.NAMES if P[n]["rec_ok"] and not P[n]["rec_room"]] == ["rec1600"]       # the one member REC lacks room for
    assert P["fine2701"]["per_wedge"] > 120.0 and 2.0 <= P["pad_min"]["per_wedge"] < 2.1
    assert abs(P["wedge13"]["per_wedge"] - 1.0) < 1e-6 and P["coarse30"]["per_wedge"] < 1.0
    assert P["turn360"]["M"] == 360 == P["turn360"]["B"] and P["turn720_from_zero"]["M"] == 720 == P["turn720_from_zero"]["B"]
    a = scg.family()["narrow_rear"].astype(np.float64)
    assert abs((a[-1] - a[0]) - np.pi / 4) < 1e-5
    # ... a 45-degree scan lies in at most three of a lane's sixteen wedges
    assert np.unique(np.floor(a / WEDGE)).size <= 3
    # wedge13's beams lie on wedge edges, to float rounding
    w = scg.family()["wedge13"].astype(np.float64) / WEDGE
    assert np.abs(w - np.round(w)).max() < 1e-6
    assert not scg.predict(np.zeros(0, np.float32))["accepted"] and not scg.predict(np.zeros(65537, np.float32))["accepted"]
    assert scg.predict(scg.family()["b65536"])["accepted"]


def test_predict_flips_at_the_exact_boundaries():
    deg, reg = scg.deg, scg.regular
    # 2 beams per wedge: float rounding decides which side 11.25 degrees itself falls on (a hair below, here: no pad); 11.2 degrees
    # lies above, 11.3 below
    p = scg.predict(reg(deg(-135.0), deg(11.25), 25))
    assert abs(p["per_wedge"] - 2.0) < 1e-6 and p["beam_pad"] == (int(np.ceil(p["per_wedge"] - 1e-9)) if p["per_wedge"] >= 2.0 else 0)
    p = scg.predict(reg(deg(-135.0), deg(11.2), 25))
    assert p["per_wedge"] > 2.0 and (p["beam_pad"], p["beam_margin"]) == (3, 8)
    assert scg.predict(reg(deg(-135.0), deg(11.3), 24))["beam_pad"] == 0
    # 120 beams per wedge: 0.1875 degrees itself falls on either side by rounding; 0.1876 lies below 120, 0.1874 above
    p = scg.predict(reg(deg(-135.0), deg(0.1875), 1441))
    assert abs(p["per_wedge"] - 120.0) < 1e-4 and p["beam_pad"] == (120 if p["per_wedge"] <= 120.0 else 0)
    p = scg.predict(reg(deg(-135.0), deg(0.1876), 1441))
    assert p["per_wedge"] < 120.0 and (p["beam_pad"], p["beam_margin"]) == (120, 128)
    p = scg.predict(reg(deg(-135.0), deg(0.1874), 1441))
    assert p["per_wedge"] > 120.0 and p["beam_pad"] == 0
    # the table's columns and REC's room
    cols = {B: scg.predict(reg(deg(-150.0), deg(0.19), B)) for B in (1599, 1600)}
    assert (cols[1599]["ltd_cols"], cols[1599]["rec"]) == (1856, True) and (cols[1600]["ltd_cols"], cols[1600]["rec"]) == (1920, False)
    assert 1856 <= scg.REC_MAX_COLS < 1920
    # the count limit
    assert scg.predict(reg(deg(-160.0), deg(0.0195), 16383))["quad_ok"] and not scg.predict(reg(deg(-160.0), deg(0.0195), 16384))["quad_ok"]
    # the span against a turn: quad_ok up to 2 pi - 1e-3, virtual beams up to a wedge less
    for span, quad_ok in ((2.0 * np.pi - 2e-3, True), (2.0 * np.pi - 0.5e-3, False)):
        a = np.linspace(-np.pi, -np.pi + span, 361).astype(np.float32)
        assert scg.predict(a)["quad_ok"] == quad_ok
    for span, padded in ((2.0 * np.pi - WEDGE - 2e-3, True), (2.0 * np.pi - WEDGE - 0.5e-3, False)):
        a = np.linspace(-np.pi, -np.pi + span, 361).astype(np.float32)
        assert (scg.predict(a)["beam_pad"] > 0) == padded
    # 2e-6 rad of irregularity: one beam 1.5e-6 off the grid keeps REC, 3e-6 off loses it (the pad stays: a quarter spacing is far)
    for off, rec_ok in ((1.5e-6, True), (3e-6, False)):
        a = scg.family()["narrow_rear"].copy()
        a[40] = np.float32(float(a[40]) + off)
        p = scg.predict(a)
        assert p["rec_ok"] == rec_ok and p["beam_pad"] == 45
    # the switches the tests set
    assert scg.predict(scg.family()["hokuyo"], no_beam_pad=True)["beam_margin"] == 0
    assert not scg.predict(scg.family()["hokuyo"], no_rec=True)["rec_ok"]


def test_planned_kernels_and_forms():
    P = {n: scg.predict(a) for n, a in scg.family().items()}
    assert scg.planned(P["fine2701"], 65536) == ("k_rays_sweep", scg.WHY_SWEEP_LDS)
    assert scg.planned(P["turn360"], 65536)[0] == "k_rays_sweep"
    assert scg.planned(P["coarse30"], 65536) == ("k_rays_skip", scg.WHY_SMALL)                    # fewer than 2^23 rays
    assert scg.planned(P["over_turn"], 65536) == ("k_rays_skip", scg.WHY_NO_WINDOWS)
    assert scg.planned(P["b16384"], 65536) == ("k_rays_skip", scg.WHY_NO_WINDOWS)
    assert all(scg.planned(p, 2000) == ("k_rays_skip", scg.WHY_SMALL) for p in P.values())
    assert scg.planned(P["descending"], 4096, forced_sweep=True) == (None, scg.WHY_NO_WINDOWS)
    assert scg.form(P["rec1599"]) == dict(global_fields=False, hybrid=False, turned_directions=True)
    assert scg.form(P["rec1600"]) == dict(global_fields=False, hybrid=False, turned_directions=False)
    assert scg.form(P["rec1599"], hybrid=True)["hybrid"] and not scg.form(P["rec1600"], hybrid=True)["hybrid"]
    assert scg.form(P["rec1600"], hybrid=True)["global_fields"]


def test_beam_grid_is_the_hosts(engine_mod, member):
    """mcl_host_search_beam_grid gives M, heading_step and max_dev, or refuses where the statement does"""
    name, ang = member
    for n_head in {1, 8, 72, scg.predict(ang)["M"] or 5}:
        want = scg.beam_grid(ang, n_head)
        if want["refusal"] is None:
            got = engine_mod.host_search_beam_grid(ang, n_head)
            assert (got["M"], got["heading_step"], got["delta"], got["max_dev"]) == (want["M"], want["heading_step"], want["delta"], want["max_dev"])
            assert got["max_dev"] <= 4e-6
        else:
            with pytest.raises(engine_mod.EngineError) as ei:
                engine_mod.host_search_beam_grid(ang, n_head)
            assert ei.value.status == engine_mod.MCL_ERR_INVALID_ARG
            if want["max_dev"] is not None:
                assert ei.value.max_dev == want["max_dev"]
    if name in ("turn360", "turn720_from_zero"):
        assert scg.beam_grid(ang, 72)["M"] == ang.size                              # B == M: a full turn


# ---- the ambiguity cap, from the statement alone
def lf_pose_sets(engine_mod, g):
    """name -> poses (n, 3): every set of poses tests/test_gpu_side_scan_geometries.py holds to tests/lfield_ref.py under LF4"""
    return {"lattice": sg.lattice(engine_mod, g, LF_STRIDE, N_HEAD)[3],
            "window": np.concatenate([rr.window(s, g.resolution, **g.window_fields) for s in scg.seeds(g)]),
            "query": g.query_poses, "particles": g.particles.T}


def lf_scan(orc, g, name):
    """the member's scan for the calls under the likelihood field: without the reading of 0, whose end point is the pose itself --
    the query poses and the refinement's windows lie on cell corners and edges on purpose"""
    return scg.scan_for(orc, g.oracle(orc), scg.family()[name], g.true_pose, seed=scg.PERTURB_SEED.get(name, 7), zero=False)


@pytest.mark.parametrize("name", scg.SIDE)
def test_ambiguous_beams_stay_within_the_cap(engine_mod, orc, name):
    g = sg.small()
    ang, obs = scg.family()[name], lf_scan(orc, g, name)
    for what, poses in lf_pose_sets(engine_mod, g).items():
        _, alts, n_amb, beams = sg.lf_statement(g, poses, ang, obs)
        print(f"{name}: {what}: {int(n_amb.sum())} ambiguous of {beams} beams")
        assert beams > 0 and sg.within_cap(n_amb, beams), (name, what, int(n_amb.sum()), beams)


# ---- useful scans
def test_the_scans_have_readings_that_count_and_readings_that_do_not(orc, member):
    """From the true pose of the 120 x 90 map no ray of the reference runs its full range (the map is shorter than the range), so a
    scan's misses are the readings scan_for writes in: wherever the set has the beams for them (24 and more) it has both."""
    name, ang = member
    g = sg.small()
    om = g.oracle(orc)
    obs = scg.scan_for(orc, om, ang, g.true_pose)
    assert obs.dtype == np.float32 and obs.shape == ang.shape
    used = lr.used_beams(ang, obs, g.max_range_m)[0].size
    rows = orc.obs_index(obs, om)
    assert used >= 1 and (rows[np.isfinite(obs)] < om.max_range_px).any()
    if ang.size >= 30:
        assert used == ang.size - 6                                                   # NaN, +-inf, negative, max range and beyond do not count
        assert np.isnan(obs[3]) and obs[23] == np.float32(g.max_range_m) and obs[29] > g.max_range_m and obs[31] == 0.0
    plain = sg.scan_at(orc, om, ang, g.true_pose)
    assert (plain > 0).all() and (plain < g.max_range_m).all()
