"""mcl_host_map_patch_plan against the host fields themselves: for an edit of a grid, every cell in which the
isotropic field, a quadrant field, a wedge field (wedges 0, 5, 10, 15, both rules) or the likelihood field of the edited grid
differs from that of the old grid lies inside the window the plan returns for the edit's stop-bit changes.  The fields come from
the existing mcl_host_skip_field* / mcl_host_likelihood_field functions; nothing here runs on a device."""
import math

import numpy as np
import pytest

WEDGES = (0, 5, 10, 15)
RES = 0.05
REACH = 254


def walled(W, H, inner=True):
    g = np.zeros((H, W), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    if inner:
        g[H // 5, W // 8:W // 2] = 100                       # a few inner walls, and a patch of unknown space
        g[H // 3:H - H // 4, W - W // 6] = 100
        g[H - H // 6:H - H // 6 + 3, W // 10:W // 10 + min(300, W // 2)] = 100
        g[H // 2:H // 2 + H // 10, W // 12:W // 12 + W // 10] = -1
    return g


def lf_reach_of(engine_mod):
    K = engine_mod.host_likelihood_table(RES).size - 1
    r = math.isqrt(K)
    return K, r if r * r >= K else r + 1


_FIELDS = {}


def fields_of(engine_mod, key, grid):
    """every host field of a grid, padded-grid fields under 'skip', the likelihood field under 'lf' (made once per grid)"""
    if key not in _FIELDS:
        f = {"iso": engine_mod.host_skip_field(grid)}
        for q in range(4):
            f[f"quadrant {q}"] = engine_mod.host_skip_field_dir(grid, q)
        for k in WEDGES:
            f[f"wedge {k} tight"] = engine_mod.host_skip_field_wedge_tight(grid, k)
            f[f"wedge {k} euclid"] = engine_mod.host_skip_field_wedge(grid, k)
        f["lf"] = engine_mod.host_likelihood_field(grid, RES)
        _FIELDS[key] = f
    return _FIELDS[key]


def stop_box(old, new):
    ys, xs = np.nonzero((old > 50) != (new > 50))
    assert ys.size, "the edit changes a stop bit"
    return int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())


def assert_inside(engine_mod, key_old, old, key_new, new):
    """returns (window, lf_window, cells changed per field)"""
    H, W = old.shape
    K, reach = lf_reach_of(engine_mod)
    win, lfw = engine_mod.host_map_patch_plan(W, H, stop_box(old, new), reach)
    fo, fn = fields_of(engine_mod, key_old, old), fields_of(engine_mod, key_new, new)
    changed = {}
    for name in fo:
        x0, y0, x1, y1 = lfw if name == "lf" else win
        diff = fo[name] != fn[name]
        changed[name] = int(diff.sum())
        outside = diff.copy()
        outside[y0:y1 + 1, x0:x1 + 1] = False
        assert not outside.any(), (name, win, lfw, [tuple(int(v) for v in t) for t in np.argwhere(outside)[:5]])
    assert changed["iso"] > 0 and changed["lf"] > 0
    return win, lfw, changed


def grids_600(engine_mod):
    m0 = walled(600, 560)
    cx, cy = 300, 290
    assert not (m0[cy - 40:cy + 40, cx - 40:cx + 40] > 50).any()           # open space around the centre
    mA = m0.copy()
    mA[cy, cx] = 100
    mC = m0.copy()
    y = 560 - 560 // 6
    assert (mC[y:y + 3, 60:360] == 100).all()
    mC[y:y + 3, 60:360] = 0
    return m0, mA, mC, (cx, cy)


def test_one_cell_set_in_open_space_has_an_interior_window(engine_mod):
    m0, mA, _, (cx, cy) = grids_600(engine_mod)
    win, lfw, changed = assert_inside(engine_mod, "m0", m0, "mA", mA)
    assert win == (cx + 1 - REACH, cy + 1 - REACH, cx + 1 + REACH, cy + 1 + REACH)
    assert win[0] > 0 and win[1] > 0 and win[2] < 600 and win[3] < 560           # interior on all four sides
    K, reach = lf_reach_of(engine_mod)
    assert lfw == (cx - reach, cy - reach, cx + reach, cy + reach)
    assert all(changed[f"quadrant {q}"] > 0 for q in range(4)) and all(changed[f"wedge {k} tight"] > 0 for k in WEDGES)


def test_the_same_cell_cleared_again(engine_mod):
    m0, mA, _, _ = grids_600(engine_mod)
    assert_inside(engine_mod, "mA", mA, "m0", m0)


def test_a_wall_of_3_by_300_removed(engine_mod):
    m0, _, mC, _ = grids_600(engine_mod)
    win, lfw, changed = assert_inside(engine_mod, "m0", m0, "mC", mC)
    assert win[2] - win[0] + 1 == min(360 + REACH, 600) - max(61 - REACH, 0) + 1
    assert changed["iso"] > 300 * 3


def test_a_map_smaller_than_the_reach_is_its_own_window(engine_mod):
    m0 = walled(90, 70, inner=False)
    m1 = m0.copy()
    m1[30:33, 40:50] = 100
    win, lfw, _ = assert_inside(engine_mod, "s0", m0, "s1", m1)
    assert win == (0, 0, 90, 70)                                             # the whole padded grid


@pytest.mark.parametrize("corner", ["first", "last"])
def test_edits_at_the_first_and_the_last_cell(engine_mod, corner):
    W, H = 300, 280
    m0 = walled(W, H)
    m1 = m0.copy()
    x, y = (0, 0) if corner == "first" else (W - 1, H - 1)
    m1[y, x] = 0                                                             # a gap in the border wall
    win, lfw, _ = assert_inside(engine_mod, "c0", m0, "c" + corner, m1)
    if corner == "first":
        assert win == (0, 0, 1 + REACH, 1 + REACH) and lfw[:2] == (0, 0)     # grid cell (0, 0) feeds padded row and column 0 too
    else:
        assert win == (W - REACH, H - REACH, W, H) and lfw[2:] == (W - 1, H - 1)


def test_the_plan_clips_and_refuses(engine_mod):
    plan = engine_mod.host_map_patch_plan
    assert plan(600, 560, (10, 20, 10, 20), 0) == ((0, 0, 11 + REACH, 21 + REACH), (0, 0, -1, -1))       # the model off: no field window
    assert plan(600, 560, (10, 20, 10, 20), 7)[1] == (3, 13, 17, 27)
    assert plan(600, 560, (-5, -5, 700, 700), 7) == ((0, 0, 600, 560), (0, 0, 599, 559))                  # clipped to the map
    assert plan(600, 560, (590, 550, 2 ** 31 - 1, 2 ** 31 - 1), 2 ** 31 - 1) == ((591 - REACH, 551 - REACH, 600, 560), (0, 0, 599, 559))
    assert plan(1, 1, (0, 0, 0, 0), 1) == ((0, 0, 1, 1), (0, 0, 0, 0))
    for box in ((600, 0, 610, 5), (0, 560, 5, 570), (-9, 3, -1, 4), (3, -9, 4, -1),                       # outside the map
                (11, 20, 10, 20), (10, 21, 10, 20)):                                                       # inverted
        with pytest.raises(engine_mod.EngineError) as ei:
            plan(600, 560, box, 7)
        assert ei.value.status == engine_mod.MCL_ERR_INVALID_ARG
    with pytest.raises(engine_mod.EngineError):
        plan(0, 560, (0, 0, 1, 1), 7)
    lib = engine_mod.load_library()
    assert lib.mcl_host_map_patch_plan(600, 560, None, 7, None, None) == engine_mod.MCL_ERR_INVALID_ARG
