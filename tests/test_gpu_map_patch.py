"""mcl_update_map_region against mcl_set_map, no tolerance anywhere.  Per case two engines of one configuration
and seed: A is given set_map(m0) and the patch (or patches), B set_map(m0) and then set_map of the edited grid.  Every map-derived
table read back from the device is compared byte for byte -- the grid, the isotropic field and its nibble copy, the quadrant
fields, the free-cell list (mcl_get_map_table), the wedge fields, their ringed copies where held, the likelihood field where on --
and then what both compute from the same particles and scan, bit for bit."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1024
SEED = 7
RES_LDS, RES_RING = 0.05, 0.025            # 12 m of range: 240 px (the LDS windows) and 479 px (ringed fields in global memory)
ANGLES = np.linspace(-2.2, 2.2, 61).astype(np.float32)


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


def walled(W, H, inner=True):
    g = np.zeros((H, W), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    if inner:
        g[H // 5, W // 8:W // 2] = 100
        g[H // 3:H - H // 4, W - W // 6] = 100
        g[H - H // 6:H - H // 6 + 3, W // 10:W // 10 + W // 2] = 100
        g[H // 2:H // 2 + H // 10, W // 12:W // 12 + W // 10] = -1          # unknown space: neither stop nor free
    return g


def big():
    return walled(640, 600)


def small():
    return walled(90, 70, inner=False)


def applied(m0, edits):
    m = m0.copy()
    for x0, y0, c in edits:
        c = np.asarray(c, np.int8)
        m[y0:y0 + c.shape[0], x0:x0 + c.shape[1]] = c
    return m


def engines(engine_mod, m0, res, lf=False, **cfg):
    out = []
    for _ in range(2):
        e = engine_mod.Engine(max_particles=4096, seed=SEED, keep_ray_steps=1, **cfg)
        if lf:
            e.set_likelihood_field(True)
        e.set_map(m0, res, 0.0, 0.0)
        e.set_beam_angles(ANGLES)
        out.append(e)
    return out


def tables(engine_mod, e, ring, lf):
    t = {name: e.map_table(name) for name in engine_mod.MAP_TABLES}
    t["wedges"] = e.wedge_fields()
    if ring:
        t["ring"] = e.ring_fields()
    if lf:
        t["lf"] = e.likelihood_field()
    return t


def assert_same_tables(engine_mod, a, b, ring, lf, what):
    ta, tb = tables(engine_mod, a, ring, lf), tables(engine_mod, b, ring, lf)
    for name in ta:
        ga, gb = ta[name], tb[name]
        assert ga.shape == gb.shape and ga.dtype == gb.dtype, (what, name, ga.shape, gb.shape)
        if not np.array_equal(ga, gb):
            bad = np.argwhere(ga != gb)
            raise AssertionError(f"{what}: {name}: {bad.shape[0]} entries differ; first (index, patched, set_map): "
                                 f"{[(tuple(int(v) for v in i), int(ga[tuple(i)]), int(gb[tuple(i)])) for i in bad[:5]]}")
    return ta


def scan_and_cloud(m, res):
    rng = np.random.default_rng(3)
    H, W = m.shape
    p = np.empty((3, N))
    p[0] = rng.uniform(2, W - 2, N) * res
    p[1] = rng.uniform(2, H - 2, N) * res
    p[2] = rng.uniform(-np.pi, np.pi, N)
    scan = rng.uniform(0.5, 0.4 * min(W, H) * res, ANGLES.size).astype(np.float32)
    return p, scan


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_same_behaviour(a, b, m, res, lf, what):
    p, scan = scan_and_cloud(m, res)
    out = []
    for e in (a, b):
        r = {}
        e.set_particles(p, np.full(N, 1.0 / N))
        e.sensor_update(scan)
        r["log-weights"] = bits(e.log_weights())
        if not lf:
            r["ray steps"] = e.ray_steps().copy()
        e.update((0.05, 0.0, 0.01), scan)
        r["particles after an update"] = bits(e.get_particles())
        r["weights after an update"] = bits(e.get_weights())
        e.init_global(4096)
        r["init_global"] = bits(e.get_particles())
        if lf:
            hits, st = e.global_search_pruned(scan, max_hits=16, stride_cells=4, n_headings=8)
            r["pruned search hits"] = np.frombuffer(hits.tobytes(), np.uint8)
            r["pruned search counts"] = np.array([st["n_hits"], st["n_positions"], st["n_poses"], st["used_beams"]], np.int64)
        out.append(r)
    for name in out[0]:
        assert np.array_equal(out[0][name], out[1][name]), (what, name, int((out[0][name] != out[1][name]).sum()))
    assert np.isfinite(out[0]["log-weights"].view(np.float64)).any()


def run_case(engine_mod, m0, res, edits, lf=False, behaviour=True, what=""):
    """A: the patches; B: set_map of the final grid.  Returns (the statistics of every patch, A's tables)."""
    a, b = engines(engine_mod, m0, res, lf=lf)
    ring = a.max_range_px > 243
    stats = [a.update_map_region(c, x0, y0) for x0, y0, c in edits]
    m1 = applied(m0, edits)
    b.set_map(m1, res, 0.0, 0.0)
    t = assert_same_tables(engine_mod, a, b, ring, lf, what)
    assert np.array_equal(t["grid"].reshape(m1.shape), m1)
    assert stats[-1]["free_cells"] == t["free_cells"].size == int((m1 == 0).sum())
    if behaviour:
        assert_same_behaviour(a, b, m1, res, lf, what)
    a.close()
    b.close()
    return stats, t


CELL = [[100]]
EDITS = {
    "one stop set in open space": lambda m: [(320, 300, CELL)],
    "first cell": lambda m: [(0, 0, [[0]])],
    "last cell": lambda m: [(m.shape[1] - 1, m.shape[0] - 1, [[0]])],
    "a rectangle wider than 600 cells": lambda m: [(10, 250, np.where(np.arange(3 * 620).reshape(3, 620) % 7 < 3, 100, 0))],
}


@pytest.mark.parametrize("res", [RES_LDS, RES_RING], ids=["240px", "479px"])
@pytest.mark.parametrize("edit", list(EDITS))
def test_patch_equals_set_map(engine_mod, res, edit):
    m0 = big()
    stats, _ = run_case(engine_mod, m0, res, EDITS[edit](m0), what=f"{edit}, res {res}")
    assert stats[0]["changed_stop_cells"] > 0 and stats[0]["window"][2] >= stats[0]["window"][0]
    assert stats[0]["lf_window"][2] < stats[0]["lf_window"][0]               # the model is off


@pytest.mark.parametrize("res", [RES_LDS, RES_RING], ids=["240px", "479px"])
def test_a_stop_set_and_removed_again(engine_mod, res):
    m0 = big()
    stats, t = run_case(engine_mod, m0, res, [(320, 300, CELL), (320, 300, [[0]])], what="set, then removed")
    assert [s["changed_stop_cells"] for s in stats] == [1, 1]
    assert stats[0]["window"] == (321 - 254, 301 - 254, 321 + 254, 301 + 254)


def test_three_patches_against_one_set_map(engine_mod):
    m0 = big()
    edits = [(100, 100, np.full((5, 40), 100)), (90, 98, np.full((10, 30), 0)), (500, 400, np.full((2, 2), -1)), (0, 599, np.full((1, 640), 0))]
    run_case(engine_mod, m0, RES_LDS, edits, what="patches in a row")


@pytest.mark.parametrize("which", ["stop", "first cell", "last cell", "value only"])
def test_a_map_smaller_than_the_reach(engine_mod, which):
    m0 = small()
    edits = {"stop": [(40, 30, np.full((3, 10), 100))], "first cell": [(0, 0, [[0]])], "last cell": [(89, 69, [[0]])],
             "value only": [(40, 30, [[30, -1]])]}[which]
    stats, _ = run_case(engine_mod, m0, RES_LDS, edits, what=f"90 x 70, {which}")
    if which != "value only":
        assert stats[0]["window"] == (0, 0, 90, 70)


def test_value_change_without_a_stop_change(engine_mod):
    """0 -> 30 and -1 -> 0: the grid and the free list move, nothing else is written"""
    m0 = big()
    y, x = 600 // 2, 640 // 12
    assert m0[y, x] == -1 and m0[y, x - 1] == 0
    a, b = engines(engine_mod, m0, RES_LDS)
    before = tables(engine_mod, a, False, False)
    st = a.update_map_region([[30, 0]], x - 1, y)
    assert st["changed_cells"] == 2 and st["changed_stop_cells"] == 0 and st["window"][2] < st["window"][0]
    m1 = applied(m0, [(x - 1, y, [[30, 0]])])
    b.set_map(m1, RES_LDS, 0.0, 0.0)
    after = assert_same_tables(engine_mod, a, b, False, False, "value only")
    assert st["free_cells"] == after["free_cells"].size == before["free_cells"].size           # one cell left the list, one joined
    assert not np.array_equal(after["free_cells"], before["free_cells"]) and not np.array_equal(after["grid"], before["grid"])
    for name in before:
        if name not in ("grid", "free_cells"):
            assert np.array_equal(before[name], after[name]), name
    assert_same_behaviour(a, b, m1, RES_LDS, False, "value only")
    a.close()
    b.close()


def test_the_identical_rectangle_touches_nothing(engine_mod):
    m0 = big()
    e = engine_mod.Engine(max_particles=4096, seed=SEED)
    e.set_likelihood_field(True)
    e.set_map(m0, RES_LDS, 0.0, 0.0)
    e.set_beam_angles(ANGLES)
    _, scan = scan_and_cloud(m0, RES_LDS)
    e.global_search(scan, max_hits=4, stride_cells=8, n_headings=8)
    vol = e.search_scores().copy()
    st = e.update_map_region(m0[100:300, 50:400], 50, 100)
    assert st["changed_cells"] == 0 and st["changed_stop_cells"] == 0
    assert st["window"][2] < st["window"][0] and st["lf_window"][2] < st["lf_window"][0] and st["free_cells"] == int((m0 == 0).sum())
    assert np.array_equal(bits(e.search_scores()), bits(vol))                # the volume belongs to the map still held
    st = e.update_map_region([[30]], 320, 300)                                # a value alone: the map epoch moves
    assert st["changed_cells"] == 1
    with pytest.raises(engine_mod.EngineError) as ei:
        e.search_scores()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    e.close()


def test_row_stride_above_the_width(engine_mod):
    m0 = big()
    sheet = np.zeros((40, 100), np.int8)
    sheet[5:25, 10:13] = 100
    view = sheet[:, 3:60]                                                     # 57 cells of every 100
    assert view.strides == (100, 1)
    stats, _ = run_case(engine_mod, m0, RES_LDS, [(200, 300, view)], behaviour=False, what="row_stride > width")
    assert stats[0]["changed_stop_cells"] == 60


@pytest.mark.parametrize("where", ["interior", "at the map edge", "value only"])
def test_likelihood_field_on(engine_mod, where):
    m0 = big()
    edits = {"interior": [(320, 300, np.full((2, 3), 100))], "at the map edge": [(3, 2, np.full((4, 2), 100)), (637, 596, [[100]])],
             "value only": [(320, 300, [[30]])]}[where]
    stats, _ = run_case(engine_mod, m0, RES_LDS, edits, lf=True, what=f"likelihood field, {where}")
    K = engine_mod.host_likelihood_table(RES_LDS).size - 1
    reach = int(np.ceil(np.sqrt(K)))
    if where == "interior":
        assert stats[0]["lf_window"] == (320 - reach, 300 - reach, 322 + reach, 301 + reach)
    elif where == "at the map edge":
        assert stats[0]["lf_window"][:2] == (0, 0) and stats[1]["lf_window"][2:] == (639, 599)
    else:
        assert stats[0]["lf_window"][2] < stats[0]["lf_window"][0]


def test_the_patch_keeps_the_rule_of_the_last_set_map(engine_mod, monkeypatch):
    m0 = big()
    edit = (320, 300, np.full((3, 3), 100))
    m1 = applied(m0, [edit])
    monkeypatch.setenv("MCL_WEDGE_METRIC", "0")                               # read at mcl_set_map: the Euclidean rule
    a, b = engines(engine_mod, m0, RES_LDS)
    b.set_map(m1, RES_LDS, 0.0, 0.0)
    monkeypatch.delenv("MCL_WEDGE_METRIC")
    a.update_map_region(edit[2], edit[0], edit[1])
    t = assert_same_tables(engine_mod, a, b, False, False, "Euclidean rule kept")
    b.set_map(m1, RES_LDS, 0.0, 0.0)                                          # the tight rule
    tight = b.wedge_fields()
    win = t["wedges"][:, 301 - 254:301 + 254, 321 - 254:321 + 254] != tight[:, 301 - 254:301 + 254, 321 - 254:321 + 254]
    assert win.any()                                                          # the rules differ inside the window that was rebuilt
    a.close()
    b.close()


def test_refusals_change_nothing(engine_mod):
    m0 = small()
    e = engine_mod.Engine(max_particles=256)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.update_map_region(CELL, 3, 3)
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    with pytest.raises(engine_mod.EngineError) as ei:
        e.map_table("grid")
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    e.set_map(m0, RES_LDS, 0.0, 0.0)
    before = tables(engine_mod, e, False, False)
    for cells, x0, y0 in ((np.full((2, 2), 100), 89, 10), (np.full((2, 2), 100), 10, 69), (CELL, 90, 0), (CELL, 0, 70),
                          (np.zeros((0, 3), np.int8), 1, 1), (np.zeros((3, 0), np.int8), 1, 1), (CELL, 2 ** 32 - 1, 0)):
        with pytest.raises(engine_mod.EngineError) as ei:
            e.update_map_region(cells, x0, y0)
        assert ei.value.status == engine_mod.MCL_ERR_INVALID_ARG, (cells.shape if hasattr(cells, "shape") else cells, x0, y0)
    buf = np.full((4, 4), 100, np.int8)
    assert e.lib.mcl_update_map_region(e._h, None, 1, 1, 2, 2, 2, None) == engine_mod.MCL_ERR_INVALID_ARG
    assert e.lib.mcl_update_map_region(e._h, buf.ctypes.data, 1, 1, 4, 2, 3, None) == engine_mod.MCL_ERR_INVALID_ARG     # row_stride < width
    assert e.lib.mcl_update_map_region(None, buf.ctypes.data, 1, 1, 2, 2, 4, None) == engine_mod.MCL_ERR_INVALID_ARG
    need = np.zeros(1, np.uint64)
    assert e.lib.mcl_get_map_table(e._h, 99, None, 0, None) == engine_mod.MCL_ERR_INVALID_ARG
    assert e.lib.mcl_get_map_table(e._h, 0, buf.ctypes.data, 16, need.ctypes.data_as(engine_mod.C.POINTER(engine_mod.C.c_size_t))) == engine_mod.MCL_ERR_INVALID_ARG
    assert int(need[0]) == 90 * 70
    after = tables(engine_mod, e, False, False)
    for name in before:
        assert np.array_equal(before[name], after[name]), name
    assert e.update_map_region(np.zeros((2, 2)), 88, 68)["changed_cells"] == 3              # the last rectangle that fits: three wall cells cleared
    e.close()


def test_group_patch_against_group_set_map(engine_mod):
    m0 = big()
    edit = (320, 300, np.full((3, 5), 100))
    m1 = applied(m0, [edit])
    groups = []
    for _ in range(2):
        g = engine_mod.Group([0, 0], max_particles=N // 2, seed=SEED)
        g.set_map(m0, RES_LDS, 0.0, 0.0)
        g.set_beam_angles(ANGLES)
        groups.append(g)
    ga, gb = groups
    ga.update_map_region(edit[2], edit[0], edit[1])
    gb.set_map(m1, RES_LDS, 0.0, 0.0)
    for i in range(2):
        assert_same_tables(engine_mod, ga.engine(i), gb.engine(i), False, False, f"group, shard {i}")
    p, scan = scan_and_cloud(m1, RES_LDS)
    out = []
    for g in (ga, gb):
        g.set_particles(p, np.full(N, 1.0 / N))
        g.update((0.05, 0.0, 0.01), scan)
        out.append((bits(g.get_particles()), bits(g.get_weights())))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    with pytest.raises(engine_mod.EngineError):
        ga.update_map_region(edit[2], 638, 0)                                 # leaves the map: the group reports the engine's refusal
    ga.close()
    gb.close()
