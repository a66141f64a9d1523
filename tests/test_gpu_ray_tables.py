"""The tables under the ray stage, read back from the device (mcl_get_wedge_fields, mcl_get_ring_fields, mcl_get_sweep_table) and
held to their CPU twins byte for byte / bit for bit, no tolerance anywhere:

* the wedge fields mcl_set_map builds (k_row_tables, then k_wedge_field_tight, or k_wedge_field under MCL_WEDGE_METRIC=0) against
  mcl_host_skip_field_wedge_tight / mcl_host_skip_field_wedge in the stored encoding -- the host functions whose validity
  tests/test_wedge_tight.py proves against a polygon brute force and a march -- on the ten geometries of tests/side_geometries.py,
  sibal1, a 300 x 300 crop of the Spielberg map, and two bands of the whole 2000 x 2000 map;
* the mirrored, ringed copies k_ring_field makes of them, every byte of the allocation (ring, row padding and tail included),
  against tests/ray_tables_ref.ring_ref;
* the per-scan fp64 table of k_build_ltd against ray_tables_ref.ltd_ref on the oracle's float log table.

Every expected side comes from the host library or numpy; nothing is regenerated from the device."""
import os

import numpy as np
import pytest

import ray_tables_ref as rt
import side_geometries as sg
from conftest import make_engine
from test_wedge_tight import _sub_grid

pytestmark = pytest.mark.gpu

K = 16
FAMILY = sg.NAMES + ("small",)
WEDGE_MAPS = FAMILY + ("sibal1", "spielberg_crop")
RULES = {"tight": "host_skip_field_wedge_tight", "euclid": "host_skip_field_wedge"}


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in list(os.environ):
        if k.startswith("MCL_"):
            monkeypatch.delenv(k)


def map_of(request, name):
    """(data, resolution, origin_x, origin_y) of a named map"""
    if name == "small":
        g = sg.small()
        return g.data, g.resolution, g.origin_x, g.origin_y
    if name in sg.NAMES:
        g = sg.family()[name]
        return g.data, g.resolution, g.origin_x, g.origin_y
    if name == "sibal1":
        m = request.getfixturevalue("sibal1")
        return m.data, m.resolution, m.origin_x, m.origin_y
    if name == "sibal1_479":                                 # the 0.025 m map of test_479_px_map_both_rules: 479 px of range
        m = request.getfixturevalue("sibal1")
        return np.kron(m.data, np.ones((2, 2), np.int8)).astype(np.int8), 0.025, m.origin_x, m.origin_y
    assert name == "spielberg_crop"
    sub, res = _sub_grid(request, "spielberg")
    return sub, res, 0.0, 0.0


_TWINS = {}


def twin(engine_mod, request, name, rule):
    """(K, Hp, Wp): the host twin of every wedge field of the map under `rule`, in the stored encoding (made once, left unchanged)"""
    if (name, rule) not in _TWINS:
        data = map_of(request, name)[0]
        f = np.stack([rt.encode(getattr(engine_mod, RULES[rule])(data, k)) for k in range(K)])
        f.setflags(write=False)
        _TWINS[(name, rule)] = f
    return _TWINS[(name, rule)]


def assert_fields(got, want, what):
    """got: (K, Hp, Wps) as read back, want: (K, Hp, Wp).  Per wedge, so that a failure names it."""
    Kk, Hp, Wp = want.shape
    assert got.dtype == np.uint8 and got.shape[:2] == (Kk, Hp) and got.shape[2] == (Wp + 7) // 8 * 8, (what, got.shape, want.shape)
    for k in range(Kk):
        if not np.array_equal(got[k, :, :Wp], want[k]):
            d = [(k,) + t for t in rt.first_diffs(got[k, :, :Wp], want[k])]
            raise AssertionError(f"{what}, wedge {k}: {int((got[k, :, :Wp] != want[k]).sum())} bytes differ; first (k, y, x, got, want): {d}")
    assert not got[:, :, Wp:].any(), f"{what}: the padding columns [Wp, Wps) must hold the memset's 0"


# ---- wedge fields, both rules
@pytest.mark.parametrize("name", WEDGE_MAPS)
def test_wedge_fields_equal_the_host_twins_under_both_rules(request, engine_mod, monkeypatch, name):
    data, res, ox, oy = map_of(request, name)
    e = engine_mod.Engine(max_particles=256)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.wedge_fields()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    e.set_map(data, res, ox, oy)
    tight = e.wedge_fields()
    monkeypatch.setenv("MCL_WEDGE_METRIC", "0")              # read at mcl_set_map
    e.set_map(data, res, ox, oy)
    euclid = e.wedge_fields()
    buf = np.empty(tight.size + 8, np.uint8)
    for n in (tight.size - 1, tight.size + 8, 0):
        assert e.lib.mcl_get_wedge_fields(e._h, buf.ctypes.data, n, None) == -1          # MCL_ERR_INVALID_ARG
    e.close()
    Wp = data.shape[1] + 1
    assert_fields(tight, twin(engine_mod, request, name, "tight"), f"{name}, tight rule")
    assert_fields(euclid, twin(engine_mod, request, name, "euclid"), f"{name}, Euclidean rule")
    # the two rules differ on every one of these maps (stop bytes are 255 under both), so neither half passes on the other's field
    assert ((tight[:, :, :Wp] == 255) == (euclid[:, :, :Wp] == 255)).all()
    assert (tight[:, :, :Wp] > euclid[:, :, :Wp]).any()
    if name == "fine":                                       # the only member with skips above 127 (up to 145): the cap at work
        assert max(int(engine_mod.host_skip_field_wedge_tight(data, k).max()) for k in range(K)) > 127
        assert (tight[:, :, :Wp] == 127).any()


@pytest.mark.parametrize("k", [0, 5])
def test_bench_map_at_its_real_size_two_bands(engine_mod, spielberg, k):
    """The whole 2000 x 2000 Spielberg map under the default rule; for r0 = 700 and 1000 the 32 rows of data rows r0 .. r0 + 31
    (padded rows r0 + 1 .. r0 + 32) against the host twin of the band [r0 - 256, r0 + 32 + 256) over the full width
    (tests/test_ray_tables_ref.py: a value depends only on stops within 255 cells).  Wedge 0 lies next to an axis, 5 next to a
    diagonal."""
    data = spielberg.data
    assert data.shape == (2000, 2000)
    e = engine_mod.Engine(max_particles=256)
    e.set_map(data, spielberg.resolution, spielberg.origin_x, spielberg.origin_y)
    got = e.wedge_fields()
    e.close()
    assert got.shape == (K, 2001, 2008)
    for r0 in (700, 1000):
        band = engine_mod.host_skip_field_wedge_tight(np.ascontiguousarray(data[r0 - 256:r0 + 32 + 256]), k)
        want = rt.encode(band[257:289])
        mid = got[k, r0 + 1:r0 + 33, :2001]
        assert np.array_equal(mid, want), (k, r0, int((mid != want).sum()), [(k, y + r0 + 1, x, g, w) for y, x, g, w in rt.first_diffs(mid, want)])
        assert not got[k, r0 + 1:r0 + 33, 2001:].any()
        assert int(band[257:289].max()) > 127 and (want == 255).any()


def test_a_map_after_a_map_leaves_nothing_behind(request, engine_mod):
    """wide, then narrow, then tiny on one engine (the buffers are dropped and reserved again): after each call the fields, padding
    columns included, are those of a fresh engine with that map alone -- and the host twin's."""
    e = engine_mod.Engine(max_particles=256)
    for name in ("wide", "narrow", "tiny"):
        data, res, ox, oy = map_of(request, name)
        e.set_map(data, res, ox, oy)
        got = e.wedge_fields()
        f = engine_mod.Engine(max_particles=256)
        f.set_map(data, res, ox, oy)
        fresh = f.wedge_fields()
        f.close()
        assert got.shape == fresh.shape
        assert np.array_equal(got, fresh), (name, [t for t in rt.first_diffs(got, fresh)])
        assert_fields(got, twin(engine_mod, request, name, "tight"), f"{name} after another map")
    e.close()


# ---- ring fields
@pytest.mark.parametrize("name,force", [("fine", False), ("small", True), ("narrow", True), ("wide", True), ("sibal1_479", False)])
def test_ring_fields_every_byte_of_the_allocation(request, engine_mod, monkeypatch, name, force):
    """fine (600 px) and the 479-px map take the global form by themselves; small, narrow and wide with MCL_SWEEP_GLOBAL=1 (read at
    mcl_create) -- narrow and wide put the 64-byte pitch rounding and the tail length at their extremes."""
    data, res, ox, oy = map_of(request, name)
    if force:
        monkeypatch.setenv("MCL_SWEEP_GLOBAL", "1")
    e = engine_mod.Engine(max_particles=256)
    e.set_map(data, res, ox, oy)
    P = e.max_range_px
    assert (P > 243) != force
    if name == "sibal1_479":
        assert P == 479
    H, W = data.shape
    layout = engine_mod.host_sweep_global_layout(W, H, P)
    assert layout["ok"]
    wf = e.wedge_fields()
    ring = e.ring_fields()
    assert e.lib.mcl_get_ring_fields(e._h, ring.ctypes.data, ring.size - 1) == -1        # MCL_ERR_INVALID_ARG
    e.close()
    assert_fields(wf, twin(engine_mod, request, name, "tight"), name)                  # (the 479-px map: here only)
    want = rt.ring_ref(wf[:, :, :W + 1], P, layout)
    assert ring.dtype == np.uint8 and ring.shape == want.shape == (layout["alloc"],)
    if not np.array_equal(ring, want):
        bad = np.flatnonzero(ring != want)
        d = [(int(i // layout["stride"]), int(i % layout["stride"] // layout["pitch"]), int(i % layout["pitch"]), int(ring[i]), int(want[i]))
             for i in bad[:5]]
        raise AssertionError(f"{name}: {bad.size} bytes differ; first (k, y, x, got, want): {d}")
    # the expected side is not vacuous: grid bytes that are no stops, mirrored differently per quadrant
    assert (want != 255).any() and (ring.reshape(K, -1)[0] != ring.reshape(K, -1)[8]).any()


def test_ring_fields_not_ready_in_the_lds_form(request, engine_mod):
    data, res, ox, oy = map_of(request, "small")
    e = engine_mod.Engine(max_particles=256)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.ring_fields()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    e.set_map(data, res, ox, oy)
    assert e.wedge_fields().shape == (K, data.shape[0] + 1, (data.shape[1] + 1 + 7) // 8 * 8)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.ring_fields()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    e.close()


# ---- sweep table
N_CLOUD = 2048


def beam_set(orc, which):
    if which == "b1081":
        return orc.beam_angles()
    if which == "b61":
        return sg.angles(orc, 61)
    a = np.sort(np.random.default_rng(40).uniform(-2.2, 2.2, 40)).astype(np.float32)          # unevenly spaced: no virtual beams
    assert np.all(np.diff(a) > 1e-3) and np.diff(a).max() > 4 * np.diff(a).min()
    return a


def geometry(name):
    return sg.small() if name == "small" else sg.family()[name]


def sweep_engine(engine_mod, g, ang):
    e = make_engine(engine_mod, g, ang, N_CLOUD, seed=5, ray_kernel=engine_mod.RAYS_SWEEP)
    p = sg.cloud_around(g, np.random.default_rng(12), N_CLOUD)
    e.set_particles(p, np.full(N_CLOUD, 1.0 / N_CLOUD))
    return e


def assert_table(orc, om, L, e, ang, scan, what):
    """the engine's table after a sensor_update with `scan` against ltd_ref, as uint64; returns (table, margin)"""
    P = om.max_range_px
    e.sensor_update(scan)
    assert e.ray_kernel_name() == "k_rays_sweep"
    tab, margin = e.sweep_table()
    assert tab.dtype == np.float64 and tab.shape[0] == P + 129 and tab.shape[1] % 64 == 0 and tab.shape[1] > ang.size + 2 * margin, what
    want = rt.ltd_ref(L, orc.obs_index(scan, om), ang.size, P, margin, tab.shape[1])
    gb, wb = tab.view(np.uint64), want.view(np.uint64)
    if not np.array_equal(gb, wb):
        d = [(r, c, tab[r, c], want[r, c]) for r, c in np.argwhere(gb != wb)[:5]]
        raise AssertionError(f"{what}: {int((gb != wb).sum())} entries differ; first (row, column, got, want): {d}")
    # the two properties nothing else states: the rows under "none left" repeat it, margins and the last row add exactly zero
    assert np.array_equal(gb[:127], np.broadcast_to(gb[127], (127, gb.shape[1]))) and not gb[-1].any()
    assert not gb[:, :margin].any() and not gb[:, margin + ang.size:].any()
    return tab, margin


@pytest.mark.parametrize("beams", ["b1081", "b61", "uneven40"])
@pytest.mark.parametrize("name", ["small", "coarse", "fine"])
def test_sweep_table_follows_the_scan_bit_for_bit(orc, engine_mod, name, beams):
    """small (239 px), coarse (48 px) and fine (600 px: the global form) x 1081 evenly spaced beams (virtual beams: a margin), the
    stock 61 and 40 unevenly spaced ones (no margin).  The scan holds NaN, +-inf, negative, zero and beyond-range readings."""
    g = geometry(name)
    om = g.oracle(orc)
    P = om.max_range_px
    assert P == {"small": 239, "coarse": 48, "fine": 600}[name]
    ang = beam_set(orc, beams)
    L = orc.eng_log_table(orc.sensor_table(P))
    e = sweep_engine(engine_mod, g, ang)
    with pytest.raises(engine_mod.EngineError) as ei:        # no ray stage has run yet
        e.sweep_table()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    scan = sg.odd_scan(sg.scan_at(orc, om, ang, g.true_pose))
    assert np.isnan(scan).any() and np.isinf(scan).any() and (scan < 0).any() and (scan == 0).any() and (scan > sg.MAX_RANGE).any()
    tab1, margin = assert_table(orc, om, L, e, ang, scan, f"{name}, {beams}, first scan")
    assert (margin > 0) == (beams != "uneven40")
    if beams == "b1081":
        assert margin >= 90                                  # a wedge of 22.5 degrees holds 90 beams a quarter of a degree apart
    buf = np.empty(tab1.size + 1, np.float64)
    assert e.lib.mcl_get_sweep_table(e._h, buf.ctypes.data, tab1.size + 1, None) == -1       # MCL_ERR_INVALID_ARG
    # a second scan on the same engine: the table follows it
    scan2 = sg.odd_scan(sg.scan_at(orc, om, ang, sg.mirrored_pose(g))[::-1].copy())
    assert not np.array_equal(orc.obs_index(scan2, om), orc.obs_index(scan, om))
    tab2, _ = assert_table(orc, om, L, e, ang, scan2, f"{name}, {beams}, second scan")
    assert not np.array_equal(tab1.view(np.uint64), tab2.view(np.uint64))
    e.close()


def test_sweep_table_after_fewer_beams_keeps_no_old_column(orc, engine_mod):
    """1081 beams, then the 61-beam set on the same engine: the table is dropped with the beams (NOT_READY until a ray stage has
    built it again) and the new one is the 61-beam table in every entry, zero columns included."""
    g = sg.small()
    om = g.oracle(orc)
    L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
    a1081, a61 = beam_set(orc, "b1081"), beam_set(orc, "b61")
    e = sweep_engine(engine_mod, g, a1081)
    tab1, _ = assert_table(orc, om, L, e, a1081, sg.odd_scan(sg.scan_at(orc, om, a1081, g.true_pose)), "1081 beams")
    e.set_beam_angles(a61)
    with pytest.raises(engine_mod.EngineError) as ei:
        e.sweep_table()
    assert ei.value.status == engine_mod.MCL_ERR_NOT_READY
    tab2, _ = assert_table(orc, om, L, e, a61, sg.odd_scan(sg.scan_at(orc, om, a61, g.true_pose)), "61 beams after 1081")
    assert tab2.shape[1] < tab1.shape[1]
    e.close()
