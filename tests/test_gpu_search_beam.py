"""The global search under the beam model on the GPU (mcl_global_search_beam, DESIGN.md §4.17, rules B1-B6 of
include/mcl_hip_engine.h): the ray table and the score volume against the numpy statement tests/beam_search_ref.py bit for bit,
for every entry width, tile plan and march level; the hits against S5 restated; that it finds a known pose; that the sensor
model in force does not matter; the refusals; that an engine which searches runs the same updates as one that never does; and
how far the table is from mcl_query_scans, whose float beam angles sit off the grid."""
import numpy as np
import pytest

import beam_search_ref as br
from conftest import make_engine, tracking_cloud
from side_geometries import odd_scan

pytestmark = pytest.mark.gpu

OX, OY = -3.0, -2.25
MAX_RANGE = 12.0
W, H = 120, 90


class SmallMap:
    """120 x 90 cells: an outer wall with two gaps (beams leave the map there), interior walls, a pillar, a post of one cell (on
    the lattice of stride 3, whose position count is then no multiple of 64), unknown cells.  At 0.05 m MAX_RANGE_PX is 240
    (8-bit table entries), at 0.025 m 479 (16-bit)."""

    def __init__(self, resolution=0.05):
        g = np.zeros((H, W), np.int8)
        g[0, :] = g[-1, :] = 100
        g[:, 0] = g[:, -1] = 100
        g[0, 30:40] = 0
        g[40:50, -1] = 0
        g[30, 20:70] = 100
        g[30:75, 85] = 100
        g[55:60, 40:45] = 100
        g[64, 64] = 100
        g[60:80, 5:15] = -1
        g[10:14, 100:110] = -1
        self.data, self.resolution, self.origin_x, self.origin_y = g, np.float32(resolution), OX, OY


def angles(orc, B):
    """B beams of the Hokuyo's 1081, evenly spaced over its 270 degrees (B = 1: the first)"""
    full = orc.beam_angles()
    return full[::1080 // (B - 1)].copy() if B > 1 else full[:1].copy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Case:
    """a map, a scan geometry and a lattice with the numpy statement of its table (computed once, shared, left unchanged)"""
    _cache = {}

    def __init__(self, orc, engine_mod, res, B, stride, n_head):
        self.m = SmallMap(res)
        self.om = orc.OracleMap(self.m.data, self.m.resolution, OX, OY)
        self.ang = angles(orc, B)
        self.stride, self.n_head = stride, n_head
        self.cells, self.xy = engine_mod.host_search_lattice(self.m.data, self.m.resolution, OX, OY, stride_cells=stride)
        self.theta = engine_mod.host_search_headings(n_headings=n_head)
        self.g = br.grid(self.ang, n_head)
        key = (res, B, stride, self.g["M"])
        if key not in Case._cache:
            S = br.table(orc, self.om, self.xy, self.g["phi"])
            S.setflags(write=False)
            Case._cache[key] = S
        self.S = Case._cache[key]
        pose = (OX + 25.5 * float(self.m.resolution), OY + 15.5 * float(self.m.resolution), 0.4)
        a = pose[2] + self.ang.astype(np.float64)
        self.scan = orc.cast_many(self.om, np.full(a.size, pose[0]), np.full(a.size, pose[1]), a)[0].astype(np.float32)
        self.orc = orc

    def volume(self, obs, beam_stride=1):
        return br.volume(self.orc, self.om, self.S, obs, self.n_head, self.g["heading_step"], beam_stride)

    def engine(self, engine_mod, n=64, **cfg):
        return make_engine(engine_mod, self.m, self.ang, n, **cfg)


def check(c, e, obs, beam_stride=1, **kw):
    """one search: the stats, the last tile's table and the volume against the statement"""
    hits, st = e.global_search_beam(obs, stride_cells=c.stride, n_headings=c.n_head, beam_stride=beam_stride, **kw)
    n_pos = c.cells.size
    assert st["n_positions"] == n_pos and st["n_poses"] == n_pos * c.n_head
    assert st["used_beams"] == -(-c.ang.size // beam_stride)
    assert st["grid_angles"] == c.g["M"] and st["tile_positions"] % 256 == 0
    assert st["n_tiles"] == -(-n_pos // st["tile_positions"])
    first, R = e.search_beam_table()
    assert first == (st["n_tiles"] - 1) * st["tile_positions"] and R.shape == (n_pos - first, c.g["M"])
    assert np.array_equal(R, c.S[first:])
    V = e.search_scores(c.n_head)
    want = c.volume(obs, beam_stride)
    assert not np.isnan(V).any() and not (bits(V) == bits(np.float64(-0.0))).any()
    assert np.array_equal(bits(V), bits(want))
    return hits, st, V


# ---- 1. table and volume are the statement, bit for bit
@pytest.mark.parametrize("n_head", [72, 8, 1])
def test_55_beams(engine_mod, orc, n_head):
    c = Case(orc, engine_mod, 0.05, 55, 3, n_head)
    assert c.cells.size > 256 and c.cells.size % 64 != 0 and c.g["M"] == 72
    _, st, V = check(c, c.engine(engine_mod), c.scan, max_hits=0)
    assert st["n_tiles"] == 1 and np.unique(V).size > 100
    # level 3 is the guard's share: at most the 8 of 72 grid angles whose sine or cosine is +-0.5 (every second sample of such a
    # ray from a cell centre lies on a cell edge) and, elsewhere, the chance of a sample within 2^-30 cell of an edge: below 1 %
    assert st["level3_rays"] <= c.S.size * 8 // 72 + c.S.size // 100


def test_1081_beams_wrap(engine_mod, orc):
    c = Case(orc, engine_mod, 0.05, 1081, 8, 72)
    assert c.g["M"] == 1440 and c.g["heading_step"] == 20 and 18 * 20 + 1080 >= 1440      # k s + j wraps from k = 18 on
    _, st, _ = check(c, c.engine(engine_mod), c.scan, max_hits=0)
    assert st["level3_rays"] <= c.S.size * 8 // 1440 + c.S.size // 100      # (as above: 8 of 1440 angles)


def test_one_beam(engine_mod, orc):
    c = Case(orc, engine_mod, 0.05, 1, 3, 8)
    assert c.g["M"] == 8 and c.g["heading_step"] == 1
    check(c, c.engine(engine_mod), c.scan, max_hits=0)


def test_beam_stride_and_odd_readings(engine_mod, orc):
    c = Case(orc, engine_mod, 0.05, 55, 3, 72)
    obs = odd_scan(c.scan)
    check(c, c.engine(engine_mod), obs, beam_stride=3, max_hits=0)
    check(c, c.engine(engine_mod), obs, beam_stride=1, max_hits=0)     # (every odd reading is a used beam here)
    check(c, c.engine(engine_mod), obs, beam_stride=100, max_hits=0)   # beam 0 alone, a stride beyond M


def test_16_bit_entries(engine_mod, orc):
    c = Case(orc, engine_mod, 0.025, 55, 4, 8)
    assert c.om.max_range_px == 479                                    # (int)(12 / (double)0.025f), above 255: two bytes per entry
    _, st, _ = check(c, c.engine(engine_mod), c.scan, max_hits=0)
    # two bytes per entry: the same budget holds half the positions
    _, st2, _ = check(c, c.engine(engine_mod), c.scan, max_hits=0, table_budget_bytes=256 * 72 * 2)
    assert st2["tile_positions"] == 256 and st2["n_tiles"] >= 3


# ---- 2. tiles
def test_tiles(engine_mod, orc):
    c = Case(orc, engine_mod, 0.05, 55, 3, 72)
    e = c.engine(engine_mod)
    obs = odd_scan(c.scan)
    one, st1, V1 = check(c, e, obs, max_hits=64)
    assert st1["n_tiles"] == 1
    for budget, T in ((256 * 72 + 71, 256), (512 * 72, 512)):
        many, st, V = check(c, e, obs, max_hits=64, table_budget_bytes=budget)
        assert st["tile_positions"] == T and st["n_tiles"] >= 3 and c.cells.size % T != 0
        assert np.array_equal(bits(V), bits(V1))
        assert st["n_hits"] == st1["n_hits"] and many.tobytes() == one.tobytes()
        assert st["level3_rays"] == st1["level3_rays"]


# ---- 3. the literal march alone gives the same table
def test_forced_exact_march(engine_mod, orc):
    c = Case(orc, engine_mod, 0.05, 55, 3, 8)
    _, st, V = check(c, c.engine(engine_mod), c.scan, max_hits=0)
    _, stx, Vx = check(c, c.engine(engine_mod, debug_force_exact=1), c.scan, max_hits=0)
    assert stx["level3_rays"] == c.cells.size * 72 > st["level3_rays"]
    assert np.array_equal(bits(V), bits(Vx))
    # ... in tiles too: the list of each tile is filled and overrun
    _, stt, _ = check(c, c.engine(engine_mod, debug_force_exact=1), c.scan, max_hits=0, table_budget_bytes=256 * 72)
    assert stt["level3_rays"] == c.cells.size * 72 and stt["n_tiles"] >= 3


# ---- 4. the hits are S5
@pytest.mark.parametrize("nms", [0, 1])
def test_hits_are_s5(engine_mod, orc, nms):
    c = Case(orc, engine_mod, 0.05, 55, 3, 8)
    e = c.engine(engine_mod)
    hits, st, V = check(c, e, odd_scan(c.scan), max_hits=4096, nms=nms)
    want = br.hits(V, c.cells, c.stride, nms, W, H)
    assert want.size > 5 and st["n_hits"] == want.size
    m = min(4096, want.size)
    assert len(hits) == m and np.array_equal(hits["index"], want[:m])
    k, p = want[:m] // c.cells.size, want[:m] % c.cells.size
    assert np.array_equal(bits(hits["log_likelihood"]), bits(V[k, p]))
    assert np.array_equal(bits(hits["pose"][:, :2]), bits(c.xy[p]))
    assert np.array_equal(bits(hits["pose"][:, 2]), bits(c.theta[k]))
    none, st0 = e.global_search_beam(odd_scan(c.scan), max_hits=0, stride_cells=c.stride, n_headings=c.n_head, nms=nms)
    assert len(none) == 0 and st0["n_hits"] == want.size               # max_hits 0: still counted


# ---- 5. it localises
def test_known_pose_ranks_first(engine_mod, orc):
    m = SmallMap()
    om = orc.OracleMap(m.data, m.resolution, OX, OY)
    ang = angles(orc, 55)
    cells, xy = engine_mod.host_search_lattice(m.data, m.resolution, OX, OY, stride_cells=2)
    theta = engine_mod.host_search_headings(n_headings=72)
    p, k = int(np.flatnonzero(cells == 15 * W + 25)[0]), 50          # the lattice cell (col 25, row 15): free, in the asymmetric lower left
    a = theta[k] + ang.astype(np.float64)
    obs = orc.cast_many(om, np.full(a.size, xy[p, 0]), np.full(a.size, xy[p, 1]), a)[0].astype(np.float32)
    e = make_engine(engine_mod, m, ang, 64)
    hits, st = e.global_search_beam(obs, max_hits=8, stride_cells=2, n_headings=72)
    assert st["n_hits"] >= 1 and hits[0]["index"] == k * cells.size + p
    assert np.array_equal(bits(hits[0]["pose"]), bits([xy[p, 0], xy[p, 1], theta[k]]))
    # ... and the hits seed a cloud, as the likelihood-field search's do
    counts = engine_mod.seed_counts(hits["log_likelihood"], 64)
    e.init_particles_mixture(hits["pose"], np.diag([0.01, 0.01, 0.01]), counts)
    assert e.particle_count() == 64


# ---- 6. model and mode
def expect(engine_mod, status, fn, *args, **kw):
    with pytest.raises(engine_mod.EngineError) as ei:
        fn(*args, **kw)
    assert ei.value.status == status, str(ei.value)
    return str(ei.value)


def test_the_sensor_model_in_force_does_not_matter(engine_mod, orc):
    c = Case(orc, engine_mod, 0.05, 55, 3, 8)
    e = c.engine(engine_mod)
    h0, st0 = e.global_search_beam(c.scan, stride_cells=3, n_headings=8)
    V0 = e.search_scores()
    e.set_likelihood_field(True)
    h1, st1 = e.global_search_beam(c.scan, stride_cells=3, n_headings=8)
    assert np.array_equal(bits(V0), bits(e.search_scores())) and h0.tobytes() == h1.tobytes() and st0["n_hits"] == st1["n_hits"]
    e.global_search(c.scan, stride_cells=3, n_headings=8)             # the field's search shares the volume's buffers ...
    e.set_likelihood_field(False)
    h2, _ = e.global_search_beam(c.scan, stride_cells=3, n_headings=8)
    assert np.array_equal(bits(V0), bits(e.search_scores())) and h0.tobytes() == h2.tobytes()


def test_refusals(engine_mod, orc):
    INVALID, NOT_READY = engine_mod.MCL_ERR_INVALID_ARG, engine_mod.MCL_ERR_NOT_READY
    m, ang = SmallMap(), angles(orc, 55)
    obs = np.full(55, 1.0, np.float32)
    e = engine_mod.Engine(max_particles=64)
    assert "map" in expect(engine_mod, NOT_READY, e.global_search_beam, obs)
    e.set_map(m.data, m.resolution, OX, OY)
    assert "beam" in expect(engine_mod, NOT_READY, e.global_search_beam, obs)
    expect(engine_mod, NOT_READY, e.search_beam_table)                 # before any beam search
    e.set_beam_angles(ang)
    for fields in (dict(stride_cells=0), dict(n_headings=0), dict(beam_stride=0), dict(nms=2), dict(reserved=(0, 0, 0, 1))):
        expect(engine_mod, INVALID, e.global_search_beam, obs, **fields)
    expect(engine_mod, INVALID, e.global_search_beam, obs[:54])        # n_beams != B
    expect(engine_mod, INVALID, e.global_search_beam, obs, max_hits=65537)
    assert "divide" in expect(engine_mod, INVALID, e.global_search_beam, obs, n_headings=7)
    assert "256 positions" in expect(engine_mod, INVALID, e.global_search_beam, obs, table_budget_bytes=256 * 72 - 1)
    assert e.search_bytes() < 1 << 20                                  # ... refused before the volume or a table was asked for
    expect(engine_mod, NOT_READY, e.search_beam_table)
    _, st = e.global_search_beam(obs, n_headings=8, table_budget_bytes=256 * 72)
    assert e.search_beam_table()[1].shape[1] == 72 and e.search_scores().size == st["n_poses"]
    e.set_map(m.data, m.resolution, OX, OY)                            # a new map: table and volume are gone
    expect(engine_mod, NOT_READY, e.search_beam_table)
    expect(engine_mod, NOT_READY, e.search_scores)
    uneven = ang.copy()
    uneven[20] += np.float32(1e-4)
    e.set_beam_angles(uneven)
    assert "evenly" in expect(engine_mod, INVALID, e.global_search_beam, obs)
    p = engine_mod.Engine(max_particles=64, weight_mode=engine_mod.WEIGHT_PRODUCT)
    p.set_map(m.data, m.resolution, OX, OY)
    p.set_beam_angles(ang)
    assert "LOG" in expect(engine_mod, INVALID, p.global_search_beam, obs)


# ---- 7. read-only
@pytest.mark.parametrize("n,kernel", [(2000, None), (196608, "k_rays_sweep")], ids=["three-launch", "sweep"])
def test_search_leaves_the_updates_alone(engine_mod, orc, n, kernel):
    c = Case(orc, engine_mod, 0.05, 55, 3, 8)
    pose = (OX + 25.5 * 0.05, OY + 15.5 * 0.05, 0.4)
    cloud = tracking_cloud(np.random.default_rng(11), n, pose=pose, sig=(0.2, 0.2, 0.2))
    a, b = c.engine(engine_mod, n), c.engine(engine_mod, n)
    assert a.search_bytes() == 0 and b.search_bytes() == 0
    for e in (a, b):
        e.set_particles(cloud, np.full(n, 1.0 / n))
    b.global_search_beam(c.scan, max_hits=4, stride_cells=3, n_headings=8)
    for t in range(3):
        for e in (a, b):
            e.update((0.05, 0.0, 0.0), c.scan)
        _, st = b.global_search_beam(c.scan, max_hits=4, stride_cells=2 + t % 2, n_headings=8, table_budget_bytes=(0, 256 * 72)[t % 2])
        assert st["device_bytes"] == b.search_bytes() > 0
    if kernel:
        assert a.ray_kernel_name() == kernel == b.ray_kernel_name()
    assert a.search_bytes() == 0
    assert np.array_equal(bits(a.get_particles()), bits(b.get_particles()))
    assert np.array_equal(bits(a.get_weights()), bits(b.get_weights()))
    assert np.array_equal(bits(a.expected_pose()), bits(b.expected_pose()))
    assert np.array_equal(bits(a.log_weights()), bits(b.log_weights()))


# ---- 8. how far the table is from mcl_query_scans (a condition, not parity: B3)
HEADINGS = (0, 19, 38, 57)


@pytest.mark.parametrize("B,beam_step,bound", [(1081, 8, 0.01), (55, 1, 0.05)])
def test_distance_from_query_scans(engine_mod, orc, B, beam_step, bound):
    """The share of table entries that differ from the step mcl_query_scans reports for the same pose and beam, over every
    position of the stride-2 lattice, 4 headings and (1081 beams: every 8th; 55 beams: every) beam.  The float beam angles sit up
    to 4e-6 rad off the grid, so a ray that grazes a corner may stop a step apart; the 55-beam grid holds the 30 and 60 degree
    rays that run along cell edges.  First the oracle alone, on the CPU, over the same set; then the engine, held to the
    issue's bounds of 1 % and 5 %.  Measured: see profiles/beam_search.md."""
    m = SmallMap()
    om = orc.OracleMap(m.data, m.resolution, OX, OY)
    ang = angles(orc, B)
    cells, xy = engine_mod.host_search_lattice(m.data, m.resolution, OX, OY, stride_cells=2)
    theta = engine_mod.host_search_headings(n_headings=72)
    g = br.grid(ang, 72)
    js = np.arange(0, B, beam_step)
    n_pos = cells.size
    # the oracle alone: the grid angle against theta_k + (double)a_j
    K, J = np.meshgrid(np.array(HEADINGS), js, indexing="ij")
    mi = (K * g["heading_step"] + J) % g["M"]                                       # (4, n_j)
    x = np.broadcast_to(xy[:, 0, None, None], (n_pos,) + K.shape).ravel()
    y = np.broadcast_to(xy[:, 1, None, None], (n_pos,) + K.shape).ravel()
    on_grid = orc.cast_many(om, x, y, np.broadcast_to(g["phi"][mi], (n_pos,) + K.shape).ravel(), use_omp=True)[1]
    off_grid = orc.cast_many(om, x, y, np.broadcast_to(theta[K] + ang.astype(np.float64)[J], (n_pos,) + K.shape).ravel(), use_omp=True)[1]
    share_cpu = float(np.mean(on_grid != off_grid))
    print(f"beam table vs float-angle rays, oracle: B={B} share={share_cpu:.5f} of {on_grid.size}")
    assert share_cpu <= bound
    # the engine: its table against its own pose query
    e = make_engine(engine_mod, m, ang, 64)
    _, st = e.global_search_beam(np.full(B, 1.0, np.float32), max_hits=0, stride_cells=2, n_headings=72)
    first, R = e.search_beam_table()
    assert first == 0 and R.shape == (n_pos, g["M"])
    got = R[:, mi]                                                                   # (n_pos, 4, n_j)
    assert np.array_equal(got.ravel(), on_grid)                                      # (the table is the statement here too)
    differ = 0
    for i, k in enumerate(HEADINGS):
        poses = np.column_stack([xy, np.full(n_pos, theta[k])])
        steps = e.expected_scans(poses, want_steps=True)[1]
        differ += int(np.count_nonzero(steps[:, js] != got[:, i, :]))
    share = differ / got.size
    print(f"beam table vs mcl_query_scans, engine: B={B} share={share:.5f} of {got.size} level3={st['level3_rays']}")
    assert share <= bound
