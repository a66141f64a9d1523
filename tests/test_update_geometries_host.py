"""The host half of the filter's own stages over the geometry family of tests/side_geometries.py, without a device: the KLD bin
rule, the free-cell list and the injected poses of recovery, and the block plan, pooled field and round schedule of the pruned
search, each against the statement the GPU tests (tests/test_gpu_update_geometries.py) hold the device to.  These decide the
inputs of those tests: a statement that is unsound on a geometry (an origin of (4096.3, -8191.7), a map inside one bin, a map
with one free cell) is found here, before the device is compared with it."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import lfield_ref as lr
import search_pruned_ref as pr
import side_geometries as sg
from test_kld_host import np_bins
from test_recovery_host import child_draws, free_cells, injected_poses

ALL = sg.NAMES + ("small",)
SEED = 0x5EED_0000_0000_0009 + 777
# the bin grids at the default 0.5 m bins: ceil(W res / 0.5) x ceil(H res / 0.5) with res the float widened to double --
# float32(0.05) lies above 0.05, so 120 cells are 6.00000009 m and take 13 bins, not 12; float32(0.02) lies below 0.02
DEFAULT_GRID = dict(narrow=(4, 31), wide=(52, 3), coarse=(32, 24), fine=(6, 5), spielberg_res=(14, 11), far_origin=(13, 10),
                    tiny=(1, 1), open=(9, 7), one_free=(5, 4), small=(13, 10))
N_FREE = dict(open=4800, one_free=1)


def geometry(name):
    if name == "small":
        if "small" not in geometry.__dict__:
            geometry.small = sg.small()
        return geometry.small
    return sg.family()[name]


@pytest.fixture(params=ALL)
def geo(request):
    return geometry(request.param)


# ---- 1. the KLD bin rule
@pytest.mark.parametrize("form", ["default", "cell", "huge"])
def test_kld_bins(engine_mod, geo, form):
    g = geo
    k = engine_mod.default_kld_config(**sg.kld_forms(g)[form])
    nx, ny = sg.kld_grid(g, k)
    if form == "default":
        assert (nx, ny) == DEFAULT_GRID[g.name]
    elif form == "cell":
        # (W res) / res in doubles is W or the next double above it: the grid has W columns or one more, which no pose on the
        # map reaches
        assert nx in (g.W, g.W + 1) and ny in (g.H, g.H + 1)
        print(f"{g.name}: one-cell bins: grid {nx} x {ny} for {g.W} x {g.H} cells")
    else:
        assert (nx, ny) == (1, 1)
    args = (g.W, g.H, g.resolution, g.origin_x, g.origin_y, k)

    def same(p, chunk):
        for lo in range(0, p.shape[1], chunk):
            x, y, th = (np.ascontiguousarray(r[lo:lo + chunk]) for r in p)
            got = engine_mod.host_kld_bins(x, y, th, *args)
            assert got == np_bins(x, y, th, *args), (g.name, form, lo)
        return got
    same(g.particles, 4096)
    same(g.particles, 64)
    same(np.ascontiguousarray(g.query_poses.T), 64)
    same(np.ascontiguousarray(g.query_poses.T), 1)
    edges = sg.edge_poses(g, k, np.random.default_rng(31))
    assert edges.shape == (3, 2000)
    same(edges, 2000)
    same(edges, 5)                                              # (a count hides a wrong bin among many: five at a time do not)
    # the grid is what the rule says it is: one pose in every bin of one heading layer occupies nx * ny bins, and one pose just
    # past the grid's far corner one more (the outside bin)
    if nx * ny <= 20000:
        cx, cy = np.meshgrid(np.arange(nx), np.arange(ny))
        x = g.origin_x + (cx.ravel() + 0.5) * float(k.bin_x_m)
        y = g.origin_y + (cy.ravel() + 0.5) * float(k.bin_y_m)
        th = np.full(x.size, 0.1)
        assert engine_mod.host_kld_bins(x, y, th, *args) == np_bins(x, y, th, *args) == nx * ny
        x = np.append(x, g.origin_x + (nx + 0.5) * float(k.bin_x_m))
        y, th = np.append(y, y[-1]), np.append(th, 0.1)
        assert engine_mod.host_kld_bins(x, y, th, *args) == nx * ny + 1
    if form != "cell":
        # every heading bin of one cell of the grid
        th = -np.pi + (np.arange(36) + 0.5) * (2 * np.pi / 36)
        p = np.array(g.true_pose)
        assert engine_mod.host_kld_bins(np.full(36, p[0]), np.full(36, p[1]), th, *args) == 36
    if g.name == "tiny" and form == "default":
        # 0.45 m x 0.35 m inside one 0.5 m bin: every pose on the map shares (0, 0), so the count is the headings'
        assert same(g.particles, 4096) <= 36 + 1


# ---- 2. the free cells and the injected poses
def test_free_cells_and_injected_poses(orc, geo):
    g, om = geo, geo.oracle(orc)
    free = free_cells(g.data)
    n_free = int((g.data == 0).sum())
    assert free.size == n_free and np.array_equal(free, np.flatnonzero(g.data.ravel() == 0))
    if g.name in N_FREE:
        assert n_free == N_FREE[g.name]
    else:
        assert n_free % 64 != 0, n_free                         # a last wave of the list that is not full
    print(f"{g.name}: {n_free} free cells of {g.W * g.H}")
    coin, pick, hb = child_draws(SEED, 1, 4096)
    p = injected_poses(pick, hb, free, g.W, g.resolution, g.origin_x, g.origin_y)
    assert p.shape == (3, 4096) and np.isfinite(p).all() and (p[2] >= -np.pi).all() and (p[2] < np.pi).all()
    # the picks cover the list: floor(pick n_free / 2^53)
    at = np.array([(int(v) * n_free) >> 53 for v in pick])
    assert at.min() >= 0 and at.max() < n_free
    if n_free > 1:
        assert np.unique(at).size > min(n_free, 4096) // 4
    # every pose lies in the free cell it was drawn for under the oracle's own world-to-cell rule (a truncation of
    # (x - origin) / res, not a rounding: col res + origin must not fall short of the cell's low edge)
    col, row = sg.oracle_cells(om, p[0], p[1])
    want_col, want_row = (free[at] % np.uint64(g.W)).astype(np.int64), (free[at] // np.uint64(g.W)).astype(np.int64)
    short = (col != want_col) | (row != want_row)
    print(f"{g.name}: {int(short.sum())} of 4096 injected poses fall in a neighbour of their cell under the oracle's truncation")
    inside = (col >= 0) & (col < g.W) & (row >= 0) & (row < g.H)
    assert inside.all()
    assert (g.data[row, col] == 0).all(), (g.name, int((g.data[row, col] != 0).sum()))
    if g.name == "one_free":
        assert np.unique(p[0]).size == 1 and np.unique(p[1]).size == 1
        assert (col == 19).all() and (row == 13).all()


def test_injected_coordinates_on_far_origin_are_within_an_ulp_of_the_real_value():
    """exactly, in rationals: col * res + origin as the statement forms it (one rounded product, one rounded sum) against the real
    value, for every column and row of far_origin, where an ulp of a coordinate is 9.1e-13 m (x) and 1.8e-12 m (y)"""
    g = sg.family()["far_origin"]
    res = np.float64(np.float32(g.resolution))
    worst = 0.0
    for origin, count in ((g.origin_x, g.W), (g.origin_y, g.H)):
        for c in range(count):
            stated = np.float64(c) * res + np.float64(origin)
            real = Fr(c) * Fr(float(res)) + Fr(origin)
            ulp = Fr(float(np.spacing(np.float64(abs(float(real))))))
            err = abs(Fr(float(stated)) - real) / ulp
            worst = max(worst, float(err))
            assert err <= 1, (origin, c, float(err))
    assert float(np.spacing(np.float64(4096.3))) == 2.0 ** -40 and float(np.spacing(np.float64(8191.7))) == 2.0 ** -40
    print(f"far_origin: the stated coordinate lies within {worst:.3f} ulp of the real value")


# ---- 3. the pruned search, host side
def field_of(engine_mod, g):
    if "field" not in g.memo:
        g.memo["field"] = (engine_mod.host_likelihood_field(g.data, g.resolution), lr.K_of(2.0, g.resolution))
    return g.memo["field"]


def test_block_plan_and_pooled_field(engine_mod, geo):
    g = geo
    D, K = field_of(engine_mod, g)
    assert np.array_equal(D, lr.field(g.data, g.resolution))
    pooled = {}
    for stride in g.strides:
        n_pos = sg.lattice_ref(g, stride)[0].size
        for S in (2, 4, 8):
            got, want = engine_mod.host_search_blocks(g.data, block=S, stride_cells=stride), pr.blocks(g.data, stride, S)
            for key in ("n_blocks", "w", "nbx", "nby"):
                assert got[key] == want[key], (g.name, stride, S, key)
            assert np.array_equal(got["blocks"], want["blocks"])
            w = (S - 1) * stride + 2
            assert got["w"] == w and got["blocks"][:, 2].sum() == n_pos
            if g.name == "one_free" or (g.name == "tiny" and stride == 3 and S >= 4):
                assert got["n_blocks"] == 1 and got["blocks"][0].tolist() == [got["blocks"][0][0], got["blocks"][0][1], n_pos]
            if g.name == "open":
                assert got["n_blocks"] == got["nbx"] * got["nby"]                        # no dead block
            if w not in pooled:
                pooled[w] = True
                out = engine_mod.host_lf_pool(D, K, w)
                assert out.shape == (g.H + w - 1, g.W + w - 1)
                assert np.array_equal(out, pr.pool(D, K, w)), (g.name, w)
                if g.name == "open":
                    assert (out == K).all()
                if w > max(g.W, g.H):
                    assert (out[w - 1:g.H, w - 1:g.W] == D.min()).all()                 # a window over the whole map


def scheduled(engine_mod, U, V, data, stride, S, nms, max_hits, first_pairs):
    """the rounds of P4 / P5 with mcl_host_search_prune_next deciding every round's size: (pairs scored, rounds, hits)"""
    pmap, ix, iy = pr.lattice_grid(data, stride)
    b = pr.blocks(data, stride, S)
    n_head, n_pos = V.shape
    pairs = U.size
    order = np.argsort(-U, kind="stable")
    rank = np.empty(pairs, np.int64)
    rank[order] = np.arange(pairs)
    Us = U[order]
    pose_rank = rank[np.arange(n_head)[:, None] * b["n_blocks"] + b["block_of_pos"][None, :]]
    idx = np.arange(V.size).reshape(V.shape)
    n, rounds = engine_mod.host_search_prune_next(pairs, 0, 0, first_pairs), 0
    while True:
        rounds += 1
        scored = pose_rank < n
        cand = pr.mark(np.where(scored, V, -np.inf), pmap, ix, iy, nms, scored)
        ci, cv = idx[cand], V[cand]
        best = ci[np.lexsort((ci, -cv))]
        c = V.reshape(-1)[best[max_hits - 1]] if best.size >= max_hits else -np.inf
        if n == pairs or c > Us[n]:
            return n, rounds, best[:max_hits]
        j = 0
        if best.size >= max_hits:
            below = np.flatnonzero(Us < c)
            j = int(below[0]) if below.size else pairs
        nxt = engine_mod.host_search_prune_next(pairs, n, j, first_pairs)
        assert n < nxt <= pairs
        n = nxt


def test_round_schedule_on_the_geometrys_lattice(engine_mod, geo):
    """a synthetic volume with ties over the geometry's lattice, U the block maximum: the rounds mcl_host_search_prune_next gives
    are those of search_pruned_ref.schedule, and the hits are the exhaustive ones"""
    g = geo
    rng = np.random.default_rng(17)
    n_head = 5
    for stride in g.strides:
        pmap, ix, iy = pr.lattice_grid(g.data, stride)
        for S in (2, 4, 8):
            b = pr.blocks(g.data, stride, S)
            V = rng.integers(-9, 0, (n_head, ix.size)).astype(np.float64)
            V[rng.random(V.shape) < 0.05] = -np.inf
            if g.name == "open":
                V[:] = -3.0                                     # an all-ties volume, as the device gives on this map
            U = np.full((n_head, b["n_blocks"]), -np.inf)
            np.maximum.at(U, (np.arange(n_head)[:, None].repeat(ix.size, 1), b["block_of_pos"][None, :].repeat(n_head, 0)), V)
            U = U.reshape(-1)
            for nms, max_hits in ((0, 1), (1, 16), (1, 65536)):
                want = pr.schedule(U, V, g.data, stride, S, nms, max_hits, 3)
                got = scheduled(engine_mod, U, V, g.data, stride, S, nms, max_hits, 3)
                assert got[:2] == (want["pairs_scored"], want["rounds"]), (g.name, stride, S, nms, max_hits)
                assert np.array_equal(got[2], want["hits"])
                cand = pr.mark(V, pmap, ix, iy, nms, np.ones(V.shape, bool))
                idx = np.arange(V.size).reshape(V.shape)
                ci, cv = idx[cand], V[cand]
                assert np.array_equal(want["hits"], ci[np.lexsort((ci, -cv))][:max_hits])
                if g.name == "open":
                    assert want["pairs_scored"] == U.size                            # the strict rule scores everything
                if g.name == "one_free" or (g.name == "tiny" and stride == 3 and S >= 4):
                    assert U.size == n_head


# ---- what the GPU tests start from
def test_the_clouds_are_what_the_gpu_tests_need(orc, geo):
    g, om = geo, geo.oracle(orc)
    rng = np.random.default_rng(5)
    p = sg.cloud_around(g, rng, 4096)
    wall, off = sg.cloud_shares(om, p)
    print(f"{g.name}: tracking cloud of 4 cells: {wall:.3f} in walls, {off:.3f} off the map")
    if g.name == "tiny":
        assert off > 0.1 and wall > 0.02                        # kept so: the filter must cope with both
    if g.name == "one_free":
        assert wall > 0.5
    if g.name == "open":
        assert wall == 0.0
    q = sg.global_cloud(g, rng, 4096)
    wall, off = sg.cloud_shares(om, q)
    assert 0.03 < off < 0.08, (g.name, off)
    m = sg.mirrored_pose(g)
    col, row = sg.oracle_cells(om, m[0], m[1])
    assert g.data[row, col] == 0
    if g.name != "one_free":
        assert (int(col), int(row)) != g.true_cell
