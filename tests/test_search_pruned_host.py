"""The host side of the global search with exact pruning (rules P1, P2 and P4 of include/mcl_hip_engine.h), without
a device: the pooled field against a brute force, the bound table against its definition, the block plan, the round schedule of
tests/search_pruned_ref.py on hand-made arrays, and that the library exports the call."""
import numpy as np
import pytest

import search_pruned_ref as pr


def walled(W, H):
    g = np.zeros((H, W), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    g[H // 3, W // 5:W // 2] = 100
    g[H // 2:, 2 * W // 3] = 100
    g[2, 2] = g[H - 3, W - 4] = 100
    return g


# ---- P2: the pooled field
@pytest.mark.parametrize("W,H,w", [(37, 23, 3), (37, 23, 16), (12, 9, 16), (9, 12, 2), (5, 4, 1)])
def test_pool_is_the_window_minimum(engine_mod, W, H, w):
    """windows hanging off every edge (low corners from -(w - 1) up, so the first and last w - 1 rows and columns of the output),
    a window larger than the map, w = 1 (the field itself)"""
    D = engine_mod.host_likelihood_field(walled(W, H), 0.05)
    K = 1600
    got = engine_mod.host_lf_pool(D, K, w)
    want = pr.pool(D, K, w)
    assert got.shape == (H + w - 1, W + w - 1)
    assert np.array_equal(got, want)
    assert got[0, 0] == min(K, D[0, 0]) and got[-1, -1] == min(K, D[-1, -1])            # one cell of the map in the window
    if w == 1:
        assert np.array_equal(got, D)


def test_pool_of_a_map_without_obstacles(engine_mod):
    D = engine_mod.host_likelihood_field(np.zeros((11, 17), np.int8), 0.05)
    assert (D == 1600).all()
    got = engine_mod.host_lf_pool(D, 1600, 9)
    assert got.shape == (19, 25) and (got == 1600).all()


def test_pool_refusals(engine_mod):
    D = np.zeros((4, 5), np.uint16)
    for K, w in ((-1, 2), (65536, 2), (10, 0), (10, 65537)):
        with pytest.raises(engine_mod.EngineError):
            engine_mod.host_lf_pool(D, K, w)


# ---- P2: the bound table
def test_bound_table_is_the_suffix_maximum(engine_mod):
    # a table with -inf entries: z_rand = 0 and a narrow sigma, so exp underflows far from an obstacle
    lf = engine_mod.host_likelihood_table(0.05, z_rand=0.0, sigma_hit_m=0.02)
    assert np.isneginf(lf).any() and np.isfinite(lf[0])
    ub = engine_mod.host_search_bound_table(lf)
    assert np.array_equal(ub.view(np.uint32), pr.bound_table(lf).view(np.uint32))
    assert np.isneginf(ub[-1]) and ub[0] == lf.max()
    # no monotonicity assumed
    lf = np.array([1.0, -np.inf, 3.0, 2.0, -np.inf, 2.5, -7.0], np.float32)
    ub = engine_mod.host_search_bound_table(lf)
    assert np.array_equal(ub, np.array([3.0, 3.0, 3.0, 2.5, 2.5, 2.5, -7.0], np.float32))
    assert np.array_equal(engine_mod.host_search_bound_table(np.array([-np.inf], np.float32)), np.array([-np.inf], np.float32))


# ---- P1: the block plan
@pytest.mark.parametrize("W,H,stride,S", [(37, 23, 2, 8), (37, 23, 1, 4), (37, 23, 3, 2), (33, 17, 2, 8), (64, 32, 2, 8), (7, 5, 3, 8)])
def test_block_plan(engine_mod, W, H, stride, S):
    """map sizes that are no multiple of S * stride (a last block row and column with fewer lattice cells), one that is"""
    g = walled(W, H)
    got = engine_mod.host_search_blocks(g, block=S, stride_cells=stride)
    want = pr.blocks(g, stride, S)
    for k in ("n_blocks", "w", "nbx", "nby"):
        assert got[k] == want[k], k
    assert np.array_equal(got["blocks"], want["blocks"])
    assert got["w"] == (S - 1) * stride + 2
    cells, _ = engine_mod.host_search_lattice(g, 0.05, 0.0, 0.0, stride_cells=stride)
    assert got["blocks"][:, 2].sum() == cells.size
    assert (got["blocks"][:, 2] >= 1).all() and (got["blocks"][:, 2] <= S * S).all()


def test_block_with_a_single_position_and_dead_blocks(engine_mod):
    g = np.full((40, 40), 100, np.int8)
    g[33, 35] = 0                                      # stride 2: lattice cell (17, 16), block (2, 2) of S = 8
    g[1, 1] = 0
    got = engine_mod.host_search_blocks(g, block=8, stride_cells=2)
    assert got["n_blocks"] == 2 and got["nbx"] == 3 and got["nby"] == 3
    assert got["blocks"].tolist() == [[0, 0, 1], [2, 2, 1]]
    assert engine_mod.host_search_blocks(np.full((8, 8), 100, np.int8), block=4)["n_blocks"] == 0


def test_block_plan_refusals(engine_mod):
    g = np.zeros((8, 8), np.int8)
    for S in (1, 3, 16, -2):
        with pytest.raises(engine_mod.EngineError):
            engine_mod.host_search_blocks(g, block=S)
    with pytest.raises(engine_mod.EngineError):
        engine_mod.host_search_blocks(g, block=8, stride_cells=0)
    with pytest.raises(engine_mod.EngineError):
        engine_mod.host_search_blocks(g, block=8, stride_cells=10000)          # w above 65536


# ---- P4: the round schedule
def test_round_sizes(engine_mod):
    nxt = engine_mod.host_search_prune_next
    assert nxt(100000, 0) == pr.first_round(100000) == 1562
    assert nxt(5000, 0) == pr.first_round(5000) == 1024
    assert nxt(300, 0) == pr.first_round(300) == 300
    assert nxt(300, 0, first_pairs=7) == pr.first_round(300, 7) == 7
    assert nxt(300, 0, first_pairs=301) == 300
    assert nxt(1000, 100, first_below_c=150) == 200                 # doubling wins
    assert nxt(1000, 100, first_below_c=250) == 250                 # the ranks down to c win
    assert nxt(1000, 600, first_below_c=10) == 1000
    assert nxt(1000, 100, first_below_c=1000) == 1000
    assert nxt((1 << 62) + 1, 1 << 62, first_below_c=3) == (1 << 62) + 1            # no overflow in 2 n
    for bad in ((0, 0, 0), (10, 11, 0), (10, -1, 0), (10, 1, -1)):
        with pytest.raises(engine_mod.EngineError):
            nxt(*bad)


def line_map(n):
    """one row of n free cells: at stride 1 and S = 2 the blocks are pairs of neighbouring positions"""
    return np.zeros((1, n), np.int8)


def test_schedule_on_hand_made_arrays():
    # 8 positions in a row, 1 heading, S = 2: 4 blocks = 4 pairs.  The scores; U = the block maximum plus a slack
    g = line_map(8)
    V = np.array([[1.0, 5.0, 2.0, 2.5, 9.0, 3.0, 0.0, -np.inf]])
    U = np.array([5.5, 3.0, 9.5, 0.5])
    # the first round scores the best pair alone (block 2): 9.0 is a candidate, and 9.0 > 5.5, the bound of what is unscored
    r = pr.schedule(U, V, g, 1, 2, nms=1, max_hits=1, first_pairs=1)
    assert r == dict(hits=r["hits"], pairs_scored=1, rounds=1) and r["hits"].tolist() == [4]
    # two hits: after round 1 there is one candidate, so no c: the doubling alone.  Round 2 (ranks 0, 1: blocks 2, 0) has the
    # candidates 9 and 5, and c = 5 > 3, the bound of rank 2
    r = pr.schedule(U, V, g, 1, 2, nms=1, max_hits=2, first_pairs=1)
    assert (r["pairs_scored"], r["rounds"], r["hits"].tolist()) == (2, 2, [4, 1])
    # without nms: round 1 has candidates 9 and 3, c = 3 is not above 5.5; the first rank below 3 is 3 (U = 0.5), doubling gives 2:
    # round 2 scores ranks 0..2, c = 5 > 0.5
    r = pr.schedule(U, V, g, 1, 2, nms=0, max_hits=2, first_pairs=1)
    assert (r["pairs_scored"], r["rounds"], r["hits"].tolist()) == (3, 2, [4, 1])
    # a provisional candidate that an unscored neighbour would beat: position 3 (2.5) beside position 4 (9.0).  U of block 2 set
    # low on purpose is not allowed (U must bound), so make block 1 rank first by a loose bound: 2.5 is then a candidate of round 1,
    # but not above t = 9.5, and the call goes on: the first rank with U < 2.5 is 3, so round 2 scores the ranks 1 and 2
    U2 = np.array([5.5, 20.0, 9.5, 0.5])
    r = pr.schedule(U2, V, g, 1, 2, nms=1, max_hits=1, first_pairs=1)
    assert (r["pairs_scored"], r["rounds"], r["hits"].tolist()) == (3, 2, [4])


def test_schedule_with_equal_scores_scores_everything():
    """every score equal to every bound: c > t never holds, so the strict rule ends only when nothing is unscored"""
    g = line_map(8)
    V = np.full((2, 8), -3.0)
    U = np.full(8, -3.0)
    r = pr.schedule(U, V, g, 1, 2, nms=0, max_hits=3, first_pairs=1)
    assert r["pairs_scored"] == 8 and r["hits"].tolist() == [0, 1, 2]
    assert r["rounds"] == 3                                  # 1 pair: two candidates, no c; 2 pairs: c = t, no U below c; all
    r = pr.schedule(U, V, g, 1, 2, nms=1, max_hits=3, first_pairs=1)
    assert r["pairs_scored"] == 8 and r["hits"].tolist() == [0]            # the lowest index of each neighbourhood: pose 0 alone


def test_schedule_matches_an_exhaustive_marking():
    """random volumes with ties, U = the block maximum (the tightest bound): the reported hits are the exhaustive ones"""
    rng = np.random.default_rng(5)
    g = walled(23, 17)
    for stride, S, nms in ((1, 2, 1), (2, 4, 1), (1, 8, 0), (1, 4, 1)):
        pmap, ix, iy = pr.lattice_grid(g, stride)
        b = pr.blocks(g, stride, S)
        n_head, n_pos = 3, ix.size
        V = rng.integers(-6, 0, (n_head, n_pos)).astype(np.float64)
        V[rng.random(V.shape) < 0.05] = -np.inf
        U = np.full((n_head, b["n_blocks"]), -np.inf)
        np.maximum.at(U, (np.arange(n_head)[:, None].repeat(n_pos, 1), b["block_of_pos"][None, :].repeat(n_head, 0)), V)
        everything = np.ones(V.shape, bool)
        cand = pr.mark(V, pmap, ix, iy, nms, everything)
        idx = np.arange(V.size).reshape(V.shape)
        ci, cv = idx[cand], V[cand]
        want = ci[np.lexsort((ci, -cv))]
        for max_hits in (1, 5, want.size + 3):
            r = pr.schedule(U.reshape(-1), V, g, stride, S, nms, max_hits, first_pairs=2)
            assert r["hits"].tolist() == want[:max_hits].tolist(), (stride, S, nms, max_hits)


# ---- the library has the call
def test_library_exports_the_pruned_search(engine_mod):
    lib = engine_mod.load_library()
    for name in ("mcl_default_search_prune_config", "mcl_global_search_pruned", "mcl_get_search_bounds", "mcl_host_search_blocks",
                 "mcl_host_lf_pool", "mcl_host_search_bound_table", "mcl_host_search_prune_next"):
        assert name in engine_mod.EXPORTS
        assert hasattr(lib, name), name
    c = engine_mod.search_prune_config()
    assert (c.block, c.first_pairs, list(c.reserved)) == (8, 0, [0] * 6)
    assert lib.mcl_abi_version() == 1
