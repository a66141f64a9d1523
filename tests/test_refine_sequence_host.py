"""The host side of the pose refinement over a scan sequence (mcl_host_refine_sequence_offsets, DESIGN.md §4.23, rule RS1 of
include/mcl_hip_engine.h) against the numpy restatement tests/refine_sequence_ref.py, without a device; the statement the feature
exists for -- the anchor scan cannot rank the two congruent corridors, the sequence can -- on tests/lfield_ref.py alone; the cap on
ambiguous beams of the fixture tests/test_gpu_refine_sequence.py holds the device to; the refusals; the binding."""
import ctypes as C
import math

import numpy as np
import pytest

import lfield_ref as lr
import refine_ref as rr
import refine_sequence_ref as rs
from test_gpu_global_search import MAX_RANGE, angles, scan_at


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. RS1
@pytest.mark.parametrize("rel", [rs.REL3, rs.REL2, rs.REL16], ids=["REL3", "REL2", "REL16"])
@pytest.mark.parametrize("fields", [dict(half_theta=0), dict(half_theta=1), rr.FIXTURE_WINDOW, {}, dict(half_theta=2, step_theta_rad=0.0123)])
def test_offsets_are_rs1(engine_mod, rel, fields):
    got = engine_mod.host_refine_sequence_offsets(rr.SEEDS, rel, **fields)
    want = rs.offsets(rr.SEEDS, rel, **fields)
    nt = 2 * rr.cfg_of(**fields)["half_theta"] + 1
    assert got.shape == want.shape == (3, nt, len(rel), 3)
    assert np.array_equal(bits(got), bits(want))
    # a rotation: the displacement keeps its length
    assert np.allclose(np.hypot(got[..., 0], got[..., 1]), np.hypot(rel[:, 0], rel[:, 1])[None, None, :], atol=1e-12)


def test_zero_rel_and_row_order(engine_mod):
    F = rr.FIXTURE_WINDOW
    got = engine_mod.host_refine_sequence_offsets(rr.SEEDS, np.zeros((2, 3)), **F)
    for m in range(3):
        th = rr.window(rr.SEEDS[m], rr.RES, **F)[::81, 2]                          # R1's headings: one per 9 x 9 positions
        assert np.array_equal(bits(got[m, :, 0, 2]), bits(th)) and np.array_equal(bits(got[m, :, 1, 2]), bits(th))
    assert np.all(np.abs(got[..., :2]) == 0.0)
    # row order: ((m * nt + it) * S + s) * 3; one seed alone gives that seed's rows; one rel row gives that scan's column
    full = engine_mod.host_refine_sequence_offsets(rr.SEEDS, rs.REL3, **F)
    assert full.flags["C_CONTIGUOUS"] and full.shape == (3, 7, 3, 3)
    for m in range(3):
        assert np.array_equal(bits(engine_mod.host_refine_sequence_offsets(rr.SEEDS[m], rs.REL3, **F)[0]), bits(full[m]))
    for s in range(3):
        assert np.array_equal(bits(engine_mod.host_refine_sequence_offsets(rr.SEEDS, rs.REL3[s], **F)[:, :, 0]), bits(full[:, :, s]))
    # the anchor's rows of REL3 (its last): the window heading itself
    assert np.array_equal(bits(full[0, :, 2, 2]), bits(rr.window(rr.SEEDS[0], rr.RES, **F)[::81, 2]))


# ---- 2. the twin statement, on lfield_ref alone
@pytest.fixture(scope="module")
def twin(orc):
    m = rs.twin_map()
    ang = angles(orc, 61)
    return m, ang, rs.twin_scans(m, ang), rs.twin_seeds()


def test_the_anchor_scan_cannot_rank_the_twins_and_the_sequence_can(engine_mod, twin):
    m, ang, scans, seeds = twin
    W = rs.TWIN_WINDOW
    assert rr.offsets(**W).shape[0] == 45
    one = rs.statement(lr, m, ang, scans[1:], seeds, np.zeros((1, 3)), MAX_RANGE, **W)
    seq = rs.statement(lr, m, ang, scans, seeds, rs.REL5, MAX_RANGE, **W)
    for vol, ref in one + seq:
        assert all(int(r[2].sum()) == 0 and not r[1] for r in ref)                  # no ambiguous beam: the statement is unique
    best_one = [float(vol.max()) for vol, _ in one]
    best_seq = [float(vol.max()) for vol, _ in seq]
    print("anchor scan maxima (twin, truth)", best_one, "summed", best_seq)
    assert bits(best_one[0]) == bits(best_one[1])
    assert best_seq[1] - best_seq[0] > 40.0
    assert engine_mod.seed_counts(best_one, 1000).tolist() == [500, 500]
    assert engine_mod.seed_counts(best_seq, 1000).tolist() == [0, 1000]


def test_fixture_of_the_independent_statement_meets_the_cap(orc):
    """SEEDS[0], FIXTURE_WINDOW, REL2, perturbed scans: ambiguous beams at most 1e-5 of all beams, or 2 where that is fewer than one"""
    m = rr.SmallMap()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    ang = angles(orc, 61)
    from side_geometries import compose
    scans = rs.perturbed(np.stack([scan_at(orc, om, ang, compose(rr.P_STAR, r)) for r in rs.REL2]))
    (vol, ref), = rs.statement(lr, m, ang, scans, rr.SEEDS[:1], rs.REL2, MAX_RANGE, **rr.FIXTURE_WINDOW)
    beams = vol.size * sum(lr.used_beams(ang, s, MAX_RANGE)[0].size for s in scans)
    n_amb = sum(int(r[2].sum()) for r in ref)
    print("ambiguous beams", n_amb, "of", beams)
    assert beams > 0 and n_amb <= max(1e-5 * beams, 2)


# ---- 3. the refusals
def test_refusals(engine_mod):
    INVALID = engine_mod.MCL_ERR_INVALID_ARG
    f = engine_mod.host_refine_sequence_offsets

    def refused(*a, **kw):
        with pytest.raises(engine_mod.EngineError) as ei:
            f(*a, **kw)
        assert ei.value.status == INVALID

    for fields in (dict(half_xy=-1), dict(half_theta=-1), dict(step_theta_rad=0.0), dict(step_xy_cells=math.nan), dict(beam_stride=0),
                   dict(reserved=(0, 1, 0)), dict(half_xy=0, half_theta=16384)):
        refused(rr.SEEDS, rs.REL2, **fields)
    refused(np.zeros((0, 3)), rs.REL2)                                              # M = 0
    refused(np.zeros((4097, 3)), rs.REL2, half_theta=0)
    refused(rr.SEEDS, np.zeros((0, 3)))                                             # S = 0
    refused(rr.SEEDS, np.zeros((engine_mod.MAX_SEARCH_SCANS + 1, 3)))
    for bad in (math.nan, math.inf, -math.inf):
        for col in range(3):
            r, s = rs.REL2.copy(), rr.SEEDS.copy()
            r[0, col] = bad
            s[1, col] = bad
            refused(rr.SEEDS, r)
            refused(s, rs.REL2)
    # the row cap: 9 x 32767 x 16 = 4 718 448 rows; 4 x 32767 x 16 = 2 097 088 fit
    assert engine_mod.MAX_REFINE_SEQ_ROWS == 1 << 21
    refused(np.zeros((9, 3)), np.zeros((16, 3)), half_xy=0, half_theta=16383)
    assert f(np.zeros((4, 3)), np.zeros((16, 3)), half_xy=0, half_theta=16383).shape == (4, 32767, 16, 3)
    refused(np.zeros((5, 3)), np.zeros((16, 3)), half_xy=0, half_theta=16383)       # 2 621 360
    # the C call itself: null pointers, a wrong n, the null config
    lib, cfg = engine_mod.load_library(), engine_mod.default_refine_config(half_theta=1)
    s, r, out = np.ascontiguousarray(rr.SEEDS.T), np.ascontiguousarray(rs.REL2), np.zeros(3 * 3 * 2 * 3)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mcl_host_refine_sequence_offsets(C.byref(cfg), vp(s), 3, vp(r), 2, vp(out), out.size) == engine_mod.MCL_OK
    assert lib.mcl_host_refine_sequence_offsets(C.byref(cfg), None, 3, vp(r), 2, vp(out), out.size) == INVALID
    assert lib.mcl_host_refine_sequence_offsets(C.byref(cfg), vp(s), 3, None, 2, vp(out), out.size) == INVALID
    assert lib.mcl_host_refine_sequence_offsets(C.byref(cfg), vp(s), 3, vp(r), 2, None, out.size) == INVALID
    assert lib.mcl_host_refine_sequence_offsets(C.byref(cfg), vp(s), 3, vp(r), 2, vp(out), out.size - 1) == INVALID
    big = np.zeros(3 * 21 * 2 * 3)
    assert lib.mcl_host_refine_sequence_offsets(None, vp(s), 3, vp(r), 2, vp(big), big.size) == engine_mod.MCL_OK
    assert np.array_equal(bits(big.reshape(3, 21, 2, 3)), bits(f(rr.SEEDS, rs.REL2)))
    # the Python wrappers' own checks
    with pytest.raises(ValueError):
        f(rr.SEEDS, np.zeros((2, 2)))
    with pytest.raises(ValueError):
        f(np.zeros((3, 4)), rs.REL2)
    with pytest.raises(AttributeError):
        f(rr.SEEDS, rs.REL2, no_such_field=1)
    # a null engine is refused before any device is touched
    assert lib.mcl_refine_poses_sequence(None, None, None, 0, None, None, 0, 0, None, None) == INVALID


# ---- 4. the binding
def test_symbols_and_abi_version(engine_mod):
    lib = engine_mod.load_library()
    for name in ("mcl_refine_poses_sequence", "mcl_host_refine_sequence_offsets"):
        assert name in engine_mod.EXPORTS and hasattr(lib, name)
    lib.mcl_abi_version.restype = C.c_int
    assert lib.mcl_abi_version() == 1
    assert len(lib.mcl_refine_poses_sequence.argtypes) == 10 and len(lib.mcl_host_refine_sequence_offsets.argtypes) == 7
    for name in ("refine_poses_sequence", "propose_from_scans"):
        assert hasattr(engine_mod.Engine, name)
