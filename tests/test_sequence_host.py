"""The host side of the search over a scan sequence (rule SQ1 of include/mcl_hip_engine.h), without a device: the
offsets table against a numpy statement of SQ1, the zero sequence, mcl_host_relative_poses, the refusals."""
import ctypes as C
import math

import numpy as np
import pytest

from monte_carlo_localization_amd import engine as E

EPS = np.finfo(np.float64).eps

REL = np.array([[0.0, 0.0, 0.0],
                [-0.5, 0.0, 0.0],
                [-1.25, 0.3, -0.2],
                [2.0, -7.5, 3.0],
                [1e-9, -1e3, -3.1]])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- SQ1
@pytest.mark.parametrize("n_head", [1, 2, 5, 72])
def test_offsets_are_sq1(n_head):
    got = E.host_search_sequence_offsets(REL, n_headings=n_head)
    assert got.shape == (n_head, len(REL), 3)
    theta = E.host_search_headings(n_headings=n_head)
    # theta_ks is one rounded add of two doubles: numpy's add is the same operation, so the bits agree
    assert np.array_equal(bits(got[:, :, 2]), bits(theta[:, None] + REL[None, :, 2]))
    # the displacement goes through the C library's cos / sin, which numpy's need not match in the last bit: the host function is
    # the definition, numpy guards the formula.  Both are within an ulp of the true cosine and sine (relative error <= EPS), each
    # product and the final add round once more (EPS / 2 each, relative to terms no larger than |dx| + |dy|): the two statements
    # differ by less than 2 EPS (|dx| + |dy|) per side; 4 EPS (|dx| + |dy|) bounds the difference.
    ck, sk = np.cos(theta)[:, None], np.sin(theta)[:, None]
    dx, dy = REL[None, :, 0], REL[None, :, 1]
    tol = 4 * EPS * (np.abs(dx) + np.abs(dy))
    assert np.all(np.abs(got[:, :, 0] - (ck * dx - sk * dy)) <= tol)
    assert np.all(np.abs(got[:, :, 1] - (sk * dx + ck * dy)) <= tol)
    # a rotation keeps the length
    assert np.allclose(np.hypot(got[:, :, 0], got[:, :, 1]), np.broadcast_to(np.hypot(dx, dy), (n_head, len(REL))), rtol=1e-14, atol=0)


def test_offsets_with_the_c_librarys_own_cosine():
    """math.cos / math.sin are the C library's: with them the table is restated bit for bit (products and sum rounded separately)"""
    n_head = 7
    got = E.host_search_sequence_offsets(REL, n_headings=n_head)
    theta = E.host_search_headings(n_headings=n_head)
    for k in range(n_head):
        ck, sk = math.cos(theta[k]), math.sin(theta[k])
        for s, (dx, dy, dt) in enumerate(REL.tolist()):
            want = np.array([ck * dx - sk * dy, sk * dx + ck * dy, theta[k] + dt])
            assert np.array_equal(bits(got[k, s]), bits(want)), (k, s)


@pytest.mark.parametrize("n_head", [1, 2, 72])
def test_a_zero_sequence_moves_nothing(n_head):
    got = E.host_search_sequence_offsets(np.zeros((3, 3)), n_headings=n_head)
    theta = E.host_search_headings(n_headings=n_head)
    assert np.all(got[:, :, :2] == 0.0)
    assert np.array_equal(bits(got[:, :, 2]), bits(np.broadcast_to(theta[:, None], (n_head, 3))))
    # ... and so SQ2's adds return the lattice pose itself, whatever the sign of the zero
    x = np.array([-3.0 + 25.5 * 0.05, 0.0, 1e-300])
    assert np.array_equal(bits(x[None, None, :] + got[:, :, :1]), bits(np.broadcast_to(x, (n_head, 3, 3))))
    assert theta[0] == -math.pi and got[0, 0, 2] == -math.pi


def test_one_row_is_a_sequence_of_one():
    a = E.host_search_sequence_offsets((0.5, -0.25, 0.1), n_headings=4)
    b = E.host_search_sequence_offsets([(0.5, -0.25, 0.1)], n_headings=4)
    assert a.shape == (4, 1, 3) and np.array_equal(bits(a), bits(b))


# ---- mcl_host_relative_poses
def compose(a, r):
    """a o r: the pose r, given in a's frame, in a's parent frame"""
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * r[0] - s * r[1], a[1] + s * r[0] + c * r[1], a[2] + r[2]])


ODOM = np.array([[10.0, -4.0, 3.0],
                 [10.4, -4.2, -3.1],            # the heading crosses +-pi between the scans
                 [9.0, -3.0, 0.2],
                 [9.5, -3.5, -0.7],
                 [0.0, 0.0, 0.0]])


@pytest.mark.parametrize("anchor", [0, 1, 3, -1])
def test_relative_poses_compose_back(anchor):
    rel = E.relative_poses(ODOM, anchor=anchor)
    a = anchor % len(ODOM)
    assert rel.shape == ODOM.shape
    assert np.array_equal(bits(rel[a]), np.zeros(3, np.uint64))               # exactly +0.0
    assert np.all(rel[:, 2] > -math.pi) and np.all(rel[:, 2] <= math.pi)
    for s in range(len(ODOM)):
        back = compose(ODOM[a], rel[s])
        assert np.all(np.abs(back[:2] - ODOM[s, :2]) <= 1e-12)
        d = back[2] - ODOM[s, 2]
        assert abs(d - 2 * math.pi * round(d / (2 * math.pi))) <= 1e-12


def test_relative_heading_wraps():
    odom = np.array([[0.0, 0.0, 3.0], [0.0, 0.0, -3.0], [0.0, 0.0, 3.0 - math.pi], [0.0, 0.0, 3.0 + math.pi]])
    rel = E.relative_poses(odom, anchor=0)
    assert abs(rel[1, 2] - (2 * math.pi - 6.0)) <= 1e-15                       # -6 wraps to +0.283...
    assert -math.pi < rel[2, 2] <= math.pi and -math.pi < rel[3, 2] <= math.pi  # (near the cut, on either side of it, but inside)
    assert abs(abs(rel[2, 2]) - math.pi) <= 1e-15 and abs(abs(rel[3, 2]) - math.pi) <= 1e-15
    rel = E.relative_poses(odom, anchor=1)
    assert abs(rel[0, 2] - (6.0 - 2 * math.pi)) <= 1e-15
    # exactly -pi is not in the interval: it becomes +pi
    assert E.relative_poses([[0.0, 0.0, 0.0], [0.0, 0.0, -math.pi]], anchor=0)[1, 2] == math.pi
    assert E.relative_poses([[0.0, 0.0, 0.0], [0.0, 0.0, math.pi]], anchor=0)[1, 2] == math.pi


def test_relative_poses_feed_the_offsets():
    """a straight drive along the robot's own x axis: every earlier scan sits behind the anchor, whatever the odometry frame"""
    th = 0.7
    odom = np.array([[1.0 + 0.5 * t * math.cos(th), 2.0 + 0.5 * t * math.sin(th), th] for t in range(4)])
    rel = E.relative_poses(odom)
    assert np.allclose(rel, [[-1.5, 0, 0], [-1.0, 0, 0], [-0.5, 0, 0], [0, 0, 0]], rtol=0, atol=1e-12)
    off = E.host_search_sequence_offsets(rel, n_headings=4)                    # headings -pi, -pi/2, 0, pi/2
    assert np.allclose(off[2, 0, :2], [-1.5, 0.0], rtol=0, atol=1e-12) and np.allclose(off[3, 0, :2], [0.0, -1.5], rtol=0, atol=1e-12)


# ---- the refusals that need no device
def test_refusals():
    lib, INVALID = E.load_library(), E.MCL_ERR_INVALID_ARG
    c = E.default_search_config(n_headings=4)
    rel, out = np.zeros((2, 3)), np.empty(4 * 2 * 3)
    f = lib.mcl_host_search_sequence_offsets
    assert f(C.byref(c), ptr(rel), 2, ptr(out), out.size) == E.MCL_OK
    assert f(None, ptr(rel), 2, ptr(out), out.size) == INVALID
    assert f(C.byref(c), None, 2, ptr(out), out.size) == INVALID
    assert f(C.byref(c), ptr(rel), 2, None, out.size) == INVALID
    assert f(C.byref(c), ptr(rel), 2, ptr(out), out.size - 1) == INVALID
    assert f(C.byref(c), ptr(rel), 0, ptr(out), 0) == INVALID
    big = np.zeros((E.MAX_SEARCH_SCANS + 1, 3))
    room = np.empty(4 * len(big) * 3)
    assert f(C.byref(c), ptr(big), len(big), ptr(room), room.size) == INVALID
    assert f(C.byref(c), ptr(big), E.MAX_SEARCH_SCANS, ptr(room), 4 * E.MAX_SEARCH_SCANS * 3) == E.MCL_OK
    for bad in (math.nan, math.inf, -math.inf):
        for col in range(3):
            r = np.zeros((2, 3))
            r[1, col] = bad
            assert f(C.byref(c), ptr(r), 2, ptr(out), out.size) == INVALID
    for fields in (dict(n_headings=0), dict(stride_cells=0), dict(beam_stride=0), dict(nms=2), dict(reserved=(1, 0, 0, 0))):
        with pytest.raises(E.EngineError) as ei:
            E.host_search_sequence_offsets(rel, **fields)
        assert ei.value.status == INVALID
    with pytest.raises(ValueError):
        E.host_search_sequence_offsets(np.zeros((2, 2)))

    g = lib.mcl_host_relative_poses
    odom, res = np.zeros((3, 3)), np.empty((3, 3))
    assert g(ptr(odom), 3, 2, ptr(res)) == E.MCL_OK
    assert g(None, 3, 2, ptr(res)) == INVALID and g(ptr(odom), 3, 2, None) == INVALID
    assert g(ptr(odom), 0, 0, ptr(res)) == INVALID
    assert g(ptr(odom), 3, 3, ptr(res)) == INVALID and g(ptr(odom), 3, -1, ptr(res)) == INVALID
    odom[1, 2] = math.nan
    assert g(ptr(odom), 3, 2, ptr(res)) == INVALID
    with pytest.raises(E.EngineError):
        E.relative_poses(ODOM, anchor=len(ODOM))
    # more poses than a search takes are fine here
    assert E.relative_poses(np.zeros((40, 3))).shape == (40, 3)
