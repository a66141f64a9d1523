"""The fixture of tests/test_gpu_refine_beam.py (mcl_refine_poses_beam), decided by the oracle alone through the
statement tests/refine_beam_ref.py, without a device: on refine_ref.SmallMap, seed LATTICE_POSE, the 61-beam scan cast from P*, the
window FIXTURE_WINDOW has one best pose, three heading steps from the seed, better than the centre and near P*; its covariance is
positive definite; and on this table RB3's order and the in-order sum give the same bits."""
import numpy as np
import pytest

import refine_beam_ref as rb
import refine_ref as rr


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fixture_terms(orc):
    m = rr.SmallMap()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    ang = rr.angles(orc, 61)
    obs = rr.perturbed_scan(orc, om, ang, rr.P_STAR)
    win = rr.window(rr.LATTICE_POSE, rr.RES, **rr.FIXTURE_WINDOW)
    return rb.terms(orc, om, win, ang, obs)


def test_fixture_finds_the_pose(fixture_terms):
    F = rr.FIXTURE_WINDOW
    V = rb.q3(fixture_terms)
    assert V.shape == (567,) and np.isfinite(V).all()
    assert np.unique(V).size == V.size                      # all distinct: R3's tie rules do not decide the best
    wb = rr.best(V, **F)
    d = rr.offsets(**F)[wb]
    centre = (V.size - 1) // 2
    print("best offset", d, "score", V[wb], "centre", V[centre])
    assert tuple(d) == (0, 0, 3)
    assert V[wb] > V[centre]
    assert abs(V[wb] - -96.420) < 1e-3 and abs(V[centre] - -98.678) < 1e-3
    assert np.all(np.abs(d - np.array(rr.P_STAR_STEPS)) <= 2.0)
    _, _, cov, S = rr.moments(rr.LATTICE_POSE, rr.RES, V, **F)
    assert S >= 1.0 and np.linalg.eigvalsh(cov).min() > 0.0


def test_q3_order_is_the_in_order_sum_on_this_fixture(fixture_terms):
    """a fact about the fixture and the default table, not about the rule: RB3 fixes Q3's order"""
    assert np.array_equal(bits(rb.q3(fixture_terms)), bits(rb.in_order(fixture_terms)))


def test_q3_is_a_lane_sum_and_a_butterfly():
    """the written-out order on terms where the order shows: 130 terms of very different size"""
    rng = np.random.default_rng(5)
    t = (rng.normal(0.0, 1.0, (4, 130)) * 10.0 ** rng.integers(-8, 8, (4, 130))).astype(np.float64)
    got = rb.q3(t)
    for n in range(4):
        lanes = [0.0] * 64
        for u in range(130):
            lanes[u % 64] += float(t[n, u])
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
        assert bits(got[n]) == bits(lanes[0])
    assert not np.array_equal(bits(got), bits(rb.in_order(t)))
