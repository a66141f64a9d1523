"""The recovery proposal, host side (no GPU): mcl_host_recovery_proposal against the restatement in recovery_mix_ref.py --
thresholds exactly floor((s_k / s_M) 2^53), non-decreasing and ending at 2^53, an empty range for a zero weight, factors
mcl_host_gaussian_factor's bit for bit, every refusal of P1 with the component named, weights=NULL as all ones."""
import math
import re

import numpy as np
import pytest

import recovery_mix_ref as ref

NAN, INF = float("nan"), float("inf")
TWO53 = 2 ** 53
MCL_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def eng(engine_mod):
    return engine_mod


def rand_cov(rng):
    a = rng.normal(size=(3, 3))
    return a @ a.T * rng.uniform(0.01, 2.0)


def mixture(rng, M):
    means = np.column_stack([rng.uniform(-50, 50, M), rng.uniform(-50, 50, M), rng.uniform(-math.pi, math.pi, M)])
    covs = np.stack([rand_cov(rng) for _ in range(M)])
    return means, covs


WEIGHT_SETS = [
    [1.0],
    [0.0, 2.5],
    [2.5, 0.0],
    [1.0, 1.0, 1.0],
    [0.1, 0.2, 0.3, 0.4],
    [1.0, 0.0, 3.0, 0.25],
    [0.0, 0.0, 1e-300, 0.0],
    [1e308, 1e-308, 7e307],
    [5e-324, 5e-324, 5e-324],
    [3.0, 1.0, 0.0, 0.0],
]


@pytest.mark.parametrize("w", WEIGHT_SETS)
def test_thresholds_are_the_floor_rule(eng, w):
    rng = np.random.default_rng(len(w))
    means, covs = mixture(rng, len(w))
    thr, _ = eng.host_recovery_proposal(means, covs, w)
    total = 0.0
    for v in w:
        total += v
    s, want = 0.0, []
    for v in w:
        s += v
        want.append(int(math.floor((s / total) * 2 ** 53)))
    want[-1] = TWO53
    assert [int(t) for t in thr] == want == ref.thresholds(w)
    assert all(int(a) <= int(b) for a, b in zip(thr, thr[1:])) and int(thr[-1]) == TWO53
    lo = 0
    for k, v in enumerate(w):
        if v == 0.0:
            assert int(thr[k]) == lo or k == len(w) - 1, "a zero weight must leave an empty range"
        lo = int(thr[k])
    # a zero-weight component is never the first k with pick < t_k
    picks = np.array(sorted({0, 1, TWO53 - 1, TWO53 // 2} | {max(int(t) - 1, 0) for t in thr} | {min(int(t), TWO53 - 1) for t in thr}),
                     np.uint64)
    comp = ref.component_of(picks, thr)
    assert comp.min() >= 0 and comp.max() <= len(w) - 1
    assert all(w[k] > 0.0 for k in comp)


@pytest.mark.parametrize("M", [1, 2, 17, 4096])
def test_random_mixtures(eng, M):
    rng = np.random.default_rng(100 + M)
    means, covs = mixture(rng, M)
    w = rng.uniform(0.0, 1.0, M)
    w[rng.uniform(size=M) < 0.2] = 0.0
    w[M // 2] = 0.7
    thr, fac = eng.host_recovery_proposal(means, covs, w)
    assert [int(t) for t in thr] == ref.thresholds(w)
    for k in range(M):
        assert np.array_equal(fac[k, :3].view(np.uint64), means[k].view(np.uint64))
        L = eng.host_gaussian_factor(covs[k])
        want = np.array([L[0, 0], L[1, 0], L[1, 1], L[2, 0], L[2, 1], L[2, 2]])
        assert np.array_equal(fac[k, 3:].view(np.uint64), want.view(np.uint64)), k
    # ... and they are factors: L L^T gives the covariance back (the restatement's too; entry by entry the two may differ where a
    # pivot cancels, so the product is what is compared)
    for f in (fac, ref.factors(means, covs)):
        L = np.zeros((M, 3, 3))
        L[:, 0, 0], L[:, 1, 0], L[:, 1, 1], L[:, 2, 0], L[:, 2, 1], L[:, 2, 2] = (f[:, 3 + i] for i in range(6))
        back = L @ L.transpose(0, 2, 1)
        assert (np.abs(back - covs).max(axis=(1, 2)) <= 1e-12 * np.abs(covs).max(axis=(1, 2))).all()


def test_null_weights_are_all_ones(eng):
    rng = np.random.default_rng(3)
    for M in (1, 3, 7, 1000):
        means, covs = mixture(rng, M)
        a = eng.host_recovery_proposal(means, covs, None)
        b = eng.host_recovery_proposal(means, covs, np.ones(M))
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
        assert [int(t) for t in a[0]] == ref.thresholds([1.0] * M)


def test_singular_covariances_are_allowed(eng):
    means = np.zeros((3, 3))
    covs = np.stack([np.zeros((3, 3)), np.diag([0.04, 0.09, 0.0]), np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.5]])])
    _, fac = eng.host_recovery_proposal(means, covs)
    assert np.array_equal(fac[0, 3:], np.zeros(6))
    assert np.array_equal(fac[1, 3:], [0.2, 0.0, 0.3, 0.0, 0.0, 0.0])
    assert np.array_equal(fac[2, 3:], [1.0, 1.0, 0.0, 0.0, 0.0, math.sqrt(0.5)])


def _bad(eng, means, covs, w, component):
    with pytest.raises(eng.EngineError) as ex:
        eng.host_recovery_proposal(means, covs, w)
    assert ex.value.status == MCL_ERR_INVALID_ARG
    if component is None:
        assert not re.search(r"component \d", str(ex.value)), str(ex.value)
    else:
        assert f"component {component} " in str(ex.value), str(ex.value)


@pytest.mark.parametrize("at", [0, 2, 4])
def test_refusals_name_the_component(eng, at):
    rng = np.random.default_rng(9)
    M = 5
    means, covs = mixture(rng, M)
    w = np.array([1.0, 0.0, 2.0, 0.5, 0.25])
    eng.host_recovery_proposal(means, covs, w)
    for bad in (NAN, INF, -INF):
        for col in range(3):
            m = means.copy()
            m[at, col] = bad
            _bad(eng, m, covs, w, at)
    c = covs.copy(); c[at, 0, 1] += 1e-3 * np.abs(c[at]).max()           # not symmetric
    _bad(eng, means, c, w, at)
    c = covs.copy(); c[at] = np.diag([1.0, -1.0, 1.0])                   # not positive semi-definite
    _bad(eng, means, c, w, at)
    c = covs.copy(); c[at, 2, 2] = NAN
    _bad(eng, means, c, w, at)
    for bad in (-1.0, -5e-324, NAN, INF):
        ww = w.copy()
        ww[at] = bad
        _bad(eng, means, covs, ww, at)
    with pytest.raises(ValueError):
        ref.thresholds([1.0, -1.0])
    with pytest.raises(ValueError):
        ref.factors(means, c)


def test_refused_sums_and_counts(eng):
    import ctypes as C
    rng = np.random.default_rng(11)
    means, covs = mixture(rng, 3)
    _bad(eng, means, covs, [0.0, 0.0, 0.0], None)                        # the sum must be > 0
    _bad(eng, means, covs, [1.5e308, 1.5e308, 0.0], None)                # ... and finite: every weight is, their sum is not
    lib = eng.load_library()
    m1, c1 = mixture(rng, 1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    thr, fac = np.full(1, 7, np.uint64), np.full(9, 7.0)
    for M in (0, -1, 4097, 2 ** 31 - 1):
        assert lib.mcl_host_recovery_proposal(C.c_int32(M), p(m1), p(c1), None, p(thr), p(fac)) == MCL_ERR_INVALID_ARG
    assert lib.mcl_host_recovery_proposal(C.c_int32(1), None, p(c1), None, p(thr), p(fac)) == MCL_ERR_INVALID_ARG
    assert lib.mcl_host_recovery_proposal(C.c_int32(1), p(m1), None, None, p(thr), p(fac)) == MCL_ERR_INVALID_ARG
    bad = np.array([-1.0])
    assert lib.mcl_host_recovery_proposal(C.c_int32(1), p(m1), p(c1), p(bad), p(thr), p(fac)) == MCL_ERR_INVALID_ARG
    assert thr[0] == 7 and (fac == 7.0).all(), "a refused call must write nothing"
    # outputs are optional
    assert lib.mcl_host_recovery_proposal(C.c_int32(1), p(m1), p(c1), None, None, None) == 0
    assert lib.mcl_host_recovery_proposal(C.c_int32(1), p(m1), p(c1), None, p(thr), None) == 0 and thr[0] == TWO53


def test_restated_draw_uses_streams_10_and_11(orc):
    """the restatement's normals against the oracle's Philox, one child at a time, across the high word of the counter"""
    seed, upd = 0x0123_4567_89AB_CDEF, 3
    first = (1 << 32) - 4
    g = np.arange(first, first + 8, dtype=np.uint64)
    n0, n1, n2 = ref.mix_normals(seed, upd, g)
    for i, gi in enumerate(int(v) for v in g):
        o = orc.eng_philox4x32((gi & 0xFFFFFFFF, upd, 10, gi >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u1 = (((int(o[0]) << 32 | int(o[1])) >> 11) + 1) * 2.0 ** -53
        u2 = ((int(o[2]) << 32 | int(o[3])) >> 11) * 2.0 ** -53
        r = math.sqrt(-2.0 * math.log(u1))
        assert n0[i] == pytest.approx(r * math.cos(2 * math.pi * u2), rel=1e-14, abs=1e-15)
        assert n1[i] == pytest.approx(r * math.sin(2 * math.pi * u2), rel=1e-14, abs=1e-15)
        o = orc.eng_philox4x32((gi & 0xFFFFFFFF, upd, 11, gi >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        u1 = (((int(o[0]) << 32 | int(o[1])) >> 11) + 1) * 2.0 ** -53
        u2 = ((int(o[2]) << 32 | int(o[3])) >> 11) * 2.0 ** -53
        assert n2[i] == pytest.approx(math.sqrt(-2.0 * math.log(u1)) * math.cos(2 * math.pi * u2), rel=1e-14, abs=1e-15)
