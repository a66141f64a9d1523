"""The host side of the pruned search over a scan sequence (mcl_global_search_sequence_pruned, DESIGN.md §4.21, rules PS1 - PS5 of
include/mcl_hip_engine.h), without a device: both libraries export the call, the Python wrapper refuses wrong shapes before it
touches the library, and the arithmetic tests/test_gpu_search_sequence_pruned.py holds the device's bounds to -- the fold of PS3 --
is itself checked here: its order, +0.0 as its start, -inf.  (tools/search_pruned_check.cpp runs the host functions the call
plans with as a stand-alone program for a sanitizer build.)"""
import numpy as np
import pytest

from search_sequence_pruned_ref import bits, fold


# ---- the library has the call
@pytest.mark.parametrize("legacy", [False, True])
def test_both_libraries_export_the_call(engine_mod, legacy):
    lib = engine_mod.load_library(legacy=legacy)
    assert "mcl_global_search_sequence_pruned" in engine_mod.EXPORTS
    assert hasattr(lib, "mcl_global_search_sequence_pruned")
    assert lib.mcl_abi_version() == 1
    # a null engine is refused before anything else is read
    f = lib.mcl_global_search_sequence_pruned
    assert f(None, None, None, None, None, 1, 1, 1, None, None, None) == engine_mod.MCL_ERR_INVALID_ARG


# ---- the wrapper's shape checks come before the library
class NoLibrary:
    """an Engine's stand-in whose library and handle raise when touched"""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper touched {name} before it checked the shapes")


@pytest.mark.parametrize("scans,rel", [
    (np.ones(61, np.float32), np.zeros((1, 3))),               # scans not (S, B)
    (np.ones((2, 3, 61), np.float32), np.zeros((2, 3))),
    (np.ones((2, 61), np.float32), np.zeros(3)),               # rel not (S, 3)
    (np.ones((2, 61), np.float32), np.zeros((2, 2))),
    (np.ones((2, 61), np.float32), np.zeros((3, 3))),          # one row per scan
    (np.ones((2, 61), np.float32), np.zeros((2, 3, 1))),
])
def test_wrapper_refuses_wrong_shapes_without_a_device(engine_mod, scans, rel):
    with pytest.raises(ValueError):
        engine_mod.Engine.global_search_sequence_pruned(NoLibrary(), scans, rel)


def test_wrapper_signature(engine_mod):
    import inspect
    p = inspect.signature(engine_mod.Engine.global_search_sequence_pruned).parameters
    assert list(p)[:6] == ["self", "scans", "rel", "max_hits", "block", "first_pairs"]
    assert (p["max_hits"].default, p["block"].default, p["first_pairs"].default) == (16, 0, 0)


# ---- the fold of PS3 / SQ4 as the GPU test states it
def test_fold_is_in_scan_order_from_plus_zero():
    # three addends whose sum depends on the order: (a + b) + c != a + (b + c)
    a, b, c = np.float64(1e16), np.float64(-1e16), np.float64(1.0)
    assert fold([a, b, c]) == 1.0 and fold([a, c, b]) == 0.0 and fold([c, a, b]) == 0.0
    x = np.array([0.1, -3.75, 1e-9]), np.array([0.2, 1e-17, -1e-9]), np.array([0.3, 3.75, 5e-324])
    want = ((np.float64(0.0) + x[0]) + x[1]) + x[2]
    assert np.array_equal(bits(fold(x)), bits(want))
    assert not np.array_equal(bits(fold(x)), bits(fold(x[::-1])))           # (0.1 + 0.2) + 0.3 != (0.3 + 0.2) + 0.1
    # the start is +0.0: one addend comes back bit for bit, except that -0.0 becomes +0.0 (SQ4: never -0.0)
    one = np.array([-7.25, 5e-324, -np.inf, 0.0])
    assert np.array_equal(bits(fold([one])), bits(one))
    assert np.array_equal(bits(fold([np.array([-0.0])])), bits(np.array([0.0])))
    # the inputs stay as they were
    keep = x[0].copy()
    fold(x)
    assert np.array_equal(keep, x[0])


def test_fold_with_minus_infinity():
    ninf = -np.inf
    u = [np.array([-1.0, ninf, -2.0, ninf]), np.array([-3.0, -1.0, ninf, ninf]), np.array([-0.5, -0.5, -0.5, ninf])]
    got = fold(u)
    assert got[0] == -4.5 and np.isneginf(got[1:]).all() and not np.isnan(got).any()
    # a bound of -inf still dominates a score of -inf, and only that
    assert (got >= np.array([-4.5, ninf, ninf, ninf])).all()
    assert not (got[1] >= -1e308)


def test_fold_identities_of_the_gpu_test():
    """(ii) two scans: (0.0 + Ua) + Ub; (iii) three identical scans: ((0.0 + U) + U) + U, which is not 3 * U in general"""
    rng = np.random.default_rng(21)
    Ua, Ub = -rng.uniform(1.0, 300.0, 4096), -rng.uniform(1.0, 300.0, 4096)
    assert np.array_equal(bits(fold([Ua, Ub])), bits((0.0 + Ua) + Ub))
    assert np.array_equal(bits(fold([Ua, Ub])), bits(fold([Ub, Ua])))       # two addends commute; three need not (above)
    three = fold([Ua, Ua, Ua])
    assert np.array_equal(bits(three), bits((Ua + Ua) + Ua))
    assert np.allclose(three, 3.0 * Ua, rtol=1e-15, atol=0.0)              # (close to 3 U; the GPU test compares with the fold, never with 3 U)
