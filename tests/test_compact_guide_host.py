"""The guide of the compact parent list (csrc/mcl_compact_guide.h) through its host twins mcl_host_compact_guide and
mcl_host_compact_search -- the code the scan kernel fills the table with and the resampling kernel searches with.

    s = max(0, bit_width(q_total) - m), bucket of a threshold = thr >> s, bmax = q_total >> s
    guide[b] = first p with ccdf[p] >= (b << s), b = 0 .. bmax; guide[b + 1] is n_compact beyond bmax

The search must select numpy.searchsorted(ccdf, thr, side="right") clamped to n - 1 -- the upper_bound of the two-level search
it replaces -- for every threshold below the total; every word 0 .. bmax must have exactly one writer; and for a threshold of
bucket b the answer must lie in [guide[b], guide[b + 1]].  No GPU."""
import numpy as np
import pytest

from monte_carlo_localization_amd import engine

SIZES = [1, 2, 63, 64, 65, 127, 4097]
M = 17
POISON = 0xFFFFFFFF
# totals: below 2^m (s = 0), just below and exactly at a power of two, one of no special form near the top of the fixed-point range
TOTALS = {"s0": 70001, "pow2-1": (1 << 40) - 1, "pow2": 1 << 40, "big": (1 << 58) + 977}


def make_list(n, pattern, total, seed):
    """n strictly positive integer weights of the pattern that add up to `total` exactly; returns their CDF as uint64"""
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        w = np.ones(n)
    elif pattern == "lognormal":
        w = np.exp(3.0 * rng.standard_normal(n))
    else:                                   # one entry with all but n - 1 units of the total
        w = np.zeros(n)
    q = [max(1, int(v / max(w.sum(), 1e-300) * (total - n))) for v in w] if pattern != "heavy" else [1] * n
    heavy = int(rng.integers(0, n)) if pattern == "heavy" else int(np.argmax(w))
    q[heavy] += total - sum(q)              # the remainder goes to one entry (the largest; all of it for "heavy")
    assert min(q) >= 1 and sum(q) == total
    ccdf = np.array(np.cumsum(np.array(q, dtype=object)), dtype=np.uint64)
    assert int(ccdf[-1]) == total
    return ccdf


def thresholds(ccdf, seed):
    q = int(ccdf[-1])
    rng = np.random.default_rng(seed)
    c = ccdf.astype(object)
    edge = [0, q - 1] + [int(v) + d for v in c for d in (-1, 0, 1)]
    edge = np.array([v for v in edge if 0 <= v < q], dtype=np.uint64)
    return np.concatenate((edge, rng.integers(0, q, 20000, dtype=np.uint64)))


@pytest.mark.parametrize("total_kind", list(TOTALS))
@pytest.mark.parametrize("pattern", ["equal", "lognormal", "heavy"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", [M, 8])
def test_guide_and_search(m, n, pattern, total_kind):
    total = TOTALS[total_kind]
    ccdf = make_list(n, pattern, total, seed=n * 131 + len(pattern))
    guide, s, bmax, written = engine.host_compact_guide(ccdf, m, fill=POISON)
    # the shift and the bucket count, restated
    assert s == max(0, total.bit_length() - m) and bmax == total >> s and guide.size == bmax + 2
    assert (s == 0) == (total < (1 << m))
    # every word 0 .. bmax written exactly once (bmax + 1 stores, none left poisoned), nothing behind them touched
    assert written == bmax + 1
    assert not (guide[: bmax + 1] == POISON).any() and guide[bmax + 1] == POISON
    # ... with the value of the definition: the first entry at or above the boundary
    bounds = np.arange(bmax + 1, dtype=np.uint64) << np.uint64(s)
    assert np.array_equal(guide[: bmax + 1], np.searchsorted(ccdf, bounds, side="left").astype(np.uint32))
    assert guide[0] == 0
    # the search against upper_bound
    thr = thresholds(ccdf, seed=7 * n + m)
    want = np.minimum(np.searchsorted(ccdf, thr, side="right"), n - 1)
    got = engine.host_compact_search(ccdf, guide, s, bmax, thr)
    assert np.array_equal(got, want)
    # the range property: for the lowest and the highest threshold of every bucket (the answer is monotone in between) the first
    # entry above it lies in [guide[b], guide[b + 1]], guide[b + 1] = n beyond bmax
    nxt = np.concatenate((guide[1: bmax + 1].astype(np.int64), [n]))
    lo_thr = bounds
    hi_thr = np.minimum((np.arange(1, bmax + 2, dtype=np.uint64) << np.uint64(s)) - np.uint64(1), np.uint64(total - 1))
    live = lo_thr < np.uint64(total)        # (bucket bmax holds no threshold when its boundary is the total itself)
    for t in (lo_thr, hi_thr):
        ans = np.searchsorted(ccdf, t, side="right")
        assert (ans[live] >= guide[: bmax + 1][live]).all() and (ans[live] <= nxt[live]).all()


def test_refusals():
    ccdf = np.array([3, 5, 9], np.uint64)
    lib = engine.load_library()
    import ctypes as C
    g = np.zeros(16, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # a total that is not the list's last entry, a bucket count outside 8 .. 20, a CDF that does not increase, a wrong guide size
    assert lib.mcl_host_compact_guide(p(ccdf), 3, C.c_uint64(10), 8, None, 0, None, None, None) != 0
    assert lib.mcl_host_compact_guide(p(ccdf), 3, C.c_uint64(9), 7, None, 0, None, None, None) != 0
    assert lib.mcl_host_compact_guide(p(ccdf), 3, C.c_uint64(9), 21, None, 0, None, None, None) != 0
    flat = np.array([3, 3, 9], np.uint64)
    assert lib.mcl_host_compact_guide(p(flat), 3, C.c_uint64(9), 8, p(g), 10, None, None, None) != 0
    assert lib.mcl_host_compact_guide(p(ccdf), 3, C.c_uint64(9), 8, p(g), 9, None, None, None) != 0
    assert lib.mcl_host_compact_guide(p(ccdf), 3, C.c_uint64(9), 8, p(g), 10, None, None, None) == 0
