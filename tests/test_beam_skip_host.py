"""Beam skipping's host rules (mcl_host_beam_skip_thresholds / mcl_host_beam_skip_plan) without a
device: the integer thresholds against their definitions by brute force, the mask against AMCL's literal loop in Python floats
(tests/beam_skip_ref.py), every refusal of the config, the ABI (symbols, struct layouts against a compiled probe)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import beam_skip_ref as br
import lfield_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [1, 2, 3, 64, 2000, 8193, (1 << 27) - 1]
THRESHOLDS = [0.0, 0.3, 1.0 / 3.0, 0.5, 1.0 - 2.0 ** -53, 1.0]


def least_count(t, n, got):
    """the least c in [1, n + 1] with c / n > t (Python's int / int is the correctly rounded quotient, as (double)c / (double)n
    is): by brute force where n is small; else `got` is checked to be it -- c / n does not decrease with c, so it is the least
    iff it passes, or is n + 1, and its predecessor does not pass"""
    if n <= 8193:
        return next((c for c in range(1, n + 1) if c / n > t), n + 1)
    assert 1 <= got <= n + 1
    assert got == n + 1 or got / n > t
    assert got == 1 or not ((got - 1) / n > t)
    return got


def least_skipped(et, n_used):
    return next((s for s in range(n_used + 1) if float(s) >= et * float(n_used)), n_used + 1)


@pytest.mark.parametrize("n", NS)
def test_min_count_is_the_least_count_that_passes(engine_mod, n):
    rng = np.random.default_rng(n)
    ts = THRESHOLDS + list(rng.random(40))
    for k in sorted(set(int(v) for v in rng.integers(0, n + 1, 12)) | {0, n, n // 2, n // 3}):      # threshold * n an integer,
        t = k / n                                                                                  # and one ulp either side
        ts += [t, math.nextafter(t, 0.0), math.nextafter(t, 2.0)]
    for t in ts:
        if not 0.0 <= t <= 1.0:
            continue
        _, got, _ = engine_mod.host_beam_skip_thresholds(0.05, n, 5, threshold=t)
        assert got == least_count(t, n, got), (n, t, got)
    assert engine_mod.host_beam_skip_thresholds(0.05, n, 5, threshold=0.0)[1] == 1
    assert engine_mod.host_beam_skip_thresholds(0.05, n, 5, threshold=1.0)[1] == n + 1


@pytest.mark.parametrize("n_used", [0, 1, 2, 3, 59, 1039, 1081, 65536])
def test_min_skipped_is_the_least_number_that_passes(engine_mod, n_used):
    rng = np.random.default_rng(n_used)
    ets = [0.0, 0.1, 0.5, 0.9, 1.0, math.nextafter(1.0, 2.0), 1.5, 2.0, 1e300] + list(rng.random(40)) + list(1.0 + rng.random(4))
    for k in range(0, n_used + 1, max(1, n_used // 9)):
        if n_used:
            e = k / n_used
            ets += [e, math.nextafter(e, 0.0), math.nextafter(e, 2.0)]
    for et in ets:
        if et < 0.0:
            continue
        got = engine_mod.host_beam_skip_thresholds(0.05, 7, n_used, error_threshold=et)[2]
        assert got == least_skipped(et, n_used), (n_used, et, got)
        if et == 0.0:
            assert got == 0                         # always integrates all
        if et > 1.0 and n_used:
            assert got == n_used + 1                # never does


@pytest.mark.parametrize("res", [0.05, 0.0579, 0.1, 0.025, 1.0])
def test_ka_is_k_of_the_distance(engine_mod, res):
    for d in (0.5, 0.3, 0.05, 1.0, 2.0, 3.3, 0.5000001):
        ka = engine_mod.host_beam_skip_thresholds(res, 10, 1, distance_m=d)[0]
        assert ka == lr.K_of(d, res) == br.Ka_of(d, res), (res, d)
    assert engine_mod.host_beam_skip_thresholds(res, 10, 1, distance_m=1e6)[0] == 65536 == br.Ka_of(1e6, res)


def check_plan(engine_mod, counts, n, **fields):
    c = engine_mod.default_beam_skip_config(**fields)
    kept, n_skipped, integrate_all = engine_mod.host_beam_skip_plan(counts, n, **fields)
    want = br.amcl_mask(counts, n, c.threshold, c.error_threshold)
    assert np.array_equal(kept, want[0]) and (n_skipped, integrate_all) == want[1:], (n, fields, counts)
    return kept, n_skipped, integrate_all


@pytest.mark.parametrize("n", [1, 3, 64, 2000, 8193])
def test_plan_is_amcls_loop(engine_mod, n):
    rng = np.random.default_rng(100 + n)
    for trial in range(30):
        nu = int(rng.integers(1, 80))
        t = float(rng.choice(THRESHOLDS + [rng.random()]))
        et = float(rng.choice([0.0, 0.5, 0.9, 1.0, 1.5, rng.random()]))
        _, mc, ms = engine_mod.host_beam_skip_thresholds(0.05, n, nu, threshold=t, error_threshold=et)
        counts = rng.integers(0, n + 1, nu).astype(np.uint32)
        near = rng.random(nu) < 0.5                                     # half of the counts at min_count - 1 and at min_count
        counts[near] = np.clip(mc - 1 + rng.integers(0, 2, nu)[near], 0, n)
        kept, n_skipped, integrate_all = check_plan(engine_mod, counts, n, threshold=t, error_threshold=et)
        assert n_skipped == int((counts.astype(np.int64) < mc).sum())
        assert integrate_all == int(n_skipped >= ms)


def test_plan_at_its_edges(engine_mod):
    n, nu = 2000, 20
    _, mc, ms = engine_mod.host_beam_skip_thresholds(0.05, n, nu)
    assert ms == 18
    for below in range(nu + 1):                                          # the flip at exactly min_skipped
        counts = np.where(np.arange(nu) < below, mc - 1, mc).astype(np.uint32)
        kept, n_skipped, integrate_all = check_plan(engine_mod, counts, n)
        assert n_skipped == below and integrate_all == int(below >= ms)
        assert np.array_equal(kept, np.where((np.arange(nu) < below) & (below < ms), 2, 1))
    kept, n_skipped, integrate_all = check_plan(engine_mod, np.full(nu, n, np.uint32), n)                   # all kept
    assert (kept == 1).all() and (n_skipped, integrate_all) == (0, 0)
    kept, n_skipped, integrate_all = check_plan(engine_mod, np.zeros(nu, np.uint32), n, error_threshold=1.5)  # all skipped
    assert (kept == 2).all() and (n_skipped, integrate_all) == (nu, 0)
    kept, n_skipped, integrate_all = check_plan(engine_mod, np.zeros(nu, np.uint32), n)                     # ... unless too many
    assert (kept == 1).all() and (n_skipped, integrate_all) == (nu, 1)
    kept, n_skipped, integrate_all = check_plan(engine_mod, np.zeros(0, np.uint32), n)                      # no used beam
    assert kept.size == 0 and (n_skipped, integrate_all) == (0, 1)
    kept, n_skipped, integrate_all = check_plan(engine_mod, np.full(nu, n, np.uint32), n, threshold=1.0, error_threshold=2.0)
    assert (kept == 2).all() and n_skipped == nu                          # threshold 1 keeps nothing


def test_config_refusals(engine_mod):
    bad = [dict(distance_m=0.0), dict(distance_m=-0.5), dict(distance_m=math.nan), dict(distance_m=math.inf),
           dict(threshold=-1e-9), dict(threshold=1.0000001), dict(threshold=math.nan), dict(threshold=math.inf),
           dict(error_threshold=-0.1), dict(error_threshold=math.nan), dict(error_threshold=math.inf),
           dict(reserved=(1, 0)), dict(reserved=(0, 1))]
    for b in bad:
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_beam_skip_thresholds(0.05, 10, 1, **b)
        assert ei.value.status == -1, b
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_beam_skip_plan([1, 2], 10, **b)
        assert ei.value.status == -1, b
    for res, n, nu in [(0.0, 10, 1), (-1.0, 10, 1), (math.nan, 10, 1), (math.inf, 10, 1), (0.05, 0, 1), (0.05, -1, 1),
                       (0.05, 1 << 31, 1), (0.05, 10, -1)]:
        with pytest.raises(engine_mod.EngineError) as ei:
            engine_mod.host_beam_skip_thresholds(res, n, nu)
        assert ei.value.status == -1, (res, n, nu)
    lib = engine_mod.load_library()
    c = engine_mod.default_beam_skip_config()
    assert lib.mcl_host_beam_skip_thresholds(None, C.c_float(0.05), 10, 1, None, None, None) == -1
    assert lib.mcl_host_beam_skip_plan(C.byref(c), None, 1, 10, None, None, None) == -1      # counts missing
    assert lib.mcl_host_beam_skip_thresholds(C.byref(c), C.c_float(0.05), 10, 1, None, None, None) == 0
    assert lib.mcl_set_beam_skip(None, C.byref(c)) == -1 and lib.mcl_get_beam_skip_state(None, None, None, 0, None) == -1
    with pytest.raises(AttributeError):
        engine_mod.default_beam_skip_config(no_such_field=1)


def test_defaults_are_amcls(engine_mod):
    c = engine_mod.default_beam_skip_config()
    assert (c.distance_m, c.threshold, c.error_threshold, tuple(c.reserved)) == (0.5, 0.3, 0.9, (0, 0))


def test_symbols_and_struct_layouts(engine_mod, tmp_path):
    names = ["mcl_default_beam_skip_config", "mcl_set_beam_skip", "mcl_get_beam_skip_state", "mcl_host_beam_skip_thresholds",
             "mcl_host_beam_skip_plan"]
    lib, leg = engine_mod.load_library(), engine_mod.load_library(legacy=True)
    for n in names:
        assert n in engine_mod.EXPORTS and hasattr(lib, n) and hasattr(leg, n), n
    lib.mcl_abi_version.restype = C.c_int
    assert lib.mcl_abi_version() == 1
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcl_hip_engine.h"\n'
                     'int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mcl_beam_skip_config_t),'
                     'offsetof(mcl_beam_skip_config_t, threshold), offsetof(mcl_beam_skip_config_t, error_threshold),'
                     'offsetof(mcl_beam_skip_config_t, reserved), sizeof(mcl_beam_skip_state_t),'
                     'offsetof(mcl_beam_skip_state_t, min_count), offsetof(mcl_beam_skip_state_t, n_used),'
                     'offsetof(mcl_beam_skip_state_t, integrate_all), offsetof(mcl_beam_skip_state_t, ka));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    cfg, st = engine_mod.BeamSkipConfig, engine_mod.BeamSkipState
    assert got == [C.sizeof(cfg), cfg.threshold.offset, cfg.error_threshold.offset, cfg.reserved.offset, C.sizeof(st),
                   st.min_count.offset, st.n_used.offset, st.integrate_all.offset, st.ka.offset]
