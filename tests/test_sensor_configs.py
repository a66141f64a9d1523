"""Sensor models other than the reference's defaults, without a GPU.

Every z_* / sigma_hit of mcl_config_t is public and read from mcl_config.yaml, and outside the defaults the table can hold zeros
(z_rand = 0: the Gaussian underflows where no other term applies), i.e. -inf log-table entries.  Checked here: the engine's
host table equals the oracle's bit for bit over a grid of models and ranges; the generalised E4 (the finite entries sum exactly
in any order, -inf exactly where T = 0, no NaN); E5's rule for -inf log-weights in the oracle (also when every particle has
one); and the configurations mcl_create and mcl_host_sensor_table refuse before any device is opened."""
import math
from fractions import Fraction

import numpy as np
import pytest

DEFAULTS = dict(z_hit=0.80, z_short=0.01, z_max=0.07, z_rand=0.12, sigma_hit=8.0)
SENSOR_MODELS = {
    "default": {},
    "zrand0": dict(z_rand=0.0),
    "zrand0_sigma0.5": dict(z_rand=0.0, sigma_hit=0.5),
    "zrand0_sigma2": dict(z_rand=0.0, sigma_hit=2.0),
    "zrand0_sigma30": dict(z_rand=0.0, sigma_hit=30.0),
    "sigma0.5": dict(sigma_hit=0.5),
    "sigma2": dict(sigma_hit=2.0),
    "sigma30": dict(sigma_hit=30.0),
    "heavy_short": dict(z_hit=0.2, z_short=0.6, z_max=0.05, z_rand=0.15, sigma_hit=4.0),
    "hit_only_sigma2": dict(z_hit=1.0, z_short=0.0, z_max=0.0, z_rand=0.0, sigma_hit=2.0),
    "hit_only_sigma8": dict(z_hit=1.0, z_short=0.0, z_max=0.0, z_rand=0.0, sigma_hit=8.0),
}
RANGES_PX = [50, 207, 479, 999]
MAX_BEAMS = 1081


def model(name):
    return {**DEFAULTS, **SENSOR_MODELS[name]}


@pytest.mark.parametrize("P", RANGES_PX)
@pytest.mark.parametrize("name", list(SENSOR_MODELS))
def test_host_table_bit_exact_and_generalised_e4(orc, engine_mod, name, P):
    """The engine's table equals the oracle's bit for bit, and the log table meets E4 as DESIGN §3 states it: no NaN, -inf
    exactly where T = 0, and the finite entries -- all multiples of 2^(e_min - 23) -- need at most 53 bits for any sum of
    1081 of them, so a sum of finite entries is exact in any order (checked with Fractions on random draws)."""
    k = model(name)
    T = orc.sensor_table(P, **k)
    assert np.array_equal(engine_mod.host_sensor_table(P, engine_mod.default_config(**k)), T)
    L = orc.eng_log_table(T)                                    # L[r, d] = f(T[d, r])
    assert not np.isnan(L).any()
    assert np.array_equal(L == -np.inf, T.T == 0.0)
    assert not (L == np.inf).any()
    fin = L[np.isfinite(L)]
    assert fin.size > 0 and (fin <= 0.0).all()
    mag = np.abs(fin[fin != 0.0]).astype(np.float32)
    assert (mag >= np.finfo(np.float32).tiny).all()             # no subnormal entries: the exponent bounds the spacing
    e_min = int(np.frexp(mag)[1].min()) - 1                     # |v| in [2^e, 2^(e+1)): ulp 2^(e - 23)
    top = math.ceil(math.log2(MAX_BEAMS * float(mag.max())))
    assert top - (e_min - 23) <= 53, (top, e_min)
    rng = np.random.default_rng(P)
    v = fin[rng.integers(0, fin.size, MAX_BEAMS)].astype(np.float64)
    exact = sum(Fraction(float(t)) for t in v)
    for _ in range(3):
        s = 0.0
        for t in rng.permutation(v):
            s += t
        assert Fraction(s) == exact


def test_zero_z_rand_tables_hold_minus_inf(orc):
    """The counts the issue computed: without z_rand the 479-px table at the default sigma and the 207-px one at sigma 2 hold
    -inf entries (r > d, r < P, Gaussian underflowed), so a particle's log-weight can be -inf."""
    assert (orc.eng_log_table(orc.sensor_table(479, **model("zrand0"))) == -np.inf).sum() == 14594
    assert (orc.eng_log_table(orc.sensor_table(207, **model("zrand0_sigma2"))) == -np.inf).sum() == 8385
    assert np.isfinite(orc.eng_log_table(orc.sensor_table(479))).all()


def _old_formula(orc, logw):
    w = orc.eng_det_exp(logw - logw.max())
    return w, np.floor(w * 2.0 ** 36).astype(np.uint64)


@pytest.mark.parametrize("n", [1, 7, 2000])
def test_all_minus_inf_log_weights_give_zero_weights_and_index_zero(orc, n):
    """E5: logw = -inf -> w = q = 0, also when the maximum is -inf; then Q = 0 and E6 draws parent 0 in both modes, and the
    pose is the reference's over all-zero weights, (0, 0, atan2(0, 0)) = (0, 0, 0)."""
    logw = np.full(n, -np.inf)
    w, q, mx = orc.eng_weights_from_log(logw)
    assert mx == -np.inf
    assert np.array_equal(w, np.zeros(n)) and not np.signbit(w).any()
    assert np.array_equal(q, np.zeros(n, np.uint64))
    k53 = orc.eng_philox_k53(7, 0, 0, n)
    assert np.array_equal(orc.eng_resample_indices(q, 0, n_children=n, k53=k53), np.zeros(n, np.int32))
    assert np.array_equal(orc.eng_resample_indices(q, 1, n_children=n, k0=orc.eng_philox_k0(7, 0)), np.zeros(n, np.int32))
    p = np.random.default_rng(n).normal(size=(3, n))
    assert np.array_equal(orc.expected_pose(p, w), np.zeros(3))


def test_partly_minus_inf_log_weights(orc):
    """Where logw = -inf: w = q = 0 exactly; everywhere else the same bits as det_exp(logw - max), floor(w 2^36) -- what the
    formula gave before the rule (it only differs when the maximum itself is -inf)."""
    rng = np.random.default_rng(3)
    n = 5000
    logw = -rng.uniform(300.0, 1200.0, n)                       # spread wide enough that some weights underflow to 0
    dead = rng.random(n) < 0.5
    logw[dead] = -np.inf
    w, q, mx = orc.eng_weights_from_log(logw)
    assert mx == logw[~dead].max()
    assert (w[dead] == 0.0).all() and (q[dead] == 0).all()
    want_w, want_q = _old_formula(orc, logw[~dead])
    assert np.array_equal(w[~dead], want_w) and np.array_equal(q[~dead], want_q)
    assert (w[~dead] == 0.0).any() and (w[~dead] == 1.0).sum() >= 1
    # the resampling never picks a -inf particle
    idx = orc.eng_resample_indices(q, 0, n_children=n, k53=orc.eng_philox_k53(5, 1, 0, n))
    assert not dead[idx].any()
    idx = orc.eng_resample_indices(q, 1, n_children=n, k0=orc.eng_philox_k0(5, 1))
    assert not dead[idx].any()


def test_det_exp_keeps_nan(orc):
    """The rule is applied where the weights are formed, on logw == -inf: det_exp itself still passes NaN through."""
    assert math.isnan(orc.eng_det_exp([float("nan")])[0])
    assert orc.eng_det_exp([-np.inf])[0] == 0.0


def test_sharded_host_oracle_follows_e5(orc, sibal1_oracle):
    """tests/oracle_shard.py (the CPU stand-in of a shard) forms its weights by the same rule."""
    from oracle_shard import OracleShard
    ang = orc.beam_angles(angle_step=60)
    s = OracleShard(sibal1_oracle, ang, seed=1)
    s.p = np.zeros((3, 4))
    s.logw = np.array([-np.inf, -np.inf, -np.inf, -np.inf])
    s.stage_weights(-np.inf)
    assert np.array_equal(s.w, np.zeros(4)) and np.array_equal(s.q, np.zeros(4, np.uint64))
    assert s.scalars()[1] == 0.0 and np.array_equal(s.scalars()[3:7], np.zeros(4))
    s.logw = np.array([-np.inf, -20.0, -np.inf, -21.0])
    s.stage_weights(-20.0)
    w, q, _ = orc.eng_weights_from_log(s.logw)
    assert np.array_equal(s.w, w) and np.array_equal(s.q, q)


# ---- refusals: mcl_create checks the config before it looks for a device, so these run anywhere
REFUSED = [
    ("z_hit", float("nan")), ("z_hit", -0.1), ("z_short", float("inf")), ("z_short", -1e-9), ("z_max", float("nan")),
    ("z_max", -0.07), ("z_rand", float("-inf")), ("z_rand", -0.12),
    ("sigma_hit", 0.0), ("sigma_hit", -8.0), ("sigma_hit", float("nan")), ("sigma_hit", float("inf")),
    ("squash_factor", float("inf")), ("squash_factor", float("nan")), ("max_range_m", float("inf")), ("max_range_m", float("nan")),
    ("motion_dispersion_x", float("nan")), ("motion_dispersion_x", -0.05), ("motion_dispersion_y", float("inf")),
    ("motion_dispersion_y", -0.025), ("motion_dispersion_theta", float("nan")), ("motion_dispersion_theta", -0.25),
]


def _create_rc(engine_mod, cfg):
    import ctypes as C
    lib = engine_mod.load_library()
    h = C.c_void_p()
    rc = lib.mcl_create(C.byref(cfg), C.byref(h))
    if rc == engine_mod.MCL_OK:              # (cannot happen for the configs below; never leak a handle if it did)
        lib.mcl_destroy(h)
    return rc, lib.mcl_last_error(None).decode()


@pytest.mark.parametrize("field,value", REFUSED, ids=[f"{f}={v}" for f, v in REFUSED])
def test_create_refuses_bad_config(engine_mod, field, value):
    cfg = engine_mod.default_config(**{field: value})
    rc, msg = _create_rc(engine_mod, cfg)
    assert rc == -1, (rc, msg)                   # MCL_ERR_INVALID_ARG, not MCL_ERR_NO_DEVICE: refused before the device check
    stem = field.split("_")[0] if field.startswith(("z_", "motion_")) else field
    assert stem in msg, msg
    with pytest.raises(engine_mod.EngineError, match="mcl_create rc=-1"):
        engine_mod.Engine(**{field: value})


def test_create_refuses_all_zero_mixture(engine_mod):
    cfg = engine_mod.default_config(z_hit=0.0, z_short=0.0, z_max=0.0, z_rand=0.0)
    rc, msg = _create_rc(engine_mod, cfg)
    assert rc == -1 and "all 0" in msg, (rc, msg)
    with pytest.raises(engine_mod.EngineError, match="mcl_create rc=-1"):
        engine_mod.Engine(z_hit=0.0, z_short=0.0, z_max=0.0, z_rand=0.0)


SENSOR_REFUSED = [r for r in REFUSED if r[0].startswith("z_") or r[0] == "sigma_hit"]


@pytest.mark.parametrize("field,value", SENSOR_REFUSED, ids=[f"{f}={v}" for f, v in SENSOR_REFUSED])
def test_host_sensor_table_refuses_bad_sensor_fields(engine_mod, field, value):
    with pytest.raises(engine_mod.EngineError, match="rc=-1"):
        engine_mod.host_sensor_table(50, engine_mod.default_config(**{field: value}))


def test_host_sensor_table_refuses_all_zero_mixture(engine_mod):
    with pytest.raises(engine_mod.EngineError, match="rc=-1"):
        engine_mod.host_sensor_table(50, engine_mod.default_config(z_hit=0.0, z_short=0.0, z_max=0.0, z_rand=0.0))


def test_boundary_values_are_accepted(orc, engine_mod):
    """Zero terms of the mixture (one left non-zero) are a valid model: the host table is built, and equals the oracle's."""
    for k in (dict(z_hit=0.0), dict(z_rand=0.0), dict(z_hit=0.0, z_short=0.0, z_max=0.0, z_rand=1.0),
              dict(z_hit=0.0, z_short=1.0, z_max=0.0, z_rand=0.0)):
        kk = {**DEFAULTS, **k}
        T = orc.sensor_table(60, **kk)
        assert np.array_equal(engine_mod.host_sensor_table(60, engine_mod.default_config(**kk)), T)
