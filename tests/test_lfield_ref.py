"""The likelihood-field sensor model on the host (no GPU): the numpy restatement's field (tests/lfield_ref.py) against a brute
force on small maps, the engine's host restatements (mcl_host_likelihood_field / mcl_host_likelihood_table) against it exactly,
the log-weight restatement against a scalar statement, the defaults and the refused configurations."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lfield_ref as lr
from conftest import GOLDEN

RES = 0.05


@pytest.fixture(scope="module")
def E(engine_mod):
    return engine_mod


def brute(grid, K):
    g = np.asarray(grid)
    H, W = g.shape
    occ = np.argwhere(g > 50)
    if occ.size == 0:
        return np.full((H, W), K, np.uint16)
    yy, xx = np.indices((H, W))
    d2 = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    for oy, ox in occ:
        d2 = np.minimum(d2, (yy - oy) ** 2 + (xx - ox) ** 2)
    return np.minimum(d2, K).astype(np.uint16)


def small_maps():
    rng = np.random.default_rng(17)
    maps = {}
    maps["random"] = rng.choice(np.array([-1, 0, 50, 51, 100], np.int8), size=(23, 37), p=[0.1, 0.8, 0.04, 0.03, 0.03])
    b = np.zeros((19, 19), np.int8)
    b[0, :] = b[-1, :] = b[:, 0] = b[:, -1] = 100
    maps["borders"] = b
    s = np.zeros((31, 17), np.int8)
    s[4, 13] = 100
    maps["single"] = s
    maps["none"] = rng.choice(np.array([-1, 0, 50], np.int8), size=(9, 14))
    maps["non_square"] = rng.choice(np.array([0, 100], np.int8), size=(7, 61), p=[0.97, 0.03])
    maps["corner"] = np.zeros((40, 3), np.int8)
    maps["corner"][39, 2] = 127
    return maps


MAPS = small_maps()


@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("max_occ", [0.2, 0.5, 2.0])
def test_restatement_field_is_the_brute_force(name, max_occ):
    g = MAPS[name]
    K = lr.K_of(max_occ, RES)
    assert np.array_equal(lr.field(g, RES, max_occ), brute(g, K))


@pytest.mark.parametrize("name", sorted(MAPS))
@pytest.mark.parametrize("max_occ", [0.2, 0.5, 2.0])
def test_host_field_is_the_restatement(E, name, max_occ):
    g = MAPS[name]
    assert np.array_equal(E.host_likelihood_field(g, RES, max_occ_dist_m=max_occ), lr.field(g, RES, max_occ))


@pytest.mark.parametrize("mapname", ["Spielberg_map", "sibal1"])
def test_host_field_on_fixture_maps(E, maps_mod, mapname):
    m = maps_mod.load_npz(os.path.join(GOLDEN, f"map_{mapname}.npz"))
    near = 255.5 * float(np.float32(m.resolution))          # K just below the uint16 limit
    for max_occ in (2.0, near):
        assert lr.K_of(max_occ, m.resolution) <= 65535
        assert np.array_equal(E.host_likelihood_field(m.data, m.resolution, max_occ_dist_m=max_occ),
                              lr.field(m.data, m.resolution, max_occ))


TABLES = [
    dict(),
    dict(z_rand=0.0, sigma_hit_m=0.01),                       # the Gaussian underflows: log(0) = -inf from some k on
    dict(z_hit=0.95, z_rand=0.05, sigma_hit_m=0.5, max_occ_dist_m=4.0),
    dict(z_hit=0.0, z_rand=1.0),
    dict(max_occ_dist_m=255.5 * float(np.float32(RES))),      # K near the limit
]


# (every table with K <= 65535 at its resolution; the refusal above it is tested below)
TABLE_CASES = [(f, r, mr, sq) for f in TABLES for r, mr, sq in [(RES, 12.0, 2.2), (0.1, 30.0, 1.0), (0.025, 8.0, 3.5)]
               if lr.K_of(f.get("max_occ_dist_m", 2.0), r) <= 65535]


@pytest.mark.parametrize("fields,res,max_range,squash", TABLE_CASES)
def test_host_table_is_the_restatement(E, fields, res, max_range, squash):
    cfg = E.default_config(max_range_m=max_range, squash_factor=squash)
    got = E.host_likelihood_table(res, cfg, **fields)
    want = lr.table(res, max_range_m=max_range, squash_factor=squash, **fields)
    assert got.size == lr.K_of(fields.get("max_occ_dist_m", 2.0), res) + 1
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if fields.get("z_rand") == 0.0:
        assert np.isneginf(got).any() and np.isfinite(got[0])


def test_defaults_and_mirror(E):
    c = E.default_likelihood_field_config()
    assert (c.z_hit, c.z_rand, c.sigma_hit_m, c.max_occ_dist_m, list(c.reserved)) == (0.5, 0.5, 0.2, 2.0, [0, 0])
    assert C.sizeof(E.LikelihoodFieldConfig) == 40
    assert E.default_likelihood_field_config(sigma_hit_m=0.3).sigma_hit_m == 0.3
    assert lr.K_of(2.0, RES) == 1600 and E.host_likelihood_table(RES).size == 1601


BAD = [("sigma_hit_m", 0.0), ("sigma_hit_m", -0.2), ("sigma_hit_m", math.nan), ("sigma_hit_m", math.inf),
       ("max_occ_dist_m", 0.0), ("max_occ_dist_m", -1.0), ("max_occ_dist_m", math.nan), ("max_occ_dist_m", math.inf),
       ("z_hit", -0.1), ("z_hit", math.nan), ("z_hit", math.inf), ("z_rand", -1.0), ("z_rand", math.inf),
       ("max_occ_dist_m", 13.0),                               # K = 67600 > 65535 at 0.05 m
       ("reserved", (1, 0)), ("reserved", (0, 7))]


@pytest.mark.parametrize("field,value", BAD)
def test_refused_configs(E, field, value):
    g = MAPS["single"]
    for call in (lambda: E.host_likelihood_table(RES, **{field: value}),
                 lambda: E.host_likelihood_field(g, RES, **{field: value})):
        with pytest.raises(E.EngineError) as ex:
            call()
        assert ex.value.status == -1


def test_refused_both_zero(E):
    with pytest.raises(E.EngineError) as ex:
        E.host_likelihood_table(RES, z_hit=0.0, z_rand=0.0)
    assert ex.value.status == -1


def test_log_weight_restatement_against_a_scalar_statement():
    """lfield_ref.log_weights against a plain loop over particles and beams (LF3-LF5), on a small map with particles whose end
    points leave it; and the ambiguity flag on an end point placed exactly on a cell edge."""
    g = MAPS["random"]
    D = lr.field(g, RES, 0.5)
    Lf = lr.table(RES, max_occ_dist_m=0.5)
    K = Lf.size - 1
    rng = np.random.default_rng(3)
    n = 64
    ox, oy = -0.3, 0.2
    p = np.stack([rng.uniform(ox - 0.5, ox + 37 * RES + 0.5, n), rng.uniform(oy - 0.5, oy + 23 * RES + 0.5, n), rng.uniform(-4, 4, n)])
    ang = np.linspace(-2.0, 2.0, 21).astype(np.float32)
    r = rng.uniform(0.0, 1.5, 21).astype(np.float32)
    r[[2, 5, 7, 11, 13]] = [np.nan, np.inf, -0.25, 12.0, 13.0]
    got, alts, n_amb = lr.log_weights(p, ang, r, D, Lf, RES, ox, oy, 12.0, chunk=7)
    res = float(np.float32(RES))
    for i in range(n):
        acc = 0.0
        for j in range(21):
            rj = float(r[j])
            if not (rj >= 0.0 and rj < 12.0):
                continue
            a = p[2, i] + float(ang[j])
            cx = math.floor((p[0, i] + rj * math.cos(a) - ox) / res)
            cy = math.floor((p[1, i] + rj * math.sin(a) - oy) / res)
            d = int(D[cy, cx]) if 0 <= cx < D.shape[1] and 0 <= cy < D.shape[0] else K
            acc += float(Lf[d])
        assert got[i] == acc or (i in alts and acc in alts[i]), i
    # an end point on a cell edge is flagged and both neighbours' sums are listed
    p1 = np.array([[ox + 10 * res], [oy + 10.5 * res], [0.0]])
    w, alts, n_amb = lr.log_weights(p1, np.zeros(1, np.float32), np.array([0.0], np.float32), D, Lf, RES, ox, oy, 12.0)
    assert n_amb.tolist() == [1] and 0 in alts
    assert set(alts[0]) == {float(Lf[D[10, 9]]), float(Lf[D[10, 10]])}
