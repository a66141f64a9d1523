"""mcl_host_search_beam_grid (rule B1 of include/mcl_hip_engine.h) on the host: the angle grid a scan and a
heading count share, against the numpy statement tests/beam_search_ref.py, and what it refuses.  No device is opened."""
import numpy as np
import pytest

import beam_search_ref as br


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def hokuyo(orc):
    return orc.beam_angles()


@pytest.mark.parametrize("pick,n_head,M,s", [
    (slice(None), 72, 1440, 20),
    (slice(None), 1440, 1440, 1),
    (slice(None), 1, 1440, 1440),
    (slice(None, None, 20), 72, 72, 1),
    (slice(None, None, 20), 8, 72, 9),
    (slice(0, 1), 72, 72, 1),
    (slice(0, 1), 5, 5, 1),
])
def test_grid_is_the_statement(engine_mod, hokuyo, pick, n_head, M, s):
    ang = hokuyo[pick].copy()
    got, want = engine_mod.host_search_beam_grid(ang, n_head), br.grid(ang, n_head)
    assert (got["M"], got["heading_step"]) == (M, s) == (want["M"], want["heading_step"])
    assert got["delta"] == want["delta"] == 6.283185307179586 / M
    assert got["max_dev"] == want["max_dev"] <= 4e-6
    a0 = float(ang[0])
    assert np.array_equal(bits(got["phi"]), bits((a0 - 3.141592653589793) + np.arange(M, dtype=np.float64) * got["delta"]))
    assert np.array_equal(bits(got["phi"]), bits(want["phi"]))


def test_the_recorded_deviations(engine_mod, hokuyo):
    """the figures rule B1 quotes for a Hokuyo's angles"""
    assert abs(engine_mod.host_search_beam_grid(hokuyo, 72)["max_dev"] - 2.7e-7) < 0.05e-7
    assert abs(engine_mod.host_search_beam_grid(hokuyo[::20], 72)["max_dev"] - 1.5e-7) < 0.05e-7


def test_headings_sit_on_the_grid(engine_mod, hokuyo):
    """theta_k + a_0 is the grid angle of index k s, to rounding: the identity the score's index (k s + j) mod M rests on"""
    g = engine_mod.host_search_beam_grid(hokuyo, 72)
    theta = engine_mod.host_search_headings(n_headings=72)
    assert np.abs(theta + float(hokuyo[0]) - g["phi"][np.arange(72) * g["heading_step"]]).max() < 1e-14


def refused(engine_mod, ang, n_head):
    with pytest.raises(engine_mod.EngineError) as ei:
        engine_mod.host_search_beam_grid(ang, n_head)
    assert ei.value.status == engine_mod.MCL_ERR_INVALID_ARG
    return ei.value


def test_refusals(engine_mod, hokuyo):
    refused(engine_mod, hokuyo, 7)                                       # 7 does not divide 1440
    refused(engine_mod, hokuyo, 0)
    moved = hokuyo.copy()
    moved[500] += np.float32(1e-4)
    assert refused(engine_mod, moved, 72).max_dev > 9e-5                 # one angle off the grid
    nudged = hokuyo.copy()
    nudged[500] += np.float32(2e-6)                                      # ... and one within the bound
    assert engine_mod.host_search_beam_grid(nudged, 72)["max_dev"] < 4e-6
    refused(engine_mod, hokuyo[::-1].copy(), 72)                         # descending
    refused(engine_mod, np.zeros(5, np.float32), 72)                     # no increment
    inc = 6.283185307179586 / 50.0
    refused(engine_mod, (np.arange(100) * inc).astype(np.float32), 50)   # B = 100 > M = 50
    assert engine_mod.host_search_beam_grid((np.arange(50) * inc).astype(np.float32), 50)["M"] == 50      # B == M is a full turn
    refused(engine_mod, (np.arange(3) * 1e-4).astype(np.float32), 72)    # M = 62832 > 16384
    fine = (np.arange(3) * (6.283185307179586 / 16384.0)).astype(np.float32)
    assert engine_mod.host_search_beam_grid(fine, 64)["M"] == 16384
    bad = hokuyo.copy()
    bad[3] = np.nan
    refused(engine_mod, bad, 72)
    refused(engine_mod, np.zeros(0, np.float32), 72)
