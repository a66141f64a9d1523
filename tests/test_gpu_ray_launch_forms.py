"""The scenarios of tools/ray_launch_trace.py -- one per branch of the ray stage's host code (launch_rays: every form of k_rays_sweep, the
k_rays_skip / k_rays_march paths, both sorts, the stale layout and the prep fold, the COUNT instantiations, mcl_stage_rays, and the two
legacy kernels) -- held to the oracle.  Per scenario: the kernel and the form its name promises were reached (a scenario that does
not reach its branch compares nothing), and the log-weights of 256 sampled particles are the oracle's, bit for bit (cpp:586-650 ray
cast, 545-579 table, as in tests/test_gpu_sweep.py).  The tool compares two builds of the library over the same list; this module
keeps the list from rotting."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ray_launch_trace as rlt                                    # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sc", rlt.SCENARIOS, ids=[sc["name"] for sc in rlt.SCENARIOS])
def test_form_is_reached_and_log_weights_are_the_oracles(orc, engine_mod, sc):
    r = rlt.run(engine_mod, orc, sc)
    assert r["kernel"] == sc["kernel"]
    if sc["kernel"] == rlt.SWEEP:
        assert r["variant"] == sc["variant"]
    om, p = r["om"], r["particles"]
    pick = np.random.default_rng(3).choice(sc["n"], 256, replace=False)
    L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
    want, _, _ = orc.eng_log_weights(om, np.ascontiguousarray(p[:, pick]), r["ang"], orc.obs_index(r["scan"], om), L)
    assert np.array_equal(r["logw"][pick], want)
