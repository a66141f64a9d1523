"""dist.py's failure protocol, the dense exchange: a rank that has failed exports no records, so what it answers its peers'
parent requests with must not be the unwritten buffer.  The peers run their motion and ray stages on the answer before the error
word voids the update; with large values in it the CPU stand-in's motion model (the reference's angle normalisation, a loop of
2 pi steps) does not return, and the world hangs instead of raising ShardedUpdateError on every rank within seconds."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("call", ["stage_resample_indices", "stage_distinct_parents"])
def test_a_failed_rank_answers_parent_requests_with_zeros(tmp_path, call):
    store = os.path.join(str(tmp_path), "rendezvous")
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MCL_TEST_STORE=store, OMP_NUM_THREADS="2",
                   MCL_DIST_FAIL=f"1:1:{call}", MCL_TEST_EXPECT_FAIL="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker_stale_buffers.py"), "oracle", str(tmp_path),
                                       "96", "3", "0", "sync"], env=env))
    try:
        for p in procs:
            assert p.wait(timeout=90) == 0                  # (a world that passes takes a few seconds)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    res = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    for r in range(2):
        f = res[r]["failures"]
        assert f.shape == (1, 3) and int(f[0, 0]) == 0 and f[0, 2] < 10.0
        assert res[r]["poses"].shape == (2, 3) and np.isfinite(res[r]["poses"]).all()
        assert np.array_equal(res[r]["poses"], res[0]["poses"])
