"""The sensor mount through dist.py's one-device path (the staged calls): a ShardedFilter of one rank with the
HIP engine, the mount set through ShardedFilter.set_sensor_mount, in the device-ordered flow and in the stage-by-stage flow.  The
comparisons are made in the worker (tests/dist_worker_mount.py), which needs its own process for torch.distributed; this test
starts it, as tests/test_dist.py starts tests/dist_worker.py, and reads what it recorded."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_one_rank_sharded_filter_with_a_mount_equals_one_mounted_engine(tmp_path, engine_mod):
    # the device-ordered flow runs from the shards' compact lists: more particles than the one-workgroup tail holds (it writes no
    # list), and enough beams that fewer than a quarter of the set keeps a non-zero fixed-point weight (the list's room)
    n, B = 16384, 541
    env = {k: v for k, v in os.environ.items() if not k.startswith("MCL_")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_worker_mount.py"), str(tmp_path), str(n), str(B)], env=env)
    try:
        assert p.wait(timeout=300) == 0
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
    r = np.load(os.path.join(tmp_path, "rank0.npz"))
    print(f"one rank, {n} x {B}, mount (-0.4, 0.3, 2.5): host waits ordered {r['ordered_waits'].tolist()}, stage by stage {r['sync_waits'].tolist()}; "
          f"exchanges {r['ordered_kinds'].tolist()} / {r['sync_kinds'].tolist()}; log-weights that differ from the base poses' "
          f"{r['ordered_differs'].tolist()} / {r['sync_differs'].tolist()}")
    # the device-ordered flow waits once per update from the second on (the first has no lists yet), the other for every value
    assert r["ordered_kinds"].tolist() == ["dense", "lists", "lists"], r["ordered_kinds"]
    assert r["ordered_waits"][1:].tolist() == [1, 1] and min(r["sync_waits"][1:]) >= 4
