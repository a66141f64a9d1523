"""Worker of tests/test_gpu_sensor_mount_dist.py: ONE rank of a ShardedFilter (monte_carlo_localization_amd/dist.py) over gloo with
the HIP engine and a sensor mount set through ShardedFilter.set_sensor_mount -- the staged calls driven from Python
(mcl_stage_resample*, mcl_stage_rays / mcl_stage_rays_async, mcl_stage_weights*, mcl_scan_weights) -- in the device-ordered flow and
in the stage-by-stage flow (MCL_DIST_SYNC=1), three updates each, beside one plain mounted engine with the same seed and
particles.  After every update: particles, fixed-point weights and log-weights equal the plain engine's bit for bit, the sensor
poses are mount_poses of the particles, and the log-weights are the oracle's at sensor_poses().  Writes what it saw to an .npz;
any mismatch ends it with a non-zero status."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

MOUNT = (-0.4, 0.3, 2.5)
SEED = 2024


def read_q(torch, e, n, device):
    qt = torch.empty(n, dtype=torch.int64, device=device)
    e.export_state(0, 0, 0, qt.data_ptr())
    return qt.cpu().numpy().view(np.uint64)


def main():
    out_dir, n, B = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    import torch
    import torch.distributed as dist
    dist.init_process_group(backend="gloo", init_method="file://" + os.path.join(out_dir, "rendezvous"), rank=0, world_size=1)
    import side_geometries as sg
    import whole_set as ws
    from monte_carlo_localization_amd import engine
    from monte_carlo_localization_amd.dist import ShardedFilter
    from oracle import oracle as orc
    g = sg.small()
    om = g.oracle(orc)
    ang = sg.angles(orc, B)
    L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
    s, c = np.sin(g.true_pose[2]), np.cos(g.true_pose[2])
    sensor = (g.true_pose[0] + (c * MOUNT[0] - s * MOUNT[1]), g.true_pose[1] + (s * MOUNT[0] + c * MOUNT[1]), g.true_pose[2] + MOUNT[2])
    obs = sg.perturbed_scan(orc, om, ang, sensor, seed=g.perturb_seed)
    action = (g.res, 0.0, 0.01)
    p0 = sg.cloud_around(g, np.random.default_rng(77), n)
    w0 = np.full(n, 1.0 / n)
    device = torch.device("cuda", 0)
    record = {}
    for flow in ("ordered", "sync"):
        os.environ.pop("MCL_DIST_SYNC", None)
        if flow == "sync":
            os.environ["MCL_DIST_SYNC"] = "1"

        def make():
            e = engine.Engine(max_particles=n, device=0, seed=SEED, resample_mode=0)
            e.set_map(g.data, g.resolution, g.origin_x, g.origin_y)
            e.set_beam_angles(ang)
            return e
        shard, one = make(), make()
        shard.set_particles(p0, w0)
        sf = ShardedFilter(shard, n, device, overlap=False)
        assert sf.device_ordered == (flow == "ordered"), (flow, sf.device_ordered)
        sf.set_sensor_mount(MOUNT)
        assert np.array_equal(shard.sensor_mount(), np.array(MOUNT))
        one.set_sensor_mount(MOUNT)
        one.set_particles(p0, w0)
        waits, differs, kinds = [], [], []
        for k in range(3):
            pose = sf.update(action, obs)
            one.update(action, obs)
            tag = f"{flow} flow, update {k}: "
            parts = shard.get_particles()
            ws.assert_same(tag + "resample indices", shard.resample_indices(), one.resample_indices())
            ws.assert_same(tag + "particles", parts, one.get_particles())
            ws.assert_same(tag + "fixed-point weights", read_q(torch, shard, n, device), read_q(torch, one, n, device))
            ws.assert_same(tag + "log-weights", shard.log_weights(), one.log_weights())
            sp = shard.sensor_poses()
            ws.assert_same(tag + "sensor poses", sp, shard.mount_poses(parts))
            oi = orc.obs_index(obs, om)
            ws.assert_same(tag + "log-weights at the sensor poses", shard.log_weights(), orc.eng_log_weights(om, sp, ang, oi, L)[0])
            differs.append(int((shard.log_weights() != orc.eng_log_weights(om, parts, ang, oi, L)[0]).sum()))
            assert differs[-1] > n // 2, (tag, differs)             # (the mount is seen)
            np.testing.assert_allclose(pose, one.expected_pose(), rtol=0, atol=1e-12)
            waits.append(sf.host_waits)
            kinds.append(sf.exchange_bytes["kind"])
        record[flow + "_waits"] = np.array(waits)
        record[flow + "_differs"] = np.array(differs)
        record[flow + "_kinds"] = np.array(kinds)
        shard.close()
        one.close()
    np.savez(os.path.join(out_dir, "rank0.npz"), **record)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
