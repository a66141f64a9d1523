"""Group: several GPUs behind one handle, driven by one process (mcl_group_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import Config, load_library
from .host import _c, _check, _mount3, _p, _patch_cells, default_config, default_motion_config


class Group:
    """Several GPUs behind one handle, driven by this one process (mcl_group_*): the particle set is sharded contiguously
    over `devices`; results are bit-identical to one Engine holding all particles."""

    def __init__(self, devices, cfg: Config | None = None, **over):
        self.lib = load_library()
        self.cfg = cfg if cfg is not None else default_config(**over)
        if cfg is not None:
            for k, v in over.items():
                setattr(self.cfg, k, v)
        dev = np.ascontiguousarray(np.asarray(devices, np.int32))
        h = C.c_void_p()
        _check(self.lib.mcl_group_create(C.byref(self.cfg), _p(dev), dev.size, C.byref(h)),
               "mcl_group_create", lambda: self.lib.mcl_group_last_error(None).decode())
        self._h = h
        self.size = int(dev.size)
        self.n_total = 0

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mcl_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        _check(rc, what, lambda: self.lib.mcl_group_last_error(self._h).decode())

    def set_map(self, grid, resolution, origin_x, origin_y):
        g = _c(grid, np.int8)
        H, W = g.shape
        self._chk(self.lib.mcl_group_set_map(self._h, _p(g), W, H, resolution, origin_x, origin_y), "mcl_group_set_map")

    def update_map_region(self, cells2d, x0: int, y0: int):
        """mcl_group_update_map_region: Engine.update_map_region on every engine of the group."""
        c = _patch_cells(cells2d)
        self._chk(self.lib.mcl_group_update_map_region(self._h, _p(c), x0, y0, c.shape[1], c.shape[0], c.strides[0]), "mcl_group_update_map_region")

    def set_beam_angles(self, angles):
        a = _c(angles, np.float32)
        self._chk(self.lib.mcl_group_set_beam_angles(self._h, _p(a), a.size), "mcl_group_set_beam_angles")
        self.n_beams = a.size

    def set_particles(self, p_colmajor, weights):
        p = _c(p_colmajor, np.float64)
        w = _c(weights, np.float64)
        self.n_total = int(p.shape[1])
        self._chk(self.lib.mcl_group_set_particles(self._h, _p(p), _p(w), self.n_total), "mcl_group_set_particles")

    def init_particles_pose(self, pose, n_total):
        q = _c(pose, np.float64)
        self.n_total = int(n_total)
        self._chk(self.lib.mcl_group_init_particles_pose(self._h, _p(q), n_total), "mcl_group_init_particles_pose")

    def init_global(self, n_total):
        self.n_total = int(n_total)
        self._chk(self.lib.mcl_group_init_global(self._h, n_total), "mcl_group_init_global")

    def init_particles_gaussian(self, mean, cov, n_total):
        m, c = _c(mean, np.float64), _c(cov, np.float64)
        assert m.size == 3 and c.size == 9
        self.n_total = int(n_total)
        self._chk(self.lib.mcl_group_init_particles_gaussian(self._h, _p(m), _p(c), n_total), "mcl_group_init_particles_gaussian")

    def set_motion_model(self, model="diff", **fields):
        """Engine.set_motion_model on every shard."""
        if model is None:
            self._chk(self.lib.mcl_group_set_motion_model(self._h, None), "mcl_group_set_motion_model")
            return None
        c = default_motion_config(model=model, **fields)
        self._chk(self.lib.mcl_group_set_motion_model(self._h, C.byref(c)), "mcl_group_set_motion_model")
        return c

    def set_sensor_mount(self, mount):
        """Engine.set_sensor_mount on every shard (mcl_group_set_sensor_mount)."""
        m = _mount3(mount)
        self._chk(self.lib.mcl_group_set_sensor_mount(self._h, _p(m)), "mcl_group_set_sensor_mount")

    def update(self, action, obs):
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_group_update(self._h, _p(a), _p(o), o.size), "mcl_group_update")

    def expected_pose(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_group_expected_pose(self._h, _p(out)), "mcl_group_expected_pose")
        return out

    def get_particles(self):
        out = np.empty((3, self.n_total))
        self._chk(self.lib.mcl_group_get_particles(self._h, _p(out), self.n_total), "mcl_group_get_particles")
        return out

    def get_weights(self):
        out = np.empty(self.n_total)
        self._chk(self.lib.mcl_group_get_weights(self._h, _p(out), self.n_total), "mcl_group_get_weights")
        return out

    def resample_indices(self):
        out = np.empty(self.n_total, np.int32)
        self._chk(self.lib.mcl_group_get_resample_indices(self._h, _p(out), self.n_total), "mcl_group_get_resample_indices")
        return out

    def stage_timings(self):
        out = np.empty(6)
        self._chk(self.lib.mcl_group_get_stage_timings(self._h, _p(out)), "mcl_group_get_stage_timings")
        return out

    def engine(self, i) -> "Engine":
        """Non-owning view of shard i's engine (diagnostics: sample_particles, counters, ...)."""
        from .engine import Engine          # (here, not at the top: engine.py re-exports Group)
        h = C.c_void_p()
        self._chk(self.lib.mcl_group_engine(self._h, i, C.byref(h)), "mcl_group_engine")
        e = Engine.__new__(Engine)
        e.lib, e.cfg, e._h, e.n, e.n_beams, e._borrowed = self.lib, self.cfg, h, self.n_total // self.size, getattr(self, "n_beams", 0), True
        return e

    def exchange_bytes(self):
        out = np.zeros(2, np.uint64)
        self._chk(self.lib.mcl_group_exchange_bytes(self._h, _p(out)), "mcl_group_exchange_bytes")
        return dict(weights_received_per_device=int(out[0]), parent_records_from_peers=int(out[1]),
                    lists=bool(self.lib.mcl_group_exchanged_lists(self._h)))
