"""ctypes binding of the C ABI in include/mcl_hip_engine.h (libmcl_hip_engine.so): Engine, one engine on one GPU.

This is plumbing only: every numeric step runs in the HIP library.  There is no fallback -- if the shared library is missing or
no gfx950 device is visible the constructor raises.  The ABI itself (constants, structures, signatures, loader) is abi.py, the
CPU twins and config helpers are host.py, Group is group.py; this module re-exports all of them.
"""
from __future__ import annotations

import ctypes as C
import os  # noqa: F401  (part of this module's namespace since before the split)

import numpy as np

from .abi import *  # noqa: F401,F403
from .host import *  # noqa: F401,F403
from .abi import _HERE, _libs  # noqa: F401
from .host import (_c, _check, _defaults, _host_mount_call, _mount3, _offsets3, _p, _patch_cells, _proposal_arrays,  # noqa: F401
                   _rel_rows)


class Engine:
    """One engine == one GPU == one particle shard."""

    def __init__(self, cfg: Config | None = None, **over):
        self.cfg = cfg if cfg is not None else default_config(**over)
        if cfg is not None:
            for k, v in over.items():
                setattr(self.cfg, k, v)
        # (the predecessors of the windowed ray kernel live in the legacy build of the library: load_library)
        self.lib = load_library(legacy=int(self.cfg.ray_kernel) in (RAYS_QUAD, RAYS_CELL))
        h = C.c_void_p()
        _check(self.lib.mcl_create(C.byref(self.cfg), C.byref(h)), "mcl_create", lambda: self.lib.mcl_last_error(None).decode())
        self._h = h
        self.n = 0
        self.n_beams = 0

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.mcl_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        _check(rc, what, lambda: self.lib.mcl_last_error(self._h).decode())

    # -- map / beams
    def set_map(self, grid, resolution, origin_x, origin_y):
        g = _c(grid, np.int8)
        H, W = g.shape
        self._chk(self.lib.mcl_set_map(self._h, _p(g), W, H, np.float32(resolution), origin_x, origin_y), "mcl_set_map")
        self.map_shape = (H, W)
        self.map_resolution = float(np.float32(resolution))

    def update_map_region(self, cells2d, x0: int, y0: int) -> dict:
        """mcl_update_map_region: the cells [x0, x0 + w) x [y0, y0 + h) of the map replaced by cells2d (h, w), every map-derived
        table brought to what set_map of the edited grid would build.  Returns the statistics of the patch."""
        c = _patch_cells(cells2d)
        st = MapPatchStats()
        self._chk(self.lib.mcl_update_map_region(self._h, _p(c), x0, y0, c.shape[1], c.shape[0], c.strides[0], C.byref(st)), "mcl_update_map_region")
        return dict(changed_cells=int(st.changed_cells), changed_stop_cells=int(st.changed_stop_cells), window=tuple(st.window),
                    lf_window=tuple(st.lf_window), free_cells=int(st.free_cells), ms=float(st.ms))

    def map_table(self, name: str) -> np.ndarray:
        """A map-derived table as stored on the device (mcl_get_map_table), flat: one of MAP_TABLES."""
        which, dt = MAP_TABLES[name]
        need = C.c_size_t()
        self._chk(self.lib.mcl_get_map_table(self._h, which, None, 0, C.byref(need)), "mcl_get_map_table")
        out = np.empty(need.value // np.dtype(dt).itemsize, dt)
        self._chk(self.lib.mcl_get_map_table(self._h, which, _p(out), need.value, None), "mcl_get_map_table")
        return out

    @property
    def max_range_px(self) -> int:
        v = C.c_int32()
        self._chk(self.lib.mcl_get_max_range_px(self._h, C.byref(v)), "mcl_get_max_range_px")
        return v.value

    def sensor_table(self):
        P = self.max_range_px
        out = np.empty((P + 1) * (P + 1), np.float64)
        self._chk(self.lib.mcl_get_sensor_table(self._h, _p(out), out.size), "mcl_get_sensor_table")
        return out.reshape(P + 1, P + 1)      # [d, r]

    def set_beam_angles(self, angles):
        a = _c(angles, np.float32)
        self._chk(self.lib.mcl_set_beam_angles(self._h, _p(a), a.size), "mcl_set_beam_angles")
        self.n_beams = a.size

    # -- particles
    def set_particles(self, xyz_colmajor, weights):
        p = _c(xyz_colmajor, np.float64)
        assert p.ndim == 2 and p.shape[0] == 3
        w = _c(weights, np.float64)
        n = p.shape[1]
        assert w.size == n
        self._chk(self.lib.mcl_set_particles(self._h, _p(p), _p(w), n), "mcl_set_particles")
        self.n = self.particle_count()

    def set_particles_shard(self, xyz_colmajor, weights, max_weight_of_the_whole_set):
        """set_particles for one shard of a larger set: weights are quantised against the whole set's maximum weight."""
        p = _c(xyz_colmajor, np.float64)
        w = _c(weights, np.float64)
        n = p.shape[1]
        assert p.ndim == 2 and p.shape[0] == 3 and w.size == n
        self._chk(self.lib.mcl_set_particles_shard(self._h, _p(p), _p(w), n, max_weight_of_the_whole_set), "mcl_set_particles_shard")
        self.n = self.particle_count()

    def init_particles_pose(self, pose, n, first_global_index=0, n_total=None):
        p = _c(pose, np.float64)
        self._chk(self.lib.mcl_init_particles_pose(self._h, _p(p), n, first_global_index, n_total or n), "mcl_init_particles_pose")
        self.n = self.particle_count()

    def init_global(self, n, first_global_index=0, n_total=None):
        self._chk(self.lib.mcl_init_global(self._h, n, first_global_index, n_total or n), "mcl_init_global")
        self.n = self.particle_count()

    def init_particles_gaussian(self, mean, cov, n, first_global_index=0, n_total=None):
        """A Gaussian cloud around `mean` with the 3 x 3 covariance `cov` (an /initialpose, or a cluster of pose_clusters), drawn on
        the device (mcl_init_particles_gaussian)."""
        m, c = _c(mean, np.float64), _c(cov, np.float64)
        assert m.size == 3 and c.size == 9
        self._chk(self.lib.mcl_init_particles_gaussian(self._h, _p(m), _p(c), n, first_global_index, n_total or n), "mcl_init_particles_gaussian")
        self.n = self.particle_count()

    def init_particles_mixture(self, means, covs, counts, n=None, first_global_index=0, n_total=None):
        """One cloud from several Gaussians -- the hits of global_search, or clusters (mcl_init_particles_mixture): means (M, 3),
        covs (M, 3, 3) or one (3, 3) for all, counts (M,) particles per component of the whole set (seed_counts makes them from hit
        scores).  n / first_global_index: this engine's shard of the set (default: all of it)."""
        m, k = _c(means, np.float64).reshape(-1, 3), _c(counts, np.int64).ravel()
        c = _c(covs, np.float64)
        c = _c(np.broadcast_to(c.reshape(-1, 3, 3), (m.shape[0], 3, 3)), np.float64)
        assert k.size == m.shape[0]
        n_total = int(k.sum()) if n_total is None else int(n_total)
        n = n_total - first_global_index if n is None else int(n)
        self._chk(self.lib.mcl_init_particles_mixture(self._h, m.shape[0], _p(m), _p(c), _p(k), n, first_global_index, n_total),
                  "mcl_init_particles_mixture")
        self.n = self.particle_count()

    # -- odometry motion models (off by default: the reference's model)
    def set_motion_model(self, model="diff", **fields):
        """Selects the motion model of the updates that follow: "diff" / "omni" with mcl_default_motion_config's values (AMCL's
        alphas) overridden by `fields`, or None / "reference" for the reference's model."""
        if model is None:
            self._chk(self.lib.mcl_set_motion_model(self._h, None), "mcl_set_motion_model")
            return None
        c = default_motion_config(model=model, **fields)
        self._chk(self.lib.mcl_set_motion_model(self._h, C.byref(c)), "mcl_set_motion_model")
        return c

    def motion_model(self) -> MotionConfig:
        c = MotionConfig()
        self._chk(self.lib.mcl_get_motion_model(self._h, C.byref(c)), "mcl_get_motion_model")
        return c

    # -- sensor mount (off by default)
    def set_sensor_mount(self, mount):
        """The sensor's pose (mx, my, mtheta) in the base frame for the sensor stages that follow (mcl_set_sensor_mount); None or
        (0, 0, 0) = no mount.  The particles stay base poses."""
        m = _mount3(mount)
        self._chk(self.lib.mcl_set_sensor_mount(self._h, _p(m)), "mcl_set_sensor_mount")

    def sensor_mount(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_get_sensor_mount(self._h, _p(out)), "mcl_get_sensor_mount")
        return out

    def mount_poses(self, poses):
        """The sensor poses (3, k) of the base poses (3, k), k <= 65536, formed on the device with the current mount
        (mcl_mount_poses): bit for bit what the sensor stages use.  With no mount a copy."""
        p = np.ascontiguousarray(poses, np.float64)
        if p.ndim != 2 or p.shape[0] != 3:
            raise ValueError("poses must be (3, k): the rows x, y, theta")
        out = np.empty_like(p)
        self._chk(self.lib.mcl_mount_poses(self._h, _p(p), p.shape[1], _p(out)), "mcl_mount_poses")
        return out

    def sensor_poses(self):
        """The (3, n) sensor poses the last sensor stage read (mcl_get_sensor_poses); MCL_ERR_NOT_READY when none has run with a
        mount or the particles have changed since."""
        out = np.empty((3, self.n), np.float64)
        self._chk(self.lib.mcl_get_sensor_poses(self._h, _p(out), self.n), "mcl_get_sensor_poses")
        return out

    def sensor_update_fuse(self, obs):
        """Weighs a further scan into the posterior of the last weighting call (mcl_sensor_update_fuse): the log-weights of `obs`
        under the current beams, mount and sensor model add to the ones in place.  Two lidars:
            e.set_sensor_mount(front); e.set_beam_angles(a_front); e.update(action, scan_front)
            e.set_sensor_mount(rear);  e.set_beam_angles(a_rear);  e.sensor_update_fuse(scan_rear)"""
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_sensor_update_fuse(self._h, _p(o), o.size), "mcl_sensor_update_fuse")

    # -- scan de-skew: per-beam sensor offsets (off by default)
    def set_beam_offsets(self, offsets):
        """The (3, n_beams) table of per-beam sensor offsets (rows ox, oy, dtheta: the sensor's pose when beam j was taken, in the
        sensor's frame at the scan's reference time) for the updates that follow (mcl_set_beam_offsets); None = off.  A node:
            e.set_beam_offsets(host_scan_motion_offsets(twist * sweep_time, B, mount=m)); e.update(action, scan)"""
        if offsets is None:
            self._chk(self.lib.mcl_set_beam_offsets(self._h, None, 0), "mcl_set_beam_offsets")
            return
        o = np.ascontiguousarray(offsets, np.float64)
        if o.ndim != 2 or o.shape[0] != 3:
            raise ValueError("beam offsets are (3, n_beams): the rows ox, oy, dtheta")
        self._chk(self.lib.mcl_set_beam_offsets(self._h, _p(o), o.shape[1]), "mcl_set_beam_offsets")

    def beam_offsets(self):
        """(the table (3, B) as given -- zeros when off --, rule DS1's float angles (B,) -- the beam angles when off --, whether
        offsets are on) (mcl_get_beam_offsets)."""
        o, a, on = np.empty((3, self.n_beams), np.float64), np.empty(self.n_beams, np.float32), C.c_int32()
        self._chk(self.lib.mcl_get_beam_offsets(self._h, _p(o), _p(a), self.n_beams, C.byref(on)), "mcl_get_beam_offsets")
        return o, a, bool(on.value)

    def beam_origins(self, poses):
        """(x, y), each (k, B): rule DS2's origin of every beam of the SENSOR poses (3, k), k <= 65536, formed on the device with the
        current table (mcl_beam_origins): bit for bit where the ray stage casts from (a garbage heading -- NaN, |theta| >= 1e6 -- is
        marched literally from here, its walk having no pixel position).  Offsets off: every beam at the pose."""
        p = np.ascontiguousarray(poses, np.float64)
        if p.ndim != 2 or p.shape[0] != 3:
            raise ValueError("poses must be (3, k): the rows x, y, theta")
        out = np.empty((2, p.shape[1], self.n_beams), np.float64)
        self._chk(self.lib.mcl_beam_origins(self._h, _p(p), p.shape[1], _p(out)), "mcl_beam_origins")
        return out[0], out[1]

    def _proposal_to_base(self, means, covs):
        """The searches and refinements work in the sensor frame: with a mount set, their means and covariances go to the base frame
        (host_sensor_unmount, host_sensor_mount_cov) before they become a proposal.  No mount: the arrays as they are."""
        m = self.sensor_mount()
        if not m.any():
            return means, covs
        means = np.ascontiguousarray(means, np.float64).reshape(-1, 3)
        covs = np.ascontiguousarray(covs, np.float64).reshape(-1, 3, 3)
        base = host_sensor_unmount(m, means.T).T
        return base, np.stack([host_sensor_mount_cov(m, means[i], covs[i], to_base=True) for i in range(means.shape[0])])

    def update_scan(self, action, ranges, angle_step):
        a, r = _c(action, np.float64), _c(ranges, np.float32)
        self._chk(self.lib.mcl_update_scan(self._h, _p(a), _p(r), r.size, angle_step), "mcl_update_scan")
        self.n = self.particle_count()

    def get_particles(self):
        out = np.empty((3, self.n), np.float64)
        self._chk(self.lib.mcl_get_particles(self._h, _p(out), self.n), "mcl_get_particles")
        return out

    def get_weights(self):
        out = np.empty(self.n, np.float64)
        self._chk(self.lib.mcl_get_weights(self._h, _p(out), self.n), "mcl_get_weights")
        return out

    def sample_particles(self, k, uniforms=None):
        u = _c(uniforms, np.float64)
        out = np.empty((3, k), np.float64)
        self._chk(self.lib.mcl_sample_particles(self._h, k, _p(u), _p(out)), "mcl_sample_particles")
        return out

    def particle_mean(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_particle_mean(self._h, _p(out)), "mcl_particle_mean")
        return out

    # -- update
    def update(self, action, obs, normals=None, uniforms=None):
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        nrm, u = _c(normals, np.float64), _c(uniforms, np.float64)
        rows = self.kld_state()[1] if (nrm is not None or u is not None) else self.n    # (KLD on: the size of this update's draw)
        if nrm is not None:
            assert nrm.size == 3 * rows
        if u is not None:
            assert u.size == rows
        self._chk(self.lib.mcl_update(self._h, _p(a), _p(o), o.size, _p(nrm), _p(u)), "mcl_update")
        self.n = self.particle_count()

    # -- KLD-adaptive particle count (off by default)
    def set_kld(self, on=True, **fields):
        """Switches KLD sampling on with mcl_default_kld_config's values overridden by `fields` (max_particles defaults to the
        smaller of 4194304 and the engine's max_particles), or off (on=False)."""
        if not on:
            self._chk(self.lib.mcl_set_kld(self._h, None), "mcl_set_kld")
            return None
        fields.setdefault("max_particles", min(4194304, int(self.cfg.max_particles)))
        k = default_kld_config(**fields)
        self._chk(self.lib.mcl_set_kld(self._h, C.byref(k)), "mcl_set_kld")
        return k

    def kld_state(self):
        """(bins the last update's draw occupied or -1, children the next update draws)"""
        b, n = C.c_int64(), C.c_int64()
        self._chk(self.lib.mcl_get_kld_state(self._h, C.byref(b), C.byref(n)), "mcl_get_kld_state")
        return b.value, n.value

    # -- recovery by random-particle injection (off by default)
    def set_recovery(self, on=True, **fields):
        """Switches recovery on with mcl_default_recovery_config's values overridden by `fields`, or off (on=False); either way
        the averages start unset."""
        if not on:
            self._chk(self.lib.mcl_set_recovery(self._h, None), "mcl_set_recovery")
            return None
        c = default_recovery_config(**fields)
        self._chk(self.lib.mcl_set_recovery(self._h, C.byref(c)), "mcl_set_recovery")
        return c

    def recovery_state(self):
        """(S, F, p of the next update, children the last update injected); S and F are NaN while unset"""
        st, k = (C.c_double * 3)(), C.c_int64()
        self._chk(self.lib.mcl_get_recovery_state(self._h, st, C.byref(k)), "mcl_get_recovery_state")
        return st[0], st[1], st[2], k.value

    def set_recovery_state(self, S, F):
        """Sets the averages (NaN = unset): restores a saved state, or forces the p of the next update."""
        st = (C.c_double * 2)(S, F)
        self._chk(self.lib.mcl_set_recovery_state(self._h, st), "mcl_set_recovery_state")

    # -- the proposal of an injecting update (sensor resetting)
    def set_recovery_proposal(self, means, covs=None, weights=None):
        """The Gaussian mixture the next injecting update draws its injected children from (mcl_set_recovery_proposal): means
        (M, 3), covs (M, 3, 3), weights (M,) or None for equal ones.  means=None clears it (free cells again).  One shot: the first
        resampling update that injects consumes it."""
        if means is None:
            self._chk(self.lib.mcl_set_recovery_proposal(self._h, 0, None, None, None), "mcl_set_recovery_proposal")
            return
        M, m, c, w = _proposal_arrays(means, covs, weights)
        if M == 0:
            raise ValueError("a proposal needs at least one component (None clears it)")
        self._chk(self.lib.mcl_set_recovery_proposal(self._h, M, _p(m), _p(c), _p(w) if w is not None else None), "mcl_set_recovery_proposal")

    def recovery_proposal(self):
        """The proposal in place (mcl_get_recovery_proposal): (thresholds, factors) as host_recovery_proposal returns them, or None."""
        n = C.c_int32()
        self._chk(self.lib.mcl_get_recovery_proposal(self._h, C.byref(n), None, None), "mcl_get_recovery_proposal")
        if n.value == 0:
            return None
        thr, fac = np.zeros(n.value, np.uint64), np.zeros((n.value, 9), np.float64)
        self._chk(self.lib.mcl_get_recovery_proposal(self._h, None, _p(thr), _p(fac)), "mcl_get_recovery_proposal")
        return thr, fac

    def propose_from_scan(self, obs, max_hits=16, refine=True, weights="equal", cov=None, refine_fields=None, pruned=False,
                          **search_fields):
        """Sets the proposal from where the scan `obs` fits the map: the search of the sensor model in use (global_search +
        refine_poses with the likelihood field on, else global_search_beam + refine_poses_beam; the model is never switched and an
        error of the search propagates), hits at -inf dropped, one component per hit from the refined mean and covariance.
        refine=False: the hit poses with the covariance `cov` (default: one lattice step, diag((stride_cells res)^2 twice,
        (2 pi / n_headings)^2)).  weights: "equal" (the default: the same update's sensor model ranks the components anyway, and
        with a thousand beams exp(ll - max) gives everything to one hit) or "likelihood" (seed_counts' shares).  No hit left:
        the proposal is cleared.  Returns the hits.  `search_fields` override mcl_default_search_config, `refine_fields`
        mcl_default_refine_config.  pruned=True (likelihood field only): the same hits from global_search_pruned.
            if e.recovery_state()[2] > 0: e.propose_from_scan(scan)
            e.update(action, scan)"""
        if weights not in ("equal", "likelihood"):
            raise ValueError('weights must be "equal" or "likelihood"')
        lf = self.lib.mcl_get_likelihood_table(self._h, None, 0, None) == MCL_OK
        if pruned and not lf:
            raise EngineError("propose_from_scan: pruned=True needs the likelihood-field model (global_search_pruned)", MCL_ERR_NOT_READY)
        search = self.global_search_pruned if pruned else self.global_search if lf else self.global_search_beam
        hits, _ = search(obs, max_hits=max_hits, **search_fields)
        hits = hits[np.isfinite(hits["log_likelihood"])]
        if hits.size == 0:
            self.set_recovery_proposal(None)
            return hits
        ll = hits["log_likelihood"]
        if refine:
            r, _ = (self.refine_poses if lf else self.refine_poses_beam)(hits["pose"], obs, **(refine_fields or {}))
            means, covs, ll = r["mean"], r["cov"], r["best_log_likelihood"]
        else:
            means = hits["pose"]
            if cov is None:
                sc = default_search_config(**search_fields)
                res = getattr(self, "map_resolution", 0.0)
                cov = np.diag([(sc.stride_cells * res) ** 2, (sc.stride_cells * res) ** 2, (2.0 * np.pi / sc.n_headings) ** 2])
            covs = np.broadcast_to(_c(cov, np.float64).reshape(3, 3), (hits.size, 3, 3))
        w = seed_counts(ll, 1 << 30).astype(np.float64) if weights == "likelihood" else None
        self.set_recovery_proposal(*self._proposal_to_base(means, covs), w)
        return hits

    def propose_from_scans(self, scans, rel, max_hits=16, refine=True, weights="equal", cov=None, refine_fields=None, pruned=True,
                           **search_fields):
        """propose_from_scan over a scan sequence joined by odometry: the hits of global_search_sequence_pruned
        (pruned=False: of global_search_sequence), refined by refine_poses_sequence against the same scans, so that the few
        hypotheses the proposal holds are ranked by every scan and not by the anchor's alone.  Likelihood-field model only
        (MCL_ERR_NOT_READY otherwise; the model is never switched).  propose_from_scan's rules: hits at -inf dropped, one
        component per hit from the refined mean and covariance (refine=False: the hit poses with `cov`, default one lattice
        step), weights "equal" or "likelihood" (seed_counts' shares of the summed scores), the proposal cleared when no hit is
        left.  Returns the hits.
            if e.recovery_state()[2] > 0: e.propose_from_scans(scans, relative_poses(odom))
            e.update(action, scans[-1])"""
        if weights not in ("equal", "likelihood"):
            raise ValueError('weights must be "equal" or "likelihood"')
        if self.lib.mcl_get_likelihood_table(self._h, None, 0, None) != MCL_OK:
            raise EngineError("propose_from_scans: needs the likelihood-field model (the sequence searches and refine_poses_sequence read its field)",
                              MCL_ERR_NOT_READY)
        search = self.global_search_sequence_pruned if pruned else self.global_search_sequence
        hits, _ = search(scans, rel, max_hits=max_hits, **search_fields)
        hits = hits[np.isfinite(hits["log_likelihood"])]
        if hits.size == 0:
            self.set_recovery_proposal(None)
            return hits
        ll = hits["log_likelihood"]
        if refine:
            r, _ = self.refine_poses_sequence(hits["pose"], scans, rel, **(refine_fields or {}))
            means, covs, ll = r["mean"], r["cov"], r["best_log_likelihood"]
        else:
            means = hits["pose"]
            if cov is None:
                sc = default_search_config(**search_fields)
                res = getattr(self, "map_resolution", 0.0)
                cov = np.diag([(sc.stride_cells * res) ** 2, (sc.stride_cells * res) ** 2, (2.0 * np.pi / sc.n_headings) ** 2])
            covs = np.broadcast_to(_c(cov, np.float64).reshape(3, 3), (hits.size, 3, 3))
        w = seed_counts(ll, 1 << 30).astype(np.float64) if weights == "likelihood" else None
        self.set_recovery_proposal(*self._proposal_to_base(means, covs), w)
        return hits

    # -- likelihood-field sensor model (off by default)
    def set_likelihood_field(self, on=True, **fields):
        """Switches the likelihood-field sensor model on with mcl_default_likelihood_field_config's values (AMCL's) overridden by
        `fields` -- z_hit, z_rand, sigma_hit_m, max_occ_dist_m -- or back to the beam model (on=False)."""
        if not on:
            self._chk(self.lib.mcl_set_likelihood_field(self._h, None), "mcl_set_likelihood_field")
            return None
        c = default_likelihood_field_config(**fields)
        self._chk(self.lib.mcl_set_likelihood_field(self._h, C.byref(c)), "mcl_set_likelihood_field")
        return c

    # -- beam skipping for the likelihood field (off by default)
    def set_beam_skip(self, on=True, **fields):
        """Switches beam skipping on with mcl_default_beam_skip_config's values (AMCL's) overridden by keyword (distance_m,
        threshold, error_threshold), or off.  The likelihood field must be on; switching the field off switches this off too."""
        if not on:
            self._chk(self.lib.mcl_set_beam_skip(self._h, None), "mcl_set_beam_skip")
            return
        c = default_beam_skip_config(**fields)
        self._chk(self.lib.mcl_set_beam_skip(self._h, C.byref(c)), "mcl_set_beam_skip")

    def beam_skip_state(self):
        """What the last update with beam skipping decided (mcl_get_beam_skip_state, rule BS6): the record's fields plus `counts`
        (uint32) and `kept` (uint8: 0 not used, 1 summed, 2 skipped), one entry per beam of the scan."""
        B = int(self.n_beams)
        counts, kept, st = np.zeros(B, np.uint32), np.zeros(B, np.uint8), BeamSkipState()
        self._chk(self.lib.mcl_get_beam_skip_state(self._h, _p(counts), _p(kept), B, C.byref(st)), "mcl_get_beam_skip_state")
        out = {name: int(getattr(st, name)) for name, _ in BeamSkipState._fields_}
        out["counts"], out["kept"] = counts, kept
        return out

    def likelihood_field(self):
        """The device's field D of the current map: shape (H, W), uint16."""
        if getattr(self, "map_shape", None) is None:
            raise EngineError("mcl_get_likelihood_field: no map set", MCL_ERR_NOT_READY)
        H, W = self.map_shape
        out = np.empty((H, W), np.uint16)
        self._chk(self.lib.mcl_get_likelihood_field(self._h, _p(out), out.size), "mcl_get_likelihood_field")
        return out

    def likelihood_table(self):
        """The device's table Lf: K + 1 float32 entries."""
        K = C.c_int32()
        self._chk(self.lib.mcl_get_likelihood_table(self._h, None, 0, C.byref(K)), "mcl_get_likelihood_table")
        out = np.empty(K.value + 1, np.float32)
        self._chk(self.lib.mcl_get_likelihood_table(self._h, _p(out), out.size, None), "mcl_get_likelihood_table")
        return out

    # -- the tables under the ray stage, as stored on the device (read-only; tests/test_gpu_ray_tables.py)
    def wedge_fields(self):
        """The wedge fields mcl_set_map built: (WEDGES, Hp, Wps) uint8 in the stored encoding, padding columns included; the
        padded grid is [:, :, :Wp] with Wp = map width + 1."""
        dims = (C.c_int32 * 3)()
        self._chk(self.lib.mcl_get_wedge_fields(self._h, None, 0, dims), "mcl_get_wedge_fields")
        out = np.empty((WEDGES, dims[0], dims[2]), np.uint8)
        self._chk(self.lib.mcl_get_wedge_fields(self._h, _p(out), out.size, None), "mcl_get_wedge_fields")
        return out

    def ring_fields(self):
        """The mirrored, ringed copies of the wedge fields (the global-field and hybrid forms), the whole allocation of
        host_sweep_global_layout as a flat uint8 array; EngineError NOT_READY on an engine that holds none."""
        if getattr(self, "map_shape", None) is None:
            raise EngineError("mcl_get_ring_fields: no map set", MCL_ERR_NOT_READY)
        H, W = self.map_shape
        out = np.empty(max(host_sweep_global_layout(W, H, self.max_range_px)["alloc"], 1), np.uint8)
        self._chk(self.lib.mcl_get_ring_fields(self._h, _p(out), out.size), "mcl_get_ring_fields")
        return out

    def sweep_table(self):
        """((rows, cols) float64, beam_margin): the fp64 table of the last scan as RAYS_SWEEP's ray stage used it."""
        dims = (C.c_int32 * 3)()
        self._chk(self.lib.mcl_get_sweep_table(self._h, None, 0, dims), "mcl_get_sweep_table")
        out = np.empty((dims[0], dims[1]), np.float64)
        self._chk(self.lib.mcl_get_sweep_table(self._h, _p(out), out.size, None), "mcl_get_sweep_table")
        return out, int(dims[2])

    def sort_order(self):
        """The order of the last update's ray stage (radix ordering path): dict(keys, perm, bbox, tilemap, n, fine, fine_sub) -- the
        sorted keys and the particle index per slot, the layout words and tile map the keys were made from (tilemap None for a map
        of more than 8192 tiles), the fine bits of the keys and how many of them per axis are sub-cell bits (None: the rule's).  EngineError NOT_READY when the last ray stage did not order that way."""
        n, fine = C.c_int64(), C.c_int32()
        self._chk(self.lib.mcl_get_sort_order(self._h, None, None, 0, None, None, 0, C.byref(n), C.byref(fine)), "mcl_get_sort_order")
        keys, perm, bbox = np.empty(n.value, np.uint32), np.empty(n.value, np.uint32), np.empty(7, np.int32)
        H, W = self.map_shape
        ntx, nty = sort_tile_grid(W, H)
        tm = np.empty(ntx * nty, np.int32) if ntx * nty <= 8192 else None
        self._chk(self.lib.mcl_get_sort_order(self._h, _p(keys), _p(perm), n.value, _p(bbox), _p(tm) if tm is not None else None,
                                              tm.size if tm is not None else 0, None, None), "mcl_get_sort_order")
        return dict(keys=keys, perm=perm, bbox=bbox, tilemap=tm, n=int(n.value), fine=int(fine.value) & 15,
                    fine_sub=(int(fine.value) >> 4) - 1 if int(fine.value) >> 4 else None)

    def sort_record_form(self) -> str:
        """'heading' when the gather of the last update's radix ordering read (heading, 0, px, py) records the resampling kernel had
        left and took the sincos itself, 'full' when it read (cos, sin, px, py) beside the heading column (mcl_get_sort_record_form)."""
        f = C.c_int32()
        self._chk(self.lib.mcl_get_sort_record_form(self._h, C.byref(f)), "mcl_get_sort_record_form")
        return "heading" if f.value else "full"

    def particle_count(self) -> int:
        n = C.c_int64()
        self._chk(self.lib.mcl_get_particle_count(self._h, C.byref(n)), "mcl_get_particle_count")
        return n.value

    def pose_clusters(self, max_clusters=16, **cfg_fields):
        """The pose hypotheses of the particle set (mcl_pose_clusters): a structured array (CLUSTER_DTYPE) of the
        max_clusters heaviest clusters, heaviest first, and {n_clusters, q_total, q_outside, n_outside}.  `cfg_fields` override
        mcl_default_cluster_config (bin_x_m, bin_y_m, n_theta_bins)."""
        cfg = default_cluster_config(**cfg_fields)
        out = np.zeros(int(max_clusters), CLUSTER_DTYPE)
        n = C.c_int64()
        tot = (C.c_uint64 * 3)()
        self._chk(self.lib.mcl_pose_clusters(self._h, C.byref(cfg), int(max_clusters), _p(out) if out.size else None, C.byref(n), tot),
                  "mcl_pose_clusters")
        return out[:min(n.value, out.size)], dict(n_clusters=n.value, q_total=int(tot[0]), q_outside=int(tot[1]), n_outside=int(tot[2]))

    def cluster_labels(self):
        """Per particle, the rank of its cluster in the last pose_clusters, or -1 (no cluster)."""
        out = np.empty(self.particle_count(), np.int32)
        self._chk(self.lib.mcl_get_cluster_labels(self._h, _p(out), out.size), "mcl_get_cluster_labels")
        return out

    @staticmethod
    def _query_poses(poses):
        """(K, 3) poses, or one length-3 pose, as the K x 3 column-major array the ABI takes"""
        p = np.asarray(poses, np.float64)
        if p.ndim == 1:
            p = p.reshape(1, -1)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("poses must be (K, 3) or a single (x, y, theta)")
        return _c(p.T, np.float64)

    def expected_scans(self, poses, want_steps=False):
        """The expected scan of every pose (mcl_query_scans): the ranges in metres of the beams last set, a
        (K, B) float32 array -- what a particle at that pose would see -- and, with want_steps, the step indices (uint16) too.
        `poses`: (K, 3) rows of (x, y, theta), or one pose.  Reads the map and the beams only: the particle set is untouched."""
        p = self._query_poses(poses)
        K = p.shape[1]
        ranges = np.empty((K, self.n_beams), np.float32)
        steps = np.empty((K, self.n_beams), np.uint16) if want_steps else None
        self._chk(self.lib.mcl_query_scans(self._h, _p(p) if K else None, K, _p(ranges), _p(steps) if want_steps else None), "mcl_query_scans")
        return (ranges, steps) if want_steps else ranges

    def score_poses(self, poses, obs, tol_steps=2):
        """How well the scan `obs` supports every pose (mcl_score_poses): a structured array (POSE_SCORE_DTYPE) with the
        log-likelihood a particle at that pose would get from sensor_update(obs) under the engine's sensor model, and the beams
        that are valid / agree with the cast ray within tol_steps / hit nothing in range.  weight_mode LOG only."""
        p = self._query_poses(poses)
        K = p.shape[1]
        o = _c(obs, np.float32)
        out = np.zeros(K, POSE_SCORE_DTYPE)
        self._chk(self.lib.mcl_score_poses(self._h, _p(p) if K else None, K, _p(o), o.size, int(tol_steps), _p(out)), "mcl_score_poses")
        return out

    def query_counters(self):
        out = np.zeros(2, np.uint64)
        self._chk(self.lib.mcl_get_query_counters(self._h, _p(out)), "mcl_get_query_counters")
        return dict(level3_rays=int(out[0]), device_bytes=int(out[1]))

    # -- global search (the likelihood-field model must be on)
    def global_search(self, obs, max_hits=16, **fields):
        """Scores every pose of a lattice over the map's free cells against the scan `obs` and reports the best-fitting ones
        (mcl_global_search): a structured array (SEARCH_HIT_DTYPE: pose, log_likelihood, index) of at most max_hits hits, best
        first, and {n_hits, n_positions, n_poses, used_beams, device_bytes}.  `fields` override mcl_default_search_config
        (stride_cells, n_headings, beam_stride, nms).  Reads the map, the beams and the likelihood field only."""
        c = default_search_config(**fields)
        o = _c(obs, np.float32)
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(4, np.uint64)
        self._chk(self.lib.mcl_global_search(self._h, C.byref(c), _p(o), o.size, int(max_hits), _p(hits) if hits.size else None, C.byref(n), _p(st)),
                  "mcl_global_search")
        self._search_poses = int(st[1])
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]))

    def global_search_pruned(self, obs, max_hits=16, block=0, first_pairs=0, prune_reserved=(0, 0, 0, 0, 0, 0), **fields):
        """global_search's hits from the blocks of poses an upper bound cannot rule out (mcl_global_search_pruned):
        the same structured array, bit for bit, without the score volume.  block: lattice positions per block side (2, 4 or 8; 0:
        the default), first_pairs: the (block, heading) pairs the first round scores (0: the default).  n_hits is the number of
        hits written, not the candidates of the volume.  Returns (hits, {n_hits, n_positions, n_poses, used_beams, device_bytes,
        pairs, pairs_scored, rounds, guard_fallbacks})."""
        c, pc = default_search_config(**fields), search_prune_config(block, first_pairs, prune_reserved)
        o = _c(obs, np.float32)
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(8, np.uint64)
        self._chk(self.lib.mcl_global_search_pruned(self._h, C.byref(c), C.byref(pc), _p(o), o.size, int(max_hits), _p(hits) if hits.size else None,
                                                    C.byref(n), _p(st)), "mcl_global_search_pruned")
        self._search_pairs = int(st[4])
        return hits[:n.value], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                    device_bytes=int(st[3]), pairs=int(st[4]), pairs_scored=int(st[5]), rounds=int(st[6]),
                                    guard_fallbacks=int(st[7]))

    def global_search_sequence_pruned(self, scans, rel, max_hits=16, block=0, first_pairs=0, prune_reserved=(0, 0, 0, 0, 0, 0), **fields):
        """global_search_sequence's hits from the blocks of poses an upper bound on the summed score cannot rule out
        (mcl_global_search_sequence_pruned): the same structured array, bit for bit, without the score volume.
        `scans`: (S, B) ranges; `rel`: (S, 3) rows of (dx, dy, dtheta); block and first_pairs as in global_search_pruned.  Returns
        (hits, {global_search_pruned's keys, n_scans}); used_beams counts all scans' beams."""
        o, r = np.asarray(scans, np.float32), np.asarray(rel, np.float64)
        if o.ndim != 2:
            raise ValueError("scans must be (S, B)")
        if r.ndim != 2 or r.shape[1] != 3 or r.shape[0] != o.shape[0]:
            raise ValueError("rel must be (S, 3), one row per scan")
        o, r = _c(o, np.float32), _c(r, np.float64)
        c, pc = default_search_config(**fields), search_prune_config(block, first_pairs, prune_reserved)
        S = o.shape[0]
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(9, np.uint64)
        self._chk(self.lib.mcl_global_search_sequence_pruned(self._h, C.byref(c), C.byref(pc), _p(o) if S else None, _p(r) if S else None, S,
                                                             o.shape[1], int(max_hits), _p(hits) if hits.size else None, C.byref(n), _p(st)),
                  "mcl_global_search_sequence_pruned")
        self._search_pairs = int(st[4])
        return hits[:n.value], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                    device_bytes=int(st[3]), pairs=int(st[4]), pairs_scored=int(st[5]), rounds=int(st[6]),
                                    guard_fallbacks=int(st[7]), n_scans=int(st[8]))

    def search_bounds(self):
        """The bounds U of the last global_search_pruned or global_search_sequence_pruned (mcl_get_search_bounds): one double per (block, heading) pair, pair =
        k * n_blocks + b in host_search_blocks' order.  Raises before a pruned search and after set_map."""
        out = np.empty(getattr(self, "_search_pairs", 0) or 1, np.float64)
        self._chk(self.lib.mcl_get_search_bounds(self._h, _p(out), out.size), "mcl_get_search_bounds")
        return out

    def global_search_sequence(self, scans, rel, max_hits=16, **fields):
        """global_search over a sequence of scans joined by odometry (mcl_global_search_sequence): every lattice
        pose is the robot's pose at the anchor, and scan s is scored from where that pose puts the robot at scan s.  `scans`:
        (S, B) ranges; `rel`: (S, 3) rows of (dx, dy, dtheta), the pose at scan s in the anchor's frame (relative_poses makes
        them from odometry).  Returns what global_search returns, plus n_scans; used_beams counts all scans' beams.
            rel = relative_poses(odom)
            hits, _ = e.global_search_sequence(scans, rel)
            r, _ = e.refine_poses_sequence(hits["pose"], scans, rel)"""
        c = default_search_config(**fields)
        o = _c(np.atleast_2d(np.asarray(scans, np.float32)), np.float32)
        if o.ndim != 2:
            raise ValueError("scans must be (S, B)")
        r = _rel_rows(rel)
        if r.shape[0] != o.shape[0]:
            raise ValueError("scans and rel must have one row per scan")
        S = o.shape[0]
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(5, np.uint64)
        self._chk(self.lib.mcl_global_search_sequence(self._h, C.byref(c), _p(o) if S else None, _p(r) if S else None, S, o.shape[1], int(max_hits),
                                                      _p(hits) if hits.size else None, C.byref(n), _p(st)), "mcl_global_search_sequence")
        self._search_poses = int(st[1])
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]), n_scans=int(st[4]))

    def global_search_streamed(self, scans, rel=None, max_hits=16, budget_bytes=0, slab_headings=0, stream_reserved=(0, 0, 0, 0, 0),
                               **fields):
        """global_search (one scan, rel None) or global_search_sequence in slabs of headings (mcl_global_search_streamed, DESIGN.md
        §4.16): the same hits, bit for bit, from at most `budget_bytes` of slab buffers (0: 1 GiB), for lattices of up to 2^40
        poses.  slab_headings = 0 takes the largest slab that fits.  Keeps no volume (search_scores raises afterwards).  Returns
        (hits, {n_hits, n_positions, n_poses, used_beams, device_bytes, slab_headings, n_slabs, headings_scored,
        candidates_compacted})."""
        c = default_search_config(**fields)
        sc = search_stream_config(budget_bytes, slab_headings, stream_reserved)
        o = _c(np.atleast_2d(np.asarray(scans, np.float32)), np.float32)
        if o.ndim != 2:
            raise ValueError("scans must be (B,) or (S, B)")
        S = o.shape[0]
        r = None
        if rel is not None:
            r = _rel_rows(rel)
            if r.shape[0] != S:
                raise ValueError("scans and rel must have one row per scan")
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(8, np.uint64)
        self._chk(self.lib.mcl_global_search_streamed(self._h, C.byref(c), C.byref(sc), _p(o) if o.size else None,
                                                      _p(r) if r is not None and r.size else None, S, o.shape[1], int(max_hits),
                                                      _p(hits) if hits.size else None, C.byref(n), _p(st)), "mcl_global_search_streamed")
        self._search_poses = 0
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]), slab_headings=int(st[4]), n_slabs=int(st[5]),
                                                    headings_scored=int(st[6]), candidates_compacted=int(st[7]))

    def global_search_beam(self, obs, max_hits=16, table_budget_bytes=0, **fields):
        """global_search under the beam model (mcl_global_search_beam): the lattice ranked by the table sum over
        cast rays that every update weights particles with, from a per-position ray table shared by all headings.  The scan must
        be evenly spaced and n_headings must divide its angle grid (host_search_beam_grid).  The likelihood field may be on or
        off.  `table_budget_bytes` (0: 256 MiB) bounds the table: the lattice is walked in tiles of positions.  Returns (hits,
        {n_hits, n_positions, n_poses, used_beams, device_bytes, grid_angles, tile_positions, n_tiles, level3_rays})."""
        c = default_search_config(**fields)
        o = _c(obs, np.float32)
        hits = np.zeros(int(max_hits), SEARCH_HIT_DTYPE)
        n, st = C.c_int64(), np.zeros(8, np.uint64)
        self._chk(self.lib.mcl_global_search_beam(self._h, C.byref(c), _p(o), o.size, int(table_budget_bytes), int(max_hits),
                                                  _p(hits) if hits.size else None, C.byref(n), _p(st)), "mcl_global_search_beam")
        self._search_poses, self._search_beam_M = int(st[1]), int(st[4])
        return hits[:min(n.value, hits.size)], dict(n_hits=n.value, n_positions=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]),
                                                    device_bytes=int(st[3]), grid_angles=int(st[4]), tile_positions=int(st[5]),
                                                    n_tiles=int(st[6]), level3_rays=int(st[7]))

    def search_beam_table(self):
        """The ray table of the last tile of the last global_search_beam (mcl_get_search_beam_table): (first_position, steps) with
        steps of shape (n_positions_of_the_tile, M), uint16 -- E3's step from each position at each grid angle.  M is the
        grid_angles this object's last global_search_beam reported (the C call takes the size and checks it)."""
        first, cnt = C.c_int64(), C.c_int64()
        self._chk(self.lib.mcl_get_search_beam_table(self._h, None, 0, C.byref(first), C.byref(cnt)), "mcl_get_search_beam_table")
        M = getattr(self, "_search_beam_M", 0)
        out = np.empty(cnt.value * M, np.uint16)
        self._chk(self.lib.mcl_get_search_beam_table(self._h, _p(out), out.size, None, None), "mcl_get_search_beam_table")
        return int(first.value), out.reshape(cnt.value, M)

    def search_scores(self, n_headings=None):
        """The score volume of the last global_search or global_search_sequence (mcl_get_search_scores): n_headings * n_positions doubles, heading-major;
        with n_headings, reshaped to (n_headings, n_positions)."""
        out = np.empty(getattr(self, "_search_poses", 0) or 1, np.float64)
        self._chk(self.lib.mcl_get_search_scores(self._h, _p(out), out.size), "mcl_get_search_scores")
        return out.reshape(int(n_headings), -1) if n_headings else out

    def search_bytes(self) -> int:
        """Bytes of device memory the search's buffers have asked for so far (0 on an engine that never searched)."""
        v = C.c_uint64()
        self._chk(self.lib.mcl_get_search_bytes(self._h, C.byref(v)), "mcl_get_search_bytes")
        return int(v.value)

    # -- pose refinement (the likelihood-field model must be on)
    def refine_poses(self, poses, obs, **fields):
        """Scores a dense window of poses around every seed pose against the scan `obs` (mcl_refine_poses): a structured array
        (REFINE_DTYPE: best, best_log_likelihood, seed_log_likelihood, best_index, mean, cov, weight_sum), one record per seed, and
        {n_win, n_poses, used_beams, device_bytes}.  `poses`: (M, 3) rows of (x, y, theta), or one pose -- the hits of global_search,
        cluster means, an /initialpose.  `fields` override mcl_default_refine_config (half_xy, half_theta, step_xy_cells,
        step_theta_rad, beam_stride).  Reads the beams and the likelihood field only.  The chain from one scan to a cloud:
            hits, _ = e.global_search(obs)
            r, _ = e.refine_poses(hits["pose"], obs)
            e.init_particles_mixture(r["mean"], r["cov"], seed_counts(r["best_log_likelihood"], n))"""
        c = default_refine_config(**fields)
        p = self._query_poses(poses)
        M = p.shape[1]
        o = _c(obs, np.float32)
        out = np.zeros(M, REFINE_DTYPE)
        st = np.zeros(4, np.uint64)
        self._chk(self.lib.mcl_refine_poses(self._h, C.byref(c), _p(p) if M else None, M, _p(o), o.size, _p(out) if M else None, _p(st)),
                  "mcl_refine_poses")
        self._refine_shape = (M, int(st[0]))
        return out, dict(n_win=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]), device_bytes=int(st[3]))

    def refine_poses_beam(self, poses, obs, **fields):
        """refine_poses under the beam model (mcl_refine_poses_beam): the same window, every pose scored by the
        table sum over cast rays that every update weights particles with -- what score_poses returns with the likelihood field
        off -- in one kernel that stores no ray.  The likelihood field may be on or off.  Returns (records, {n_win, n_poses,
        used_beams, device_bytes, rays, level3_rays}).  The chain from one scan to a cloud, under one model:
            hits, _ = e.global_search_beam(obs, beam_stride=10)
            r, _ = e.refine_poses_beam(hits["pose"], obs)
            e.init_particles_mixture(r["mean"], r["cov"], seed_counts(r["best_log_likelihood"], n))"""
        c = default_refine_config(**fields)
        p = self._query_poses(poses)
        M = p.shape[1]
        o = _c(obs, np.float32)
        out = np.zeros(M, REFINE_DTYPE)
        st = np.zeros(6, np.uint64)
        self._chk(self.lib.mcl_refine_poses_beam(self._h, C.byref(c), _p(p) if M else None, M, _p(o), o.size, _p(out) if M else None, _p(st)),
                  "mcl_refine_poses_beam")
        self._refine_shape = (M, int(st[0]))
        return out, dict(n_win=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]), device_bytes=int(st[3]), rays=int(st[4]),
                         level3_rays=int(st[5]))

    def refine_poses_sequence(self, poses, scans, rel, **fields):
        """refine_poses against a sequence of scans joined by odometry (mcl_refine_poses_sequence): every seed and
        every window pose is the robot's pose at the anchor, and scan s is scored from where that pose puts the robot at scan s,
        so the records keep the ranking of the sequence search that made the seeds.  `scans`: (S, B) ranges; `rel`: (S, 3) rows
        of (dx, dy, dtheta), the pose at scan s in the anchor's frame (relative_poses makes them from odometry).  Returns
        (records, {refine_poses' keys, n_scans}); used_beams counts all scans' beams, the log-likelihoods are summed scores.
            rel = relative_poses(odom)
            hits, _ = e.global_search_sequence_pruned(scans, rel)
            r, _ = e.refine_poses_sequence(hits["pose"], scans, rel)
            e.init_particles_mixture(r["mean"], r["cov"], seed_counts(r["best_log_likelihood"], n))"""
        c = default_refine_config(**fields)
        p = self._query_poses(poses)
        M = p.shape[1]
        o = _c(np.atleast_2d(np.asarray(scans, np.float32)), np.float32)
        if o.ndim != 2:
            raise ValueError("scans must be (S, B)")
        r = _rel_rows(rel)
        if r.shape[0] != o.shape[0]:
            raise ValueError("scans and rel must have one row per scan")
        S = o.shape[0]
        out = np.zeros(M, REFINE_DTYPE)
        st = np.zeros(5, np.uint64)
        self._chk(self.lib.mcl_refine_poses_sequence(self._h, C.byref(c), _p(p) if M else None, M, _p(o) if o.size else None, _p(r) if S else None, S,
                                                     o.shape[1], _p(out) if M else None, _p(st)), "mcl_refine_poses_sequence")
        self._refine_shape = (M, int(st[0]))
        return out, dict(n_win=int(st[0]), n_poses=int(st[1]), used_beams=int(st[2]), device_bytes=int(st[3]), n_scans=int(st[4]))

    def refine_scores(self):
        """The score volume of the last refine_poses, refine_poses_beam or refine_poses_sequence (mcl_get_refine_scores): (M, n_win)
        doubles, window index ix fastest."""
        shape = getattr(self, "_refine_shape", None) or (1, 1)
        out = np.empty(shape, np.float64)
        self._chk(self.lib.mcl_get_refine_scores(self._h, _p(out), out.size), "mcl_get_refine_scores")
        return out

    def refine_bytes(self) -> int:
        """Bytes of device memory the refinement's buffers have asked for so far (0 on an engine that never refined)."""
        v = C.c_uint64()
        self._chk(self.lib.mcl_get_refine_bytes(self._h, C.byref(v)), "mcl_get_refine_bytes")
        return int(v.value)

    def sensor_update(self, obs):
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_sensor_update(self._h, _p(o), o.size), "mcl_sensor_update")

    def expected_pose(self):
        out = np.empty(3)
        self._chk(self.lib.mcl_expected_pose(self._h, _p(out)), "mcl_expected_pose")
        return out

    def stage_timings(self):
        out = np.empty(6)
        self._chk(self.lib.mcl_get_stage_timings(self._h, _p(out)), "mcl_get_stage_timings")
        return out

    # -- diagnostics
    def resample_indices(self):
        out = np.empty(self.n, np.int32)
        self._chk(self.lib.mcl_get_resample_indices(self._h, _p(out), self.n), "mcl_get_resample_indices")
        return out

    def ray_steps(self):
        """Step index of every ray of the last update (needs keep_ray_steps): uint8 up to 255 px of range, uint16 beyond."""
        if self.max_range_px > 255:
            out = np.empty(self.n * self.n_beams, np.uint16)
            self._chk(self.lib.mcl_get_ray_steps16(self._h, _p(out), out.size), "mcl_get_ray_steps16")
        else:
            out = np.empty(self.n * self.n_beams, np.uint8)
            self._chk(self.lib.mcl_get_ray_steps(self._h, _p(out), out.size), "mcl_get_ray_steps")
        return out.reshape(self.n, self.n_beams)

    def log_weights(self):
        out = np.empty(self.n, np.float64)
        self._chk(self.lib.mcl_get_log_weights(self._h, _p(out), self.n), "mcl_get_log_weights")
        return out

    def counters(self):
        out = np.zeros(4, np.uint64)
        self._chk(self.lib.mcl_get_counters(self._h, _p(out)), "mcl_get_counters")
        return dict(exact_fallback_rays=int(out[0]), off_window_particles=int(out[1]), probes=int(out[2]),
                    level2_rays=int(out[3]))

    def compact_list(self):
        """(entries of the compact parent list that describes the current weights or -1, whether the last resampling used one)"""
        n, u = C.c_int64(), C.c_int32()
        self._chk(self.lib.mcl_get_compact_list(self._h, C.byref(n), C.byref(u)), "mcl_get_compact_list")
        return n.value, bool(u.value)

    def compact_guide(self):
        """mcl_get_compact_guide: the guide of the compact parent list as the device holds it, a dict of guide (bmax + 1 uint32
        words), ccdf (the list's uint64 CDF column), s, bmax, n_compact, q_total, m and used (the last update's resampling
        searched through the guide).  EngineError (NOT_READY) without a list or a guide."""
        info = np.zeros(6, np.int64)
        self._chk(self.lib.mcl_get_compact_guide(self._h, None, 0, None, 0, _p(info)), "mcl_get_compact_guide")
        if info[1] < 0:
            raise EngineError("mcl_get_compact_guide: no compact list with a guide describes the current particles", MCL_ERR_NOT_READY)
        guide, ccdf = np.empty(int(info[1]) + 1, np.uint32), np.empty(int(info[2]), np.uint64)
        self._chk(self.lib.mcl_get_compact_guide(self._h, _p(guide), guide.size, _p(ccdf), ccdf.size, _p(info)), "mcl_get_compact_guide")
        return dict(guide=guide, ccdf=ccdf, s=int(info[0]), bmax=int(info[1]), n_compact=int(info[2]), q_total=int(np.uint64(info[3])),
                    m=int(info[4]), used=bool(info[5]))

    def compact_guide_used(self) -> bool:
        """whether the last update's resampling searched the compact list through its guide (mcl_get_compact_guide)"""
        info = np.zeros(6, np.int64)
        self._chk(self.lib.mcl_get_compact_guide(self._h, None, 0, None, 0, _p(info)), "mcl_get_compact_guide")
        return bool(info[5])

    def set_debug_count_probes(self, on):
        self._chk(self.lib.mcl_set_debug_count_probes(self._h, 1 if on else 0), "mcl_set_debug_count_probes")

    def set_debug_force_exact(self, level):
        self._chk(self.lib.mcl_set_debug_force_exact(self._h, int(level)), "mcl_set_debug_force_exact")

    def ray_kernel_ms(self):
        v = C.c_double()
        self._chk(self.lib.mcl_get_ray_kernel_ms(self._h, C.byref(v)), "mcl_get_ray_kernel_ms")
        return v.value

    def effective_sample_size(self):
        """(N_eff of the current weights, whether the last update resampled)"""
        v, r = C.c_double(), C.c_int32()
        self._chk(self.lib.mcl_get_effective_sample_size(self._h, C.byref(v), C.byref(r)), "mcl_get_effective_sample_size")
        return v.value, bool(r.value)

    def ray_kernel_id(self):
        """The MCL_RAYS_* enumerator of the kernel the last ray stage ran (mcl_get_ray_kernel_id; 0: none yet)."""
        v = C.c_int32()
        self._chk(self.lib.mcl_get_ray_kernel_id(self._h, C.byref(v)), "mcl_get_ray_kernel_id")
        return v.value

    def ray_kernel_name(self):
        return {1: "k_rays_march", 2: "k_rays_skip", 3: "k_rays_quad", 4: "k_rays_cell", 5: "k_rays_sweep", 6: "k_rays_deskew"}.get(self.ray_kernel_id(), "?")

    def ray_kernel_variant(self):
        """Form of k_rays_sweep the last ray stage ran: dict(global_fields, hybrid, turned_directions, pairs)."""
        v = (C.c_int32 * 3)()
        self._chk(self.lib.mcl_get_ray_kernel_variant(self._h, v), "mcl_get_ray_kernel_variant")
        return dict(global_fields=v[0] == 1, hybrid=v[0] == 2, turned_directions=bool(v[1]), pairs=bool(v[2]))

    RAY_KERNEL_NAMES = {0: None, 1: "k_rays_march", 2: "k_rays_skip", 3: "k_rays_quad", 4: "k_rays_cell", 5: "k_rays_sweep", 6: "k_rays_deskew"}

    def planned_ray_kernel(self, n_particles=0):
        """(kernel an update over n_particles WILL run -- None: the configured one cannot run with this map / beam set --, what
        decided): callable before the first update, once the map and the beam angles are set."""
        v, why = C.c_int32(), C.c_char_p()
        self._chk(self.lib.mcl_get_planned_ray_kernel(self._h, int(n_particles), C.byref(v), C.byref(why)), "mcl_get_planned_ray_kernel")
        return self.RAY_KERNEL_NAMES.get(v.value, "?"), (why.value or b"").decode()

    # -- multi-GPU staging (raw device pointers as ints)
    def device_ptr(self, which) -> int:
        p = C.c_void_p()
        self._chk(self.lib.mcl_device_ptr(self._h, which, C.byref(p)), "mcl_device_ptr")
        return int(p.value or 0)

    def export_state(self, d_x=0, d_y=0, d_th=0, d_q=0):
        self._chk(self.lib.mcl_export_state(self._h, C.c_void_p(d_x or None), C.c_void_p(d_y or None), C.c_void_p(d_th or None),
                                            C.c_void_p(d_q or None)), "mcl_export_state")

    def scalars(self):
        out = np.empty(8)
        self._chk(self.lib.mcl_get_scalars(self._h, _p(out)), "mcl_get_scalars")
        return out

    def host_scalars(self):
        """SCALARS as the last stage call read them back (no device access)."""
        out = np.empty(8)
        self._chk(self.lib.mcl_get_host_scalars(self._h, _p(out)), "mcl_get_host_scalars")
        return out

    def stage_propagate(self, d_px, d_py, d_pth, d_cdf, n_parents, q_total, child_first, n_children_total, action, obs):
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_stage_propagate(self._h, C.c_void_p(d_px), C.c_void_p(d_py), C.c_void_p(d_pth), C.c_void_p(d_cdf), n_parents, q_total,
                                               child_first, n_children_total, _p(a), _p(o), o.size), "mcl_stage_propagate")

    def stage_resample(self, d_px, d_py, d_pth, d_cdf, n_parents, q_total, child_first, n_children_total, action):
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_resample(self._h, C.c_void_p(d_px), C.c_void_p(d_py), C.c_void_p(d_pth), C.c_void_p(d_cdf), n_parents, q_total,
                                              child_first, n_children_total, _p(a)), "mcl_stage_resample")

    def export_records(self, d_records):
        self._chk(self.lib.mcl_export_records(self._h, C.c_void_p(d_records)), "mcl_export_records")

    def stage_resample_records(self, d_records, d_cdf, n_parents, q_total, child_first, n_children_total, action):
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_resample_records(self._h, C.c_void_p(d_records), C.c_void_p(d_cdf), n_parents, q_total, child_first,
                                                      n_children_total, _p(a)), "mcl_stage_resample_records")

    def stage_resample_indices(self, d_cdf, n_parents, q_total, child_first, n_children_total, d_parent_idx):
        self._chk(self.lib.mcl_stage_resample_indices(self._h, C.c_void_p(d_cdf), n_parents, q_total, child_first, n_children_total,
                                                      C.c_void_p(d_parent_idx)), "mcl_stage_resample_indices")

    def stage_distinct_parents(self, d_parent, n_children, n_total, d_distinct, d_slot) -> int:
        """Distinct parents (ascending) of `n_children` global parent indices + every child's position among them; returns
        their number.  All pointers are device memory (int32 in, int64 / int32 out)."""
        cnt = C.c_int64()
        self._chk(self.lib.mcl_stage_distinct_parents(self._h, C.c_void_p(d_parent), n_children, n_total, C.c_void_p(d_distinct), C.c_void_p(d_slot),
                                                      C.byref(cnt)), "mcl_stage_distinct_parents")
        return int(cnt.value)

    def export_records_at(self, d_index, count, d_out):
        """Packed records of the listed local particles (device int64 indices) -> d_out[count] (device)."""
        self._chk(self.lib.mcl_export_records_at(self._h, C.c_void_p(d_index), count, C.c_void_p(d_out)), "mcl_export_records_at")

    def stage_motion_records(self, d_records, n_records, d_record_of_child, child_first, n_children_total, action):
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_motion_records(self._h, C.c_void_p(d_records), n_records, C.c_void_p(d_record_of_child), child_first,
                                                    n_children_total, _p(a)), "mcl_stage_motion_records")

    @staticmethod
    def compact_chunk_bytes(chunk_entries) -> int:
        b = C.c_int64()
        _check(load_library().mcl_compact_chunk_bytes(chunk_entries, C.byref(b)), "mcl_compact_chunk_bytes")
        return b.value

    def export_compact(self, d_chunk, chunk_entries):
        """This shard's compact parent list -> d_chunk (device memory of compact_chunk_bytes(chunk_entries))."""
        self._chk(self.lib.mcl_export_compact(self._h, C.c_void_p(d_chunk), chunk_entries), "mcl_export_compact")

    def stage_resample_compact(self, d_chunks, n_shards, chunk_entries, counts, totals, n_per_shard, self_shard, child_first, n_children_total, action):
        a = _c(action, np.float64)
        c = np.ascontiguousarray(np.asarray(counts, np.int64))
        t = np.ascontiguousarray(np.asarray(totals, np.uint64))
        assert c.size == n_shards and t.size == n_shards
        self._chk(self.lib.mcl_stage_resample_compact(self._h, C.c_void_p(d_chunks), n_shards, chunk_entries, _p(c), _p(t), n_per_shard, self_shard,
                                                      child_first, n_children_total, _p(a)), "mcl_stage_resample_compact")

    def stage_rays(self, obs):
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_stage_rays(self._h, _p(o), o.size), "mcl_stage_rays")

    def set_reserved_cus(self, n):
        self._chk(self.lib.mcl_set_reserved_cus(self._h, n), "mcl_set_reserved_cus")

    def stage_weights(self, global_max):
        self._chk(self.lib.mcl_stage_weights(self._h, global_max), "mcl_stage_weights")

    def stage_finish(self, sums5):
        s = _c(sums5, np.float64)
        self._chk(self.lib.mcl_stage_finish(self._h, _p(s)), "mcl_stage_finish")

    # ---- the staged flow ordered on the device (include/mcl_hip_engine.h: "ORDERED ON THE DEVICE"): nothing here waits for the
    # stream except stage_complete; `stream` is a raw hipStream_t (torch.cuda.current_stream().cuda_stream)
    def stream_wait_external(self, stream):
        self._chk(self.lib.mcl_stream_wait_external(self._h, C.c_void_p(stream)), "mcl_stream_wait_external")

    def external_wait_stream(self, stream):
        self._chk(self.lib.mcl_external_wait_stream(self._h, C.c_void_p(stream)), "mcl_external_wait_stream")

    def export_compact_async(self, d_chunk, chunk_entries):
        self._chk(self.lib.mcl_export_compact_async(self._h, C.c_void_p(d_chunk), chunk_entries), "mcl_export_compact_async")

    def stage_resample_compact_async(self, d_chunks, n_shards, chunk_entries, counts, totals, n_per_shard, self_shard, child_first, n_children_total,
                                     action):
        a = _c(action, np.float64)
        c = np.ascontiguousarray(np.asarray(counts, np.int64))
        t = np.ascontiguousarray(np.asarray(totals, np.uint64))
        assert c.size == n_shards and t.size == n_shards
        self._chk(self.lib.mcl_stage_resample_compact_async(self._h, C.c_void_p(d_chunks), n_shards, chunk_entries, _p(c), _p(t), n_per_shard,
                                                            self_shard, child_first, n_children_total, _p(a)), "mcl_stage_resample_compact_async")

    def stage_keep(self, child_first, n_children_total, action):
        """Adaptive resampling kept the set: motion only, every particle its own parent (launch only)."""
        a = _c(action, np.float64)
        self._chk(self.lib.mcl_stage_keep(self._h, child_first, n_children_total, _p(a)), "mcl_stage_keep")

    def stage_rays_async(self, obs, d_local_max):
        o = _c(obs, np.float32)
        self._chk(self.lib.mcl_stage_rays_async(self._h, _p(o), o.size, C.c_void_p(d_local_max)), "mcl_stage_rays_async")

    def stage_weights_async(self, d_global_max, d_vec, n_shards, self_shard):
        self._chk(self.lib.mcl_stage_weights_async(self._h, C.c_void_p(d_global_max), C.c_void_p(d_vec), n_shards, self_shard),
                  "mcl_stage_weights_async")

    def stage_complete(self, sums5) -> bool:
        """The one host wait of a device-ordered update.  True: the ray stage's fix-up lists overflowed, run the synchronous
        stages once more (stage_rays .. stage_finish)."""
        s = _c(sums5, np.float64)
        redo = C.c_int32()
        self._chk(self.lib.mcl_stage_complete(self._h, _p(s), C.byref(redo)), "mcl_stage_complete")
        return bool(redo.value)

    # ---- the sharded update in native code: an RCCL communicator inside the engine (include/mcl_hip_engine.h: mcl_comm_*)
    @staticmethod
    def comm_available():
        """(True, "") when the library finds an RCCL to use, else (False, why)."""
        why = C.c_char_p()
        rc = load_library().mcl_comm_available(C.byref(why))
        return rc == MCL_OK, (why.value or b"").decode()

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        _check(load_library().mcl_comm_unique_id(buf), "mcl_comm_unique_id")
        return bytes(buf)

    def comm_create(self, uid: bytes, n_ranks: int, rank: int):
        """COLLECTIVE: every rank calls it with rank 0's id."""
        assert len(uid) == 128
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        self._chk(self.lib.mcl_comm_create(self._h, buf, n_ranks, rank), "mcl_comm_create")
        self._comm_ranks = n_ranks

    def comm_selftest(self):
        """COLLECTIVE: the three collectives of an update on known data."""
        self._chk(self.lib.mcl_comm_selftest(self._h), "mcl_comm_selftest")

    def comm_destroy(self):
        self._chk(self.lib.mcl_comm_destroy(self._h), "mcl_comm_destroy")

    def comm_set_lists(self, counts, totals):
        c = np.ascontiguousarray(np.asarray(counts, np.int64))
        t = np.ascontiguousarray(np.asarray(totals, np.uint64))
        assert c.size == self._comm_ranks and t.size == self._comm_ranks
        self._chk(self.lib.mcl_comm_set_lists(self._h, _p(c), _p(t)), "mcl_comm_set_lists")

    def comm_update(self, action, obs):
        """One sharded update in one native call (lists, or the dense exchange when there are none); the pose of the whole set.
        Any failure -- this rank's, a peer's, a collective that ran out of time -- raises ShardedUpdateError on EVERY rank from
        the same update (include/mcl_hip_engine.h: the failure protocol of mcl_comm_update); nothing falls back to another exchange."""
        a = _c(action, np.float64)
        o = _c(obs, np.float32)
        pose = np.zeros(3)
        rc = self.lib.mcl_comm_update(self._h, _p(a), _p(o), o.size, _p(pose))
        if rc != MCL_OK:
            raise ShardedUpdateError(f"mcl_comm_update rc={rc}: {self.lib.mcl_last_error(self._h).decode()}", rc,
                                     local=rc not in (MCL_ERR_PEER, MCL_ERR_TIMEOUT))
        return pose

    def comm_vector(self):
        vec = np.zeros(5 + 3 * self._comm_ranks + 2)
        self._chk(self.lib.mcl_comm_get_vector(self._h, _p(vec), vec.size), "mcl_comm_get_vector")
        return vec

    def comm_stats(self):
        r, p, w = C.c_uint64(), C.c_uint64(), C.c_int32()
        self._chk(self.lib.mcl_comm_stats(self._h, C.byref(r), C.byref(p), C.byref(w)), "mcl_comm_stats")
        d, wb, rb = C.c_int32(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.mcl_comm_last_exchange(self._h, C.byref(d), C.byref(wb), C.byref(rb)), "mcl_comm_last_exchange")
        return dict(list_bytes_received=r.value, list_payload_bytes=p.value, host_waits=w.value, dense=d.value == 1, kept=d.value == 2,
                    weights_received=wb.value, records_received=rb.value)

    def scan_weights(self, d_q, d_cdf, n, offset=0):
        self._chk(self.lib.mcl_scan_weights(self._h, C.c_void_p(d_q), C.c_void_p(d_cdf), n, offset), "mcl_scan_weights")


from .group import Group  # noqa: E402,F401
