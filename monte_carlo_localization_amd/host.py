"""The CPU side of the binding: the host_* twins of the device's tables and rules (mcl_host_*; no device needed), the
default_*_config / *_config helpers, and the small array helpers every call site shapes its arguments with.  Plumbing only: the
arithmetic is the library's.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import *  # noqa: F401,F403
from .abi import EngineError, MCL_ERR_INVALID_ARG, MCL_OK, load_library


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def _check(rc, what, why=None):
    """EngineError "<what> rc=<rc>", and ": <why()>" behind it where the caller has more to say, for any status but MCL_OK"""
    if rc != MCL_OK:
        raise EngineError(f"{what} rc={rc}" + (f": {why()}" if why else ""), rc)


def _defaults(struct, defaults_fn, over):
    """A `struct` filled by the C call `defaults_fn`, then the fields of `over`: an unknown one is an AttributeError, an array
    field (reserved) takes any sequence"""
    c = struct()
    getattr(load_library(), defaults_fn)(C.byref(c))
    types = dict(struct._fields_)
    for name, v in over.items():
        if name not in types:
            raise AttributeError(name)
        setattr(c, name, types[name](*v) if issubclass(types[name], C.Array) else v)
    return c


def default_config(**over) -> Config:
    return _defaults(Config, "mcl_default_config", over)


def default_kld_config(**over) -> KldConfig:
    """mcl_default_kld_config, with fields overridden by keyword."""
    return _defaults(KldConfig, "mcl_default_kld_config", over)


def default_recovery_config(**over) -> RecoveryConfig:
    """mcl_default_recovery_config, with fields overridden by keyword."""
    return _defaults(RecoveryConfig, "mcl_default_recovery_config", over)


def host_recovery_step(cfg: RecoveryConfig, S, F, reset, max_logw, sum_w, denom, n_beams):
    """One update of the recovery averages on the host (mcl_host_recovery_step; no device needed): (S, F, p of the next
    update) after folding in the likelihood of an update with SCALARS max_logw, sum_w and denominator denom (N, or the previous
    update's sum_w for a kept update); NaN = unset."""
    st, out, p = (C.c_double * 2)(S, F), (C.c_double * 2)(), C.c_double()
    _check(load_library().mcl_host_recovery_step(C.byref(cfg), st, 1 if reset else 0, max_logw, sum_w, denom, int(n_beams), out, C.byref(p)),
           "mcl_host_recovery_step")
    return out[0], out[1], p.value


def _proposal_arrays(means, covs, weights):
    """(M, means, covs, weights or None) as the C calls take them; ValueError for shapes that are not (M, 3) / (M, 3, 3) or (M, 9) / (M,)"""
    m = _c(np.atleast_2d(np.asarray(means, np.float64)), np.float64)
    c = _c(covs, np.float64)
    if m.ndim != 2 or m.shape[1] != 3 or c.size != 9 * m.shape[0]:
        raise ValueError("means must be (M, 3) and covs (M, 3, 3)")
    w = None
    if weights is not None:
        w = _c(weights, np.float64).ravel()
        if w.size != m.shape[0]:
            raise ValueError("weights must have one entry per component")
    return m.shape[0], m, c, w


def host_recovery_proposal(means, covs, weights=None):
    """What Engine.set_recovery_proposal uploads for a mixture (mcl_host_recovery_proposal, rules P1 / P2; no device needed):
    (thresholds, factors) -- M uint64 and (M, 9) doubles (mean x, y, theta, L00 L10 L11 L20 L21 L22).  A refused mixture raises
    EngineError; the message names the first component that is refused on its own."""
    M, m, c, w = _proposal_arrays(means, covs, weights)
    thr, fac = np.zeros(M, np.uint64), np.zeros((M, 9), np.float64)
    lib = load_library()
    rc = lib.mcl_host_recovery_proposal(M, _p(m) if M else None, _p(c) if M else None, _p(w) if w is not None else None,
                                        _p(thr) if M else None, _p(fac) if M else None)
    if rc != MCL_OK:
        c9 = c.reshape(M, 9) if M else c
        one = np.ones(1)
        for k in range(M if M <= 4096 else 0):
            wk = _c([w[k]], np.float64) if w is not None and w[k] != 0.0 else one     # (a zero weight alone is only an empty sum)
            mk, ck = _c(m[k], np.float64), _c(c9[k], np.float64)
            if lib.mcl_host_recovery_proposal(1, _p(mk), _p(ck), _p(wk), None, None) != MCL_OK:
                raise EngineError(f"mcl_host_recovery_proposal rc={rc}: component {k} is refused", rc)
        raise EngineError(f"mcl_host_recovery_proposal rc={rc}: n_components or the sum of the weights is refused", rc)
    return thr, fac


def default_likelihood_field_config(**over) -> LikelihoodFieldConfig:
    """mcl_default_likelihood_field_config (AMCL's defaults), with fields overridden by keyword."""
    return _defaults(LikelihoodFieldConfig, "mcl_default_likelihood_field_config", over)


def host_likelihood_field(grid, resolution, **fields) -> np.ndarray:
    """The likelihood field D of a map (mcl_host_likelihood_field; no device needed): shape (H, W), uint16."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H, W), np.uint16)
    c = default_likelihood_field_config(**fields)
    _check(load_library().mcl_host_likelihood_field(_p(g), W, H, np.float32(resolution), C.byref(c), _p(out), out.size), "mcl_host_likelihood_field")
    return out


def host_likelihood_table(resolution, cfg: Config | None = None, **fields) -> np.ndarray:
    """The table Lf (K + 1 float32 entries) of the likelihood field (mcl_host_likelihood_table; no device needed); cfg supplies
    max_range_m and squash_factor (default: mcl_default_config's)."""
    cfg = cfg or default_config()
    c = default_likelihood_field_config(**fields)
    lib, K = load_library(), C.c_int32()
    _check(lib.mcl_host_likelihood_table(C.byref(cfg), C.byref(c), np.float32(resolution), None, 0, C.byref(K)), "mcl_host_likelihood_table")
    out = np.empty(K.value + 1, np.float32)
    _check(lib.mcl_host_likelihood_table(C.byref(cfg), C.byref(c), np.float32(resolution), _p(out), out.size, None), "mcl_host_likelihood_table")
    return out


def default_beam_skip_config(**over) -> BeamSkipConfig:
    """mcl_default_beam_skip_config (AMCL's defaults), with fields overridden by keyword."""
    return _defaults(BeamSkipConfig, "mcl_default_beam_skip_config", over)


def _mount3(mount):
    m = np.ascontiguousarray(np.zeros(3) if mount is None else mount, np.float64).reshape(-1)
    if m.size != 3:
        raise ValueError("a sensor mount is (mx, my, mtheta)")
    return m


def _host_mount_call(name, mount, poses):
    m = _mount3(mount)
    p = np.ascontiguousarray(poses, np.float64)
    if p.ndim == 1 and p.size == 3:
        p = p.reshape(3, 1)
    if p.ndim != 2 or p.shape[0] != 3:
        raise ValueError("poses must be (3, n): the rows x, y, theta")
    out = np.empty_like(p)
    _check(getattr(load_library(), name)(_p(m), _p(p), p.shape[1], _p(out)), name)
    return out


def host_sensor_mount(mount, poses):
    """The sensor poses (3, n) of the base poses (3, n) under `mount` = (mx, my, mtheta) (mcl_host_sensor_mount: rule SM2 of
    DESIGN.md §4.25 with the host's libm; no device needed)."""
    return _host_mount_call("mcl_host_sensor_mount", mount, poses)


def host_sensor_unmount(mount, poses):
    """The base poses (3, n) of the sensor poses (3, n): the inverse composition (mcl_host_sensor_unmount; no device needed)."""
    return _host_mount_call("mcl_host_sensor_unmount", mount, poses)


def host_sensor_mount_cov(mount, pose, cov, to_base=False):
    """J cov J^T (3, 3) with the Jacobian of SM2 at the base pose `pose`, or (to_base=True) of its inverse at the sensor pose `pose`
    (mcl_host_sensor_mount_cov; no device needed)."""
    m = _mount3(mount)
    p = np.ascontiguousarray(pose, np.float64).reshape(-1)
    c = np.ascontiguousarray(cov, np.float64).reshape(-1)
    if p.size != 3 or c.size != 9:
        raise ValueError("pose is (x, y, theta), cov 3 x 3")
    out = np.empty((3, 3), np.float64)
    _check(load_library().mcl_host_sensor_mount_cov(_p(m), _p(p), _p(c), 1 if to_base else 0, _p(out)), "mcl_host_sensor_mount_cov")
    return out


def host_scan_motion_offsets(motion, n_beams, t=None, t_ref=1.0, mount=None):
    """The (3, n_beams) table of per-beam sensor offsets (rows ox, oy, dtheta) of a scan taken under a constant twist
    (mcl_host_scan_motion_offsets, rules DM1 / DM2 of DESIGN.md §4.26; no device needed).  motion = (u, v, w): the base's body-frame
    twist integrated over the scan's unit of t (the odometry twist times the sweep duration); t: one stamp per beam (None:
    j / (B - 1)); t_ref: the time at which the particles are the robot's pose (1.0: the end of the sweep); mount: the sensor mount."""
    mo = np.ascontiguousarray(motion, np.float64).reshape(-1)
    if mo.size != 3:
        raise ValueError("motion is (u, v, w)")
    m = None if mount is None else _mount3(mount)
    tt = None if t is None else np.ascontiguousarray(t, np.float64).reshape(-1)
    if tt is not None and tt.size != int(n_beams):
        raise ValueError("t holds one stamp per beam")
    out = np.empty((3, max(int(n_beams), 0)), np.float64)
    _check(load_library().mcl_host_scan_motion_offsets(_p(mo), _p(m), _p(tt), float(t_ref), int(n_beams), _p(out)), "mcl_host_scan_motion_offsets")
    return out


def _offsets3(offsets, n_beams=None):
    o = np.ascontiguousarray(offsets, np.float64)
    if o.ndim != 2 or o.shape[0] != 3 or (n_beams is not None and o.shape[1] != n_beams):
        raise ValueError("beam offsets are (3, n_beams): the rows ox, oy, dtheta")
    return o


def host_beam_offset_table(angles, offsets):
    """(effective float angles a' (B,), their direction pairs (2, B): cos, sin) of rule DS1, as Engine.set_beam_offsets forms them
    (mcl_host_beam_offset_table; no device needed)."""
    a = _c(angles, np.float32).reshape(-1)
    o = _offsets3(offsets, a.size)
    eff, dirs = np.empty(a.size, np.float32), np.empty((2, a.size), np.float64)
    _check(load_library().mcl_host_beam_offset_table(_p(a), _p(o), a.size, _p(eff), _p(dirs)), "mcl_host_beam_offset_table")
    return eff, dirs


def host_beam_offset_pairs(ranges, offsets, dirs, resolution):
    """The likelihood field's pair (2, B), in cells, of every beam of `ranges` under rule DS5 (mcl_host_beam_offset_pairs; no device
    needed); dirs as host_beam_offset_table returns them."""
    r = _c(ranges, np.float32).reshape(-1)
    o = _offsets3(offsets, r.size)
    d = np.ascontiguousarray(dirs, np.float64)
    if d.shape != (2, r.size):
        raise ValueError("dirs is (2, B)")
    out = np.empty((2, r.size), np.float64)
    _check(load_library().mcl_host_beam_offset_pairs(_p(r), _p(o), _p(d), r.size, float(np.float32(resolution)), _p(out)),      # (the map's float resolution, widened: set_map)
           "mcl_host_beam_offset_pairs")
    return out


def host_beam_skip_thresholds(resolution, n_particles, n_used, **fields):
    """(ka, min_count, min_skipped) of an update of n_particles particles with n_used used beams (mcl_host_beam_skip_thresholds,
    rules BS1, BS3, BS4; no device needed): the integers the engine itself forms for its kernels."""
    c = default_beam_skip_config(**fields)
    ka, mc, ms = C.c_int32(), C.c_int64(), C.c_int32()
    _check(load_library().mcl_host_beam_skip_thresholds(C.byref(c), np.float32(resolution), int(n_particles), int(n_used), C.byref(ka), C.byref(mc),
                                                        C.byref(ms)), "mcl_host_beam_skip_thresholds")
    return ka.value, mc.value, ms.value


def host_beam_skip_plan(counts_used, n_particles, **fields):
    """(kept_used, n_skipped, integrate_all) for the agreement counts of the used beams (mcl_host_beam_skip_plan, rules BS3, BS4; no
    device needed): kept_used is uint8 per used beam, 1 summed, 2 skipped."""
    c = default_beam_skip_config(**fields)
    cnt = _c(counts_used, np.uint32).ravel()
    kept = np.zeros(cnt.size, np.uint8)
    ns, ia = C.c_int32(), C.c_int32()
    _check(load_library().mcl_host_beam_skip_plan(C.byref(c), _p(cnt) if cnt.size else None, cnt.size, int(n_particles),
                                                  _p(kept) if cnt.size else None, C.byref(ns), C.byref(ia)), "mcl_host_beam_skip_plan")
    return kept, ns.value, ia.value


def default_motion_config(**over) -> MotionConfig:
    """mcl_default_motion_config (DIFF, AMCL's alphas), with fields overridden by keyword; `model` may be a name
    ("reference", "diff", "omni")."""
    if isinstance(over.get("model"), str):
        over["model"] = MOTION_MODELS[over["model"]]
    return _defaults(MotionConfig, "mcl_default_motion_config", over)


def host_motion_scalars(cfg: MotionConfig, action) -> np.ndarray:
    """The per-update scalars of an odometry model (mcl_host_motion_scalars; no device needed): 8 doubles."""
    a, out = _c(action, np.float64), np.empty(8)
    assert a.size == 3
    _check(load_library().mcl_host_motion_scalars(C.byref(cfg), _p(a), _p(out)), "mcl_host_motion_scalars")
    return out


def host_motion_sample(cfg: MotionConfig, action, xyz_colmajor, normals_nx3) -> np.ndarray:
    """The children of the poses (3, n) under an odometry model with the normals (n, 3) (mcl_host_motion_sample; no device)."""
    a, p, nrm = _c(action, np.float64), _c(xyz_colmajor, np.float64), _c(normals_nx3, np.float64)
    assert a.size == 3 and p.ndim == 2 and p.shape[0] == 3 and nrm.size == 3 * p.shape[1]
    out = np.empty_like(p)
    _check(load_library().mcl_host_motion_sample(C.byref(cfg), _p(a), _p(p), _p(nrm), p.shape[1], _p(out)), "mcl_host_motion_sample")
    return out


def host_gaussian_factor(cov) -> np.ndarray:
    """The lower Cholesky factor init_particles_gaussian draws with (mcl_host_gaussian_factor; no device needed), 3 x 3."""
    c, L = _c(cov, np.float64), np.empty(6)
    assert c.size == 9
    _check(load_library().mcl_host_gaussian_factor(_p(c), _p(L)), "mcl_host_gaussian_factor")
    return np.array([[L[0], 0.0, 0.0], [L[1], L[2], 0.0], [L[3], L[4], L[5]]])


def default_search_config(**over) -> SearchConfig:
    """mcl_default_search_config (stride 2, 72 headings, every beam, local maxima), with fields overridden by keyword."""
    return _defaults(SearchConfig, "mcl_default_search_config", over)


def search_stream_config(budget_bytes=0, slab_headings=0, reserved=(0, 0, 0, 0, 0)) -> SearchStreamConfig:
    """mcl_search_stream_config_t: 0 bytes is the default budget (1 GiB), 0 headings the largest slab that fits it."""
    return _defaults(SearchStreamConfig, "mcl_default_search_stream_config",
                     dict(budget_bytes=int(budget_bytes), slab_headings=int(slab_headings), reserved=reserved))


def host_search_slabs(n_positions, n_scans=1, budget_bytes=0, slab_headings=0, stream_reserved=(0, 0, 0, 0, 0), **fields):
    """The plan of a streamed search (mcl_host_search_slabs, rules ST4 / ST5; no device needed): (G, n_slabs, bytes) -- the headings
    per slab, the number of slabs, the device bytes of the slab buffers.  `fields` override mcl_default_search_config."""
    c = default_search_config(**fields)
    sc = search_stream_config(budget_bytes, slab_headings, stream_reserved)
    G, ns, b = C.c_int32(), C.c_int32(), C.c_uint64()
    _check(load_library().mcl_host_search_slabs(C.byref(c), C.byref(sc), int(n_positions), int(n_scans), C.byref(G), C.byref(ns), C.byref(b)),
           "mcl_host_search_slabs")
    return int(G.value), int(ns.value), int(b.value)


def search_prune_config(block=0, first_pairs=0, reserved=(0, 0, 0, 0, 0, 0)) -> SearchPruneConfig:
    """mcl_search_prune_config_t: block 0 is the default block side (mcl_default_search_prune_config's), first_pairs 0 the default
    first round (max(1024, pairs / 64))."""
    c = SearchPruneConfig()
    load_library().mcl_default_search_prune_config(C.byref(c))
    if block:
        c.block = int(block)
    c.first_pairs = int(first_pairs)
    c.reserved[:] = [int(v) for v in reserved]
    return c


def host_search_blocks(grid, block=0, **fields) -> dict:
    """The block plan of a pruned search over a map (mcl_host_search_blocks, rules P1 / P2; no device needed): {n_blocks, w, nbx,
    nby, blocks} -- the live blocks, the window of the pooled field, the block grid, and per live block (bx, by, positions in it)
    in the order of the pair numbering: pair = k * n_blocks + b.  `fields` override mcl_default_search_config."""
    g = _c(grid, np.int8)
    H, W = g.shape
    c, pc = default_search_config(**fields), search_prune_config(block)
    lib = load_library()
    n, w, nbx, nby = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    args = (C.byref(c), C.byref(pc), _p(g), W, H, C.byref(n), C.byref(w), C.byref(nbx), C.byref(nby))
    _check(lib.mcl_host_search_blocks(*args, None, 0), "mcl_host_search_blocks")
    blocks = np.empty((n.value, 3), np.int32)
    if n.value:
        _check(lib.mcl_host_search_blocks(*args, _p(blocks), n.value), "mcl_host_search_blocks")
    return dict(n_blocks=n.value, w=w.value, nbx=nbx.value, nby=nby.value, blocks=blocks)


def host_lf_pool(D, K, w) -> np.ndarray:
    """The pooled field Dp of a likelihood field D (mcl_host_lf_pool, rule P2; no device needed): shape (H + w - 1, W + w - 1),
    uint16; out[y + w - 1, x + w - 1] is the minimum over the w x w window with low corner (x, y), cells off the map counting K."""
    d = _c(D, np.uint16)
    H, W = d.shape
    out = np.empty((H + int(w) - 1, W + int(w) - 1), np.uint16)
    _check(load_library().mcl_host_lf_pool(_p(d), W, H, int(K), int(w), _p(out), out.size), "mcl_host_lf_pool")
    return out


def host_search_bound_table(lf) -> np.ndarray:
    """Ub[k] = max over j >= k of Lf[j] (mcl_host_search_bound_table, rule P2; no device needed): K + 1 float32 entries."""
    t = _c(lf, np.float32)
    out = np.empty_like(t)
    _check(load_library().mcl_host_search_bound_table(_p(t), t.size - 1, _p(out)), "mcl_host_search_bound_table")
    return out


def host_search_prune_next(pairs, n_scored, first_below_c=0, first_pairs=0) -> int:
    """The round schedule of a pruned search (mcl_host_search_prune_next, rule P4; no device needed): how many ranks have scores
    after the next round; n_scored = 0 gives the first round."""
    pc, out = search_prune_config(0, first_pairs), C.c_int64()
    _check(load_library().mcl_host_search_prune_next(C.byref(pc), int(pairs), int(n_scored), int(first_below_c), C.byref(out)),
           "mcl_host_search_prune_next")
    return out.value


def host_search_lattice(grid, resolution, origin_x, origin_y, **fields):
    """The positions of the global search's lattice over a map (mcl_host_search_lattice, rule S1; no device needed): (cells, xy) --
    the linear map cell of every position (uint32) and its pose coordinates, shape (n_positions, 2)."""
    g = _c(grid, np.int8)
    H, W = g.shape
    c = default_search_config(**fields)
    lib, n = load_library(), C.c_int64()
    args = (C.byref(c), _p(g), W, H, np.float32(resolution), float(origin_x), float(origin_y))
    _check(lib.mcl_host_search_lattice(*args, None, None, 0, C.byref(n)), "mcl_host_search_lattice")
    cells, xy = np.empty(n.value, np.uint32), np.empty((n.value, 2), np.float64)
    if n.value:
        _check(lib.mcl_host_search_lattice(*args, _p(cells), _p(xy), n.value, C.byref(n)), "mcl_host_search_lattice")
    return cells, xy


def host_search_headings(**fields) -> np.ndarray:
    """The headings of the global search (mcl_host_search_headings, rule S2; no device needed): n_headings doubles."""
    c = default_search_config(**fields)
    out = np.empty(max(int(c.n_headings), 0), np.float64)
    _check(load_library().mcl_host_search_headings(C.byref(c), _p(out), out.size), "mcl_host_search_headings")
    return out


def host_search_beam_grid(angles, n_headings=72) -> dict:
    """The angle grid of a search under the beam model (mcl_host_search_beam_grid, rule B1; no device needed): {M, heading_step,
    delta, max_dev, phi} -- the grid angles per turn, the grid steps between two headings, the grid's increment, the worst
    deviation of a beam angle from its grid angle, and the M grid angles.  Raises EngineError (with .max_dev where it was
    measured) when the scan and the heading count do not share a grid."""
    a = _c(angles, np.float32)
    lib = load_library()
    M, s, d, dev = C.c_int32(), C.c_int32(), C.c_double(), C.c_double(float("nan"))
    rc = lib.mcl_host_search_beam_grid(_p(a) if a.size else None, a.size, int(n_headings), C.byref(M), C.byref(s),
                                       C.byref(d), C.byref(dev), None, 0)
    if rc != MCL_OK:
        err = EngineError(f"mcl_host_search_beam_grid rc={rc}", rc)
        err.max_dev = dev.value
        raise err
    phi = np.empty(M.value, np.float64)
    _check(lib.mcl_host_search_beam_grid(_p(a), a.size, int(n_headings), None, None, None, None, _p(phi), phi.size), "mcl_host_search_beam_grid")
    return dict(M=int(M.value), heading_step=int(s.value), delta=d.value, max_dev=dev.value, phi=phi)


def _rel_rows(rel) -> np.ndarray:
    """(S, 3) rows of (dx, dy, dtheta), or one such row, C-contiguous float64"""
    r = np.asarray(rel, np.float64)
    if r.ndim == 1:
        r = r.reshape(1, -1)
    if r.ndim != 2 or r.shape[1] != 3:
        raise ValueError("expected (S, 3) rows of three values, or one row")
    return _c(r, np.float64)


def host_search_sequence_offsets(rel, **fields) -> np.ndarray:
    """The table a search over a scan sequence uploads (mcl_host_search_sequence_offsets, rule SQ1; no device needed): shape
    (n_headings, S, 3), [k, s] = (ax_ks, ay_ks, theta_ks) -- scan s's displacement from the anchor in the map frame at heading k,
    and its heading.  `rel`: (S, 3) rows of (dx, dy, dtheta) in the anchor's frame."""
    c = default_search_config(**fields)
    r = _rel_rows(rel)
    S = r.shape[0]
    out = np.empty((max(int(c.n_headings), 0), S, 3), np.float64)
    _check(load_library().mcl_host_search_sequence_offsets(C.byref(c), _p(r) if S else None, S, _p(out), out.size), "mcl_host_search_sequence_offsets")
    return out


def relative_poses(odom, anchor=-1) -> np.ndarray:
    """Absolute odometry poses, (S, 3) rows of (x, y, theta), as poses relative to the one at `anchor` (mcl_host_relative_poses):
    the `rel` of Engine.global_search_sequence.  anchor = -1, the default: the latest pose."""
    o = _rel_rows(odom)
    S = o.shape[0]
    a = int(anchor) + S if int(anchor) < 0 else int(anchor)
    out = np.empty((S, 3), np.float64)
    _check(load_library().mcl_host_relative_poses(_p(o) if S else None, S, a, _p(out)), "mcl_host_relative_poses")
    return out


def default_refine_config(**over) -> RefineConfig:
    """mcl_default_refine_config (a 9 x 9 x 21 window: +-2 cells in steps of half a cell, +-5 degrees in steps of half a degree,
    every beam), with fields overridden by keyword."""
    return _defaults(RefineConfig, "mcl_default_refine_config", over)


def refine_window_size(c: RefineConfig) -> int:
    """n_win of a config (rule R1), in Python's integers"""
    return (2 * int(c.half_xy) + 1) ** 2 * (2 * int(c.half_theta) + 1)


def host_refine_window(seed, resolution, **fields) -> np.ndarray:
    """The window poses around `seed` (mcl_host_refine_window, rule R1; no device needed): (n_win, 3) rows of (x, y, theta) in
    window-index order, ix fastest.  `fields` override mcl_default_refine_config."""
    c = default_refine_config(**fields)
    s = _c(seed, np.float64).ravel()
    assert s.size == 3
    n = refine_window_size(c)
    out = np.empty((n if 0 < n <= MAX_REFINE_WINDOW else 1, 3), np.float64)
    _check(load_library().mcl_host_refine_window(C.byref(c), _p(s), np.float32(resolution), _p(out), out.shape[0]), "mcl_host_refine_window")
    return out


def host_refine_reduce(seed, resolution, scores, **fields) -> np.ndarray:
    """What Engine.refine_poses reports for one seed whose window scored `scores` (mcl_host_refine_reduce, rules R3 / R4; no device
    needed): one REFINE_DTYPE record."""
    c = default_refine_config(**fields)
    s, v = _c(seed, np.float64).ravel(), _c(scores, np.float64).ravel()
    assert s.size == 3
    out = np.zeros(1, REFINE_DTYPE)
    _check(load_library().mcl_host_refine_reduce(C.byref(c), _p(s), np.float32(resolution), _p(v), v.size, _p(out)), "mcl_host_refine_reduce")
    return out[0]


def host_refine_sequence_offsets(seeds, rel, **fields) -> np.ndarray:
    """The table a refinement over a scan sequence uploads (mcl_host_refine_sequence_offsets, rule RS1; no device needed): shape
    (M, nt, S, 3), [m, it, s] = (ax, ay, theta_s) -- scan s's displacement from the anchor in the map frame at window heading it
    of seed m, and its heading.  `seeds`: (M, 3) rows of (x, y, theta), or one; `rel`: (S, 3) rows of (dx, dy, dtheta) in the
    anchor's frame.  `fields` override mcl_default_refine_config."""
    c = default_refine_config(**fields)
    p = _rel_rows(seeds)
    r = _rel_rows(rel)
    M, S, nt = p.shape[0], r.shape[0], 2 * int(c.half_theta) + 1
    rows = M * nt * S
    if rows > MAX_REFINE_SEQ_ROWS:                            # (RS1's cap, here too: such a table is never allocated)
        raise EngineError(f"mcl_host_refine_sequence_offsets rc={MCL_ERR_INVALID_ARG}: {rows} rows, more than {MAX_REFINE_SEQ_ROWS}",
                          MCL_ERR_INVALID_ARG)
    # an empty table (no seed, no scan, a refused half_theta) still goes to the C call, which names the refusal by its status
    out = np.empty((M, nt, S, 3) if rows > 0 else (1, 1, 1, 3), np.float64)
    pc = _c(p.T, np.float64)                                  # column-major, as the refinement takes its seeds
    _check(load_library().mcl_host_refine_sequence_offsets(C.byref(c), _p(pc) if M else None, M, _p(r) if S else None, S, _p(out), out.size),
           "mcl_host_refine_sequence_offsets")
    return out


def seed_counts(log_likelihoods, n) -> np.ndarray:
    """How many of n particles each hit of a global search seeds (the counts of Engine.init_particles_mixture): shares
    proportional to exp(ll - max ll), the floors of the exact shares first, the particles left over to the largest remainders,
    ties to the earlier hit.  A hit at -inf gets none.  Pure Python (exact rationals), int64."""
    import math
    from fractions import Fraction
    ll = [float(v) for v in np.asarray(log_likelihoods, np.float64).ravel()]
    n = int(n)
    if not ll or n < 0 or any(math.isnan(v) or v == math.inf for v in ll):
        raise ValueError("seed_counts: needs at least one hit, n >= 0 and scores below +inf")
    top = max(ll)
    if top == -math.inf:
        raise ValueError("seed_counts: every hit is at -inf")
    w = [Fraction(math.exp(v - top)) for v in ll]            # (exp(-inf) = 0; the best hit weighs exactly 1)
    total = sum(w)
    share = [n * v / total for v in w]
    counts = [int(v) for v in share]                         # floors (the shares are >= 0)
    order = sorted(range(len(ll)), key=lambda i: (-(share[i] - counts[i]), i))
    for i in order[:n - sum(counts)]:
        counts[i] += 1
    return np.array(counts, np.int64)


def default_cluster_config(**over) -> ClusterConfig:
    """mcl_default_cluster_config, with fields overridden by keyword."""
    return _defaults(ClusterConfig, "mcl_default_cluster_config", over)


def host_kld_bins(x, y, th, width, height, resolution, origin_x, origin_y, kld: KldConfig) -> int:
    """Pose-space bins the poses (x, y, th) occupy under the KLD bin rule (mcl_host_kld_bins; no device needed)."""
    x, y, th = _c(x, np.float64), _c(y, np.float64), _c(th, np.float64)
    assert x.size == y.size == th.size
    out = C.c_int64()
    _check(load_library().mcl_host_kld_bins(_p(x), _p(y), _p(th), x.size, width, height, np.float32(resolution), origin_x, origin_y, C.byref(kld),
                                            C.byref(out)), "mcl_host_kld_bins")
    return out.value


def host_kld_target(kld: KldConfig, bins: int, n_current: int) -> int:
    """The particle count the update after one that counted `bins` with n_current particles draws (mcl_host_kld_target)."""
    out = C.c_int64()
    _check(load_library().mcl_host_kld_target(C.byref(kld), int(bins), int(n_current), C.byref(out)), "mcl_host_kld_target")
    return out.value


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return None if a is None else np.ascontiguousarray(a, dtype=dt)


def host_sensor_table(P: int, cfg: Config | None = None) -> np.ndarray:
    """The engine's host-side sensor table (no device needed); returned as T[d, r]."""
    cfg = cfg or default_config()
    out = np.empty((P + 1) * (P + 1), np.float64)
    _check(load_library().mcl_host_sensor_table(C.byref(cfg), P, _p(out), out.size), "mcl_host_sensor_table")
    return out.reshape(P + 1, P + 1)


def host_skip_field(grid) -> np.ndarray:
    """The engine's padded skip-distance field (no device needed): shape (H+1, W+1), uint8."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    _check(load_library().mcl_host_skip_field(_p(g), W, H, _p(out), out.size), "mcl_host_skip_field")
    return out



def host_skip_field_wedge(grid, wedge: int) -> np.ndarray:
    """Skip field for rays whose direction angle lies in sector `wedge` of WEDGES equal sectors of the turn."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    _check(load_library().mcl_host_skip_field_wedge(_p(g), W, H, wedge, _p(out), out.size), "mcl_host_skip_field_wedge")
    return out


def host_sweep_global_layout(width: int, height: int, max_range_px: int) -> dict:
    """mcl_host_sweep_global_layout: {ok, pitch, rows, stride, alloc, max_offset} of the ringed copies of the wedge fields."""
    out = (C.c_int64 * 6)()
    _check(load_library().mcl_host_sweep_global_layout(width, height, max_range_px, out), "mcl_host_sweep_global_layout")
    return dict(ok=bool(out[0]), pitch=int(out[1]), rows=int(out[2]), stride=int(out[3]), alloc=int(out[4]), max_offset=int(out[5]))


def host_skip_field_wedge_tight(grid, wedge: int) -> np.ndarray:
    """The wedge field under the tight rule (jumps bounded by the distance travelled inside the wedge): what set_map builds."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    _check(load_library().mcl_host_skip_field_wedge_tight(_p(g), W, H, wedge, _p(out), out.size), "mcl_host_skip_field_wedge_tight")
    return out


SORT_KEY_LOG2, SORT_MAX_FINE = 22, 10      # bits of the coarse ordering key, and the most fine bits below it (csrc/mcl_sort_key.h)


def sort_fine_code(fine: int, fine_sub: int | None = None) -> int:
    """the fine setting as the one word the C calls take: the bits, and the sub-cell bits per axis where they are not the rule's"""
    if not 0 <= int(fine) <= SORT_MAX_FINE or (fine_sub is not None and not 0 <= 2 * int(fine_sub) <= int(fine)):
        raise EngineError(f"sort key: fine={fine} fine_sub={fine_sub} (0 .. {SORT_MAX_FINE} bits, at most half of them per axis)", MCL_ERR_INVALID_ARG)
    return int(fine) | ((int(fine_sub) + 1) << 4 if fine_sub is not None else 0)


def sort_tile_grid(width: int, height: int):
    """(tiles per row, rows of tiles) of the 32 x 32-cell tiles over the padded map: the shape of an ordering tile map."""
    return (int(width) >> 5) + 1, (int(height) >> 5) + 1


def host_sort_key(bbox, tilemap, width: int, height: int, px, py, theta, fine: int = 0, n_layout: int | None = None,
                  fine_sub: int | None = None) -> np.ndarray:
    """mcl_host_sort_key: the ordering keys (uint32) of particles at pixel coordinates (px, py) with headings theta, under the
    layout words `bbox` (7 int32) and the tile map (None when bbox[5] == 0), with `fine` bits below the coarse 22 -- the code
    the device runs, on the CPU.  n_layout: the size of the set the layout is for (its density decides the split of the bits);
    default: the number of particles given.  fine_sub: how many of the fine bits, per axis, are sub-cell bits (default: the
    rule, max(fine - 2, 0) // 4)."""
    bb = _c(np.asarray(bbox).reshape(-1)[:7], np.int32)
    x, y, t = _c(px, np.float64), _c(py, np.float64), _c(theta, np.float64)
    if bb.size != 7 or not (x.shape == y.shape == t.shape) or x.ndim != 1:
        raise ValueError("host_sort_key: bbox has 7 words; px, py, theta are 1-D and of one length")
    ntx, nty = sort_tile_grid(width, height)
    tm = None
    if tilemap is not None:
        tm = _c(tilemap, np.int32)
        if tm.size != ntx * nty:
            raise ValueError(f"host_sort_key: the tile map has {ntx} x {nty} entries for this map")
    out = np.empty(x.size, np.uint32)
    _check(load_library().mcl_host_sort_key(_p(bb), _p(tm) if tm is not None else None, ntx, width, height, _p(x), _p(y), _p(t), x.size,
                                            x.size if n_layout is None else n_layout, sort_fine_code(fine, fine_sub), _p(out)), "mcl_host_sort_key")
    return out


def host_compact_guide(ccdf, m: int, fill=None):
    """mcl_host_compact_guide: the guide of a compact parent list with the strictly increasing CDF column `ccdf` (uint64; its last
    entry is the total) for 2^m buckets, by the rule the scan kernel follows.  Returns (guide, s, bmax, words written): guide has
    bmax + 2 uint32 words, 0 .. bmax written and the last one left at `fill` (default 0xffffffff) -- the word the search's pair
    fetch touches and never uses."""
    c = _c(ccdf, np.uint64)
    if c.ndim != 1 or c.size == 0:
        raise ValueError("host_compact_guide: ccdf is 1-D and not empty")
    lib = load_library()
    s, bmax, nw = C.c_int32(), C.c_uint32(), C.c_int64()
    q = int(c[-1])
    _check(lib.mcl_host_compact_guide(_p(c), c.size, q, m, None, 0, C.byref(s), C.byref(bmax), None), "mcl_host_compact_guide")
    guide = np.full(bmax.value + 2, 0xffffffff if fill is None else fill, np.uint32)
    _check(lib.mcl_host_compact_guide(_p(c), c.size, q, m, _p(guide), bmax.value + 1, C.byref(s), C.byref(bmax), C.byref(nw)),
           "mcl_host_compact_guide")
    return guide, s.value, bmax.value, nw.value


def host_compact_search(ccdf, guide, s: int, bmax: int, thr) -> np.ndarray:
    """mcl_host_compact_search: for every threshold the list position the resampling kernel selects -- the first entry with
    ccdf > thr, searched between the two guide words of the threshold's bucket, clamped to the last entry (int64).  guide: the
    bmax + 2 words of host_compact_guide."""
    c, g, t = _c(ccdf, np.uint64), _c(guide, np.uint32), _c(thr, np.uint64)
    out = np.empty(t.size, np.int64)
    _check(load_library().mcl_host_compact_search(_p(c), c.size, _p(g), g.size, s, bmax, _p(t), t.size, _p(out)), "mcl_host_compact_search")
    return out


WEDGE_R = 255


def host_wedge_tight_table(wedge: int):
    """(values, reachable), each (511, 511) indexed [oy + 255, ox + 255]: the uncapped skip a stop cell at that offset allows
    under the tight rule, and whether the field search counts the offset as reachable in this wedge."""
    S = 2 * WEDGE_R + 1
    val, reach = np.empty((S, S), np.int32), np.empty((S, S), np.uint8)
    _check(load_library().mcl_host_wedge_tight_table(wedge, _p(val), _p(reach), val.size), "mcl_host_wedge_tight_table")
    return val, reach.astype(bool)


def host_map_patch_plan(width: int, height: int, stop_bbox, lf_reach: int = 0):
    """mcl_host_map_patch_plan: (window, lf_window), each (x0, y0, x1, y1) inclusive (x1 < x0: none) -- the padded-grid cells of the
    skip fields, and the grid cells of a likelihood field of reach lf_reach, that a stop-bit change inside the box stop_bbox
    (grid cells, inclusive) of a width x height map can alter.  EngineError INVALID_ARG for an inverted box or one outside the map."""
    box = (C.c_int32 * 4)(*[int(v) for v in stop_bbox])
    win, lfw = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    _check(load_library().mcl_host_map_patch_plan(width, height, box, lf_reach, win, lfw), "mcl_host_map_patch_plan")
    return tuple(win), tuple(lfw)


def _patch_cells(cells2d):
    c = np.asarray(cells2d, np.int8)
    if c.ndim != 2:
        raise ValueError("update_map_region: cells must be a 2-D array (rows, columns)")
    if c.strides[1] != 1 or c.strides[0] < c.shape[1]:       # (a view whose rows are contiguous is passed as it is, with its row stride)
        c = np.ascontiguousarray(c, np.int8)
    return c


def host_skip_field_dir(grid, quadrant: int) -> np.ndarray:
    """Directional skip field for rays of one direction quadrant (0:+x+y 1:-x+y 2:-x-y 3:+x-y)."""
    g = _c(grid, np.int8)
    H, W = g.shape
    out = np.empty((H + 1, W + 1), np.uint8)
    _check(load_library().mcl_host_skip_field_dir(_p(g), W, H, quadrant, _p(out), out.size), "mcl_host_skip_field_dir")
    return out
