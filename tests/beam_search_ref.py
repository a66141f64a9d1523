"""The numpy statement of the global search under the beam model (mcl_global_search_beam, DESIGN.md §4.17, rules B1-B5 of
include/mcl_hip_engine.h): the angle grid, the per-position ray table from the oracle's cast_ray, the score volume as a
beam-by-beam sum of table entries, and S5 restated for the hits.  The tests compare the engine with these bit for bit."""
import numpy as np

TWO_PI, PI = 6.283185307179586, 3.141592653589793


def grid(angles, n_headings):
    """B1: dict(M, heading_step, delta, max_dev, phi) from the float angles; the refusal conditions are the caller's to check"""
    a = np.asarray(angles, np.float32).astype(np.float64)
    B = a.size
    if B >= 2:
        inc = (a[-1] - a[0]) / float(B - 1)
        M = int(np.floor(TWO_PI / inc + 0.5))                 # llround of a positive value
    else:
        M = int(n_headings)
    delta = TWO_PI / float(M)
    max_dev = float(np.abs(a - (a[0] + np.arange(B, dtype=np.float64) * delta)).max())
    phi = (a[0] - PI) + np.arange(M, dtype=np.float64) * delta
    return dict(M=M, heading_step=M // int(n_headings), delta=delta, max_dev=max_dev, phi=phi)


def table(orc, om, xy, phi):
    """B2: S[p, m] = cast_ray's step from (x_p, y_p) at the angle phi_m"""
    n_pos, M = len(xy), phi.size
    x, y = np.repeat(xy[:, 0], M), np.repeat(xy[:, 1], M)
    return orc.cast_many(om, x, y, np.tile(phi, n_pos))[1].reshape(n_pos, M).astype(np.int64)


def volume(orc, om, S, obs, n_headings, heading_step, beam_stride=1):
    """B3: V[k, p] = sum over the used beams j, ascending, of (double)L[row_j, S[p, (k s + j) mod M]], from +0.0"""
    n_pos, M = S.shape
    rows = orc.obs_index(np.asarray(obs, np.float32), om)
    L = orc.eng_log_table(orc.sensor_table(om.max_range_px))
    V = np.zeros((n_headings, n_pos), np.float64)
    for k in range(n_headings):
        acc = np.zeros(n_pos, np.float64)
        for j in range(0, rows.size, beam_stride):
            acc += L[rows[j], S[:, (k * heading_step + j) % M]].astype(np.float64)
        V[k] = acc
    return V


def hits(V, cells, stride, nms, W, H):
    """S5 restated: the candidates' pose indices, best first.  V: (n_head, n_pos)"""
    n_head, n_pos = V.shape
    h0 = stride // 2
    cells = cells.astype(np.int64)
    ix, iy = (cells % W - h0) // stride, (cells // W - h0) // stride
    nx, ny = (W - 1 - h0) // stride + 1, (H - 1 - h0) // stride + 1
    pmap = np.full((ny + 2, nx + 2), -1, np.int64)           # a ring of "no position" around the lattice
    pmap[iy + 1, ix + 1] = np.arange(n_pos)
    idx = np.arange(n_head * n_pos).reshape(n_head, n_pos)
    cand = V > -np.inf
    if nms:
        for dk in (-1, 0, 1):
            kk = (np.arange(n_head) + dk) % n_head
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = pmap[iy + 1 + dy, ix + 1 + dx]
                    there = q >= 0
                    qq = np.where(there, q, 0)
                    Vn, jn = V[kk][:, qq], idx[kk][:, qq]
                    is_nb = there[None, :] & (jn != idx)
                    better = (V > Vn) | ((V == Vn) & (idx < jn))
                    cand &= ~is_nb | better
    c = idx[cand]
    return c[np.lexsort((c, -V[cand]))]
