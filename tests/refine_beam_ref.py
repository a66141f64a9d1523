"""Python / numpy restatement of the pose refinement under the beam model (include/mcl_hip_engine.h, DESIGN.md §4.18, rules RB2 and
RB3): the statement the device is held to.  A plain helper module (like refine_ref.py, whose map, seeds and window it reuses): no
device, no engine.

  rays:   RB2 -- the oracle's cast_ray at theta_w + (double)a_j, one ray per (window pose, used beam)
  rows:   E2 through the oracle's obs_index: every reading has a row
  table:  L = eng_log_table(sensor_table(P)), the engine's static log table
  sum:    RB3 -- the u-th used beam goes to lane u % 64 in ascending u from +0.0, then the butterfly v += v[lane ^ off],
          off = 32 ... 1, written out; in_order() is the plain left-to-right sum the fixture test compares it with"""
import numpy as np

LANES = 64


def used(B, beam_stride=1):
    """the used beams: j % beam_stride == 0, ascending"""
    return np.arange(0, B, beam_stride)


def steps(orc, om, poses, ang, beam_stride=1):
    """RB2: (n_poses, used beams) step indices"""
    poses = np.asarray(poses, np.float64).reshape(-1, 3)
    a = ang[used(ang.size, beam_stride)].astype(np.float64)
    angle = poses[:, 2:3] + a[None, :]                       # theta + (double)a_j: one rounded add
    x = np.repeat(poses[:, 0], a.size)
    y = np.repeat(poses[:, 1], a.size)
    return orc.cast_many(om, x, y, angle.ravel())[1].reshape(poses.shape[0], a.size)


def terms(orc, om, poses, ang, obs, beam_stride=1):
    """(double)L[row_j][r(w, j)] of every window pose and used beam"""
    P = om.max_range_px
    L = orc.eng_log_table(orc.sensor_table(P))
    rows = orc.obs_index(np.asarray(obs, np.float32), om)[used(ang.size, beam_stride)]
    r = steps(orc, om, poses, ang, beam_stride)
    return L[rows[None, :], r].astype(np.float64)


def q3(t):
    """RB3's order over the columns of t (n, used beams): 64 lane sums, then the butterfly"""
    with np.errstate(invalid="ignore"):
        lanes = np.zeros((t.shape[0], LANES))
        for u in range(t.shape[1]):
            lanes[:, u % LANES] += t[:, u]
        idx = np.arange(LANES)
        for off in (32, 16, 8, 4, 2, 1):
            lanes = lanes + lanes[:, idx ^ off]
    assert all(np.array_equal(lanes[:, 0].view(np.uint64), lanes[:, l].view(np.uint64)) for l in range(LANES))
    return lanes[:, 0].copy()


def in_order(t):
    s = np.zeros(t.shape[0])
    for u in range(t.shape[1]):
        s += t[:, u]
    return s


def scores(orc, om, poses, ang, obs, beam_stride=1):
    """RB3: the score of every pose"""
    return q3(terms(orc, om, poses, ang, obs, beam_stride))
