"""A family of map geometries for the side calls (the pose query and scores, the global searches, the refinements and the
likelihood-field update), and the restatement helpers their tests share, parametrised by the geometry.  A plain helper module
(like lfield_ref.py): no device, no fixtures.

Every member varies something the kernels index by or round through and the 120 x 90 map at 0.05 m (`small()`, the map of
tests/test_gpu_global_search.py and its siblings) never does: the row width, the lattice size, the resolution, the magnitude of
the coordinates, the content.

  Geometry        data, resolution, origin_x, origin_y, max_range_m, name; its true pose, its 64 query poses, its seeds of the
                  refinement, its scan
  family()        the members by name (built once, from fixed seeds)
  lattice ...     the helpers the side-call tests kept as module-level functions bound to W, H, OX, OY
  cloud_around .. what the tests of the filter's own stages share: clouds with their spread in cells, the oracle's world-to-cell
                  rule, the KLD bin grids and the poses that straddle their edges"""
import math

import numpy as np

import lfield_ref as lr

MAX_RANGE = 12.0
ODD_READINGS = ((3, np.nan), (10, np.inf), (11, -np.inf), (17, -0.5), (23, None), (29, "beyond"), (31, 0.0))


class Geometry:
    """A map and what the tests of one geometry share.  `true_cell`: (col, row) of a free cell on the lattices the geometry is
    searched with; `strides`: those lattices; `perturb_seed`: the seed of the scan's millimetre perturbation (changed where the
    default, 7, puts too many end points within lfield_ref.AMBIG of a cell edge: tests/test_side_geometries_host.py decides)."""

    def __init__(self, name, data, resolution, origin_x, origin_y, true_cell, strides=(2, 3), perturb_seed=7, max_range_m=MAX_RANGE,
                 window_fields=None):
        self.name = name
        self.data = np.ascontiguousarray(data, np.int8)
        self.data.setflags(write=False)
        self.resolution = np.float32(resolution)
        self.origin_x, self.origin_y = float(origin_x), float(origin_y)
        self.max_range_m = float(max_range_m)
        self.true_cell, self.strides, self.perturb_seed = tuple(true_cell), tuple(strides), perturb_seed
        self.window_fields = dict(window_fields or dict(half_xy=2, half_theta=3))
        self.memo = {}                                           # what a test module computed once for this geometry

    @property
    def H(self):
        return self.data.shape[0]

    @property
    def W(self):
        return self.data.shape[1]

    @property
    def res(self):
        """the float resolution widened to double"""
        return float(self.resolution)

    def at(self, col, row, theta=0.0):
        """the pose at (col, row) in cells, fractions allowed"""
        return (self.origin_x + col * self.res, self.origin_y + row * self.res, theta)

    def oracle(self, orc):
        if "oracle" not in self.memo:
            self.memo["oracle"] = orc.OracleMap(self.data, self.resolution, self.origin_x, self.origin_y, max_range_m=self.max_range_m)
        return self.memo["oracle"]

    # -- poses
    @property
    def lattice_pose(self):
        """the lattice pose of the true cell: its centre (S1's arithmetic) and heading k = 58 of 72 (S2), 110 degrees: with steps
        of half a degree no window heading puts a beam of the 61 (4.5 degrees apart) along a map axis (see tests/refine_ref.py)"""
        c, r = self.true_cell
        return (self.origin_x + (c + 0.5) * self.res, self.origin_y + (r + 0.5) * self.res, (2 * 58 - 72) * (math.pi / 72))

    @property
    def true_pose(self):
        """in the true cell, off its edges: the lattice pose moved by (+0.3 cell, -0.2 cell, +1.7 degrees)"""
        p = self.lattice_pose
        return (p[0] + 0.3 * self.res, p[1] - 0.2 * self.res, p[2] + math.radians(1.7))

    @property
    def corner(self):
        """(col, row) of a cell corner with four free cells around it where there is one, else the lower left of the true cell"""
        free = self.data == 0
        four = free[1:, 1:] & free[:-1, 1:] & free[1:, :-1] & free[:-1, :-1]
        rows, cols = np.nonzero(four)
        if rows.size == 0:
            return self.true_cell
        k = rows.size // 2
        return int(cols[k]) + 1, int(rows[k]) + 1

    @property
    def obstacle(self):
        """(col, row) of an occupied cell off the outer wall where there is one, else of any occupied cell, else None"""
        occ = self.data > 50
        inner = occ.copy()
        inner[0, :] = inner[-1, :] = inner[:, 0] = inner[:, -1] = False
        for m in (inner, occ):
            rows, cols = np.nonzero(m)
            if rows.size:
                return int(cols[rows.size // 2]), int(rows[rows.size // 2])
        return None

    def free_poses(self, rng, k):
        """k poses in free cells, off their edges"""
        rows, cols = np.nonzero(self.data == 0)
        pick = rng.integers(0, rows.size, k)
        fx, fy = rng.uniform(0.1, 0.9, k), rng.uniform(0.1, 0.9, k)
        return np.stack([self.origin_x + (cols[pick] + fx) * self.res, self.origin_y + (rows[pick] + fy) * self.res,
                         rng.uniform(-np.pi, np.pi, k)], axis=1)

    @property
    def query_poses(self):
        """64 finite poses: random free ones, a cell corner, a vertical and a horizontal cell edge, one inside an obstacle where
        there is one, one a cell off the map, one with theta = pi exactly"""
        if "query_poses" not in self.memo:
            p = self.free_poses(np.random.default_rng(101), 64)
            c, r = self.corner
            p[1] = self.at(c, r, 0.3)
            p[2] = self.at(c, r + 0.4, 1.0)
            p[3] = self.at(c + 0.3, r, -1.0)
            if self.obstacle is not None:
                p[4] = self.at(self.obstacle[0] + 0.5, self.obstacle[1] + 0.5, 0.5)
            p[5] = self.at(-1.0, self.true_cell[1] + 0.37, 0.1)
            p[6, 2] = np.pi
            p[0] = self.true_pose
            p.setflags(write=False)
            self.memo["query_poses"] = p
        return self.memo["query_poses"]

    @property
    def particles(self):
        """(3, 4096): free-space poses, then the 64 query poses"""
        if "particles" not in self.memo:
            p = np.concatenate([self.free_poses(np.random.default_rng(202), 4096 - 64), self.query_poses])
            p = np.ascontiguousarray(p.T)
            p.setflags(write=False)
            self.memo["particles"] = p
        return self.memo["particles"]

    @property
    def seeds(self):
        """the three seeds of the refinement: the true pose's lattice pose, a pose on a cell corner, a pose whose window reaches
        off the map (0.3 cell inside its left border)"""
        c, r = self.corner
        return np.array([self.lattice_pose, self.at(c, r, 0.3), self.at(0.3, self.true_cell[1] + 0.37, -2.0)])

    # -- scans
    def scan(self, orc, ang):
        """the ranges the oracle casts from the true pose, moved by about a millimetre (perturbed_scan)"""
        return perturbed_scan(orc, self.oracle(orc), ang, self.true_pose, seed=self.perturb_seed)


# ---- the restatement helpers of the side-call tests, by geometry
def angles(orc, B):
    """B beams over the Hokuyo's 270 degrees (B = 1081: the reference's own; B = 1: the first of them)"""
    full = orc.beam_angles()
    return full[np.linspace(0, full.size - 1, B).round().astype(int)].copy() if B > 1 else full[:1].copy()


def even_angles(orc, B):
    """B beams of the Hokuyo's 1081, evenly spaced over its 270 degrees (B = 1: the first): what the beam search's grid needs"""
    full = orc.beam_angles()
    return full[::1080 // (B - 1)].copy() if B > 1 else full[:1].copy()


def scan_at(orc, om, ang, pose):
    a = float(pose[2]) + ang.astype(np.float64)
    return orc.cast_many(om, np.full(a.size, pose[0]), np.full(a.size, pose[1]), a)[0].astype(np.float32)


def odd_scan(scan, max_range_m=MAX_RANGE):
    """the scan with readings that must not count under the likelihood field (NaN, +-inf, negative, max range and beyond) and one
    that must (0); under the beam model they land in the table's edge rows"""
    s = scan.copy()
    for j, v in ODD_READINGS:
        if j < s.size:
            s[j] = max_range_m if v is None else max_range_m + 1.0 if isinstance(v, str) else v
    return s


def perturbed_scan(orc, om, ang, pose, seed=7):
    """ranges cast by the oracle from `pose`, moved by about a millimetre (fixed seed): end points off the cell edges"""
    scan = scan_at(orc, om, ang, pose)
    return (scan + np.random.default_rng(seed).uniform(0.0005, 0.0015, scan.size).astype(np.float32)).astype(np.float32)


def masked(scan, beam_stride):
    """the scan with the readings of the beams a beam_stride leaves out replaced by NaN"""
    m = np.array(scan, np.float32)
    m[np.arange(m.size) % beam_stride != 0] = np.nan
    return m


def compose(a, r):
    """the pose r, given in the frame of the pose a, in the map frame"""
    c, s = np.cos(a[2]), np.sin(a[2])
    return (a[0] + c * r[0] - s * r[1], a[1] + s * r[0] + c * r[1], a[2] + r[2])


def lattice(engine_mod, m, stride, n_head):
    """(cells, xy, theta, poses): the lattice of S1 / S2 and its poses (n_head * n_pos, 3) in index order"""
    cells, xy = engine_mod.host_search_lattice(m.data, m.resolution, m.origin_x, m.origin_y, stride_cells=stride)
    theta = engine_mod.host_search_headings(n_headings=n_head)
    poses = np.empty((n_head, cells.size, 3))
    poses[:, :, :2] = xy[None]
    poses[:, :, 2] = theta[:, None]
    return cells, xy, theta, poses.reshape(-1, 3)


def scan_poses(engine_mod, m, rel, stride, n_head):
    """SQ2 in numpy: (S, n_head * n_pos, 3), the pose of every scan at every lattice pose in index order -- one IEEE add per
    coordinate of the lattice tables and the host's offsets table, so the bits are the device's"""
    cells, xy, theta, _ = lattice(engine_mod, m, stride, n_head)
    off = engine_mod.host_search_sequence_offsets(rel, n_headings=n_head)             # (n_head, S, 3)
    S = off.shape[1]
    out = np.empty((S, n_head, cells.size, 3))
    for s in range(S):
        out[s, :, :, 0] = xy[None, :, 0] + off[:, s, 0][:, None]
        out[s, :, :, 1] = xy[None, :, 1] + off[:, s, 1][:, None]
        out[s, :, :, 2] = off[:, s, 2][:, None]
    return out.reshape(S, -1, 3)


def hits_ref(m, V, cells, stride, nms):
    """S5 restated on the map m: the candidates' pose indices, best first.  V: (n_head, n_pos)"""
    H, W = m.data.shape
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


def window_scores(engine_mod, e, m, seeds, obs, beam_stride=1, **fields):
    """mcl_score_poses, under the engine's sensor model, on the window poses of mcl_host_refine_window over the map m, in chunks of
    at most 65536: ((M, n_win) log-likelihoods, the scan as scored -- the readings of the unused beams NaN (R2) --, the rays the
    literal march decided summed over the chunks)"""
    scored = masked(obs, beam_stride)
    seeds = np.atleast_2d(seeds)
    poses = np.concatenate([engine_mod.host_refine_window(s, m.resolution, **fields) for s in seeds])
    ll, level3 = [], 0
    for s in range(0, len(poses), 65536):
        ll.append(e.score_poses(poses[s:s + 65536], scored)["log_likelihood"])
        level3 += e.query_counters()["level3_rays"]
    return np.concatenate(ll).reshape(len(seeds), -1), scored, level3


# ---- statements the new tests add
def lattice_ref(m, stride):
    """S1 in numpy: (cells, xy) of the lattice of pitch `stride` over the map m, positions in row-major order"""
    H, W = m.data.shape
    h0 = stride // 2
    rows, cols = np.meshgrid(np.arange(h0, H, stride), np.arange(h0, W, stride), indexing="ij")
    keep = m.data[rows, cols] == 0
    rows, cols = rows[keep], cols[keep]
    res = float(np.float32(m.resolution))
    xy = np.stack([m.origin_x + (cols.astype(np.float64) + 0.5) * res, m.origin_y + (rows.astype(np.float64) + 0.5) * res], axis=1)
    return (rows * W + cols).astype(np.uint32), xy


def counts_ref(orc, om, steps, obs, tol):
    """Q4 in integers: (n_valid, n_agree (K,), n_miss (K,)) from cast steps (K, B) and the scan's table rows"""
    P = om.max_range_px
    row = orc.obs_index(np.asarray(obs, np.float32), om).astype(np.int64)
    valid = np.isfinite(obs) & (row < P)
    st = np.asarray(steps).astype(np.int64)
    agree = valid[None, :] & (np.abs(row[None, :] - st) <= tol)
    return int(valid.sum()), agree.sum(axis=1), (st == P).sum(axis=1)


def tile_plan(n_pos, M, P, budget_bytes=0):
    """B5: (T, tiles) -- T the largest multiple of 256 with T M (1 or 2 bytes) <= the budget (0: 256 MiB), at most n_pos rounded
    up to a multiple of 256, with T M <= 2^31"""
    width = 1 if P <= 255 else 2
    budget = budget_bytes or 256 << 20
    T = min(budget // (M * width), (1 << 31) // M) // 256 * 256
    T = min(T, -(-n_pos // 256) * 256)
    assert T >= 256
    return T, -(-n_pos // T)


def lf_statement(m, poses, ang, obs, **lf_fields):
    """(log-weights, alternatives, ambiguous beams per pose, beams) of tests/lfield_ref.py at `poses` (n, 3) over the map m"""
    D = lr.field(m.data, m.resolution, **{k: v for k, v in lf_fields.items() if k == "max_occ_dist_m"})
    Lf = lr.table(m.resolution, max_range_m=m.max_range_m, **lf_fields)
    want, alts, n_amb = lr.log_weights(np.ascontiguousarray(np.asarray(poses).T), ang, obs, D, Lf, m.resolution, m.origin_x, m.origin_y,
                                       m.max_range_m)
    return want, alts, n_amb, len(poses) * lr.used_beams(ang, obs, m.max_range_m)[0].size


def within_cap(n_amb, beams):
    """LF4's cap: ambiguous beams at most 1e-5 of all beams, or 2 beams where that is fewer than one"""
    return int(np.sum(n_amb)) <= max(1e-5 * beams, 2)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def lf_mismatches(got, want, alts):
    """the indices at which `got` is neither the statement's value nor one of the alternatives of an ambiguous pose (LF4)"""
    bad = []
    for i in np.flatnonzero(bits(got) != bits(want)):
        if not (int(i) in alts and got[i] in alts[int(i)]):
            bad.append((int(i), float(got[i]), float(want[i])))
    return bad


# ---- what the tests of the filter's own stages share (tests/test_update_geometries_host.py, test_gpu_update_geometries.py)
def wrap(th):
    return (th + np.pi) % (2 * np.pi) - np.pi


def cloud_around(g, rng, n, pose=None, sig_cells=(4.0, 4.0), sig_theta=0.3):
    """(3, n): a tracking cloud around `pose` (default: the true pose) with its spread in cells; on a map of a few cells part of
    it lies in walls and off the map (cloud_shares says how much)"""
    pose = g.true_pose if pose is None else pose
    p = np.empty((3, n))
    p[0] = pose[0] + rng.normal(0, sig_cells[0] * g.res, n)
    p[1] = pose[1] + rng.normal(0, sig_cells[1] * g.res, n)
    p[2] = wrap(pose[2] + rng.normal(0, sig_theta, n))
    return p


def global_cloud(g, rng, n, off=0.05):
    """(3, n): uniform over the map, the first `off` of the set up to two cells outside its border instead"""
    p = np.empty((3, n))
    p[0] = g.origin_x + rng.uniform(0, g.W, n) * g.res
    p[1] = g.origin_y + rng.uniform(0, g.H, n) * g.res
    p[2] = rng.uniform(-np.pi, np.pi, n)
    k = int(n * off)
    side = rng.integers(0, 4, k)
    d = rng.uniform(0.0, 2.0, k) * g.res
    p[0, :k] = np.where(side == 0, g.origin_x - d, np.where(side == 1, g.origin_x + g.W * g.res + d, p[0, :k]))
    p[1, :k] = np.where(side == 2, g.origin_y - d, np.where(side == 3, g.origin_y + g.H * g.res + d, p[1, :k]))
    return p


def oracle_cells(om, x, y):
    """(col, row) of world points under the oracle's own rule, the truncation of cast_ray (mcl_oracle.c: (int)((cx - origin_x) /
    resolution)), with the oracle map's own doubles"""
    with np.errstate(invalid="ignore"):
        col = np.trunc((np.asarray(x, np.float64) - om.origin_x) / om.resolution)
        row = np.trunc((np.asarray(y, np.float64) - om.origin_y) / om.resolution)
    return col.astype(np.int64), row.astype(np.int64)


def cloud_shares(om, p):
    """(share of the poses in occupied cells, share off the map) under oracle_cells"""
    col, row = oracle_cells(om, p[0], p[1])
    off = (col < 0) | (col >= om.width) | (row < 0) | (row >= om.height) | (p[0] < om.origin_x) | (p[1] < om.origin_y)
    wall = np.zeros(off.shape, bool)
    wall[~off] = om.grid[row[~off], col[~off]] > 50
    return float(wall.mean()), float(off.mean())


def mirrored_pose(g):
    """the true pose mirrored through the map's centre, moved to the centre of the nearest free cell that is not the true cell
    (on one_free there is none: the true pose turned by pi)"""
    rows, cols = np.nonzero(g.data == 0)
    keep = (cols != g.true_cell[0]) | (rows != g.true_cell[1])
    if not keep.any():
        return (g.true_pose[0], g.true_pose[1], float(wrap(g.true_pose[2] + np.pi)))
    rows, cols = rows[keep], cols[keep]
    mc, mr = g.W - 1 - g.true_cell[0], g.H - 1 - g.true_cell[1]
    k = int(np.argmin((cols - mc) ** 2 + (rows - mr) ** 2))
    return g.at(cols[k] + 0.5, rows[k] + 0.5, float(wrap(g.true_pose[2] + np.pi)))


def kld_forms(g):
    """name -> the bin fields of the three bin grids the tests use: the default 0.5 m, bins of one cell, bins larger than the map"""
    return dict(default={}, cell=dict(bin_x_m=g.res, bin_y_m=g.res), huge=dict(bin_x_m=2.0 * max(g.W, g.H) * g.res, bin_y_m=2.0 * max(g.W, g.H) * g.res))


def kld_grid(g, k):
    """(nx, ny) of the bin grid: ceil(W res / bin) per axis, in the header's arithmetic"""
    return int(np.ceil(np.float64(g.W) * np.float64(g.res) / np.float64(k.bin_x_m))), int(np.ceil(np.float64(g.H) * np.float64(g.res) / np.float64(k.bin_y_m)))


def edge_poses(g, k, rng, n=2000):
    """(3, n): poses straddling every edge of the map and of the bin grid by +-1 ulp and +-1 bin in one coordinate, the other
    anywhere from a bin outside to a bin outside, headings anywhere in +-2 turns with the turn's ends among them"""
    nx, ny = kld_grid(g, k)
    bx, by = float(k.bin_x_m), float(k.bin_y_m)

    def around(edges, b):
        out = []
        for e in edges:
            out += [e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf), e - b, e + b]
        return np.array(out)
    ex = around([g.origin_x, g.origin_x + g.W * g.res, g.origin_x + nx * bx], bx)
    ey = around([g.origin_y, g.origin_y + g.H * g.res, g.origin_y + ny * by], by)
    p = np.empty((3, n))
    p[0] = rng.uniform(g.origin_x - bx, g.origin_x + nx * bx + bx, n)
    p[1] = rng.uniform(g.origin_y - by, g.origin_y + ny * by + by, n)
    p[2] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
    which = rng.integers(0, 3, n)                               # x on an edge, y on an edge, both
    onx, ony = which != 1, which != 0
    p[0, onx] = ex[np.arange(int(onx.sum())) % ex.size]
    p[1, ony] = ey[(np.arange(int(ony.sum())) // 3) % ey.size]
    ends = np.array([np.pi, -np.pi, np.nextafter(np.pi, 0), np.nextafter(-np.pi, 0), 3 * np.pi, 0.0])
    p[2, ::7] = ends[np.arange(p[2, ::7].size) % ends.size]
    return p


# ---- the family
def _walled(W, H, gaps=True):
    """an outer wall (with a gap in the bottom and in the right wall: beams leave the map there), two interior walls, a block of
    unknown cells"""
    g = np.zeros((H, W), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    if gaps:
        g[0, W // 4:W // 4 + max(1, W // 12)] = 0
        g[H // 2:H // 2 + max(1, H // 9), -1] = 0
    if W >= 20 and H >= 20:
        g[H // 3, W // 6:7 * W // 12] = 100
        g[H // 3:5 * H // 6, 7 * W // 10] = 100
        g[2 * H // 3:2 * H // 3 + max(2, H // 9), 2:2 + max(2, W // 10)] = -1
        g[2:2 + max(1, H // 20), 5 * W // 6:5 * W // 6 + max(2, W // 12)] = -1
    return g


def small():
    """the 120 x 90 map at 0.05 m of the existing side-call tests (tests/test_gpu_global_search.py), as a Geometry"""
    g = np.zeros((90, 120), np.int8)
    g[0, :] = g[-1, :] = 100
    g[:, 0] = g[:, -1] = 100
    g[0, 30:40] = 0
    g[40:50, -1] = 0
    g[30, 20:70] = 100
    g[30:75, 85] = 100
    g[55:60, 40:45] = 100
    g[64, 64] = 100
    g[60:80, 5:15] = -1
    g[10:14, 100:110] = -1
    return Geometry("small", g, 0.05, -3.0, -2.25, true_cell=(25, 15))


def _build():
    rng = np.random.default_rng(20240)                           # (the unknown cells of one_free)
    fam = []

    def add(name, W, H, res, ox, oy, true_cell, post, **kw):
        g = _walled(W, H)
        if post is not None:
            g[post[1], post[0]] = 100                            # a post of one cell
        assert g[true_cell[1], true_cell[0]] == 0, name
        fam.append(Geometry(name, g, res, ox, oy, true_cell, **kw))

    add("narrow", 37, 301, 0.05, -1.0, -7.0, true_cell=(13, 43), post=(19, 61))
    add("wide", 517, 23, 0.05, -12.0, -0.5, true_cell=(43, 13), post=(61, 16))
    add("coarse", 64, 48, 0.25, -8.0, -6.0, true_cell=(13, 7), post=(31, 31))
    add("fine", 150, 110, 0.02, -1.5, -1.1, true_cell=(31, 19), post=(61, 61))
    add("spielberg_res", 120, 90, np.float32(0.05796), -3.37, 1.91, true_cell=(25, 13), post=(64, 64))
    add("far_origin", 120, 90, 0.05, 4096.3, -8191.7, true_cell=(25, 13), post=(64, 64))
    # 9 x 7: the wall, a gap, one post, one unknown cell; a window of steps of two cells is wider than the map
    t = np.zeros((7, 9), np.int8)
    t[0, :] = t[-1, :] = 100
    t[:, 0] = t[:, -1] = 100
    t[0, 2] = 0
    t[3, -1] = 0
    t[4, 5] = 100
    t[2, 6] = -1
    fam.append(Geometry("tiny", t, 0.05, 0.0, 0.0, true_cell=(1, 1), strides=(1, 3), window_fields=dict(half_xy=2, half_theta=3, step_xy_cells=2.0)))
    fam.append(Geometry("open", np.zeros((60, 80), np.int8), 0.05, -2.0, -1.5, true_cell=(25, 13)))
    # everything occupied or unknown but one cell, which lies on the lattices of stride 1, 2 and 3
    o = np.full((30, 40), 100, np.int8)
    o[rng.random(o.shape) < 0.2] = -1
    o[13, 19] = 0
    fam.append(Geometry("one_free", o, 0.05, -1.0, -0.75, true_cell=(19, 13), strides=(1,)))
    return {g.name: g for g in fam}


_FAMILY = None
NAMES = ("narrow", "wide", "coarse", "fine", "spielberg_res", "far_origin", "tiny", "open", "one_free")
DEGENERATE = ("open", "one_free")


def family():
    global _FAMILY
    if _FAMILY is None:
        _FAMILY = _build()
        assert tuple(_FAMILY) == NAMES
    return _FAMILY
