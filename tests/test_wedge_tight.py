"""The tight wedge fields (csrc/mcl_wedge.h: a stop cell bounds a jump by the distance from the origin to the part of its offset
square that lies INSIDE the wedge), checked on the CPU:
* against an independent brute force -- the closed offset square clipped against the (widened) cone as a polygon in plain
  Python, the minimum over every stop cell, the same margins;
* the property the row search rests on: along every row of offsets the value does not decrease away from ox = 0;
* the property that matters: a skipping march on these fields returns the step index of the oracle's literal march."""
import math

import numpy as np
import pytest

from test_host_precompute import padded_stops
from test_wedge_fields import open_square_meets_wedge

WIDEN, SLACK = 1e-7, 1e-6          # mcl_wedge.h: kWedgeWiden, kWedgeSlack


def _clip(poly, nx, ny):
    """Sutherland-Hodgman: the part of the convex polygon with n . p >= 0."""
    out = []
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        dp, dq = nx * p[0] + ny * p[1], nx * q[0] + ny * q[1]
        if dp >= 0:
            out.append(p)
        if (dp >= 0) != (dq >= 0):
            t = dp / (dp - dq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _dist_origin_polygon(poly):
    best = math.inf
    for i, p in enumerate(poly):
        q = poly[(i + 1) % len(poly)]
        ex, ey = q[0] - p[0], q[1] - p[1]
        l2 = ex * ex + ey * ey
        t = 0.0 if l2 == 0.0 else min(1.0, max(0.0, -(p[0] * ex + p[1] * ey) / l2))
        best = min(best, math.hypot(p[0] + t * ex, p[1] + t * ey))
    return best


def brute_value(ox, oy, k, K):
    """What a stop cell at offset (ox, oy) allows in wedge k, or None where no ray of the wedge reaches it."""
    a0, a1 = 2 * math.pi * k / K, 2 * math.pi * (k + 1) / K
    if not open_square_meets_wedge(ox, oy, a0, a1):
        return None
    g2 = max(abs(ox) - 1, 0) ** 2 + max(abs(oy) - 1, 0) ** 2
    base = math.isqrt(g2) + 1
    if g2 == 0:
        return base
    b0, b1 = a0 - WIDEN, a1 + WIDEN
    poly = [(ox - 1.0, oy - 1.0), (ox + 1.0, oy - 1.0), (ox + 1.0, oy + 1.0), (ox - 1.0, oy + 1.0)]
    poly = _clip(poly, -math.sin(b0), math.cos(b0))          # left of the lower edge
    poly = _clip(poly, math.sin(b1), -math.cos(b1))          # right of the upper edge
    assert len(poly) >= 3, (ox, oy, k)                       # the open square meets the wedge: the closed one meets the wider one
    return max(base, math.floor(_dist_origin_polygon(poly) - SLACK) + 1)


_TABLES = {}


def brute_table(k, K, R):
    """brute_value over [-R, R]^2 as an int array [oy + R, ox + R], a large number where unreachable."""
    if (k, R) not in _TABLES:
        t = np.full((2 * R + 1, 2 * R + 1), 1 << 30, np.int64)
        for oy in range(-R, R + 1):
            for ox in range(-R, R + 1):
                v = brute_value(ox, oy, k, K)
                if v is not None:
                    t[oy + R, ox + R] = v
        _TABLES[(k, R)] = t
    return _TABLES[(k, R)]


def brute_field(grid, k, K):
    S = padded_stops(grid)
    Hp, Wp = S.shape
    pad = 3        # cells outside the grid are stops; a wedge vector into a farther one passes through this ring first
    Sb = np.pad(S, pad, constant_values=True)
    ys, xs = np.nonzero(Sb)
    ys = ys - pad; xs = xs - pad
    R = max(Hp, Wp) + pad
    T = brute_table(k, K, R)
    out = np.zeros((Hp, Wp), np.int64)
    for cy in range(Hp):
        for cx in range(Wp):
            if not S[cy, cx]:
                out[cy, cx] = min(int(T[ys - cy + R, xs - cx + R].min()), 255)
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_tight_fields_equal_polygon_bruteforce(engine_mod, seed):
    rng = np.random.default_rng(seed)
    g = np.where(rng.random((14, 17)) < [0.05, 0.15][seed], 100, 0).astype(np.int8)
    K = engine_mod.WEDGES
    n_gain = 0
    for k in range(K):
        got = engine_mod.host_skip_field_wedge_tight(g, k).astype(np.int64)
        old = engine_mod.host_skip_field_wedge(g, k).astype(np.int64)
        want = brute_field(g, k, K)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:5])
        assert (got >= old).all()
        assert ((got == 0) == (old == 0)).all()
        n_gain += int((got > old).sum())
    assert n_gain > 0          # (the rule does something on these grids)


def test_tight_value_is_monotone_along_rows(engine_mod):
    """For every wedge and every row oy, |o| <= 255: over the reachable offsets the value does not decrease away from ox = 0
    (the search looks at the nearest stop of a row on either side only), and it is never below the Euclidean rule's."""
    K, R = engine_mod.WEDGES, engine_mod.WEDGE_R
    o = np.arange(-R, R + 1)
    g = np.maximum(np.abs(o) - 1, 0).astype(np.int64)
    g2 = g[:, None] ** 2 + g[None, :] ** 2
    base = np.floor(np.sqrt(g2.astype(np.float64))).astype(np.int64)
    base = np.where(base * base > g2, base - 1, base)
    base = np.where((base + 1) * (base + 1) <= g2, base + 1, base) + 1
    n_pairs = 0
    for k in range(K):
        val, reach = engine_mod.host_wedge_tight_table(k)
        val = val.astype(np.int64)
        assert reach.any()
        assert (val >= base).all()
        right_v, right_r = val[:, R:], reach[:, R:]                   # ox = 0, 1, ..
        left_v, left_r = val[:, R::-1], reach[:, R::-1]               # ox = 0, -1, ..
        for v, r in ((right_v, right_r), (left_v, left_r)):
            both = r[:, 1:] & r[:, :-1]
            assert (v[:, 1:][both] >= v[:, :-1][both]).all(), k
            n_pairs += int(both.sum())
            # the reachable offsets of a row on one side form one interval, so neighbouring pairs are all there is to compare
            assert ((np.diff(r.astype(np.int8), axis=1) != 0).sum(axis=1) <= 2).all()
    assert n_pairs > 100000
    # the table is the polygon brute force, wherever the search would look (spot check around the apex, every wedge)
    for k in range(K):
        val, reach = engine_mod.host_wedge_tight_table(k)
        T = brute_table(k, K, 12)
        for oy in range(-12, 13):
            for ox in range(-12, 13):
                if reach[oy + R, ox + R]:
                    assert val[oy + R, ox + R] == T[oy + 12, ox + 12], (k, ox, oy)
                else:
                    assert T[oy + 12, ox + 12] == 1 << 30, (k, ox, oy)


def _march(F, P, W, H, px, py, ang):
    """The walk's rule on field F (padded): first sample the own cell's skip away, ends on a stop byte or past P.
    Returns the step index, or None when a sample comes within 1e-9 px of a cell boundary."""
    ux, uy = math.cos(ang), math.sin(ang)
    s = max(int(F[int(math.floor(py)) + 1, int(math.floor(px)) + 1]), 1)
    while s <= P:
        sx_, sy_ = px + s * ux, py + s * uy
        fx, fy = sx_ - math.floor(sx_), sy_ - math.floor(sy_)
        if min(fx, 1 - fx, fy, 1 - fy) < 1e-9:
            return None
        cx, cy = int(math.floor(sx_)) + 1, int(math.floor(sy_)) + 1
        if cx < 0 or cy < 0 or cx > W or cy > H:
            return s - 1
        d = F[cy, cx]
        if d == 0:
            return s - 1
        s += int(d)
    return P


def _sub_grid(request, name):
    if name == "sibal1":
        m = request.getfixturevalue("sibal1")
        return np.ascontiguousarray(m.data[40:140, 80:200]), m.resolution
    m = request.getfixturevalue("spielberg")
    c0, r0 = int(round(-m.origin_x / m.resolution)), int(round(-m.origin_y / m.resolution))      # the cell of the world's origin
    r0, c0 = min(max(r0 - 150, 0), m.data.shape[0] - 300), min(max(c0 - 150, 0), m.data.shape[1] - 300)
    return np.ascontiguousarray(m.data[r0:r0 + 300, c0:c0 + 300]), m.resolution


@pytest.mark.parametrize("name", ["sibal1", "spielberg"])
def test_tight_march_equals_literal_march(request, engine_mod, orc, name):
    """4000 rays per map: random ones, headings exactly on multiples of pi/8 (wedge edges and axes), and rays that start in a
    free cell next to a wall and head along it (the case the rule is about), exactly and slightly off the axis."""
    sub, res = _sub_grid(request, name)
    H, W = sub.shape
    om = orc.OracleMap(sub, res, 0.0, 0.0)
    P = om.max_range_px
    K = engine_mod.WEDGES
    fields = [engine_mod.host_skip_field_wedge_tight(sub, k).astype(np.int64) for k in range(K)]
    assert sum(int((fields[k] > engine_mod.host_skip_field_wedge(sub, k)).sum()) for k in (0, 5)) > 0
    rng = np.random.default_rng(11)
    free = np.argwhere(sub == 0)
    n = 4000
    pick = free[rng.integers(0, len(free), n)]
    ang = rng.uniform(-math.pi, math.pi, n)
    ang[:256] = np.round(ang[:256] / (math.pi / 8)) * (math.pi / 8)
    # free cells with an occupied cell among their eight neighbours: heading along the wall, i.e. at right angles to the
    # direction of that neighbour (an axis or a diagonal), either way; half of them exactly, half up to 0.05 rad off
    occ = np.pad(sub > 50, 1, constant_values=False)
    near = []
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        hit = occ[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] & (sub == 0)
        near += [(r, c, math.atan2(dx, -dy)) for r, c in np.argwhere(hit)]
    assert len(near) > 100
    nw = 1200
    for i, j in enumerate(rng.integers(0, len(near), nw)):
        pick[256 + i] = near[j][:2]
        ang[256 + i] = near[j][2] + (math.pi if rng.random() < 0.5 else 0.0) + (rng.uniform(-0.05, 0.05) if i % 2 else 0.0)
    x = (pick[:, 1] + rng.random(n)) * om.resolution
    y = (pick[:, 0] + rng.random(n)) * om.resolution
    _, steps = orc.cast_many(om, x, y, ang)
    checked = 0
    for i in range(n):
        k = int(math.floor(ang[i] * K / (2 * math.pi))) % K
        r = _march(fields[k], P, W, H, x[i] / om.resolution, y[i] / om.resolution, ang[i])
        if r is None:
            continue
        checked += 1
        assert r == steps[i], (i, k, r, steps[i], x[i], y[i], ang[i])
    assert checked > 0.95 * n, checked
