"""numpy restatement of mcl_pose_clusters: bins by the KLD rule (the formulas of test_kld_host.np_bins, per
particle), components by scipy.ndimage.label on the dense occupancy plus the heading wrap, ranks by (weight_q desc, first_bin
asc), moments by math.fsum; and the bound a device sum of a fixed reduction shape must meet."""
import math

import numpy as np
from scipy import ndimage

U = 2.0 ** -53
CHUNK = 512          # particles per unit of the device's moment passes (mcl_cluster.h kChunk)


def particle_bins(x, y, th, W, H, res, ox, oy, bx, by, nth):
    """(bin of every particle, nx, ny, the outside bin): the KLD rule with this bin size."""
    res = np.float64(np.float32(res))
    nx = int(np.ceil(np.float64(W) * res / np.float64(bx)))
    ny = int(np.ceil(np.float64(H) * res / np.float64(by)))
    inv_bx, inv_by = np.float64(1.0) / np.float64(bx), np.float64(1.0) / np.float64(by)
    scale = np.float64(nth) / (np.float64(2.0) * np.float64(np.pi))
    x, y, th = (np.asarray(v, np.float64) for v in (x, y, th))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((x - np.float64(ox)) * inv_bx)
        fy = np.floor((y - np.float64(oy)) * inv_by)
        inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny) & (np.abs(th) < 1e9)
        t = np.where(inside, np.floor((th + np.float64(np.pi)) * scale), 0.0).astype(np.int64)
    it = np.mod(t, nth)
    b = (it * ny + np.where(inside, fy, 0).astype(np.int64)) * nx + np.where(inside, fx, 0).astype(np.int64)
    outside = nx * ny * nth
    return np.where(inside, b, outside), nx, ny, outside


def components(occ_bins, nx, ny, nth):
    """{bin: smallest bin of its component} for the occupied bins (26-neighbourhood, heading wraps)."""
    occ = np.zeros((nth, ny, nx), bool)
    occ.flat[occ_bins] = True
    lab, n = ndimage.label(occ, structure=np.ones((3, 3, 3), bool))
    parent = list(range(n + 1))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    if nth > 1:
        a, b = lab[0], lab[nth - 1]
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sa = a[max(0, -dy):ny - max(0, dy), max(0, -dx):nx - max(0, dx)]
                sb = b[max(0, dy):ny - max(0, -dy), max(0, dx):nx - max(0, -dx)]
                both = (sa > 0) & (sb > 0)
                for la, lb in set(zip(sa[both].tolist(), sb[both].tolist())):
                    ra, rb = find(la), find(lb)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(i) for i in range(n + 1)], np.int64)
    comp = root[lab.ravel()[occ_bins]]
    first = {}
    for b, c in zip(occ_bins.tolist(), comp.tolist()):
        if c not in first or b < first[c]:
            first[c] = b
    return {b: first[c] for b, c in zip(occ_bins.tolist(), comp.tolist())}


def chain(n):
    """The longest addition chain of the device's reduction of n terms: a lane adds up to CHUNK / 64 terms of its unit, a
    butterfly of 6, a lane adds up to ceil(units / 64) unit sums, a butterfly of 6."""
    units = -(-n // CHUNK)
    return CHUNK // 64 + 6 + -(-units // 64) + 6


def fsum_bound(terms):
    t = np.asarray(terms, np.float64)
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


def second_moments(x, y, th, q, mean):
    """The six sums of q d d^T about `mean`, each term formed as the device forms it; (sums, sums of |term|)."""
    qd = q.astype(np.float64)
    dx, dy = x - mean[0], y - mean[1]
    dt = np.array([math.remainder(v, 2.0 * math.pi) for v in (th - mean[2]).tolist()])
    qx, qy, qt = qd * dx, qd * dy, qd * dt
    out = [fsum_bound(t) for t in (qx * dx, qx * dy, qx * dt, qy * dy, qy * dt, qt * dt)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def clusters(x, y, th, q, W, H, res, ox, oy, bx=0.5, by=0.5, nth=36, moments_of=16):
    """The clusters of the set (ranked), the label of every particle, the totals.  Each cluster is a dict with the exact integer
    fields, `members` (indices, ascending), and for the first `moments_of`: the first-moment sums, their sums of |term|,
    the mean and the covariance about it."""
    x, y, th = (np.asarray(v, np.float64) for v in (x, y, th))
    q = np.asarray(q, np.uint64)
    b, nx, ny, outside = particle_bins(x, y, th, W, H, res, ox, oy, bx, by, nth)
    out_mask = b == outside
    member = (~out_mask) & (q != 0)
    Q = int(q.sum(dtype=np.uint64))
    totals = dict(q_total=Q, q_outside=int(q[out_mask].sum(dtype=np.uint64)), n_outside=int(out_mask.sum()))
    labels = np.full(x.size, -1, np.int32)
    if not member.any():
        return [], labels, totals
    occ = np.unique(b[member])
    first_of = components(occ, nx, ny, nth)
    fb = np.full(x.size, -1, np.int64)
    fb[member] = [first_of[v] for v in b[member].tolist()]
    order = np.argsort(fb, kind="stable")
    order = order[fb[order] >= 0]
    names, starts = np.unique(fb[order], return_index=True)
    cl = []
    for name, idx in zip(names.tolist(), np.split(order, starts[1:])):
        cl.append(dict(first_bin=name, members=idx, weight_q=int(q[idx].sum(dtype=np.uint64)), n_particles=idx.size,
                       n_bins=int(np.unique(b[idx]).size)))
    cl.sort(key=lambda c: (-c["weight_q"], c["first_bin"]))
    for r, c in enumerate(cl):
        labels[c["members"]] = r
        c["weight"] = float(np.float64(c["weight_q"]) / np.float64(Q))
        if r >= moments_of:
            continue
        i = c["members"]
        qd = q[i].astype(np.float64)
        s = [fsum_bound(t) for t in (qd * x[i], qd * y[i], qd * np.sin(th[i]), qd * np.cos(th[i]))]
        c["S1"], c["A1"] = np.array([v[0] for v in s]), np.array([v[1] for v in s])
        Wd = float(np.float64(c["weight_q"]))
        c["mean"] = np.array([c["S1"][0] / Wd, c["S1"][1] / Wd, math.atan2(c["S1"][2], c["S1"][3])])
        S2, _ = second_moments(x[i], y[i], th[i], q[i], c["mean"])
        c["cov"] = np.array([[S2[0], S2[1], S2[2]], [S2[1], S2[3], S2[4]], [S2[2], S2[4], S2[5]]]) / Wd
    return cl, labels, totals


def brute_force_labels(bins, member, nx, ny, nth):
    """Per particle: the smallest bin of its component, by BFS over explicit neighbours (-1: no cluster)."""
    occ = set(bins[member].tolist())
    first = {}
    for s in sorted(occ):
        if s in first:
            continue
        comp, todo = [s], [s]
        first[s] = s
        while todo:
            v = todo.pop()
            ix, r = v % nx, v // nx
            iy, it = r % ny, r // ny
            for dt in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        jx, jy, jt = ix + dx, iy + dy, (it + dt) % nth
                        if not (0 <= jx < nx and 0 <= jy < ny):
                            continue
                        nb = (jt * ny + jy) * nx + jx
                        if nb in occ and nb not in first:
                            first[nb] = s
                            todo.append(nb)
                            comp.append(nb)
    return np.array([first[v] if m else -1 for v, m in zip(bins.tolist(), member.tolist())], np.int64)


# ---- hand-built sets on a 40 x 40 map of 0.25 m cells with origin (-5, -5): 20 x 20 bins of 0.5 m
HAND_MAP = dict(W=40, H=40, res=0.25, ox=-5.0, oy=-5.0)


def at(ix, iy, it, k=1, nth=36, jitter=0.1, seed=0):
    """k poses inside bin (ix, iy, it), spread over the middle of the bin."""
    rng = np.random.default_rng(seed + 7919 * (ix + 20 * iy + 400 * it) + k)
    u = rng.uniform(-jitter, jitter, (3, k))
    x = -5.0 + (ix + 0.5 + u[0]) * 0.5
    y = -5.0 + (iy + 0.5 + u[1]) * 0.5
    th = -math.pi + (it + 0.5 + u[2]) * (2 * math.pi / nth)
    return np.vstack([x, y, th])


def hand_sets():
    """name -> (poses 3 x n, weights n, n_theta_bins, expected cluster count)."""
    s = {}
    p = np.hstack([at(4, 4, 18, 30), at(14, 14, 18, 10)])
    s["two_blobs_heavier_first"] = (p, np.ones(p.shape[1]), 36, 2)
    p = np.hstack([at(8, 8, 0, 5), at(8, 8, 35, 5)])
    s["heading_wrap_joins"] = (p, np.ones(p.shape[1]), 36, 1)
    p = np.hstack([at(8, 8, 0, 5), at(8, 8, 34, 5)])
    s["heading_gap_splits"] = (p, np.ones(p.shape[1]), 36, 2)
    p = np.hstack([at(4, 4, 10, 5), at(5, 5, 11, 5)])
    s["diagonal_joins"] = (p, np.ones(p.shape[1]), 36, 1)
    p = np.hstack([at(4, 4, 10, 5), at(6, 4, 10, 5)])
    s["one_bin_gap_splits"] = (p, np.ones(p.shape[1]), 36, 2)
    p = np.hstack([at(4, 4, 10, 5), at(5, 4, 10, 5), at(6, 4, 10, 5)])
    w = np.r_[np.ones(5), np.zeros(5), np.ones(5)]
    s["zero_weight_does_not_bridge"] = (p, w, 36, 2)
    p = np.hstack([at(10, 10, 3, 6), np.array([[100.0, 0.0, np.nan, 0.0], [0.0, -100.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1e9]])])
    s["outside_nan_huge_heading_excluded"] = (p, np.ones(p.shape[1]), 36, 1)
    p = np.hstack([at(15, 3, 7, 8), at(3, 15, 7, 8)])
    s["equal_weights_by_first_bin"] = (p, np.ones(p.shape[1]), 36, 2)
    p = np.hstack([at(4, 4, 0, 4), at(5, 4, 17, 4), at(12, 12, 30, 4)])
    s["one_heading_bin"] = (p, np.ones(p.shape[1]), 1, 2)
    p = np.hstack([at(4, 4, 0, 4, nth=2), at(5, 5, 1, 4, nth=2), at(12, 12, 1, 4, nth=2)])
    s["two_heading_bins"] = (p, np.ones(p.shape[1]), 2, 2)
    return s
