"""The global search with exact pruning (rules P1 - P5 of include/mcl_hip_engine.h) restated in numpy: the pooled
field and the bound table by brute force, the block plan, and the round schedule as a pure function of (U, the score volume, the
config).  No engine and no device: tests/test_search_pruned_host.py checks the library's host functions against these, and
tests/test_gpu_search_pruned.py holds the device's statistics to `schedule`."""
import numpy as np


def pool(D, K, w):
    """P2 by brute force: out[y + w - 1, x + w - 1] = min of D' over the w x w window with low corner (x, y)"""
    H, W = D.shape
    pad = np.full((H + 2 * (w - 1), W + 2 * (w - 1)), K, np.int64)
    pad[w - 1:w - 1 + H, w - 1:w - 1 + W] = D
    out = np.empty((H + w - 1, W + w - 1), np.uint16)
    for ys in range(H + w - 1):
        for xs in range(W + w - 1):
            out[ys, xs] = pad[ys:ys + w, xs:xs + w].min()
    return out


def bound_table(lf):
    """Ub[k] = max over j >= k of Lf[j], by its definition"""
    lf = np.asarray(lf, np.float32)
    return np.array([lf[k:].max() for k in range(lf.size)], np.float32)


def lattice_grid(data, stride):
    """S1: (pmap (ny, nx) with -1 for no position, ix, iy per position)"""
    H, W = data.shape
    h0 = stride // 2
    rows, cols = np.arange(h0, H, stride), np.arange(h0, W, stride)
    free = data[np.ix_(rows, cols)] == 0
    pmap = np.full(free.shape, -1, np.int64)
    pmap[free] = np.arange(int(free.sum()))
    iy, ix = np.nonzero(free)
    return pmap, ix, iy


def blocks(data, stride, S):
    """P1: dict(n_blocks, w, nbx, nby, blocks (n, 3): bx, by, positions; block_of_pos)"""
    pmap, ix, iy = lattice_grid(data, stride)
    ny, nx = pmap.shape
    nbx, nby = -(-nx // S), -(-ny // S)
    rows = []
    bmap = np.full((nby, nbx), -1, np.int64)
    for by in range(nby):
        for bx in range(nbx):
            held = int((pmap[by * S:by * S + S, bx * S:bx * S + S] >= 0).sum())
            if held:
                bmap[by, bx] = len(rows)
                rows.append((bx, by, held))
    return dict(n_blocks=len(rows), w=(S - 1) * stride + 2, nbx=nbx, nby=nby, blocks=np.array(rows, np.int32).reshape(-1, 3),
                block_of_pos=bmap[iy // S, ix // S])


def first_round(pairs, first_pairs=0):
    return min(first_pairs if first_pairs > 0 else max(1024, pairs // 64), pairs)


def mark(V, pmap, ix, iy, nms, scored):
    """S5 over the scored poses, a neighbour that is not scored counting as worse: the candidate mask (n_head, n_pos)"""
    n_head, n_pos = V.shape
    ny, nx = pmap.shape
    cand = scored & (V > -np.inf)
    if not nms:
        return cand
    idx = np.arange(n_head * n_pos).reshape(n_head, n_pos)
    for dk in (-1, 0, 1):
        kk = (np.arange(n_head) + dk) % n_head
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                jx, jy = ix + dx, iy + dy
                ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny)
                q = np.where(ok, pmap[np.clip(jy, 0, ny - 1), np.clip(jx, 0, nx - 1)], -1)
                ok &= q >= 0
                q = np.clip(q, 0, None)
                Vn, In, Sn = V[kk][:, q], idx[kk][:, q], scored[kk][:, q]
                consider = ok[None, :] & Sn & (In != idx)
                better = (V > Vn) | ((V == Vn) & (idx < In))
                cand &= ~consider | better
    return cand


def schedule(U, V, data, stride, S, nms, max_hits, first_pairs=0):
    """P4 / P5 from the bounds U (pairs,) and the whole volume V (n_head, n_pos): dict(hits: the pose indices reported, best first;
    pairs_scored; rounds).  Nothing here looks at more of V than the rounds have scored."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    n_head, n_pos = V.shape
    pmap, ix, iy = lattice_grid(data, stride)
    b = blocks(data, stride, S)
    n_blocks, pairs = b["n_blocks"], U.size
    assert pairs == n_head * n_blocks
    order = np.argsort(-U, kind="stable")                    # U descending, ties by pair
    rank = np.empty(pairs, np.int64)
    rank[order] = np.arange(pairs)
    Us = U[order]
    pose_rank = rank[np.arange(n_head)[:, None] * n_blocks + b["block_of_pos"][None, :]]
    idx = np.arange(n_head * n_pos).reshape(n_head, n_pos)
    n, rounds = first_round(pairs, first_pairs), 0
    while True:
        rounds += 1
        scored = pose_rank < n
        cand = mark(np.where(scored, V, -np.inf), pmap, ix, iy, nms, scored)
        ci, cv = idx[cand], V[cand]
        best = ci[np.lexsort((ci, -cv))]
        c = V.reshape(-1)[best[max_hits - 1]] if best.size >= max_hits else -np.inf
        if n == pairs or c > Us[n]:
            return dict(hits=best[:max_hits], pairs_scored=n, rounds=rounds)
        j = 0                                                # fewer than max_hits candidates: no c, the doubling alone
        if best.size >= max_hits:
            below = np.flatnonzero(Us < c)
            j = int(below[0]) if below.size else pairs
        n = max(j, min(2 * n, pairs))
