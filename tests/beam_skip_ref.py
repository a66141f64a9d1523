"""numpy restatement of beam skipping for the likelihood field (include/mcl_hip_engine.h): what the
engine's agreement counts and mask are held to.  A plain helper module beside lfield_ref.py: no device, no engine.

  Ka:      lfield_ref.K_of's expression with distance_m, held at 65536
  counts:  per used beam the number of particles whose end cell is on the map with D < Ka.  An end point within lfield_ref.AMBIG
           cell of a cell edge may land on either side in another fp64 formulation, so every used beam gets a band [lo, hi]: such
           end points taken as not agreeing (lo) and as agreeing (hi)
  mask:    AMCL's loop literally, in Python floats: a beam is kept iff cnt / n > threshold; if skipped >= n_used *
           error_threshold every used beam is integrated"""
import numpy as np

import lfield_ref as lr


def Ka_of(distance_m, resolution):
    return min(lr.K_of(distance_m, resolution), 65536)


def counts(p, angles, ranges, D, Ka, resolution, ox, oy, max_range_m, chunk=4096):
    """(lo, hi, ambiguous): the agreement counts of the used beams (LF3) in beam order as a band, and the number of ambiguous
    end points among all particles x used beams"""
    p = np.asarray(p, np.float64)
    a, r = lr.used_beams(angles, ranges, max_range_m)
    res = float(np.float32(resolution))
    lo = np.zeros(a.size, np.int64)
    n_amb = np.zeros(a.size, np.int64)
    for s in range(0, p.shape[1], chunk):
        q = p[:, s:s + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            ang = q[2][:, None] + a[None, :]
            fx = (q[0][:, None] + r[None, :] * np.cos(ang) - ox) / res
            fy = (q[1][:, None] + r[None, :] * np.sin(ang) - oy) / res
            d = lr._lookup(np.floor(fx), np.floor(fy), D)
            amb = (np.abs(fx - np.round(fx)) < lr.AMBIG) | (np.abs(fy - np.round(fy)) < lr.AMBIG)
        agree = (d >= 0) & (d < Ka)
        lo += (agree & ~amb).sum(axis=0)
        n_amb += amb.sum(axis=0)
    return lo, lo + n_amb, int(n_amb.sum())


def amcl_mask(counts_used, n, threshold, error_threshold):
    """(kept, n_skipped, integrate_all) as AMCL's likelihood_field_prob decides them, over the used beams: kept 1 summed, 2 skipped"""
    kept, skipped = [], 0
    for c in counts_used:
        if int(c) / float(n) > threshold:
            kept.append(1)
        else:
            kept.append(2)
            skipped += 1
    integrate_all = skipped >= len(kept) * error_threshold
    if integrate_all:
        kept = [1] * len(kept)
    return np.array(kept, np.uint8), skipped, int(integrate_all)
