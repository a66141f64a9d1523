"""numpy restatement of the tables under the ray stage, each from its comment (csrc/mcl_wedge.h, csrc/mcl_field_build.h above
k_ring_field, csrc/mcl_rays_sweep.h above k_build_ltd, include/mcl_hip_engine.h), not from the kernels' code: what
tests/test_gpu_ray_tables.py holds the device's bytes to.  A plain helper module (like lfield_ref.py): no device, no fixtures.

  encode    a host-twin skip field (0 = stop cell, otherwise the skip, up to 255) in the stored encoding
  ring_ref  the whole allocation of the mirrored, ringed copies of the wedge fields
  ltd_ref   the per-scan fp64 table of the sweep ray stage"""
import numpy as np

STOP = 0xFF          # the stored stop byte
CAP = 127            # the largest stored skip
UNDER = 127          # table rows below "no samples left" (mcl_rays_sweep.h: kSwUnder)


def encode(field):
    """0 becomes 255, values above 127 become 127, everything else stays as it is"""
    f = np.asarray(field).astype(np.int64)
    return np.where(f == 0, STOP, np.minimum(f, CAP)).astype(np.uint8)


def ring_ref(fields, P, layout):
    """fields: (K, Hp, Wp) stored bytes of the K wedge fields on the padded grid (the padding columns cut off); layout: the dict
    of engine.host_sweep_global_layout (pitch, rows, stride, alloc).  Field k, quadrant q = k >> log2(K / 4), fills its own
    `stride` bytes: (Hp + 4) rows of `pitch` bytes with the padded grid at offset (2, 2), mirrored in x for q in {1, 2} and in y
    for q in {2, 3} (every ray of the wedge then runs towards +x, +y); 0xFF everywhere else -- the two-cell ring, the row padding
    and every tail row up to `stride`.  What the layout must give a walk of at most P samples is asserted, not assumed."""
    fields = np.asarray(fields, np.uint8)
    K, Hp, Wp = fields.shape
    pitch, rows, stride, alloc = layout["pitch"], layout["rows"], layout["stride"], layout["alloc"]
    assert K % 4 == 0 and pitch % 64 == 0 and Wp + 4 <= pitch < Wp + 4 + 64
    assert stride == rows * pitch and alloc == K * stride
    assert (Hp + 4 + P) * pitch + (Wp + 4 + P) < stride          # the largest offset a walk can form lies in its own field
    out = np.full((K, rows, pitch), STOP, np.uint8)
    for k in range(K):
        q = k // (K // 4)
        f = fields[k]
        if q in (1, 2):
            f = f[:, ::-1]
        if q in (2, 3):
            f = f[::-1, :]
        out[k, 2:2 + Hp, 2:2 + Wp] = f
    return out.reshape(-1)


def ltd_ref(L, obs_idx, B, P, margin, cols):
    """(P + 129, cols) float64.  Row r stands for r - 127 samples left: for r <= P + 127, beam j (column j + margin) holds
    (double)L[obs_idx[j]][P - max(r - 127, 0)] -- so the 127 rows under "none left" repeat the row of none left --; the last row
    (undecided rays) is 0, and so are the columns before beam 0 and from beam B on (lanes without rays, virtual beams)."""
    L = np.asarray(L, np.float32)
    oi = np.asarray(obs_idx).astype(np.int64)
    assert L.shape == (P + 1, P + 1) and oi.shape == (B,) and margin >= 0 and margin + B < cols
    out = np.zeros((P + UNDER + 2, cols), np.float64)
    for r in range(P + UNDER + 1):
        left = max(r - UNDER, 0)
        out[r, margin:margin + B] = L[oi, P - left].astype(np.float64)
    return out


def first_diffs(got, want, n=5):
    """the first n (index..., got, want) where two arrays of one shape differ"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return [tuple(int(i) for i in ix) + (got[tuple(ix)].item(), want[tuple(ix)].item()) for ix in np.argwhere(got != want)[:n]]
