"""Whole-set checker: drives one engine through updates and compares it with the spec oracle (oracle/mcl_oracle.c) on EVERY
particle of every update -- resample indices, children, log-weights, fixed-point weights, the sums in SCALARS, the readbacks built
from them, sample_particles and particle_mean.  A plain helper module (imported like oracle_shard.py), no GPU work at import.

Rule of the chain: the expectation for the next update is built only from oracle outputs, or from engine outputs this update has
already matched on every particle -- the children, matched within 1e-13 before the oracle casts their rays.  A wrong value
anywhere in the set therefore fails the update it appears in, instead of feeding the next update's "expected" value.

The sums in SCALARS come out of a fixed-order tree on the device; they are checked against math.fsum (exactly rounded) of the
oracle's terms within (h + 2) * 2^-53 * sum |t_i|, h the longest addition chain of that tree (chain_length).  The host readbacks
composed from SCALARS (weights, expected pose, N_eff) are then checked exactly."""
import math

import numpy as np

ACTION = (0.1, 0.0, 0.02)
U = 2.0 ** -53
# Device sincos (double) within 2 ulp, glibc sin/cos within 1 ulp: a trig term w * sin(theta) may differ from numpy's by 3 ulp of
# the sine, i.e. 6 * 2^-53 of the term, on top of the sum's own rounding.
TRIG_ULPS = 3
# The ordering of the sweep's rays has no readback.  mcl_engine.hip takes the radix sort for `n >= 3000000` particles (the
# counting sort below); the tests pick their sizes on either side of this constant.
RADIX_MIN = 3000000
TINY_TAIL_MAX = 8192            # k_tiny_tail (kTinyTailMax): the one-workgroup tail of an update of at most this many particles
SWEEP_MIN_PARTICLES = 65536     # AUTO: k_rays_sweep from this many particles and 2^23 rays
SWEEP_MIN_RAYS = 1 << 23
SAMPLE_K = 4096
RED_THREADS_TOTAL = 1024 * 256  # k_weights: kRedBlocks x kRedThreads threads, each over a strided run of the particles
COLSUM_THREADS_TOTAL = 256 * 256  # k_colsum (particle_mean): 256 workgroups x kRedThreads


def chain_length(n):
    """Longest addition chain behind each of the weighted sums in SCALARS over n particles.
    k_weights + final_sums_of: ceil(n / 2^18) per thread, 6 (wave butterfly) + 4 (waves of a workgroup), then per thread of
    final_sums_of 1024 / 256 = 4 partials, 6 + 4 again: ceil(n / 2^18) + 24.
    k_tiny_tail (n <= 8192): ceil(n / 1024) per thread, 6 (wave butterfly) + 16 (waves in order): at most 30.
    ceil(n / 2^18) + 30 bounds both."""
    return -(-int(n) // RED_THREADS_TOTAL) + 30


def sum_rel_bound(n, trig=False):
    """Allowed |device sum - fsum| as a multiple of sum |t_i|: each term's own rounding (the product), the chain, and for the
    trig sums the sin/cos allowance."""
    return (chain_length(n) + 2 + (2 * TRIG_ULPS if trig else 0)) * U


def mean_chain_length(n):
    """particle_mean: k_colsum ceil(n / 2^16) per thread, 6 + 4 in the workgroup, then the host adds 256 partials in order."""
    return -(-int(n) // COLSUM_THREADS_TOTAL) + 6 + 4 + 256


def native_sample_k53(orc, seed, ctr, k):
    """The 53-bit uniforms of mcl_sample_particles without injected uniforms: Philox4x32-10 stream 4, counter (m, ctr, 4, 0),
    key = seed, bits53 of the first two words (csrc/mcl_device_math.h); ctr = the engine's update count."""
    key = (int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    out = np.empty(k, np.uint64)
    for m in range(k):
        o = orc.eng_philox4x32((m, int(ctr), 4, 0), key)
        out[m] = ((int(o[0]) << 32) | int(o[1])) >> 11
    return out


def injected_k53(u):
    """k_sample's conversion of an injected uniform: floor(max(u, 0) * 2^53), clamped below 2^53."""
    k = np.floor(np.maximum(np.asarray(u, np.float64), 0.0) * 2.0 ** 53)
    return np.minimum(k, 2.0 ** 53 - 1).astype(np.uint64)


# ------------------------------------------------------------------------------------------------------------ comparisons
def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _fail(what, bad, got, want, n):
    """AssertionError naming how many entries differ, the first few indices and both sides' values there."""
    first = bad[:5]
    def vals(a):
        a = np.asarray(a)
        return [a[..., i].tolist() for i in first]
    raise AssertionError(f"{what}: {bad.size} of {n} differ; first at {first.tolist()}: got {vals(got)}, want {vals(want)}")


def assert_same(what, got, want):
    """Bit for bit (floats compared by their bit patterns, so -inf == -inf and -0.0 != 0.0); 2-D arrays column by column."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    diff = _bits(np.ascontiguousarray(got)) != _bits(np.ascontiguousarray(want))
    if diff.ndim == 2:
        diff = diff.any(axis=0)
    bad = np.flatnonzero(diff)
    if bad.size:
        _fail(what, bad, got, want, diff.size)


def assert_close(what, got, want, rtol, atol):
    """|got - want| <= atol + rtol * |want| everywhere (numpy.testing.assert_allclose's rule); 2-D arrays column by column."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    with np.errstate(invalid="ignore"):
        diff = ~(np.abs(got - want) <= atol + rtol * np.abs(want))
    if diff.ndim == 2:
        diff = diff.any(axis=0)
    bad = np.flatnonzero(diff)
    if bad.size:
        _fail(what, bad, got, want, diff.size)


def check_sum(what, got, terms, n, trig=False):
    """A device sum against math.fsum of the oracle's terms, within sum_rel_bound(n) * sum |t_i|."""
    want = math.fsum(terms)
    tol = sum_rel_bound(n, trig) * math.fsum(np.abs(terms))
    if not abs(got - want) <= tol:
        raise AssertionError(f"{what}: got {got!r}, fsum {want!r}, |diff| {abs(got - want)!r} > bound {tol!r}")


def check_scalars(sc, w, q, mx, parts):
    """SCALARS after an update: [0] max log-weight and [2] Q (u64 bits) exactly, the six weighted sums within the bound."""
    n = w.size
    assert_same("SCALARS[0] (max log-weight)", np.array([sc[0]]), np.array([mx]))
    q_got = int(np.array([sc[2]]).view(np.uint64)[0])
    q_want = int(q.sum(dtype=np.uint64))
    if q_got != q_want:
        raise AssertionError(f"SCALARS[2] (Q): got {q_got}, want {q_want}")
    s, c = np.sin(parts[2]), np.cos(parts[2])
    for word, name, t, trig in ((1, "sum w", w, False), (3, "sum w*x", w * parts[0], False), (4, "sum w*y", w * parts[1], False),
                                (5, "sum w*sin", w * s, True), (6, "sum w*cos", w * c, True), (7, "sum w^2", w * w, False)):
        check_sum(f"SCALARS[{word}] ({name})", sc[word], t, n, trig)


def check_readbacks(e, sc, w):
    """The host's compositions of SCALARS, exactly: get_weights = w / sum w, expected_pose, N_eff."""
    s1 = sc[1]
    assert_same("get_weights", e.get_weights(), w / s1 if s1 > 0.0 else w)
    k = 1.0 / s1 if s1 > 0.0 else 1.0
    assert_same("expected_pose", e.expected_pose(), np.array([sc[3] * k, sc[4] * k, math.atan2(sc[5] * k, sc[6] * k)]))
    neff_want = sc[1] * sc[1] / sc[7] if sc[7] > 0.0 else 0.0
    assert_same("effective_sample_size", np.array([e.effective_sample_size()[0]]), np.array([neff_want]))


def check_particle_mean(got, parts):
    n = parts.shape[1]
    for r in range(3):
        want = math.fsum(parts[r]) / n
        tol = (mean_chain_length(n) + 2) * U * math.fsum(np.abs(parts[r])) / n
        if not abs(got[r] - want) <= tol:
            raise AssertionError(f"particle_mean[{r}]: got {got[r]!r}, fsum mean {want!r}, |diff| {abs(got[r] - want)!r} > {tol!r}")


def check_samples(orc, e, parts, q, seed, ctr, rng, k=SAMPLE_K):
    """sample_particles(k) with injected uniforms (the exact-CDF search) and natively (Philox stream 4); returns the native draw's
    parent indices.  Q = 0 (every weight zero, E5/E6): every draw is particle 0."""
    u = rng.random(k)
    idx = orc.eng_resample_indices(q, 0, n_children=k, k53=injected_k53(u))
    assert_same("sample_particles (injected uniforms)", e.sample_particles(k, u), parts[:, idx])
    idx = orc.eng_resample_indices(q, 0, n_children=k, k53=native_sample_k53(orc, seed, ctr, k))
    assert_same("sample_particles (Philox stream 4)", e.sample_particles(k), parts[:, idx])
    if int(q.sum(dtype=np.uint64)) == 0:
        assert (idx == 0).all()
    return idx


# ------------------------------------------------------------------------------------------------------------ the checker
class WholeSet:
    """Runs e.update and checks the whole set against the oracle after every update.

    p0: the starting particles, already matched against the oracle by the caller; q0: the oracle's fixed-point weights of the
    starting weights.  q_device: where export_state's q buffer lives ("cuda" for the engine; None: a host array, for a stand-in
    that writes through host pointers)."""

    def __init__(self, orc, om, e, ang, seed, p0, q0, mode=0, L=None, action=ACTION, q_device="cuda", rng=None,
                 sample_k=SAMPLE_K):
        self.orc, self.om, self.e, self.ang, self.seed, self.mode, self.action = orc, om, e, np.asarray(ang, np.float32), seed, mode, action
        self.L = L if L is not None else orc.eng_log_table(orc.sensor_table(om.max_range_px))
        self.p, self.q = np.ascontiguousarray(p0, np.float64), np.asarray(q0, np.uint64)
        self.q_device = q_device
        self.rng = rng if rng is not None else np.random.default_rng(12345)
        self.sample_k = sample_k
        self.upd = 0
        self.log = []

    def read_q(self, n):
        if self.q_device is None:
            q = np.empty(n, np.uint64)
            self.e.export_state(0, 0, 0, q.ctypes.data)
            return q
        import torch
        qt = torch.empty(n, dtype=torch.int64, device=torch.device(self.q_device))
        self.e.export_state(0, 0, 0, qt.data_ptr())
        return qt.cpu().numpy().view(np.uint64)

    def expected_indices(self, n):
        orc = self.orc
        if self.mode == 0:
            return orc.eng_resample_indices(self.q, 0, n_children=n, k53=orc.eng_philox_k53(self.seed, self.upd, 0, n))
        return orc.eng_resample_indices(self.q, 1, n_children=n, k0=orc.eng_philox_k0(self.seed, self.upd))

    def step(self, scan):
        orc, e, upd = self.orc, self.e, self.upd
        n = e.n
        e.update(self.action, scan)
        assert e.n == n, f"update {upd}: the set changed size ({n} -> {e.n})"
        assert e.effective_sample_size()[1], f"update {upd}: did not resample"
        tag = f"update {upd}: "
        # resample indices: the oracle's exact-CDF draw on the previous update's oracle weights
        want_idx = self.expected_indices(n)
        assert_same(tag + "resample indices", e.resample_indices(), want_idx)
        # children: the motion model on the matched parents with the spec's normals
        parts = e.get_particles()
        want_parts = orc.motion_model(self.p[:, want_idx], self.action, orc.eng_philox_normals(self.seed, upd, 0, n))
        assert_close(tag + "children", parts, want_parts, 1e-13, 1e-13)
        # log-weights of those (matched) children, bit for bit, -inf included
        oi = orc.obs_index(scan, self.om)
        want_lw, _, _ = orc.eng_log_weights(self.om, parts, self.ang, oi, self.L)
        assert_same(tag + "log-weights", e.log_weights(), want_lw)
        w, q, mx = orc.eng_weights_from_log(want_lw)
        assert_same(tag + "fixed-point weights", self.read_q(n), q)
        sc = e.scalars()
        check_scalars(sc, w, q, mx, parts)
        check_readbacks(e, sc, w)
        check_samples(orc, e, parts, q, self.seed, upd + 1, self.rng, self.sample_k)
        check_particle_mean(e.particle_mean(), parts)
        t = e.stage_timings()
        info = dict(update=upd, n=n, kernel=e.ray_kernel_name(), planned=e.planned_ray_kernel(n)[0],
                    variant=e.ray_kernel_variant(), compact_used=e.compact_list()[1], counters=e.counters(),
                    path="tiny" if t[0] == 0.0 else ("graph" if t[4] == 0.0 else "regular"), q_total=int(q.sum(dtype=np.uint64)))
        self.log.append(info)
        self.p, self.q = parts, q
        self.upd += 1
        return info
