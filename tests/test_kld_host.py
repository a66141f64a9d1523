"""KLD-adaptive particle count, host side (no GPU): the size rule (mcl_host_kld_target) and the bin rule (mcl_host_kld_bins)
against numpy statements of the formulas in include/mcl_hip_engine.h, the refused configurations, the defaults, and the ctypes
mirror of mcl_kld_config_t."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- numpy statements of the header's rules
def np_target(k, bins, n_current):
    if bins <= 1:
        t = k.max_particles
    else:
        km1 = np.float64(bins - 1)
        a = np.float64(2.0) / (np.float64(9.0) * km1)
        b = np.float64(1.0) - a + np.sqrt(a) * np.float64(k.z)
        n = np.ceil(km1 / (np.float64(2.0) * np.float64(k.err)) * (b * b * b))
        if n >= k.max_particles:
            t = k.max_particles
        else:
            ni = int(n)
            t = min(max(-(-ni // k.round_to) * k.round_to, k.min_particles), k.max_particles)
    if t <= n_current and t * 1000 >= n_current * k.shrink_permille:
        return n_current
    return t


def np_bins(x, y, th, W, H, res, ox, oy, k):
    res = np.float64(np.float32(res))
    nx = np.ceil(np.float64(W) * res / np.float64(k.bin_x_m))
    ny = np.ceil(np.float64(H) * res / np.float64(k.bin_y_m))
    inv_bx, inv_by = np.float64(1.0) / np.float64(k.bin_x_m), np.float64(1.0) / np.float64(k.bin_y_m)
    scale = np.float64(k.n_theta_bins) / (np.float64(2.0) * np.float64(np.pi))
    x, y, th = (np.asarray(v, np.float64) for v in (x, y, th))
    with np.errstate(invalid="ignore", over="ignore"):
        fx = np.floor((x - np.float64(ox)) * inv_bx)
        fy = np.floor((y - np.float64(oy)) * inv_by)
        inside = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny) & (np.abs(th) < 1e9)
        t = np.where(inside, np.floor((th + np.float64(np.pi)) * scale), 0.0).astype(np.int64)
    it = np.mod(t, k.n_theta_bins)
    b = (it * int(ny) + np.where(inside, fy, 0).astype(np.int64)) * int(nx) + np.where(inside, fx, 0).astype(np.int64)
    outside = int(nx) * int(ny) * k.n_theta_bins
    b = np.where(inside, b, outside)
    return int(np.unique(b).size)


@pytest.fixture(scope="module")
def E(engine_mod):
    return engine_mod


def test_default_kld_config(E):
    k = E.default_kld_config()
    assert (k.min_particles, k.max_particles) == (256, 4194304)
    assert (k.err, k.z, k.bin_x_m, k.bin_y_m) == (0.01, 2.326, 0.5, 0.5)
    assert (k.n_theta_bins, k.round_to, k.shrink_permille, k.reserved) == (36, 256, 800, 0)


def test_kld_struct_layout_matches_header(E, tmp_path):
    probe = tmp_path / "probe.c"
    fields = [f for f, _ in E.KldConfig._fields_]
    offs = ",".join(f"offsetof(mcl_kld_config_t, {f})" for f in fields)
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcl_hip_engine.h"\n'
                     'int main(void){size_t v[] = {sizeof(mcl_kld_config_t), ' + offs + '};'
                     'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    import ctypes
    assert got == [ctypes.sizeof(E.KldConfig)] + [getattr(E.KldConfig, f).offset for f in fields]


@pytest.mark.parametrize("bins", [0, 1, 2, 3, 10, 10 ** 3, 10 ** 6])
@pytest.mark.parametrize("over", [{}, dict(min_particles=1, max_particles=1 << 26, round_to=1),
                                  dict(min_particles=500, max_particles=100000, round_to=64, err=0.05, z=1.645),
                                  dict(round_to=1000, shrink_permille=1000), dict(shrink_permille=0, z=0.0)])
def test_target_matches_formula(E, bins, over):
    k = E.default_kld_config(**over)
    for n_current in (1, 256, 1000, 4096, 8192, 65536, 262144, 4194304):
        got = E.host_kld_target(k, bins, n_current)
        assert got == np_target(k, bins, n_current), (bins, n_current)
        assert got == n_current or k.min_particles <= got <= k.max_particles


def test_target_rounding_clamping_and_hysteresis(E):
    k = E.default_kld_config(min_particles=256, max_particles=100000, round_to=256, shrink_permille=800)
    # k <= 1: the maximum
    assert E.host_kld_target(k, 0, 5000) == 100000 and E.host_kld_target(k, 1, 5000) == 100000
    # two bins: ceil(50 * b^3) = 330, rounded up to 512; below the minimum -> the minimum (from a large set: no hysteresis)
    assert E.host_kld_target(k, 2, 100000) == np_target(k, 2, 100000) == 512
    assert E.host_kld_target(E.default_kld_config(min_particles=1000, max_particles=100000), 2, 100000) == 1000
    # many bins: clamped to the maximum
    assert E.host_kld_target(k, 10 ** 6, 1000) == 100000
    # rounded up to a multiple of round_to
    k1 = E.default_kld_config(round_to=1, min_particles=1)
    raw = E.host_kld_target(k1, 40, 10 ** 7 - 1)
    assert E.host_kld_target(k, 40, 10 ** 7 - 1) == -(-raw // 256) * 256 != raw
    # hysteresis: keep N while target <= N and target >= 0.8 N ...
    t = E.host_kld_target(k, 40, 10 ** 7 - 1)
    assert E.host_kld_target(k, 40, t) == t
    assert E.host_kld_target(k, 40, t + 1) == t + 1                      # target just below N: keep
    assert E.host_kld_target(k, 40, (t * 1000) // 800) == (t * 1000) // 800    # exactly at the edge: keep
    assert E.host_kld_target(k, 40, (t * 1000) // 800 + 1) == t            # below 0.8 N: shrink
    assert E.host_kld_target(k, 40, t - 1) == t                            # target above N: grow
    # shrink_permille = 1000: every change is taken
    kn = E.default_kld_config(shrink_permille=1000)
    assert E.host_kld_target(kn, 40, t + 1) == t


def test_invalid_configs_are_refused(E):
    bad = [dict(min_particles=0), dict(min_particles=10, max_particles=5), dict(max_particles=1 << 27), dict(err=0.0),
           dict(err=float("nan")), dict(z=-1.0), dict(z=float("inf")), dict(bin_x_m=0.0), dict(bin_y_m=-0.5),
           dict(bin_x_m=float("nan")), dict(n_theta_bins=0), dict(round_to=0), dict(shrink_permille=-1),
           dict(shrink_permille=1001), dict(reserved=1)]
    x = np.zeros(4)
    for over in bad:
        k = E.default_kld_config(**over)
        with pytest.raises(E.EngineError) as ei:
            E.host_kld_target(k, 10, 1000)
        assert ei.value.status == -1, over
        with pytest.raises(E.EngineError):
            E.host_kld_bins(x, x, x, 100, 100, 0.05, 0.0, 0.0, k)
    k = E.default_kld_config()
    with pytest.raises(E.EngineError):
        E.host_kld_target(k, 10, -1)
    with pytest.raises(E.EngineError):
        E.host_kld_bins(x, x, x, 0, 100, 0.05, 0.0, 0.0, k)
    with pytest.raises(E.EngineError):
        E.host_kld_bins(x, x, x, 100, 100, 0.0, 0.0, 0.0, k)
    # a bin grid of more than 2^31 bits
    with pytest.raises(E.EngineError):
        E.host_kld_bins(x, x, x, 200000, 200000, 0.05, 0.0, 0.0, E.default_kld_config(bin_x_m=0.01, bin_y_m=0.01))
    # the bound is on nx * ny * n_theta_bins + 1: 40000 x 40000 bins pass with one heading bin, not with two
    assert E.host_kld_bins(x, x, x, 200000, 200000, 1.0, 0.0, 0.0,
                           E.default_kld_config(bin_x_m=5.0, bin_y_m=5.0, n_theta_bins=1)) == 1
    with pytest.raises(E.EngineError):
        E.host_kld_bins(x, x, x, 200000, 200000, 1.0, 0.0, 0.0, E.default_kld_config(bin_x_m=5.0, bin_y_m=5.0, n_theta_bins=2))


def test_bins_random_clouds(E, spielberg):
    m = spielberg
    rng = np.random.default_rng(7)
    W, H = m.data.shape[1], m.data.shape[0]
    res = float(np.float32(m.resolution))
    for over in ({}, dict(bin_x_m=0.25, bin_y_m=0.3, n_theta_bins=72), dict(bin_x_m=2.0, bin_y_m=2.0, n_theta_bins=1),
                 dict(bin_x_m=0.1, bin_y_m=0.1, n_theta_bins=7)):
        k = E.default_kld_config(**over)
        for n, sig in ((5000, 0.5), (20000, 3.0), (1000, 50.0)):
            x = m.origin_x + W * res / 2 + rng.normal(0, sig, n)
            y = m.origin_y + H * res / 2 + rng.normal(0, sig, n)
            th = rng.uniform(-4 * np.pi, 4 * np.pi, n)
            got = E.host_kld_bins(x, y, th, W, H, m.resolution, m.origin_x, m.origin_y, k)
            assert got == np_bins(x, y, th, W, H, m.resolution, m.origin_x, m.origin_y, k)
            assert 1 <= got <= n


def test_bins_adversarial_poses(E):
    W, H, res, ox, oy = 200, 120, np.float32(0.05), -3.3, 1.7
    k = E.default_kld_config()
    r = float(res)
    nx, ny = math.ceil(W * r / 0.5), math.ceil(H * r / 0.5)
    xs = [ox + i * 0.5 for i in range(nx + 1)] + [ox, ox - 1e-12, ox + W * r, ox + W * r - 1e-9, ox + nx * 0.5, ox + 0.2]
    ys = [oy + j * 0.5 for j in range(ny + 1)] + [oy, oy - 1e-12, oy + H * r, oy + 0.3]
    ths = [np.pi, -np.pi, 3 * np.pi, -3 * np.pi, 0.0, 2 * np.pi, -2 * np.pi, np.nextafter(np.pi, 0), np.nextafter(-np.pi, 0),
           np.pi / 18, -np.pi / 18, 1e9, -1e9, np.nextafter(1e9, 0), -np.nextafter(1e9, 0)]
    X, Y, T = np.meshgrid(np.array(xs), np.array(ys), np.array(ths), indexing="ij")
    x, y, th = X.ravel(), Y.ravel(), T.ravel()
    bad = np.array([np.nan, np.inf, -np.inf, 0.0])
    x = np.concatenate([x, bad, np.full(4, ox + 1.0), np.full(4, ox + 1.0)])
    y = np.concatenate([y, np.full(4, oy + 1.0), bad, np.full(4, oy + 1.0)])
    th = np.concatenate([th, np.zeros(4), np.zeros(4), bad])
    got = E.host_kld_bins(x, y, th, W, H, res, ox, oy, k)
    assert got == np_bins(x, y, th, W, H, res, ox, oy, k)
    # the outside bin is one bin: many poses off the map / non-finite / |theta| >= 1e9 add exactly one
    inside = np.array([ox + 1.0, ox + 2.0]), np.array([oy + 1.0, oy + 1.0]), np.array([0.1, 0.1])
    base = E.host_kld_bins(*inside, W, H, res, ox, oy, k)
    assert base == 2
    out_x = np.array([np.nan, np.inf, ox - 1.0, ox + 100.0, ox + 1.0, ox + 1.0, ox + 1.0])
    out_y = np.array([oy + 1.0, oy + 1.0, oy + 1.0, oy + 1.0, -np.inf, oy + 1.0, oy + 1.0])
    out_t = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1e9, np.nan])
    got = E.host_kld_bins(np.concatenate([inside[0], out_x]), np.concatenate([inside[1], out_y]),
                          np.concatenate([inside[2], out_t]), W, H, res, ox, oy, k)
    assert got == base + 1
    # theta = +-pi and +-3pi share a heading bin with each other (the turn wraps), -pi + tiny is bin 0
    one = lambda t: E.host_kld_bins(np.array([ox + 1.0] * len(t)), np.array([oy + 1.0] * len(t)), np.array(t), W, H, res, ox, oy, k)
    assert one([np.pi, -np.pi, 3 * np.pi, -3 * np.pi]) == 1
    assert one([np.nextafter(-np.pi, 0), np.pi / 18 - np.pi + 1e-12]) == 2
    # empty input: no bins
    assert E.host_kld_bins(np.zeros(0), np.zeros(0), np.zeros(0), W, H, res, ox, oy, k) == 0


@pytest.mark.parametrize("n_theta", [1, 7, 36, 1000003, 50000000])
def test_heading_bins_far_from_zero(E, n_theta):
    """Headings up to |theta| < 1e9 and heading-bin counts from 1 to 5e7: the remainder the bin rule takes is exact (with 5e7
    bins the integral quotient passes 2^52, the rule's other branch)."""
    rng = np.random.default_rng(n_theta)
    W, H, res, ox, oy = 4, 4, np.float32(1.0), 0.0, 0.0
    k = E.default_kld_config(bin_x_m=4.0, bin_y_m=4.0, n_theta_bins=n_theta)
    th = np.concatenate([rng.uniform(-1e9, 1e9, 3000), rng.uniform(-50.0, 50.0, 3000),
                         np.nextafter(np.array([1e9, -1e9]), 0.0), -np.pi + 2 * np.pi * np.arange(-40, 40) / n_theta])
    x = np.full(th.size, 1.0)
    for lo in range(0, th.size, 37):
        sl = slice(lo, lo + 37)
        assert E.host_kld_bins(x[sl], x[sl], th[sl], W, H, res, ox, oy, k) == np_bins(x[sl], x[sl], th[sl], W, H, res, ox, oy, k)
