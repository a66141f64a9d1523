"""The ordering key with fine bits (csrc/mcl_sort_key.h), through its host twin mcl_host_sort_key -- the code the device runs.

    key = coarse << F | fine,   F in 0 .. 10

coarse is the 22-bit key units, cuts and windows are made from; the fine bits only order the particles inside a coarse bucket:
fs = max(F - 2, 0) // 4 further sub-cell bits per axis (y above x), then ft = F - 2 fs further heading bits, of the same
quantisations as the coarse fields (F = 2: two heading bits; F = 6: quarter cells and four heading bits).  Checked here against a
statement of the layout and the fields written out in Python, over the layouts the engine meets: a dense set on one or two tiles
(half cells), a set that straddles five tiles (no sub-cell bits left), a sparse set (32 x 32-cell buckets) and a compactly
numbered tile map with particles in the overflow tile.  No GPU."""
import math

import numpy as np
import pytest

W, H = 2000, 1500                 # a map of 63 x 47 tiles
KEY_LOG2, MAX_FINE = 22, 10
SPACE = 1 << KEY_LOG2
FINES = list(range(MAX_FINE + 1))


def py_layout(bbox, n):
    """sort_layout, restated: (cs, tb, inner, ss, ntiles)"""
    x0, y0, x1, y1, T, compact, play = (int(v) for v in bbox)
    ntx, nty = (x1 >> 5) - (x0 >> 5) + 1, (y1 >> 5) - (y0 >> 5) + 1
    ntiles = T + 1 if compact else ntx * nty
    cells = float(x1 - x0 + 1) * float(y1 - y0 + 1)
    if compact and T * 1024.0 < cells:
        cells = T * 1024.0
    cs, tb = 0, 6
    sparse = cells > 0 and n < 8.0 * cells
    if sparse:
        cs = 5
        while play > 0 and cs > 1 and (1 << cs) >= play - 2 and n * float(1 << (2 * cs - 2)) >= 128.0 * cells:
            cs -= 1
    while cs < 5 and (ntiles << (10 - 2 * cs + tb)) > SPACE:
        cs += 1
    while tb > 0 and (ntiles << (10 - 2 * cs + tb)) > SPACE:
        tb -= 1
    inner = 5 - cs
    ncell = ntiles << (2 * inner)
    while tb < 8 and (ncell << (tb + 1)) <= SPACE:
        tb += 1
    ss = 0
    if cs == 0 and tb == 8:
        per = n / cells / 32.0 if cells > 0 else 0.0
        while ss < 1 and (ncell << (tb + 2 * (ss + 1))) <= SPACE and per >= 32.0:
            ss += 1
            per *= 0.25
    return cs, tb, inner, ss, ntiles


def py_key(bbox, tilemap, ntx_abs, n, px, py, th, F):
    """one particle's key, restated with Python integers and math.floor"""
    cs, tb, inner, ss, _ = py_layout(bbox, n)
    x0, y0, x1, y1, T, compact, _ = (int(v) for v in bbox)

    def cell(g, hi):
        c = (int(math.floor(g)) + 1 if g < 1e9 else hi) if g > -1.0 else 0        # (NaN > -1 is False: cell 0)
        return min(max(c, 0), hi)
    cx, cy = cell(px, W), cell(py, H)
    fx, fy = px - math.floor(px) if math.isfinite(px) else math.nan, py - math.floor(py) if math.isfinite(py) else math.nan
    in_box = x0 <= cx <= x1 and y0 <= cy <= y1
    cx, cy = min(max(cx, x0), x1), min(max(cy, y0), y1)
    tile = int(tilemap[(cy >> 5) * ntx_abs + (cx >> 5)]) if compact else ((cy >> 5) - (y0 >> 5)) * ((x1 >> 5) - (x0 >> 5) + 1) + (cx >> 5) - (x0 >> 5)
    key = (((tile << inner) | ((cy & 31) >> cs)) << inner) | ((cx & 31) >> cs)
    ok_x, ok_y = 0.0 <= fx < 1.0, 0.0 <= fy < 1.0
    if ss:
        key = (((key << ss) | (int(fy * (1 << ss)) if ok_y else 0)) << ss) | (int(fx * (1 << ss)) if ok_x else 0)
    f = th * 0.15915494309189533577
    f = f - math.floor(f) if math.isfinite(f) else math.nan
    ok_t = 0.0 <= f < 1.0
    key = (key << tb) | (min(int(f * (1 << tb)), (1 << tb) - 1) if ok_t else 0)
    coarse = min(key, SPACE - 1)
    fs = (F - 2) // 4 if F > 2 else 0
    ft = F - 2 * fs
    fine = 0
    if in_box and key < SPACE and ok_x and ok_y and ok_t and abs(th) < 2.0 ** 32:
        qx = int(fx * (1 << (ss + fs))) & ((1 << fs) - 1)
        qy = int(fy * (1 << (ss + fs))) & ((1 << fs) - 1)
        qt = int(f * (1 << (tb + ft))) & ((1 << ft) - 1)
        fine = (((qy << fs) | qx) << ft) | qt
    return (coarse << F) | fine, fine, (fs, ft, ss, tb)


def tile_grid():
    return (W >> 5) + 1, (H >> 5) + 1


def compact_map(tiles):
    """tile map that numbers `tiles` (list of (ty, tx)) 0 .. and sends every other tile to the overflow id"""
    ntx, nty = tile_grid()
    tm = np.full(ntx * nty, len(tiles), np.int32)
    for k, (ty, tx) in enumerate(tiles):
        tm[ty * ntx + tx] = k
    return tm


# name -> (bbox words, tile map or None, n of the layout, expected (cs, ss))
def layouts():
    L = {}
    # dense, one tile, plain numbering of the box's tiles
    L["dense-1-tile"] = ([100, 70, 110, 76, 0, 0, 0], None, 4_000_000, (0, 1))
    # dense, two tiles, compact numbering
    L["dense-2-tiles"] = ([90, 70, 101, 76, 2, 1, 0], compact_map([(2, 2), (2, 3)]), 4_000_000, (0, 1))
    # five occupied tiles (+ overflow): 6 << 20 keys with half cells do not fit 2^22 -> no sub-cell bits
    L["straddle-5-tiles"] = ([60, 60, 130, 100, 5, 1, 0], compact_map([(1, 1), (1, 2), (1, 3), (2, 3), (3, 4)]), 4_000_000, (0, 0))
    # sparse: whole-tile buckets
    L["sparse"] = ([40, 40, 640, 440, 260, 1, 0], compact_map([(ty, tx) for ty in range(1, 14) for tx in range(1, 21)]), 100_000, (5, 0))
    # compact numbering whose box covers tiles no sampled particle marked: their particles share the overflow tile
    L["overflow-tile"] = ([64, 64, 159, 95, 2, 1, 0], compact_map([(2, 2), (2, 4)]), 4_000_000, (0, 1))
    return L


LAYOUTS = layouts()


def poses(name, rng, m=6000):
    x0, y0, x1, y1 = LAYOUTS[name][0][:4]
    # pixel coordinates over the box (cell c holds pixel coordinates [c - 1, c)), some beyond it on every side
    px = rng.uniform(x0 - 1 - 3, x1 + 3, m)
    py = rng.uniform(y0 - 1 - 3, y1 + 3, m)
    th = rng.uniform(-np.pi, np.pi, m)
    th[:50] = rng.uniform(-40.0, 40.0, 50)                 # several turns away
    px[50:60] = np.floor(px[50:60])                        # exactly on cell edges
    th[60:64] = [0.0, np.pi, -np.pi, 2 * np.pi]
    return px, py, th


@pytest.fixture(scope="module")
def twin(engine_mod):
    engine = engine_mod

    def keys(name, px, py, th, F):
        bbox, tm, n, _ = LAYOUTS[name]
        return engine.host_sort_key(np.array(bbox, np.int32), tm, W, H, px, py, th, fine=F, n_layout=n)
    return keys


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_layout_is_the_one_meant(name):
    bbox, _, n, (cs, ss) = LAYOUTS[name]
    got = py_layout(bbox, n)
    assert (got[0], got[3]) == (cs, ss), got


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_coarse_part_is_the_key_without_fine_bits(twin, name):
    px, py, th = poses(name, np.random.default_rng(1))
    k0 = twin(name, px, py, th, 0)
    assert k0.max() < SPACE
    for F in FINES:
        k = twin(name, px, py, th, F).astype(np.uint64)
        assert np.array_equal(k >> np.uint64(F), k0.astype(np.uint64)), F
        assert int(k.max()) < 1 << (KEY_LOG2 + F), F


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_fine_field_is_the_stated_quantisation(twin, name):
    bbox, tm, n, _ = LAYOUTS[name]
    ntx = tile_grid()[0]
    px, py, th = poses(name, np.random.default_rng(2), m=1500)
    seen_fine = False
    for F in FINES:
        k = twin(name, px, py, th, F)
        want = [py_key(bbox, tm, ntx, n, float(a), float(b), float(c), F) for a, b, c in zip(px, py, th)]
        assert np.array_equal(k, np.array([w[0] for w in want], np.uint64).astype(np.uint32)), F
        fine = np.array([w[1] for w in want])
        assert np.array_equal(k.astype(np.uint64) & np.uint64((1 << F) - 1), fine.astype(np.uint64)), F
        if F:
            # the fine bits of the particles inside the box take a good part of their values in 1500 draws: they do split the buckets
            assert len(np.unique(fine)) > (1 << F) // 4, (F, len(np.unique(fine)))
            seen_fine = True
    assert seen_fine


def test_the_two_forms_measured(twin):
    """F = 2: the two heading bits below the coarse eight, i.e. 10 heading bits.  F = 6: the next bit of fy, of fx, then four
    heading bits: quarter cells and 12 heading bits (dense layout: ss = 1, tb = 8)."""
    name = "dense-1-tile"
    rng = np.random.default_rng(3)
    m = 4000
    px, py, th = rng.uniform(100.0, 108.0, m), rng.uniform(70.0, 75.0, m), rng.uniform(-np.pi, np.pi, m)
    frac = th * 0.15915494309189533577
    frac -= np.floor(frac)
    fx, fy = px - np.floor(px), py - np.floor(py)
    k2, k6 = twin(name, px, py, th, 2), twin(name, px, py, th, 6)
    assert np.array_equal(k2 & 0x3FF, np.floor(frac * 1024).astype(np.uint32))              # 8 coarse + 2 fine heading bits
    assert np.array_equal(k6 & 0xF, np.floor(frac * 4096).astype(np.uint32) & 0xF)
    assert np.array_equal((k6 >> 4) & 1, np.floor(fx * 4).astype(np.uint32) & 1)
    assert np.array_equal((k6 >> 5) & 1, np.floor(fy * 4).astype(np.uint32) & 1)
    assert np.array_equal((k6 >> 6) & 0xFF, np.floor(frac * 256).astype(np.uint32))          # the coarse heading bin above them
    assert np.array_equal((k6 >> 14) & 1, np.floor(fx * 2).astype(np.uint32))                # the coarse half cell
    assert np.array_equal((k6 >> 15) & 1, np.floor(fy * 2).astype(np.uint32))


def test_split_named_by_the_caller(twin, engine_mod):
    """fine_sub names how many of the fine bits per axis are sub-cell bits: 2 with 1 is quarter cells and no further heading bit (the
    engine's default on the radix path), 4 with 2 eighths; the coarse part stays what it is, and a split that does not fit is refused."""
    bbox, tm, n, _ = LAYOUTS["dense-1-tile"]
    rng = np.random.default_rng(5)
    m = 4000
    px, py, th = rng.uniform(100.0, 108.0, m), rng.uniform(70.0, 75.0, m), rng.uniform(-np.pi, np.pi, m)
    fx, fy = px - np.floor(px), py - np.floor(py)

    def keys(F, fs):
        return engine_mod.host_sort_key(np.array(bbox, np.int32), tm, W, H, px, py, th, fine=F, n_layout=n, fine_sub=fs)
    k0 = keys(0, None)
    for F, fs in ((2, 1), (4, 2), (4, 1), (6, 3), (10, 5), (5, 0)):
        k = keys(F, fs)
        ft = F - 2 * fs
        frac = th * 0.15915494309189533577
        frac -= np.floor(frac)
        assert np.array_equal(k >> F, k0), (F, fs)
        assert np.array_equal(k & ((1 << ft) - 1), np.floor(frac * (1 << (8 + ft))).astype(np.uint32) & ((1 << ft) - 1)), (F, fs)
        assert np.array_equal((k >> ft) & ((1 << fs) - 1), np.floor(fx * (1 << (1 + fs))).astype(np.uint32) & ((1 << fs) - 1)), (F, fs)
        assert np.array_equal((k >> (ft + fs)) & ((1 << fs) - 1), np.floor(fy * (1 << (1 + fs))).astype(np.uint32) & ((1 << fs) - 1)), (F, fs)
    assert np.array_equal(keys(6, 1), keys(6, None)) and np.array_equal(keys(2, 0), keys(2, None))      # the rule's own splits
    with pytest.raises(engine_mod.EngineError):
        keys(2, 2)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_garbage_gives_no_fine_bits_and_no_overflow(twin, name):
    x0, y0, x1, y1 = LAYOUTS[name][0][:4]
    cx, cy = 0.5 * (x0 + x1) - 0.7, 0.5 * (y0 + y1) - 0.3            # a good position inside the box
    bad_th = [np.nan, np.inf, -np.inf, 1e300, -1e300, 2.0 ** 32, -2.0 ** 40, 1e15]
    bad_xy = [(np.nan, cy), (cx, np.nan), (np.inf, cy), (cx, -np.inf), (1e300, cy), (cx, -1e300), (x0 - 2.5, cy), (cx, y1 + 0.5),
              (x1 + 40.25, y1 + 40.25), (-5.0, -5.0), (W + 10.5, H + 10.5)]
    px = np.array([cx] * len(bad_th) + [p[0] for p in bad_xy] + [cx])
    py = np.array([cy] * len(bad_th) + [p[1] for p in bad_xy] + [cy])
    th = np.array(bad_th + [0.3] * len(bad_xy) + [0.3])
    k0 = twin(name, px, py, th, 0)
    for F in FINES[1:]:
        k = twin(name, px, py, th, F).astype(np.uint64)
        assert int(k.max()) < 1 << (KEY_LOG2 + F)
        assert np.array_equal(k >> np.uint64(F), k0.astype(np.uint64))
        assert not np.any(k[:-1] & np.uint64((1 << F) - 1)), (F, k[:-1] & np.uint64((1 << F) - 1))
    # (the last one is sound: with ten fine bits it has some)
    assert twin(name, px, py, th, 10)[-1] & 0x3FF


def test_wrong_arguments_are_refused(engine_mod):
    engine = engine_mod
    z = np.zeros(4)
    bbox = np.array(LAYOUTS["dense-1-tile"][0], np.int32)
    for bad in (dict(fine=-1), dict(fine=11)):
        with pytest.raises(engine.EngineError):
            engine.host_sort_key(bbox, None, W, H, z, z, z, **bad)
    with pytest.raises(engine.EngineError):                 # numbered tiles without a tile map
        engine.host_sort_key(np.array(LAYOUTS["dense-2-tiles"][0], np.int32), None, W, H, z, z, z)
    with pytest.raises(engine.EngineError):                 # a box beyond the padded grid
        engine.host_sort_key(np.array([0, 0, W + 1, 10, 0, 0, 0], np.int32), None, W, H, z, z, z)
