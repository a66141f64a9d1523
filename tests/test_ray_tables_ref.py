"""tests/ray_tables_ref.py pinned on the CPU: each restatement against a case written out by hand, and the band property that the
full-size check of tests/test_gpu_ray_tables.py rests on -- a wedge-field value depends only on stop cells within 255 cells, so
the host twin of a band of rows equals the host twin of the whole map on the band's middle rows."""
import numpy as np

import ray_tables_ref as rt

X = 0xFF


def test_encode_on_a_hand_written_row():
    row = np.array([0, 1, 2, 126, 127, 128, 145, 254, 255], np.uint8)
    want = np.array([255, 1, 2, 126, 127, 127, 127, 127, 127], np.uint8)
    got = rt.encode(row)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(rt.encode(row.reshape(3, 3)), want.reshape(3, 3))


def test_ring_ref_on_a_3_by_2_grid_one_wedge_of_each_quadrant(engine_mod):
    """A 2 x 1 map: the padded grid is 3 x 2.  P = 2: pitch 64, rows 2 + 4 + (2 + 2 + 1) = 11, 704 bytes per field."""
    Wp, Hp, P = 3, 2, 2
    layout = engine_mod.host_sweep_global_layout(Wp - 1, Hp - 1, P)
    assert (layout["ok"], layout["pitch"], layout["rows"], layout["stride"], layout["alloc"]) == (True, 64, 11, 704, 16 * 704)
    fields = np.empty((16, Hp, Wp), np.uint8)
    for k in range(16):
        fields[k] = np.array([[1, 2, 3], [4, 5, 6]]) + k
    got = rt.ring_ref(fields, P, layout)
    assert got.dtype == np.uint8 and got.shape == (16 * 704,)
    got = got.reshape(16, 11, 64)
    # rows 2 and 3, columns 0 .. 6 of the field; everything else is the stop byte
    hand = {0: ([X, X, 1, 2, 3, X, X], [X, X, 4, 5, 6, X, X]),                  # quadrant 0: as stored
            4: ([X, X, 7, 6, 5, X, X], [X, X, 10, 9, 8, X, X]),                 # quadrant 1: mirrored in x
            8: ([X, X, 14, 13, 12, X, X], [X, X, 11, 10, 9, X, X]),             # quadrant 2: mirrored in x and y
            12: ([X, X, 16, 17, 18, X, X], [X, X, 13, 14, 15, X, X])}           # quadrant 3: mirrored in y
    for k, (r2, r3) in hand.items():
        want = np.full((11, 64), X, np.uint8)
        want[2, :7] = r2
        want[3, :7] = r3
        assert np.array_equal(got[k], want), k
    # the wedges of one quadrant share its mirroring
    for k in range(16):
        q = k // 4
        f = fields[k][:, ::-1] if q in (1, 2) else fields[k]
        f = f[::-1] if q in (2, 3) else f
        assert np.array_equal(got[k, 2:4, 2:5], f), k
        assert int((got[k] != X).sum()) == 6


def test_ltd_ref_on_a_two_beam_table():
    """P = 3, beams with table rows 2 and 0, margin 1, 4 columns: 132 rows."""
    P, B, margin, cols = 3, 2, 1, 4
    L = (np.arange(16, dtype=np.float32).reshape(4, 4) + np.float32(0.1))       # L[row of the reading, distance]
    L[0, 3] = -np.inf
    got = rt.ltd_ref(L, np.array([2, 0], np.int32), B, P, margin, cols)
    assert got.dtype == np.float64 and got.shape == (132, 4)
    d = lambda r, c: float(L[r, c])                                             # noqa: E731  (the float widened to double)
    none_left = [0.0, d(2, 3), d(0, 3), 0.0]
    assert none_left[2] == -np.inf
    want = np.array([none_left] * 128 +                                         # 127 rows under it, and the row itself
                    [[0.0, d(2, 2), d(0, 2), 0.0],                              # one sample left
                     [0.0, d(2, 1), d(0, 1), 0.0],
                     [0.0, d(2, 0), d(0, 0), 0.0],                              # P left: the ray has not moved
                     [0.0, 0.0, 0.0, 0.0]])                                     # the undecided rays' row
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert d(2, 3) == float(np.float32(11.1)) and d(2, 3) != 11.1               # (the float's value, not the decimal's)


def test_first_diffs_names_positions_and_values():
    a = np.zeros((2, 3, 4), np.uint8)
    b = a.copy()
    b[1, 2, 3] = 7
    b[0, 1, 0] = 9
    assert rt.first_diffs(a, b) == [(0, 1, 0, 0, 9), (1, 2, 3, 0, 7)]
    assert rt.first_diffs(a, a) == []


def test_host_twin_of_a_band_equals_the_whole_map_on_its_middle_rows(engine_mod, spielberg):
    """Data rows [r0 - 256, r0 + 32 + 256) of the 2000 x 2000 map, full width, for r0 = 700 and 1000: padded row y of a field
    belongs to data row y - 1, so the band's padded rows 257 .. 288 are the whole map's r0 + 1 .. r0 + 32.  One wedge (5, next to
    the diagonal): a whole-map wedge costs as much as seven bands."""
    k = 5
    data = spielberg.data
    assert data.shape == (2000, 2000)
    whole = engine_mod.host_skip_field_wedge_tight(data, k)
    for r0 in (700, 1000):
        band = engine_mod.host_skip_field_wedge_tight(np.ascontiguousarray(data[r0 - 256:r0 + 32 + 256]), k)
        mid, want = band[257:289], whole[r0 + 1:r0 + 33]
        assert mid.shape == want.shape == (32, 2001)
        assert np.array_equal(mid, want), (r0, rt.first_diffs(mid, want))
        assert int((want == 0).sum()) > 700 and int(want.max()) == 255          # stop cells, and values the stored cap cuts
