"""A family of scan geometries -- beam sets -- for the updates and the side calls, and the rules of mcl_set_beam_angles,
choose_ray_mode, plan_sweep_form and the beam search's grid restated in numpy from their comments (`predict`).  A plain helper
module (like side_geometries.py, whose axis is the map): no device, no fixtures.

Every member but the three cut from `hokuyo` is float32(a0) + arange(B, float32) * float32(inc), the way cpp:300-310 forms a
scan's angles.  What a member varies is what the engine branches on and the Hokuyo grid of the other tests never crosses:

  hokuyo             -135 deg, 0.25 deg, 1081   the control
  turn360            -180 deg, 1 deg, 360       span + wedge >= 2 pi (no virtual beams), two beam ranges per wedge, B == M
  turn720_from_zero  0 deg, 0.5 deg, 720        angles up to 2 pi: theta + a up to 3 pi
  descending         hokuyo[::4][::-1]          a negative increment: no windowed kernel, the beam search refuses
  repeated           hokuyo[::4], beam 100 = 99 not strictly ascending
  over_turn          -200 deg, 1 deg, 400       more than a turn
  fine2701           -135 deg, 0.1 deg, 2701    225 beams per wedge (> 120: no virtual beams), more beams than 1081
  rec1599 / rec1600  -150 deg, 0.19 deg         1856 / 1920 table columns: the last with and the first without LDS room for REC
  pad_min            -135 deg, 11 deg, 25       2.05 beams per wedge: the smallest pad
  wedge13            -135 deg, 22.5 deg, 13     one beam per wedge, beams on wedge edges
  coarse30           -135 deg, 30 deg, 10       wedges without a beam inside the span
  narrow_rear        2.0 rad, 0.5 deg, 91       45 degrees: thirteen beamless wedges, a0 far from -3 pi / 4
  one, two           1 beam; 2 beams 34 deg apart
  b16383 / b16384    -160 deg, 0.0195 deg       the count limit of the windowed kernels
  b65536             -160 deg, 0.005 deg        the largest accepted set

  family()           name -> float32 angles (read-only, built once)
  predict(ang)       what the engine must decide for the set
  beam_grid(..)      rule B1 with its refusals
  scan_for, pick     the scan and the particle sample the GPU tests share"""
import numpy as np

import side_geometries as sg

WEDGES = 16
TWO_PI, PI = 6.283185307179586, 3.141592653589793
MAX_BEAMS = 65536
REC_MAX_COLS = 1912                      # kSwWinBytes + 8 ltd_cols <= 80 KiB - 64 with a 256 x 260-byte window
SWEEP_MIN_PARTICLES, SWEEP_MIN_RAYS = 65536, 1 << 23

# choose_ray_mode's sentences
WHY_NO_WINDOWS = ("beam angles are not monotone over less than a turn (or more than 16383 beams): the windowed kernels need contiguous "
                  "beam ranges per direction wedge")
WHY_SMALL = "AUTO: fewer than 65536 particles or 2^23 rays: the self-contained k_rays_skip is the quickest"
WHY_SWEEP_LDS = "AUTO: at least 65536 particles and 2^23 rays, monotone beams, MAX_RANGE_PX <= 243"
WHY_FORCED_SWEEP = "configured: MCL_RAYS_SWEEP"
# search_beam_grid's (rule B1)
NO_ASCEND = "beam search: the beam angles must ascend (increment (a_last - a_first) / (B - 1) > 0)"
NO_GRID = "beam search: the angle grid M = round(2 pi / increment) must be at most 16384"
NO_TURN = "beam search: more beams than grid angles (B <= M = round(2 pi / increment): the scan spans more than a turn)"
NO_EVEN = "beam search: the beam angles are not evenly spaced on the grid of 2 pi / M (a deviation above 4e-6 rad)"
# mcl_query.hip
NO_QUERY = "more than 65535 beams"


def regular(a0, inc, B):
    """cpp:300-310: angle_min + i * angle_increment, all in float"""
    return (np.float32(a0) + np.arange(B, dtype=np.float32) * np.float32(inc)).astype(np.float32)


def deg(d):
    return d * np.pi / 180.0


def _build():
    hok = regular(np.float32(-3.0 * np.pi / 4.0), np.float32((3.0 * np.pi / 2.0) / 1080.0), 1081)      # oracle.beam_angles()
    rep = hok[::4].copy()
    rep[100] = rep[99]
    fam = dict(
        hokuyo=hok,
        turn360=regular(deg(-180.0), deg(1.0), 360),
        turn720_from_zero=regular(0.0, deg(0.5), 720),
        descending=hok[::4][::-1].copy(),
        repeated=rep,
        over_turn=regular(deg(-200.0), deg(1.0), 400),
        fine2701=regular(deg(-135.0), deg(0.1), 2701),
        rec1599=regular(deg(-150.0), deg(0.19), 1599),
        rec1600=regular(deg(-150.0), deg(0.19), 1600),
        pad_min=regular(deg(-135.0), deg(11.0), 25),
        wedge13=regular(deg(-135.0), deg(22.5), 13),
        coarse30=regular(deg(-135.0), deg(30.0), 10),
        narrow_rear=regular(2.0, deg(0.5), 91),
        one=regular(deg(-135.0), 0.0, 1),
        two=regular(deg(-17.0), deg(34.0), 2),
        b16383=regular(deg(-160.0), deg(0.0195), 16383),
        b16384=regular(deg(-160.0), deg(0.0195), 16384),
        b65536=regular(deg(-160.0), deg(0.005), 65536),
    )
    for a in fam.values():
        a.setflags(write=False)
    return fam


NAMES = ("hokuyo", "turn360", "turn720_from_zero", "descending", "repeated", "over_turn", "fine2701", "rec1599", "rec1600", "pad_min",
         "wedge13", "coarse30", "narrow_rear", "one", "two", "b16383", "b16384", "b65536")
# the members the side calls see (tests/test_gpu_side_scan_geometries.py)
SIDE = ("turn360", "turn720_from_zero", "descending", "over_turn", "fine2701", "narrow_rear", "coarse30", "wedge13", "one")
# the seed of the scan's millimetre perturbation, where the default 7 puts too many end points within lfield_ref.AMBIG of a cell edge
# (tests/test_scan_geometries_host.py decides)
PERTURB_SEED = {"descending": 8}
_FAMILY = None


def family():
    global _FAMILY
    if _FAMILY is None:
        _FAMILY = _build()
        assert tuple(_FAMILY) == NAMES
    return _FAMILY


# ---- the rules, restated
def beam_grid(ang, n_headings=1):
    """Rule B1 (search_beam_grid) with its refusals, in its order: dict(M, heading_step, delta, max_dev, refusal) -- refusal None or
    the sentence; M None where no grid was formed.  One beam: the headings are the grid."""
    a = np.asarray(ang, np.float32).astype(np.float64)
    B = a.size
    out = dict(M=None, heading_step=None, delta=None, max_dev=None, refusal=None)
    M = int(n_headings)
    if B >= 2:
        inc = (a[-1] - a[0]) / float(B - 1)
        if not inc > 0.0:
            return dict(out, refusal=NO_ASCEND)
        turns = TWO_PI / inc
        if not turns < 16384.5:
            return dict(out, refusal=NO_GRID)
        M = int(np.floor(turns + 0.5))
    if M > 16384:
        return dict(out, refusal=NO_GRID)
    delta = TWO_PI / float(M)
    dev = np.abs(a - (a[0] + np.arange(B, dtype=np.float64) * delta))
    out.update(M=M, delta=delta, max_dev=float(dev.max()))
    if B > M:
        return dict(out, refusal=NO_TURN)
    if M % int(n_headings) != 0:
        return dict(out, refusal=f"beam search: n_headings must divide the angle grid M = {M}")
    out["heading_step"] = M // int(n_headings)
    if not out["max_dev"] <= 4e-6:
        return dict(out, refusal=NO_EVEN)
    return out


def predict(ang, no_beam_pad=False, no_rec=False):
    """What mcl_set_beam_angles, ensure_lt and plan_sweep_form decide for the float angles `ang`, from their comments:

      accepted     1 <= B <= 65536
      quad_ok      strictly ascending, fewer than 16384 beams, (double) last - first < 2 pi - 1e-3: else no windowed kernel
      per_wedge    beams per direction wedge of 2 pi / 16: wedge / inc, inc = span / (B - 1)
      beam_pad     virtual beams at either end of the scan: ceil(per_wedge - 1e-9) when quad_ok, span + wedge < 2 pi - 1e-3, every
                   angle within a quarter spacing of the grid through the first and the last, 2 <= per_wedge <= 120; else 0
      beam_margin  (beam_pad + 2 + 7) & ~7, 0 without a pad
      ltd_cols     (B + 2 margin + 64) & ~63: the columns of the sweep's fp64 table
      rec_ok       a margin, every beam within 2e-6 rad of that grid, the padded direction table within ltd_cols + 8
      rec_room     ltd_cols <= 1912: the beams' grid offsets fit the LDS behind the window
      rec          rec_ok and rec_room: the walk turns the direction by the increment instead of fetching it
      M, refusal   beam_grid(ang) at n_headings = 1 (one beam: M is None, the headings are the grid)"""
    a = np.asarray(ang, np.float32).astype(np.float64)
    B = a.size
    if not 1 <= B <= MAX_BEAMS:
        return dict(accepted=False)
    quad_ok = bool(B < 16384 and np.all(a[1:] > a[:-1]) and a[-1] - a[0] < 2.0 * np.pi - 1e-3)
    span = a[-1] - a[0] if B > 1 else 0.0
    inc = span / float(B - 1) if B > 1 else 0.0
    wedge = 2.0 * np.pi / WEDGES
    per_wedge = wedge / inc if inc > 0.0 else float("inf")
    pad = margin = 0
    grid_dev = np.abs(a - (a[0] + np.arange(B, dtype=np.float64) * inc))
    if quad_ok and inc > 0.0 and span + wedge < 2.0 * np.pi - 1e-3 and not no_beam_pad:
        if bool(np.all(grid_dev < 0.25 * inc)) and 2.0 <= per_wedge <= 120.0:
            pad = int(np.ceil(per_wedge - 1e-9))
            margin = (pad + 2 + 7) & ~7
    ltd_cols = (B + 2 * margin + 64) & ~63
    rec_ok = bool(margin > 0 and not no_rec and grid_dev.max() <= 2e-6 and B + 2 * margin + 8 <= ltd_cols + 8)
    rec_room = ltd_cols <= REC_MAX_COLS
    g = beam_grid(ang) if B >= 2 else dict(M=None, refusal=None)
    return dict(accepted=True, B=B, quad_ok=quad_ok, per_wedge=per_wedge, beam_pad=pad, beam_margin=margin, ltd_cols=ltd_cols, rec_ok=rec_ok,
                rec_room=rec_room, rec=rec_ok and rec_room, M=g["M"], refusal=g["refusal"])


def planned(pred, n, forced_sweep=False):
    """(kernel, choose_ray_mode's sentence) of an update over n particles on a map whose range fits an LDS window (MAX_RANGE_PX <=
    243), under AUTO or MCL_RAYS_SWEEP"""
    if forced_sweep:
        return ("k_rays_sweep", WHY_FORCED_SWEEP) if pred["quad_ok"] else (None, WHY_NO_WINDOWS)
    big = n >= SWEEP_MIN_PARTICLES and n * pred["B"] >= SWEEP_MIN_RAYS
    if big and pred["quad_ok"]:
        return "k_rays_sweep", WHY_SWEEP_LDS
    return "k_rays_skip", (WHY_NO_WINDOWS if big else WHY_SMALL)


def form(pred, global_fields=False, hybrid=False):
    """the variant of k_rays_sweep (global_fields, hybrid, turned_directions) plan_sweep_form picks; the hybrid form has REC's
    room condition and needs rec_ok: without either the global-field form runs in its place"""
    hyb = bool(hybrid and pred["rec"])
    return dict(global_fields=bool((global_fields or hybrid) and not hyb), hybrid=hyb, turned_directions=pred["rec"])


# ---- what the GPU tests share
def scan_for(orc, om, ang, pose, seed=7, max_range_m=sg.MAX_RANGE, zero=True):
    """the oracle's ranges from `pose`, moved by about a millimetre (side_geometries.perturbed_scan), with the readings of
    side_geometries.ODD_READINGS (NaN, +-inf, negative, zero, max range and beyond) written in where B allows.  zero=False leaves
    the reading of 0 out: under the likelihood field its end point is the pose itself, which the refinement's windows put on
    cell edges on purpose -- every such pose would be ambiguous (LF4)."""
    plain = sg.perturbed_scan(orc, om, ang, pose, seed=seed)
    s = sg.odd_scan(plain, max_range_m)
    if not zero:
        s[s == 0.0] = plain[s == 0.0]
    return s


def seeds(g):
    """the three seeds of the refinement on the map g, the first turned by 0.23 degrees: its heading of 110 degrees with window steps
    of half a degree puts beams of the scans on a grid of whole, half or tenth degrees along a map axis, and their end points -- the
    window's positions lie on cell edges -- into the ambiguity band whatever the range"""
    s = np.array(g.seeds)
    s[0, 2] += deg(0.23)
    return s


def pick(n, k, seed=5):
    """the fixed-seed sample of k of n particles (test_beam_count_multiple_of_256's)"""
    return np.random.default_rng(seed).choice(n, k, replace=False)
