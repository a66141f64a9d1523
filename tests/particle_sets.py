"""A family of particle sets -- a count and a pattern of start weights -- for the updates, and the count rules of the engine
restated from their comments.  A plain helper module (like scan_geometries.py, whose axis is the scan, and side_geometries.py,
whose axis is the map): no device, no fixtures.  Everything is a pure function of the member (n, pattern).

The constants a count is measured against:

  WAVE 64            a wavefront: __ballot / __shfl in the KLD and recovery tails of resample_motion_body, one ctop entry per
                     COMPLETE group of 64 list entries, gtop every 64 merged entries
  LEADER_GROUP 16    one leader per 16 CDF entries; k_scan_final's ragged last group: (n - 1) & 15 != 15
  TAIL_THREADS 1024  k_tiny_tail: per = ceil(n / 1024) consecutive entries per thread, sixteen wave partials
  SCAN_TILE 2048     kScanTile: one workgroup of the scan, one entry of the spine
  TINY_TAIL_MAX 8192 kTinyTailMax: up to here the one-workgroup tail (no list, no leaders, the CDF in LDS), above it the captured
                     graph with the regular scan

Counts, and the side of each constant they stand on:

  1, 2, 3            fewer than a leader group, a wave, a counting-sort bucket row; n = 1: every reduction over one term
  63 / 64 / 65       one short of a wave, a wave, one lane into the second (the partially filled wave); 64 % 16 == 0 (no ragged
                     leader group), 63 and 65 ragged
  255 / 256 / 257    either side of the resampling workgroup (256 threads): 257 starts a second block with one child
  1023 / 1024 / 1025 k_tiny_tail's per = 1 with one idle thread, per = 1 with none, per = 2 with threads 513.. idle
  2047 / 2049        either side of SCAN_TILE (set_particles' scan: one tile / two, the second with one entry)
  8191               the largest odd count of the one-workgroup tail
  8193               the smallest count of the captured graph; five scan tiles, the last with one entry; (n - 1) & 15 == 0
  12297 = 3 x 4099   odd, no power of two near; (n - 1) & 15 == 8
  16385              nine scan tiles, the last with one entry; compact_cap(16385) == 4096, the floor of the rule

Patterns of start weights (what set_particles is given, so the FIRST update draws from a chosen structure; dead weights are
exactly 0, alive ones at least a quarter of the maximum, so the fixed-point weights have exactly the intended number of non-zeros):

  flat               1 / n
  first, last        all weight on particle 0 / on particle n - 1: the first and the (ragged) last leader group, tile_excl's ends
  ends               half on each
  alive<K>           K particles at seeded positions with unequal weights, K in 63, 64, 65 clipped to n (members whose clipped K
                     coincide are listed once): a list of one short of a ctop group, exactly one, one and a ragged tail
  alive4095 / 4096 / 4097   the 16385 member only: a list one short of compact_cap, a full one, and none

With 61 beams nearly every particle stays alive after the first update, so for the members up to 8192 the pattern controls the
first draw only; that is intended.  With 271 beams (the members above 8192) a few per cent survive, and the lists inside the chain
are short and ragged too (tests/test_particle_sets_host.py holds them to that).

  members()          every (n, pattern), small counts first
  start(n, pattern)  (particles (3, n), weights (n,)), read-only, built once per member
  alive(n, pattern)  how many start weights are not 0
  compact_cap(cap), list_length(k, cap)   mcl_engine.hip's rule for the list's room, and the length mcl_get_compact_list reports
  beams_step(n)      18 (61 beams) up to 8192 particles, 4 (271 beams) above
  group_start(G, per, kind)   start sets of the device-group tests (below)"""
import numpy as np

from whole_set import TINY_TAIL_MAX

WAVE = 64
LEADER_GROUP = 16
TAIL_THREADS = 1024
SCAN_TILE = 2048

SMALL = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 8191)
LARGE = (8193, 12297, 16385)
COUNTS = SMALL + LARGE
BASE = ("flat", "first", "last", "ends")
ALIVE_K = (63, 64, 65)
CAP_K = (4095, 4096, 4097)                # at n = max_particles = 16385: compact_cap - 1, compact_cap, compact_cap + 1
# the seed of a member's cloud and alive positions where the default puts an alive count inside the chain on a multiple of 64
# (tests/test_particle_sets_host.py decides)
MEMBER_SEED = {(12297, "last"): 1, (16385, "first"): 2, (16385, "alive4096"): 1}


def compact_cap(max_particles):
    """mcl_create: compact_cap = max(4096, ceil64(cap / 4)), cap / 4 an integer division"""
    return max(4096, ((int(max_particles) // 4 + 63) // 64) * 64)


def list_length(k, max_particles):
    """the length mcl_get_compact_list reports for a scanned set with k non-zero fixed-point weights: k while it fits (0: a valid,
    empty list), else -1 (no list)"""
    return int(k) if int(k) <= compact_cap(max_particles) else -1


def patterns(n):
    ks = sorted({min(k, n) for k in ALIVE_K})
    out = BASE + tuple(f"alive{k}" for k in ks)
    if n == 16385:
        out += tuple(f"alive{k}" for k in CAP_K)
    return out


def members(counts=COUNTS):
    return [(n, p) for n in counts for p in patterns(n)]


def member_id(m):
    return f"{m[0]}-{m[1]}"


def alive(n, pattern):
    if pattern == "flat":
        return n
    if pattern in ("first", "last"):
        return 1
    if pattern == "ends":
        return min(n, 2)
    k = int(pattern[len("alive"):])
    assert pattern.startswith("alive") and 1 <= k <= n, (n, pattern)
    return k


def beams_step(n):
    return 18 if n <= TINY_TAIL_MAX else 4


def _seed(n, pattern):
    return MEMBER_SEED.get((n, pattern), 1000 * n + sum(map(ord, pattern)))


def cloud(rng, n, sig=(0.5, 0.5, 0.4)):
    """a tracking cloud about the origin of the Spielberg map (conftest.tracking_cloud)"""
    p = np.empty((3, n))
    p[0] = rng.normal(0, sig[0], n)
    p[1] = rng.normal(0, sig[1], n)
    p[2] = (rng.normal(0, sig[2], n) + np.pi) % (2 * np.pi) - np.pi
    return p


def pattern_weights(rng, n, pattern):
    w = np.zeros(n)
    if pattern == "flat":
        w[:] = 1.0 / n
    elif pattern == "first":
        w[0] = 1.0
    elif pattern == "last":
        w[n - 1] = 1.0
    elif pattern == "ends":
        w[0] = w[n - 1] = 0.5 if n > 1 else 1.0
    else:
        k = alive(n, pattern)
        at = np.sort(rng.choice(n, k, replace=False))
        w[at] = 0.25 + 0.75 * rng.random(k)
        w /= w.sum()
    return w


_START = {}


def start(n, pattern):
    key = (n, pattern)
    if key not in _START:
        rng = np.random.default_rng(_seed(n, pattern))
        p, w = cloud(rng, n), pattern_weights(rng, n, pattern)
        p.setflags(write=False)
        w.setflags(write=False)
        _START[key] = (p, w)
    return _START[key]


# ---- device groups: G shards of `per` particles each on one device
GROUPS = ((2, 1), (3, 1), (2, 65), (3, 1025), (4, 2049), (3, 4099))
# kind: the number of non-zero weights per shard, as a function of (G, per); clipped to per.  None: every particle of the shard.
#   "edges"   shard 0: its last particle only; the last shard: its first only; shards between: none (an empty list, a plateau in
#             the merged CDF); r * n_per_rank + local at local = per - 1 and local = 0
#   "w64_65"  shard 0: exactly 64; shard 1: 65, the longest (chunks of centries = 128 entries: shard 0's padded with a plateau of
#             64, gtop's second entry of chunk 0 inside the plateau); later shards: none and 1
#   "flat"    every particle: lists as long as the shards, none at 4099 (compact_cap 4096)
GROUP_KINDS = ("edges", "w64_65", "flat")


def group_alive(G, per, kind):
    """non-zero weights per shard"""
    if kind == "flat":
        return [per] * G
    if kind == "edges":
        return [1] + [0] * (G - 2) + [1]
    ks = [64, 65, 0, 1][:G]
    return [min(k, per) for k in ks]


def group_start(G, per, kind):
    """(particles (3, G * per), weights): shard s holds particles s * per .. (s + 1) * per - 1"""
    n = G * per
    rng = np.random.default_rng(7000 * G + per + sum(map(ord, kind)))
    p, w = cloud(rng, n), np.zeros(n)
    if kind == "flat":
        w[:] = 1.0 / n
    elif kind == "edges":
        w[per - 1] = 0.75                      # with per == 1 shard 0's last particle is its first
        w[(G - 1) * per] = 1.0
    else:
        for s, k in enumerate(group_alive(G, per, kind)):
            at = s * per + np.sort(rng.choice(per, k, replace=False))
            w[at] = 0.25 + 0.75 * rng.random(k)
    w /= w.sum()
    return p, w


def centries(longest):
    """mcl_group.hip / sharded.py: the chunk of the list exchange holds max(64, ceil64(longest list)) entries"""
    return max(64, ((int(longest) + 63) // 64) * 64)
