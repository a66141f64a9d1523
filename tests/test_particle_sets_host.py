"""The host half of the particle-set family of tests/particle_sets.py, without a device: that the family is what its docstring
says, that every member's start set has exactly the intended number of non-zero fixed-point weights, and -- by driving the
stand-in OracleEngine of tests/test_whole_set_checks.py through whole_set.WholeSet -- the conditions
tests/test_gpu_particle_sets.py rests on: every update of every member resamples, none is all-zero, the list-length helper agrees
with the oracle's weights, and with 271 beams the lists inside the chain are short and ragged.  A change of fixture or oracle
shows up here first."""
import numpy as np
import pytest

import particle_sets as ps
import whole_set as ws
from conftest import GOLDEN
from test_whole_set_checks import OracleEngine

SEED = 0x5EED_0000_0000_0062
UPDATES = 3


def scan_of(step):
    import os
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::step].astype(np.float32).copy()


def sample_ks(n):
    """sample_particles draws per update: more than n, one, more than n (at most 4096)"""
    return (min(ws.SAMPLE_K, 3 * n + 1), 1, min(ws.SAMPLE_K, 3 * n + 1))


def test_the_family_is_what_the_docstring_says():
    assert ps.COUNTS == (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 8191, 8193, 12297, 16385)
    assert (ps.WAVE, ps.LEADER_GROUP, ps.TAIL_THREADS, ps.SCAN_TILE, ps.TINY_TAIL_MAX) == (64, 16, 1024, 2048, 8192) and ps.TINY_TAIL_MAX == ws.TINY_TAIL_MAX
    assert all(n <= ps.TINY_TAIL_MAX for n in ps.SMALL) and all(n > ps.TINY_TAIL_MAX for n in ps.LARGE)
    assert 12297 == 3 * 4099
    # the ragged last leader group: every count but 64, 256 and 1024
    assert [n for n in ps.COUNTS if (n - 1) & 15 == 15] == [64, 256, 1024]
    assert [(n - 1) & 15 for n in ps.LARGE] == [0, 8, 0]
    # k_tiny_tail's entries per thread and the threads that own something
    per = {n: -(-n // ps.TAIL_THREADS) for n in ps.SMALL}
    assert (per[1023], per[1024], per[1025], per[2047], per[2049], per[8191]) == (1, 1, 2, 2, 3, 8)
    assert -(-1025 // per[1025]) == 513 and -(-2049 // per[2049]) == 683             # threads with work, of 1024
    assert [-(-n // ps.SCAN_TILE) for n in (2047, 2049, 8193, 16385)] == [1, 2, 5, 9]
    assert ps.patterns(1) == ps.BASE + ("alive1",) and ps.patterns(63) == ps.BASE + ("alive63",)
    assert ps.patterns(64) == ps.BASE + ("alive63", "alive64") and ps.patterns(65) == ps.BASE + ("alive63", "alive64", "alive65")
    assert ps.patterns(16385)[-3:] == ("alive4095", "alive4096", "alive4097") and "alive4096" not in ps.patterns(12297)
    m = ps.members()
    assert len(m) == len(set(m)) == 120 and m[0] == (1, "flat") and m[-1] == (16385, "alive4097")
    assert [ps.beams_step(n) for n in (1, 8191, 8192, 8193, 16385)] == [18, 18, 18, 4, 4]


def test_the_cap_rule():
    """compact_cap = max(4096, ceil64(cap / 4)) and the length mcl_get_compact_list reports"""
    assert [ps.compact_cap(c) for c in (1, 4099, 16384, 16385, 16387, 16388, 16640, 16641, 65536, 4194304)] == \
        [4096, 4096, 4096, 4096, 4096, 4160, 4160, 4160, 16384, 1048576]
    assert [ps.list_length(k, 16385) for k in (0, 1, 4095, 4096, 4097, 16385)] == [0, 1, 4095, 4096, -1, -1]
    assert ps.list_length(4099, 4099) == -1 and ps.list_length(2049, 2049) == 2049
    assert [ps.centries(k) for k in (-1, 0, 1, 64, 65, 128, 129)] == [64, 64, 64, 64, 128, 128, 192]


@pytest.mark.parametrize("member", ps.members(), ids=ps.member_id)
def test_start_sets(orc, member):
    n, pattern = member
    p, w = ps.start(n, pattern)
    assert p.shape == (3, n) and w.shape == (n,) and not p.flags.writeable and not w.flags.writeable
    assert np.isfinite(p).all() and (w >= 0.0).all() and abs(w.sum() - 1.0) < 1e-12
    q = orc.eng_quantize_weights(w)
    k = ps.alive(n, pattern)
    assert np.count_nonzero(q) == np.count_nonzero(w) == k                         # exactly the intended non-zero fixed-point weights
    if pattern == "first":
        assert np.flatnonzero(q).tolist() == [0]
    if pattern == "last":
        assert np.flatnonzero(q).tolist() == [n - 1]
    if pattern == "ends":
        assert np.flatnonzero(q).tolist() == sorted({0, n - 1})
    if pattern.startswith("alive") and k < n:
        assert len(set(q[q > 0].tolist())) > 1                                     # unequal weights
    assert ps.list_length(k, n) == (k if k <= max(4096, ((n // 4 + 63) // 64) * 64) else -1)
    assert (ps.list_length(k, n) == -1) == (member == (16385, "alive4097") or (n > 4096 and k == n))
    again = np.random.default_rng(ps._seed(n, pattern))
    assert np.array_equal(ps.cloud(again, n), p) and np.array_equal(ps.pattern_weights(again, n, pattern), w)


def run_chain(orc, om, member, plant=None):
    """three updates of the stand-in through the checker: the checker, and the alive count after each update"""
    n, pattern = member
    step = ps.beams_step(n)
    ang, scan = orc.beam_angles(angle_step=step), scan_of(step)
    p0, w0 = ps.start(n, pattern)
    e = OracleEngine(orc, om, ang, p0, w0, seed=SEED)
    c = ws.WholeSet(orc, om, e, ang, SEED, p0, orc.eng_quantize_weights(w0), q_device=None, rng=np.random.default_rng(n))
    alive = []
    for u, k in enumerate(sample_ks(n)):
        if plant is not None and u == UPDATES - 1:
            e.plant[plant[0]] = plant[1]
        c.sample_k = k
        c.step(scan)
        alive.append(int(np.count_nonzero(c.q)))
    return c, alive


@pytest.mark.parametrize("member", ps.members(), ids=ps.member_id)
def test_chain_on_the_stand_in(orc, spielberg_oracle, member):
    n, pattern = member
    c, alive = run_chain(orc, spielberg_oracle, member)
    print(f"{ps.member_id(member)}: alive after each update {alive}, lists {[ps.list_length(k, n) for k in alive]}")
    assert [r["update"] for r in c.log] == [0, 1, 2]
    assert all(r["q_total"] > 0 for r in c.log) and all(k >= 1 for k in alive)     # no update is all-zero
    for k in alive:
        assert ps.list_length(k, n) == (k if k <= ps.compact_cap(n) else -1)
    if n > ps.TINY_TAIL_MAX:
        # 271 beams: the lists the captured tail leaves are usable and ragged (a ctop group and a tail)
        assert all(k <= ps.compact_cap(n) and k % ps.WAVE != 0 for k in alive), alive
    else:
        assert alive[-1] > n // 2                                                  # 61 beams: nearly every particle stays alive


@pytest.mark.parametrize("member,what", [((65, "last"), "logw"), ((1025, "alive65"), "q"), ((8193, "ends"), "indices"), ((1, "flat"), "logw")],
                         ids=lambda v: v if isinstance(v, str) else ps.member_id(v))
def test_a_wrong_last_entry_is_named(orc, spielberg_oracle, member, what):
    """one wrong value at the LAST particle of a ragged member, planted in the stand-in's output: the checker names that entry"""
    n = member[0]

    def f(a):
        if what == "logw":
            a[n - 1] = np.nextafter(a[n - 1], np.inf)
        elif what == "q":
            a[n - 1] += np.uint64(1)
        else:
            a[n - 1] = (a[n - 1] + 1) % n
        return a
    name = {"logw": "log-weights", "q": "fixed-point weights", "indices": "resample indices"}[what]
    with pytest.raises(AssertionError, match=rf"update 2: {name}: 1 of {n} differ; first at \[{n - 1}\]"):
        run_chain(orc, spielberg_oracle, member, plant=(what, f))
