"""The guide of the compact parent list on the device (csrc/mcl_compact_guide.h; k_scan_final writes it, the multinomial draw of
k_resample_motion searches through it), at 16 384 particles -- above the 8192 of the one-workgroup tail, eight scan tiles -- and
61 beams on the Spielberg fixture.  mcl_set_particles gets weights that leave 1, 63, 64, 65 and about 600 weighted particles
(owner ranges, the ragged last group of 64, entries in several tiles) and a set in which one particle holds nearly everything
(one entry owns nearly every word: the wave's cooperative fill):

  * the guide read back equals the host twin's, word for word, and the list's CDF column is the cumulative sum of the weighted
    particles' fixed-point weights;
  * one update's resample_indices() equal the oracle's for the same Philox k53, for every child -- through the guide by default,
    and through ctop with MCL_RESAMPLE_GUIDE=0, with systematic resampling and with KLD sampling on (the first two keep no
    guide at all, and with KLD on the scans stop writing it);
  * an engine with resample_neff_permille keeps some updates: a kept update searches nothing, the scan behind it rewrites list
    and guide for the multiplied weights, and the resampling update after it draws the oracle's parents through that guide."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_engine, tracking_cloud

pytestmark = pytest.mark.gpu
N, STEP, SEED = 16384, 18, 23
M = 17                              # log2 of the guide's buckets (csrc/mcl_compact_guide.h: kGuideLog2Default)
ACTION = (0.05, 0.0, 0.01)
CASES = {"1": 1, "63": 63, "64": 64, "65": 65, "600": 601, "heavy": 601}


def scan61():
    return np.load(os.path.join(GOLDEN, "scan_Spielberg_map_origin.npz"))["ranges"][::STEP].astype(np.float32)


_sets = {}


def weighted_set(orc, case):
    """(particles, weights, fixed-point weights) of a case, made once: k particles spread over the eight scan tiles carry weight"""
    if case not in _sets:
        rng = np.random.default_rng(100 + len(case) + CASES[case])
        k = CASES[case]
        p = tracking_cloud(rng, N)
        w = np.zeros(N)
        alive = np.sort(rng.choice(N, k, replace=False))
        w[alive] = rng.uniform(0.2, 1.0, k)
        if case == "heavy":                          # one particle with nearly everything, the others a few hundred units each
            w[alive] = rng.uniform(2e-9, 8e-9, k)
            w[alive[k // 3]] = 1.0
        q = orc.eng_quantize_weights(w)
        assert np.count_nonzero(q) == k
        _sets[case] = p, w, q
    return _sets[case]


def engine_for(engine_mod, m, ang, monkeypatch, guide_env=None, cap=N, **cfg):
    monkeypatch.delenv("MCL_RESAMPLE_GUIDE", raising=False)
    monkeypatch.delenv("MCL_RESAMPLE_GUIDE_M", raising=False)
    if guide_env is not None:
        monkeypatch.setenv("MCL_RESAMPLE_GUIDE", guide_env)
    return make_engine(engine_mod, m, ang, cap, seed=SEED, **cfg)


def check_guide(engine_mod, e, q):
    """the device's list and guide for the fixed-point weights q: the CDF column, and the host twin's table word for word"""
    g = e.compact_guide()
    alive = q[q != 0]
    assert g["n_compact"] == alive.size and g["q_total"] == int(alive.sum(dtype=np.uint64))
    assert np.array_equal(g["ccdf"], np.cumsum(alive, dtype=np.uint64))
    assert g["m"] == M
    want, s, bmax, written = engine_mod.host_compact_guide(g["ccdf"], g["m"])
    assert (g["s"], g["bmax"]) == (s, bmax) and written == bmax + 1
    assert g["guide"].size == bmax + 1 and np.array_equal(g["guide"], want[: bmax + 1])
    return g


@pytest.mark.parametrize("case", list(CASES))
def test_guide_is_the_host_twins_and_the_draw_is_the_oracles(orc, engine_mod, spielberg, monkeypatch, case):
    ang = orc.beam_angles(angle_step=STEP)
    p, w, q = weighted_set(orc, case)
    e = engine_for(engine_mod, spielberg, ang, monkeypatch)
    e.set_particles(p, w)
    assert e.compact_list()[0] == CASES[case]
    g = check_guide(engine_mod, e, q)
    if case == "heavy":                              # one entry owns nearly all of the table
        assert np.bincount(g["guide"]).max() > g["bmax"] - 8
    e.update(ACTION, scan61())
    assert e.compact_list()[1] and e.compact_guide_used()
    want = orc.eng_resample_indices(q, 0, n_children=N, k53=orc.eng_philox_k53(SEED, 0, 0, N))
    got = e.resample_indices()
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} of {N} parents differ"
    assert (q[got] != 0).all()
    e.close()


@pytest.mark.parametrize("setting", ["guide-off", "systematic", "kld"])
@pytest.mark.parametrize("case", ["65", "600", "heavy"])
def test_other_draws_keep_the_ctop_search(orc, engine_mod, spielberg, monkeypatch, case, setting):
    ang = orc.beam_angles(angle_step=STEP)
    p, w, q = weighted_set(orc, case)
    mode = 1 if setting == "systematic" else 0
    e = engine_for(engine_mod, spielberg, ang, monkeypatch, guide_env="0" if setting == "guide-off" else None, resample_mode=mode)
    e.set_particles(p, w)
    if setting == "kld":
        e.set_kld(min_particles=256, max_particles=N)
        assert e.kld_state() == (-1, N)
    assert e.compact_list()[0] == CASES[case]
    if setting == "kld":
        check_guide(engine_mod, e, q)                # (written by mcl_set_particles' scan, before KLD sizing went on; not drawn through)
    else:
        with pytest.raises(engine_mod.EngineError):  # no guide is kept for an engine that cannot draw through one
            e.compact_guide()
    e.update(ACTION, scan61())
    assert e.compact_list()[1] and not e.compact_guide_used()
    if mode == 0:
        want = orc.eng_resample_indices(q, 0, n_children=N, k53=orc.eng_philox_k53(SEED, 0, 0, N))
    else:
        want = orc.eng_resample_indices(q, 1, n_children=N, k0=orc.eng_philox_k0(SEED, 0))
    assert np.array_equal(e.resample_indices(), want)
    e.close()


def test_kept_update_leaves_no_stale_guide(orc, engine_mod, spielberg, monkeypatch):
    """resample_neff_permille = 20 on a tight cloud (tests/test_gpu_parity.py's adaptive case at this size; one update of 61 beams
    leaves N_eff at 0.036 N, a second on the same set well below 0.02 N): kept and resampling updates alternate.  Room for
    65 536 particles, so that the list of a set of 16 384 always fits (room / 4) and every resampling update draws from a list.  After EVERY update the guide is the host twin's for the list that update's scan wrote; a kept
    update reports every particle as its own parent and uses neither list nor guide; a resampling update -- the ones after a kept
    update among them -- draws the oracle's parents from the weights the kept updates multiplied up."""
    ang = orc.beam_angles(angle_step=STEP)
    e = engine_for(engine_mod, spielberg, ang, monkeypatch, cap=4 * N, resample_neff_permille=20)
    p = tracking_cloud(np.random.default_rng(4), N, sig=(0.03, 0.03, 0.01))
    e.set_particles(p, np.full(N, 1.0 / N))
    q = orc.eng_quantize_weights(np.full(N, 1.0 / N))
    check_guide(engine_mod, e, q)
    kept = []
    for upd in range(7):
        n_list = e.compact_list()[0]
        e.update(ACTION, scan61())
        neff, resampled = e.effective_sample_size()
        print(f"update {upd}: list {n_list}, resampled {bool(resampled)}, N_eff / N after it {neff / N:.4f}")
        idx = e.resample_indices()
        if resampled:
            assert n_list > 0 and e.compact_list()[1] and e.compact_guide_used(), upd
            want = orc.eng_resample_indices(q, 0, n_children=N, k53=orc.eng_philox_k53(SEED, upd, 0, N))
            assert np.array_equal(idx, want), (upd, kept)
        else:
            assert np.array_equal(idx, np.arange(N)) and not e.compact_guide_used(), upd
        lw = e.log_weights()                         # (a kept update's: this scan's plus what the particle carried)
        _, q, _ = orc.eng_weights_from_log(lw)
        check_guide(engine_mod, e, q)
        kept.append(not resampled)
    print("kept:", kept)
    assert any(a and not b for a, b in zip(kept, kept[1:])), kept       # a resampling update right after a kept one
