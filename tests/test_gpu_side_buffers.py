"""The buffers the pose query, the global search and the refinement keep between calls (csrc/mcl_side_buffers.h): an engine that
has grown, shrunk and grown them again, across the three features, across a change of map and across a refused call, answers
every call with the bytes of a fresh engine that made no other call; the byte counters never fall and stand still once the sizes
have been seen; a second engine in the same process, after the first was closed, repeats the first."""
import types

import numpy as np
import pytest

from test_gpu_search_streamed import TRUE_POSE, SmallMap, angles, expect, lf_engine, odd_scan, scan_at, compose

pytestmark = pytest.mark.gpu

B = 61
REL = np.array([[-0.5, 0.0, 0.1], [-0.25, 0.05, -0.05], [0.0, 0.0, 0.0]])


def poses(K):
    rng = np.random.default_rng(K)
    return np.asarray(TRUE_POSE) + rng.normal(0.0, (0.1, 0.1, 0.2), (K, 3))


def stats_bytes(st):
    return repr(sorted((k, v) for k, v in st.items() if k != "device_bytes")).encode()


def query(K):
    def call(e, w):
        ranges, steps = e.expected_scans(poses(K), want_steps=True)
        return ranges.tobytes() + steps.tobytes()
    return call


def score(K):
    return lambda e, w: e.score_poses(poses(K), w.obs).tobytes()


def search(stride, n_head):
    def call(e, w):
        hits, st = e.global_search(w.obs, max_hits=32, stride_cells=stride, n_headings=n_head)
        assert len(hits) > 0
        return hits.tobytes() + stats_bytes(st) + e.search_scores().tobytes()
    return call


def sequence(S):
    def call(e, w):
        hits, st = e.global_search_sequence(w.scans[3 - S:], REL[3 - S:], max_hits=32, stride_cells=3, n_headings=4)
        assert len(hits) > 0 and st["n_scans"] == S
        return hits.tobytes() + stats_bytes(st) + e.search_scores().tobytes()
    return call


def streamed(G, **kw):
    def call(e, w):
        hits, st = e.global_search_streamed(w.obs, max_hits=32, slab_headings=G, stride_cells=3, n_headings=4, **kw)
        assert len(hits) > 0 and st["slab_headings"] == (G or 4)
        return hits.tobytes() + stats_bytes(st)
    return call


def refine(M):
    def call(e, w):
        r, st = e.refine_poses(poses(M), w.obs, half_xy=2, half_theta=3)
        return r.tobytes() + stats_bytes(st) + e.refine_scores().tobytes()
    return call


# the sizes of every feature grow, shrink and grow again, the features interleaved
CALLS = [("query 1", query(1)), ("search 3x3", search(3, 3)), ("refine 1", refine(1)), ("score 2", score(2)), ("query 300", query(300)),
         ("search 2x8", search(2, 8)), ("sequence 2", sequence(2)), ("refine 7", refine(7)), ("streamed G=1", streamed(1)),
         ("score 300", score(300)), ("query 2", query(2)), ("search 3x4", search(3, 4)), ("sequence 3", sequence(3)),
         ("streamed G=0", streamed(0)), ("refine 2", refine(2))]


def counters(e):
    return (e.query_counters()["device_bytes"], e.search_bytes(), e.refine_bytes())


@pytest.fixture(scope="module")
def world(orc):
    m = SmallMap()
    om = orc.OracleMap(m.data, m.resolution, m.origin_x, m.origin_y)
    ang = angles(orc, B)
    scans = np.stack([scan_at(orc, om, ang, compose(TRUE_POSE, r)) for r in REL])
    scans[2] = odd_scan(scans[2])
    cropped = types.SimpleNamespace(data=np.ascontiguousarray(m.data[:80, :100]), resolution=m.resolution, origin_x=m.origin_x,
                                    origin_y=m.origin_y)
    return types.SimpleNamespace(map=m, cropped=cropped, ang=ang, scans=scans, obs=scans[2])


@pytest.fixture(scope="module")
def fresh(engine_mod, world):
    """the bytes of a call on an engine that makes no other call (made once per call and map)"""
    seen = {}

    def get(name, call, m=None):
        key = (name, m is not None)
        if key not in seen:
            e = lf_engine(engine_mod, m or world.map, world.ang)
            seen[key] = call(e, world)
            e.close()
        return seen[key]
    return get


def test_grown_shrunk_and_grown_again_across_the_features(engine_mod, world, fresh):
    e = lf_engine(engine_mod, world.map, world.ang)
    assert counters(e) == (0, 0, 0)
    grew = set()
    for rnd in range(2):
        for name, call in CALLS:
            before = counters(e)
            assert call(e, world) == fresh(name, call), (rnd, name)
            after = counters(e)
            assert all(a >= b for a, b in zip(after, before)), (rnd, name, before, after)
            which = {"query": 0, "score": 0, "search": 1, "sequence": 1, "streamed": 1, "refine": 2}[name.split()[0]]
            assert all(a == b for i, (a, b) in enumerate(zip(after, before)) if i != which), (rnd, name, before, after)
            if after != before:
                grew.add(name)
            # the second round repeats sizes already seen: nothing is asked of the device again
            assert rnd == 0 or after == before, (name, before, after)
    # (the sequence does grow what it is meant to grow, and a smaller size after a larger one grows nothing)
    assert {"query 1", "query 300", "score 2", "score 300", "search 3x3", "search 2x8", "sequence 2", "sequence 3", "streamed G=1",
            "streamed G=0", "refine 1", "refine 7"} <= grew
    assert not grew & {"query 2", "search 3x4", "refine 2"}
    e.close()


def test_a_map_change_between_calls(engine_mod, world, fresh):
    NOT_READY = engine_mod.MCL_ERR_NOT_READY
    e = lf_engine(engine_mod, world.map, world.ang)
    for name, call in (("search 3x4", search(3, 4)), ("streamed G=1", streamed(1)), ("refine 7", refine(7))):
        assert call(e, world) == fresh(name, call)
    search(3, 4)(e, world)                                                # (a volume is kept: the streamed search dropped it)
    held = counters(e)
    c = world.cropped
    e.set_map(c.data, c.resolution, c.origin_x, c.origin_y)
    assert "no score volume" in expect(engine_mod, NOT_READY, e.search_scores)
    assert "no score volume" in expect(engine_mod, NOT_READY, e.refine_scores)
    for name, call in (("search 3x4", search(3, 4)), ("streamed G=1", streamed(1)), ("refine 7", refine(7))):
        got = call(e, world)
        assert got == fresh(name, call, c), name
        assert name == "refine 7" or got != fresh(name, call), name       # (the two lattices are not the same)
    assert counters(e) == held                                            # the smaller map fits what the larger one left
    e.close()


def test_a_refused_call_in_the_middle(engine_mod, world, fresh):
    INVALID = engine_mod.MCL_ERR_INVALID_ARG
    e = lf_engine(engine_mod, world.map, world.ang)
    kept = {name: call(e, world) for name, call in (("query 300", query(300)), ("search 3x4", search(3, 4)), ("refine 7", refine(7)))}
    held = counters(e)
    n_pos = engine_mod.host_search_lattice(world.map.data, world.map.resolution, world.map.origin_x, world.map.origin_y, stride_cells=3)[0].size
    need = engine_mod.host_search_slabs(n_pos, stride_cells=3, n_headings=4, slab_headings=1)[2]
    short = streamed(0, budget_bytes=need - 1)
    msg = expect(engine_mod, INVALID, short, e, world)
    assert str(need) in msg
    assert counters(e) == held
    assert kept["search 3x4"].endswith(e.search_scores().tobytes()) and e.search_scores().size == 4 * n_pos
    assert kept["refine 7"].endswith(e.refine_scores().tobytes())
    hits, st = e.global_search_streamed(world.obs, max_hits=32, stride_cells=3, n_headings=4, budget_bytes=need)
    assert st["slab_headings"] == 1 and e.search_bytes() == held[1] + need
    assert hits.tobytes() + stats_bytes(st) == fresh("streamed G=1", streamed(1))
    for name, call in (("query 300", query(300)), ("search 3x4", search(3, 4)), ("refine 7", refine(7))):
        assert call(e, world) == kept[name] == fresh(name, call)
    e.close()


def test_create_use_close_twice_in_one_process(engine_mod, world):
    rounds = []
    for _ in range(2):
        e = lf_engine(engine_mod, world.map, world.ang)
        out = [call(e, world) for _, call in CALLS]
        rounds.append((out, counters(e)))
        e.close()
    assert rounds[0] == rounds[1]
    assert all(v > 0 for v in rounds[0][1])
