"""The plan of the streamed global search on the host (mcl_host_search_slabs; rules ST2 / ST4 / ST5 of
include/mcl_hip_engine.h), without a device: the bytes against a restatement of ST5's formula, the largest G that fits a budget,
an explicit G, the number of slabs, the refusals."""
import pytest

from monte_carlo_localization_amd import engine as E

MIB = 1 << 20
LIMIT = 1 << 27


def bytes_ref(P, G):
    """ST5 restated"""
    L = 65536 + G * P
    return 8 * (G + 2) * P + 4 * G * P + 4 * G * P + 8 * G * P + 2 * 16 * L + 262144 + (G * P) // 16


def largest_g(P, n, budget):
    best = 0
    for G in range(1, n + 1):
        if bytes_ref(P, G) <= budget and (G + 2) * P < LIMIT:
            best = G
    return best


def refused(**kw):
    with pytest.raises(E.EngineError) as ei:
        E.host_search_slabs(**kw)
    assert ei.value.status == E.MCL_ERR_INVALID_ARG


@pytest.mark.parametrize("P,n,budget", [
    (2611, 72, 8 * MIB),              # a few headings per slab
    (2611, 72, 0),                    # the default budget, 1 GiB: every heading in one slab
    (990_211, 72, 0),                 # about Spielberg at stride 2: several slabs in 1 GiB
    (990_211, 360, 256 * MIB),
    (3_960_001, 72, 1 << 40),         # about Spielberg at stride 1, a budget without bounds: ST4 binds
    (9_533, 16384, 64 * MIB),
    (1, 1, 3 * MIB),
])
def test_the_largest_slab_that_fits(P, n, budget):
    G, slabs, b = E.host_search_slabs(P, n_headings=n, budget_bytes=budget)
    want = largest_g(P, n, budget or 1 << 30)
    assert want >= 1 and G == want
    assert b == bytes_ref(P, G) and b <= (budget or 1 << 30)
    assert (G + 2) * P < LIMIT
    assert slabs == -(-n // G)
    if P == 3_960_001:
        assert bytes_ref(P, G + 1) <= budget and (G + 3) * P >= LIMIT          # (it is ST4 that stopped G here)


def test_bytes_grow_with_g_and_an_explicit_g_is_honoured():
    P, n = 2611, 72
    last = 0
    for G in range(1, n + 1):
        got, slabs, b = E.host_search_slabs(P, n_headings=n, slab_headings=G)
        assert got == G and slabs == -(-n // G) and b == bytes_ref(P, G)
        assert b > last
        last = b
    # G above n_headings counts as n_headings: one slab
    assert E.host_search_slabs(P, n_headings=n, slab_headings=n + 1) == (n, 1, bytes_ref(P, n))
    assert E.host_search_slabs(P, n_headings=1, slab_headings=5) == (1, 1, bytes_ref(P, 1))
    # the scans do not change the plan; a lattice beyond 2^27 poses is planned
    assert E.host_search_slabs(P, n_scans=16, n_headings=n, slab_headings=7) == E.host_search_slabs(P, n_headings=n, slab_headings=7)
    G, slabs, b = E.host_search_slabs(9_533, n_headings=16384, budget_bytes=64 * MIB)
    assert 9_533 * 16384 >= LIMIT and slabs > 1 and b <= 64 * MIB


def test_refusals():
    P, n = 2611, 72
    refused(n_positions=P, n_headings=n, stream_reserved=(0, 0, 0, 0, 1))
    refused(n_positions=P, n_headings=n, stream_reserved=(1, 0, 0, 0, 0))
    refused(n_positions=P, n_headings=n, slab_headings=-1)
    # a budget too small for G = 1, by one byte; with that byte it fits
    refused(n_positions=P, n_headings=n, budget_bytes=bytes_ref(P, 1) - 1)
    assert E.host_search_slabs(P, n_headings=n, budget_bytes=bytes_ref(P, 1))[0] == 1
    # an explicit G that the budget does not hold
    refused(n_positions=P, n_headings=n, slab_headings=8, budget_bytes=bytes_ref(P, 8) - 1)
    # ST4: (G + 2) * n_positions >= 2^27, explicit and at G = 1
    P4 = 1 << 20
    assert E.host_search_slabs(P4, n_headings=200, slab_headings=125, budget_bytes=1 << 40)[0] == 125       # 127 * 2^20 < 2^27
    refused(n_positions=P4, n_headings=200, slab_headings=126, budget_bytes=1 << 40)                        # 128 * 2^20
    refused(n_positions=(LIMIT + 2) // 3, n_headings=4, budget_bytes=1 << 40)
    # 2^40 poses per call
    assert E.host_search_slabs(P4, n_headings=(1 << 20) - 1, budget_bytes=1 << 40)[0] == 125
    refused(n_positions=P4, n_headings=1 << 20, budget_bytes=1 << 40)
    # the search config's own refusals, the scans, the positions
    refused(n_positions=P, n_headings=0)
    refused(n_positions=P, reserved=(0, 0, 0, 1))
    refused(n_positions=P, n_scans=0)
    refused(n_positions=P, n_scans=17)
    refused(n_positions=0)
