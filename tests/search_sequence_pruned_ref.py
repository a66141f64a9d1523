"""What the tests of the pruned search over a scan sequence share: the fold of PS3 / SQ4 in numpy.  A plain helper
module (like search_pruned_ref.py): no engine and no device.  tests/test_search_sequence_pruned_host.py checks it,
tests/test_gpu_search_sequence_pruned.py holds the device's bounds to it."""
import numpy as np


def fold(terms):
    """((+0.0 + t_0) + t_1) + ... in the order given, in fp64, one rounded add per term; the terms are left as they are"""
    total = np.zeros_like(np.asarray(terms[0], np.float64))
    for t in terms:
        total = total + np.asarray(t, np.float64)
    return total


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
