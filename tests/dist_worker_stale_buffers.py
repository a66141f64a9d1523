"""tests/dist_worker.py with every fresh float64 buffer of torch.empty holding 1e18 instead of whatever the heap held: what a
rank hands its peers without having written it is then the same in every run (tests/test_dist_failed_rank_reply.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

_empty = torch.empty


def _stale(*args, **kw):
    t = _empty(*args, **kw)
    if t.dtype == torch.float64:
        t.fill_(1e18)
    return t


torch.empty = _stale

import dist_worker  # noqa: E402

if __name__ == "__main__":
    dist_worker.main()
