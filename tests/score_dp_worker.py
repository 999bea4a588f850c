"""Rank function of the sum_over_ranks host test (spawned by
tests/test_score_host.py over gloo, never collected by pytest): every rank
holds totals of its own and asks wavenet.evaluate.sum_over_ranks for the
sum."""
import os
import sys

import numpy as np
import torch


def totals(rank):
    return np.array([1.5 + rank, 10.0 * (rank + 1), 3.0 * rank, 2.0 + rank])


def worker(rank, world, port, out_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import util  # noqa: F401  (repository root and package on sys.path)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from wavenet import parallel
    from wavenet import evaluate as ev
    parallel.init_from_env(backend='gloo')
    mine = torch.from_numpy(totals(rank))
    got = ev.sum_over_ranks(mine, 'cpu')
    assert torch.equal(mine, torch.from_numpy(totals(rank)))   # not in place
    np.save(os.path.join(out_dir, 'sum%d.npy' % rank), got.numpy())
    torch.distributed.destroy_process_group()
