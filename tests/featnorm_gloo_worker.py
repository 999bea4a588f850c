"""Rank function of the feature-statistics all-reduce test (spawned by
tests/test_featnorm_host.py, never collected by pytest): `world` gloo ranks on
the CPU, each with the sums of its own shard of frames, push them through
wavenet.parallel.sum_float64_over_ranks -- the callable train.py hands to
DeviceCorpus as stats_allreduce -- and save what they got."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def shard_frames(rank, world, C=5):
    """Rank `rank`'s frames [F_r, C] float32: different lengths and scales."""
    rng = np.random.default_rng(100 + rank)
    return (rng.standard_normal((37 + 11 * rank, C)) * (3 + rank) - 10) \
        .astype(np.float32)


def worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, 'tensorflow-wavenet_amd'), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import featnorm_ref
    from wavenet import features, parallel
    r, w, _ = parallel.init_from_env(backend='gloo')
    assert (r, w) == (rank, world) and parallel.is_distributed()
    fr = shard_frames(rank, world)
    n, s1, s2 = featnorm_ref.sums(fr[None])[:3]
    mine = features.FeatureStats.from_sums(n, s1, s2)
    total = features.FeatureStats.from_vector(
        parallel.sum_float64_over_ranks(mine.vector()))
    total.save(os.path.join(out_dir, 'rank%d.npz' % rank))
    torch.distributed.destroy_process_group()
