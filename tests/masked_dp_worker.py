"""Rank function of the masked-loss data-parallel host test (spawned by
tests/test_masked_loss_host.py over gloo, never collected by pytest): every
rank holds its shard of one padded batch with lengths of its own, asks
parallel.masked_denominator for the common denominator, computes the float64
masked reference (tests/masked_ref.py) with it and averages the gradients
over the ranks as the optimizer does."""
import os
import sys

import numpy as np
import torch


def batch(world):
    """The global padded batch: (dilations, Q, codes [2 * world, T], lengths)."""
    B, T, Q = 2 * world, 23, 16
    rng = np.random.default_rng(11)
    codes = rng.integers(0, Q, (B, T)).astype(np.int32)
    lengths = np.array([T, 9, 1, 17, 2, T, 5, 20][:B])
    return [1, 2, 4, 1, 2], Q, codes, lengths


def variables(Q):
    from wavenet import WaveNetModel
    import lc_ref
    net = WaveNetModel(2, [1, 2, 4, 1, 2], 2, 8, 8, 16,
                       quantization_channels=Q, use_biases=True, device='cpu',
                       seed=3)
    return lc_ref.model_tree(net)


def worker(rank, world, port, out_dir):
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    import util  # noqa: F401  (repository root and package on sys.path)
    import lc_ref
    import masked_ref
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from wavenet import parallel
    parallel.init_from_env(backend='gloo')
    dil, Q, codes, lengths = batch(world)
    lo, hi = parallel.shard_range(codes.shape[0], rank, world)
    den = parallel.masked_denominator(lengths[lo:hi])
    loss, g = masked_ref.loss_and_grads(
        variables(Q), dil, codes[lo:hi], lengths[lo:hi], use_biases=True,
        quantization_channels=Q, denominator=den)
    flat = torch.from_numpy(np.concatenate(
        [a.reshape(-1) for _, a in lc_ref.flatten(g)]))

    class Bucket(object):
        grads = flat
    scale = parallel.allreduce_gradients(Bucket)
    mloss = parallel.allreduce_mean_scalar(torch.tensor(loss,
                                                        dtype=torch.float64))
    np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), den=den,
             grads=(Bucket.grads * scale).numpy(), loss=mloss.numpy())
    torch.distributed.destroy_process_group()
