"""Rank process of the data-parallel context test (started by
tests/test_gpu_lc_context.py, never collected by pytest): every rank trains
the same local-conditioning model with the upsampler and the frame-context
convolution on its shard of
one batch of frames and offsets, and saves its own parameters."""
import json
import sys
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import MID, cfg_with, model_kwargs  # noqa: E402


def main():
    spec = json.loads(sys.argv[1])
    from wavenet import WaveNetModel, parallel, optimizer_factory
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local % torch.cuda.device_count())
    B, T, steps, Lc = spec['B'], spec['T'], spec['steps'], spec['lc']
    scales = tuple(spec['scales'])
    hop = int(np.prod(scales))
    cfg = cfg_with(MID, batch_size=B // world, use_biases=True)
    net = WaveNetModel(seed=5, local_condition_channels=Lc,
                       local_condition_upsample_scales=scales,
                       local_condition_context=spec['p'],
                       **model_kwargs(cfg))
    rng = np.random.default_rng(17)
    audio = rng.uniform(-1, 1, (steps, B, T)).astype(np.float32)
    F = (T + 3 * hop) // hop + 1
    frames = rng.standard_normal((steps, B, F, Lc)).astype(np.float32)
    offs = rng.integers(0, 2 * hop, (steps, B))
    parallel.broadcast_parameters(net)
    opt = optimizer_factory['adam'](learning_rate=spec['lr'], momentum=0.9)
    lo, hi = parallel.shard_range(B, rank, world)
    net.dp_overlap_allreduce = bool(spec.get('overlap', False))
    for s in range(steps):
        loss = net.loss(audio[s, lo:hi], local_condition_batch=frames[s, lo:hi],
                        local_condition_offset=offs[s, lo:hi])
        opt.minimize(loss)
    torch.cuda.synchronize()
    np.savez(spec['out'] % rank, params=net.params.cpu().numpy(),
             lc_ctx=net._seg(net.params, 'lc_ctx').cpu().numpy())
    if parallel.is_distributed():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
