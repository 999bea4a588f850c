"""Rank process of the data-parallel clipping test (started by
tests/test_gpu_clip_ema.py, never collected by pytest): `world` ranks share
the visible GPU over gloo, every rank runs the real model on its shard of one
global batch -- net.loss -> optimizer.minimize with an active clip_norm and
EMA weights -- and saves ITS OWN parameters, shadow and per-step norms, so
that the test can compare the ranks bit for bit."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from util import MID, cfg_with, build_pair  # noqa: E402


def batch(spec):
    """The global batch of every step: [steps, B, T] float32."""
    return np.random.default_rng(23).uniform(
        -1, 1, (spec['steps'], spec['B'], spec['T'])).astype(np.float32)


def main():
    spec = json.loads(sys.argv[1])
    from wavenet import parallel, optimizer_factory
    rank, world, local = parallel.init_from_env()
    torch.cuda.set_device(local % torch.cuda.device_count())
    cfg = cfg_with(MID, batch_size=spec['B'] // world)
    net, _ = build_pair(cfg)
    parallel.broadcast_parameters(net)
    opt = optimizer_factory[spec['opt']](
        learning_rate=spec['lr'], momentum=0.9, clip_norm=spec['clip_norm'],
        ema_decay=spec['ema_decay'])
    audio = batch(spec)
    lo, hi = parallel.shard_range(spec['B'], rank, world)
    norms = []
    for s in range(spec['steps']):
        opt.minimize(net.loss(audio[s, lo:hi]))
        norms.append(float(opt.last_grad_norm))
    torch.cuda.synchronize()
    np.savez(spec['out'] % rank, params=net.params.cpu().numpy(),
             shadow=opt._shadow.cpu().numpy(), norms=np.asarray(norms))
    if parallel.is_distributed():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
