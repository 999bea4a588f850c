"""Cost of global-norm clipping and EMA weights: the training step of the
default model (wavenet_params.json, batch 8 x 16000 samples) with the plain
Adam optimizer, with clip_norm alone, with ema_decay alone and with both --
one model, four optimizers, one process.

Each timed round runs `--steps` steps (loss + update) of one arm after
`--warmup` untimed ones of every arm, and the rounds go plain / clip / ema /
both / plain ... so that clock and thermal drift hit all arms alike.  The
clip threshold is far above any norm (the clip never acts: the launches and
their traffic are what is timed, the trajectory stays the plain one).  Prints
one JSON line: per-step medians over the rounds, each arm's difference from
the plain arm, and the spread of each arm's rounds (the noise the differences
have to be read against).  The plain arm makes exactly the calls the
optimizer made before the keywords existed.

    python tools/clip_step_time.py [--steps 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(params, B):
    from wavenet import WaveNetModel
    return WaveNetModel(
        batch_size=B, dilations=params['dilations'],
        filter_width=params['filter_width'],
        residual_channels=params['residual_channels'],
        dilation_channels=params['dilation_channels'],
        skip_channels=params['skip_channels'],
        quantization_channels=params['quantization_channels'],
        use_biases=params['use_biases'], scalar_input=params['scalar_input'],
        initial_filter_width=params['initial_filter_width'])


def timed(net, opt, audio, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        opt.minimize(net.loss(audio))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import optimizer_factory
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    B, T = a.batch, a.samples
    rng = np.random.default_rng(a.seed)
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T)).astype(
        np.float32)).cuda()
    net = build(params, B)
    arms = (('plain', {}), ('clip', dict(clip_norm=1e6)),
            ('ema', dict(ema_decay=0.9999)),
            ('both', dict(clip_norm=1e6, ema_decay=0.9999)))
    opts = {k: optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9,
                                         **kw) for k, kw in arms}
    for k, _ in arms:
        timed(net, opts[k], audio, a.warmup)
    ms = {k: [] for k, _ in arms}
    for _ in range(a.rounds):
        for k, _ in arms:
            ms[k].append(timed(net, opts[k], audio, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(config='wavenet_params.json', batch=B, samples=T,
               bucket_floats=int(net.params.numel()), steps=a.steps,
               rounds=a.rounds,
               grad_norm=float(opts['both'].last_grad_norm),
               device=torch.cuda.get_device_name(0))
    for k, _ in arms:
        out[k + '_ms'] = round(med[k], 3)
        out[k + '_rounds_ms'] = [round(v, 3) for v in ms[k]]
        out[k + '_spread_ms'] = round(max(ms[k]) - min(ms[k]), 3)
        if k != 'plain':
            out[k + '_extra_ms'] = round(med[k] - med['plain'], 3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
