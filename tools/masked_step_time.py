"""Cost of the masked loss: the training step of the default model
(wavenet_params.json, batch 8 x 16000 samples) with `lengths` against the same
step without, one model, one process.

The lengths are drawn once from a fixed seed between T / 2 and T (one clip
keeps the full T).  Each timed round runs `--steps` steps (loss + Adam update)
of one kind after `--warmup` untimed ones of both, and the rounds alternate
unmasked / masked / unmasked ... so that clock and thermal drift hit both
alike.  Prints one JSON line: per-step medians over the rounds, their
difference, and the spread of each kind's rounds (the noise the difference
has to be read against).  The stack launches and GEMMs still compute all
B * T rows; only the loss kernel skips the padding.

    python tools/masked_step_time.py [--steps 20] [--rounds 5] [--out FILE]
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


def timed(net, opt, audio, lengths, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = net.loss(audio, lengths=lengths)
        opt.minimize(loss)
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
    lengths = rng.integers(T // 2, T + 1, B)
    lengths[0] = T
    net = build(params, B)
    opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
    kinds = (('unmasked', None), ('masked', lengths))
    for _, n in kinds:
        timed(net, opt, audio, n, a.warmup)
    ms = {k: [] for k, _ in kinds}
    for _ in range(a.rounds):
        for k, n in kinds:
            ms[k].append(timed(net, opt, audio, n, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(config='wavenet_params.json', batch=B, samples=T,
               lengths=lengths.tolist(), real_samples=int(lengths.sum()),
               steps=a.steps, rounds=a.rounds,
               unmasked_ms=round(med['unmasked'], 3),
               masked_ms=round(med['masked'], 3),
               extra_ms=round(med['masked'] - med['unmasked'], 3),
               extra_pct=round(100 * (med['masked'] / med['unmasked'] - 1), 2),
               unmasked_rounds_ms=[round(v, 3) for v in ms['unmasked']],
               masked_rounds_ms=[round(v, 3) for v in ms['masked']],
               unmasked_spread_ms=round(max(ms['unmasked'])
                                        - min(ms['unmasked']), 3),
               masked_spread_ms=round(max(ms['masked']) - min(ms['masked']),
                                      3),
               device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
