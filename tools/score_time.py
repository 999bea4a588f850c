"""Cost of scoring: time per call of net.score at the default model
(wavenet_params.json, batch 8 x 16000 samples), with and without `lengths`,
next to net.loss(..., backward=False) at the same shape in the same process.
That loss call is the yardstick: it makes the same forward pass and reads the
same logits once (wn_xent / wn_xent_masked without dlogits), and scoring
changed nothing in it.

Each timed round runs `--calls` calls of one kind after `--warmup` untimed ones
of every kind, and the rounds alternate between the kinds so that clock and
thermal drift hit all alike.  Writes (and prints) one line per kind -- the
median over the rounds, every round, their spread -- and the differences
score - loss with the spread they have to be read against.

    python tools/score_time.py [--calls 20] [--rounds 7] [--out profiles/score_time.txt]
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


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel
    p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    B, T = a.batch, a.samples
    net = WaveNetModel(
        batch_size=B, dilations=p['dilations'],
        filter_width=p['filter_width'],
        residual_channels=p['residual_channels'],
        dilation_channels=p['dilation_channels'],
        skip_channels=p['skip_channels'],
        quantization_channels=p['quantization_channels'],
        use_biases=p['use_biases'], scalar_input=p['scalar_input'],
        initial_filter_width=p['initial_filter_width'])
    rng = np.random.default_rng(a.seed)
    q = torch.from_numpy(rng.integers(0, net.Q, (B, T)).astype(np.int32)).cuda()
    lengths = rng.integers(T // 2, T + 1, B)
    lengths[0] = T
    kinds = [
        ('loss_fwd', lambda: net.loss_from_codes(q, backward=False)),
        ('score', lambda: net.score_from_codes(q)),
        ('loss_fwd_lengths',
         lambda: net.loss_from_codes(q, backward=False, lengths=lengths)),
        ('score_lengths', lambda: net.score_from_codes(q, lengths=lengths)),
        ('score_lengths_per_sample',
         lambda: net.score_from_codes(q, lengths=lengths, per_sample=True)),
    ]
    for _, fn in kinds:
        timed(fn, a.warmup)
    ms = {k: [] for k, _ in kinds}
    for _ in range(a.rounds):
        for k, fn in kinds:
            ms[k].append(timed(fn, a.calls))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    lines = ['score_time: %s, default model, %d x %d, %d calls per round, %d '
             'rounds alternating, ms per call'
             % (torch.cuda.get_device_name(0), B, T, a.calls, a.rounds),
             'lengths = %s' % lengths.tolist()]
    for k, _ in kinds:
        lines.append('%-26s median %.3f  spread %.3f  rounds %s'
                     % (k, med[k], spread[k],
                        ' '.join('%.3f' % v for v in ms[k])))
    for s, l in (('score', 'loss_fwd'), ('score_lengths', 'loss_fwd_lengths')):
        lines.append('%s - %s = %+.3f ms (%+.2f %%), spreads %.3f / %.3f'
                     % (s, l, med[s] - med[l],
                        100 * (med[s] / med[l] - 1), spread[s], spread[l]))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    return 0


if __name__ == '__main__':
    sys.exit(main())
