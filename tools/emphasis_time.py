"""Cost of pre-emphasis and de-emphasis: wn_preemphasis and wn_deemphasis,
each launch alone between two device events on an idle stream, at 8 x 16000
(a training batch) and at 1 x 160000 (one ten-second utterance: 40 chunk
iterations of one workgroup); and the default model's training step
(wavenet_params.json, 8 x 16000, the shape bench.py times) with and without
the pre-emphasis of every batch, in interleaved rounds of one process.
Reported, not gated: each arm's rounds and their spread are the noise a
difference has to be read against; bench.py itself does not pre-emphasise, so
its number is that of the arm without.

    python tools/emphasis_time.py [--launches 200] [--steps 20] [--rounds 5]
        [--out profiles/emphasis_time.txt]
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


def launch_us(fn, launches):
    """Microseconds of each of `launches` single launches: one event pair
    per launch, nothing else on the stream."""
    for _ in range(10):
        fn()
    us = []
    for _ in range(launches):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        us.append(s.elapsed_time(e) * 1e3)
    return us


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--alpha', type=float, default=0.97)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel, _lib, optimizer_factory
    from wavenet.emphasis import Emphasis
    dev = torch.device('cuda', 0)
    lines = ['device: %s' % torch.cuda.get_device_name(0),
             'alpha %g, chunk %d samples' % (a.alpha, Emphasis.chunk())]
    rng = np.random.default_rng(0)
    alpha = float(np.float32(a.alpha))
    for B, T in ((8, 16000), (1, 160000)):
        x = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T))
                             .astype(np.float32)).to(dev)
        out = torch.empty_like(x)
        st = _lib.stream()

        def pre():
            _lib.call('wn_preemphasis', _lib.ptr(x), _lib.ptr(out), T, T, B,
                      T, None, alpha, st)

        def de():
            _lib.call('wn_deemphasis', _lib.ptr(x), _lib.ptr(out), T, T, B, T,
                      None, None, None, alpha, st)
        for name, fn in (('wn_preemphasis', pre), ('wn_deemphasis', de)):
            us = launch_us(fn, a.launches)
            lines.append('%d x %d: %s median %.2f us, min %.2f us per call '
                         '(%d floats)' % (B, T, name, statistics.median(us),
                                          min(us), B * T))
    # the training step
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    B, T = 8, 16000
    net = WaveNetModel(
        batch_size=B, dilations=params['dilations'],
        filter_width=params['filter_width'],
        residual_channels=params['residual_channels'],
        dilation_channels=params['dilation_channels'],
        skip_channels=params['skip_channels'],
        quantization_channels=params['quantization_channels'],
        use_biases=params['use_biases'], scalar_input=params['scalar_input'],
        initial_filter_width=params['initial_filter_width'])
    opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T))
                             .astype(np.float32)).to(dev)
    emph = Emphasis(a.alpha)
    bufs = [torch.empty_like(audio), torch.empty_like(audio)]
    arms = ('off', 'pre-emphasis')

    def timed(arm, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            batch = audio if arm == 'off' else \
                emph.pre(audio, out=bufs[k & 1])
            opt.minimize(net.loss(batch))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    for arm in arms:
        timed(arm, a.warmup)
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for arm in arms:
            ms[arm].append(timed(arm, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append('training step 8 x 16000, default model (median of %d rounds '
                 'of %d steps): off %.3f ms, pre-emphasis %.3f ms (%+.3f ms)'
                 % (a.rounds, a.steps, med['off'], med['pre-emphasis'],
                    med['pre-emphasis'] - med['off']))
    for arm in arms:
        lines.append('%s rounds (ms): %s, spread %.3f'
                     % (arm, [round(v, 3) for v in ms[arm]],
                        max(ms[arm]) - min(ms[arm])))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
