"""Cost of input noise: wn_code_noise and wn_mu_law_encode_noisy (and
wn_mu_law_encode, which the fused kernel replaces in the step), each launch
alone between two device events on an idle stream at 8 x 16000; and the
default model's training step (wavenet_params.json, 8 x 16000, the shape
bench.py times) with and without `input_noise`, in interleaved rounds of one
process.  Reported, not gated: each arm's rounds and their spread are the
noise a difference has to be read against; bench.py itself passes no
input_noise, so its number is that of the arm without.

    python tools/input_noise_step_time.py [--launches 200] [--steps 20]
        [--rounds 5] [--out profiles/input_noise_step_time.txt]
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
    ap.add_argument('--prob', type=float, default=0.5)
    ap.add_argument('--width', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel, _lib, optimizer_factory
    from wavenet.input_noise import InputNoise, step_keys
    from wavenet.ops import mu_law_tables
    dev = torch.device('cuda', 0)
    noise = InputNoise(a.prob, a.width, 1234)
    lines = ['device: %s' % torch.cuda.get_device_name(0),
             'prob %g, width %d' % (noise.prob, noise.width)]
    rng = np.random.default_rng(0)
    B, T, Q = 8, 16000, 256
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T))
                             .astype(np.float32)).to(dev)
    q = torch.empty((B, T), dtype=torch.int32, device=dev)
    q_in = torch.empty_like(q)
    keys = torch.from_numpy(step_keys(0, B)).to(dev)
    thr, _ = mu_law_tables(Q)
    st = _lib.stream()

    def encode():
        _lib.call('wn_mu_law_encode', _lib.ptr(audio), _lib.ptr(q), B * T,
                  _lib.ptr(thr), Q, st)

    def codes():
        _lib.call('wn_code_noise', _lib.ptr(q), _lib.ptr(q_in), _lib.ptr(keys),
                  None, B, T, Q, noise.seed, noise.thresh, noise.width, st)

    def fused():
        _lib.call('wn_mu_law_encode_noisy', _lib.ptr(audio), _lib.ptr(q),
                  _lib.ptr(q_in), _lib.ptr(keys), None, B, T, _lib.ptr(thr),
                  Q, noise.seed, noise.thresh, noise.width, st)
    for name, fn in (('wn_mu_law_encode', encode), ('wn_code_noise', codes),
                     ('wn_mu_law_encode_noisy', fused)):
        us = launch_us(fn, a.launches)
        lines.append('%d x %d: %s median %.2f us, min %.2f us per call'
                     % (B, T, name, statistics.median(us), min(us)))
    # the training step
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
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
    arms = ('off', 'input_noise')
    count = [0]

    def timed(arm, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            if arm == 'off':
                loss = net.loss(audio)
            else:
                # (the keys of a step, staged per call as train.py does)
                count[0] += 1
                loss = net.loss(audio, input_noise=noise,
                                noise_keys=step_keys(count[0], B))
            opt.minimize(loss)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    for arm in arms:
        timed(arm, a.warmup)
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for arm in arms:
            ms[arm].append(timed(arm, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    diff = med['input_noise'] - med['off']
    lines.append('training step 8 x 16000, default model (median of %d rounds '
                 'of %d steps): off %.3f ms, input_noise %.3f ms (%+.3f ms)'
                 % (a.rounds, a.steps, med['off'], med['input_noise'], diff))
    spread = {}
    for arm in arms:
        spread[arm] = max(ms[arm]) - min(ms[arm])
        lines.append('%s rounds (ms): %s, spread %.3f'
                     % (arm, [round(v, 3) for v in ms[arm]], spread[arm]))
    lines.append('the difference of the medians is %s the larger spread of an '
                 'arm\'s own rounds (%.3f ms)'
                 % ('within' if abs(diff) <= max(spread.values())
                    else 'ABOVE', max(spread.values())))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
