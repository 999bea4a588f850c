"""Cost of linear prediction: wn_lpc_from_mel, wn_lpc_analysis and
wn_lpc_synthesis, each launch alone between two device events on an idle
stream, at 8 x 160000 (eight ten-second utterances), 32 x 16000 and 8 x 16000
(the training batch; 80 mels, hop 256, order 16), with wn_melspec and
wn_deemphasis on the same audio beside them; one clip's synthesis chain
(1 x 160000) in nanoseconds per sample; and the default model's training step
(wavenet_params.json, 8 x 16000, 80 mels computed from the batch) with and
without the excitation of every batch.
Every figure is the median of `--rounds` rounds, the arms taken in turn inside
a round; the rounds' spread (max - min) is the noise a difference has to be
read against.  Reported, not gated.

    python tools/lpc_time.py [--launches 50] [--steps 20] [--rounds 5]
        [--out profiles/lpc_time.txt]
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
    """Median microseconds of `launches` single launches: one event pair per
    launch, nothing else on the stream."""
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
    return statistics.median(us)


def rounds_of(arms, rounds, measure):
    """{name: [one figure per round]}: the arms in turn inside every round."""
    got = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            got[name].append(measure(fn))
    return got


def speech_like(rng, B, T):
    """float32 [B, T]: noise plus a pulse train through two resonators."""
    from scipy.signal import lfilter
    x = 0.05 * rng.standard_normal((B, T))
    x[:, ::128] += 1.0
    for fc, bw in ((700.0, 80.0), (2600.0, 150.0)):
        r = np.exp(-np.pi * bw / 16000.0)
        x = lfilter([1.0], [1.0, -2 * r * np.cos(2 * np.pi * fc / 16000.0),
                            r * r], x, axis=1)
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel, _lib, features, optimizer_factory
    from wavenet.emphasis import Emphasis
    from wavenet.lpc import LinearPrediction
    dev = torch.device('cuda', 0)
    spec = features.MelSpec(16000, n_fft=1024, hop=256, n_mels=80)
    lp = LinearPrediction(spec, order=16)
    emph = Emphasis(0.97)
    lines = ['device: %s' % torch.cuda.get_device_name(0),
             '80 mels, n_fft 1024, hop 256, order 16; analysis tile %d samples; '
             'medians of %d rounds of %d launches, (spread: max - min over the '
             'rounds)' % (lp.analysis_tile(), a.rounds, a.launches)]
    rng = np.random.default_rng(0)

    def fmt(name, v, extra=''):
        return '  %-18s %9.2f us (spread %.2f)%s' % (
            name, statistics.median(v), max(v) - min(v), extra)
    for B, T in ((8, 160000), (32, 16000), (8, 16000), (1, 160000)):
        x = torch.from_numpy(speech_like(rng, B, T)).to(dev)
        frames = spec(x)
        cf = lp.coefficients(frames)
        e = lp.analysis(x, cf)
        out = torch.empty_like(x)
        y = lp.synthesis(e, cf)
        err = float((y - x).abs().max())
        # (the entries themselves: no host work between the two events)
        st = _lib.stream()
        F = int(frames.shape[1])
        win, basis, melw = spec.device_tables(dev)
        pinv, ctab, lagwin = lp._tables(dev)
        fr_out, cf_out = torch.empty_like(frames), torch.empty_like(cf)
        P = _lib.ptr

        def melspec():
            _lib.call('wn_melspec', P(x), T, B, T, None, P(win), P(basis),
                      P(melw), spec.n_fft, spec.hop, spec.n_bins, spec.n_mels,
                      spec.floor, P(fr_out), st)

        def from_mel():
            _lib.call('wn_lpc_from_mel', P(frames), B, F, spec.n_mels, None,
                      P(pinv), spec.n_bins, P(ctab), P(lagwin), lp.order,
                      P(cf_out), st)

        def analysis():
            _lib.call('wn_lpc_analysis', P(x), T, P(cf), F, lp.order,
                      spec.hop, None, B, T, 1.0, P(out), T, st)

        def synthesis():
            _lib.call('wn_lpc_synthesis', P(e), T, P(cf), F, lp.order,
                      spec.hop, None, B, T, 1.0, P(out), T, st)

        def de():
            _lib.call('wn_deemphasis', P(e), P(out), T, T, B, T, None, None,
                      None, float(emph.alpha32), st)
        arms = [('wn_melspec', melspec), ('wn_lpc_from_mel', from_mel),
                ('wn_lpc_analysis', analysis),
                ('wn_lpc_synthesis', synthesis), ('wn_deemphasis', de)]
        for _, fn in arms:                      # warm every shape
            for _ in range(5):
                fn()
        got = rounds_of(arms, a.rounds, lambda fn: launch_us(fn, a.launches))
        lines.append('%d x %d (%d frames per clip; round trip max |y - x| '
                     '%.2g):' % (B, T, frames.shape[1], err))
        for name, _ in arms:
            extra = ''
            if name == 'wn_lpc_synthesis':
                extra = ', %.2f ns per sample of one clip\'s chain' % (
                    statistics.median(got[name]) * 1e3 / T)
            lines.append(fmt(name, got[name], extra))
    # the training step
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    scales, B, T, Lc = (4, 8, 8), 8, 16000, 80
    net = WaveNetModel(
        batch_size=B, dilations=params['dilations'],
        filter_width=params['filter_width'],
        residual_channels=params['residual_channels'],
        dilation_channels=params['dilation_channels'],
        skip_channels=params['skip_channels'],
        quantization_channels=params['quantization_channels'],
        use_biases=params['use_biases'], scalar_input=params['scalar_input'],
        initial_filter_width=params['initial_filter_width'],
        local_condition_channels=Lc, local_condition_upsample_scales=scales)
    opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
    audio = torch.from_numpy(speech_like(rng, B, T)).to(dev)
    bufs = [torch.empty_like(audio), torch.empty_like(audio)]
    state = {'k': 0}

    def step(with_lpc):
        lc = net.local_condition_from_audio(spec, audio)
        batch = audio
        if with_lpc:
            state['k'] += 1
            batch = lp.analysis(audio, lp.coefficients_of(audio),
                                out=bufs[state['k'] & 1])
        opt.minimize(net.loss(batch, local_condition_batch=lc,
                              local_condition_offset=0))

    def timed(with_lpc):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step(with_lpc)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.steps * 1e3
    for arm in (False, True):
        for _ in range(a.warmup):
            step(arm)
    ms = rounds_of([('off', False), ('--lpc_order 16', True)], a.rounds, timed)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append('training step 8 x 16000, default model, --lc_features mel '
                 '(80 mels, scales 4,8,8; median of %d rounds of %d steps): '
                 'off %.3f ms, --lpc_order 16 %.3f ms (%+.3f ms)'
                 % (a.rounds, a.steps, med['off'], med['--lpc_order 16'],
                    med['--lpc_order 16'] - med['off']))
    for arm, v in ms.items():
        lines.append('  %s rounds (ms): %s, spread %.3f'
                     % (arm, [round(t, 3) for t in v], max(v) - min(v)))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
