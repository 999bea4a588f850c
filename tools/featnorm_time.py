"""Cost of the feature normalisation: wn_feature_stats and
wn_feature_normalize, each launch alone between two device events on an idle
stream, at 8 x 63 x 80 (the frames of a training batch of 8 x 16000 samples
at hop 256) and at one utterance-sized [1, 4000, 80]; and the default
LC-upsampler training step (tools/melspec_time.py's shape: wavenet_params.json,
8 x 16000, Lc 80, scales 4,5,10, features from the audio every step) with and
without a normaliser, in interleaved rounds of one process.  Reported, not
gated: each arm's rounds and their spread are the noise a difference has to be
read against.

    python tools/featnorm_time.py [--launches 200] [--steps 20] [--rounds 5]
        [--out profiles/featnorm_time.txt]
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
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel, _lib, features, optimizer_factory
    dev = torch.device('cuda', 0)
    lines = ['device: %s' % torch.cuda.get_device_name(0)]
    rng = np.random.default_rng(0)
    _lib.load()
    parts = _lib.load().wn_feature_stats_partials_count()
    for B, F, C in ((8, 63, 80), (1, 4000, 80)):
        x = torch.from_numpy((rng.standard_normal((B, F, C)) * 11 - 10)
                             .astype(np.float32)).to(dev)
        out = torch.empty_like(x)
        acc = torch.zeros((2, C), dtype=torch.float64, device=dev)
        scratch = torch.empty(parts * 2 * C, dtype=torch.float64, device=dev)
        norm = features.Normalizer.from_stats(
            features.FeatureStats(C).update(x), 4.0)
        shift, scale = (torch.from_numpy(v).to(dev)
                        for v in (norm.shift, norm.scale))
        st = _lib.stream()

        def stats():
            _lib.call('wn_feature_stats', _lib.ptr(x), B, F, C, None,
                      _lib.ptr(acc), _lib.ptr(scratch), st)

        def normalize():
            _lib.call('wn_feature_normalize', _lib.ptr(x), _lib.ptr(out), B,
                      F, C, None, _lib.ptr(shift), _lib.ptr(scale), -4.0, 4.0,
                      st)
        for name, fn in (('wn_feature_stats', stats),
                         ('wn_feature_normalize', normalize)):
            us = launch_us(fn, a.launches)
            lines.append('%d x %d x %d: %s median %.2f us, min %.2f us per '
                         'call (%d floats)' % (B, F, C, name,
                                               statistics.median(us), min(us),
                                               B * F * C))
    # the training step
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    scales, B, T, Lc = (4, 5, 10), 8, 16000, 80
    raw = features.MelSpec(params['sample_rate'], hop=200, n_mels=Lc)
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
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T))
                             .astype(np.float32)).to(dev)
    normed = raw.with_normalizer(features.Normalizer.from_stats(
        features.FeatureStats(Lc).update(raw(audio)), 4.0))
    arms = (('raw', raw), ('normalised', normed))

    def timed(spec, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            lc = net.local_condition_from_audio(spec, audio)
            opt.minimize(net.loss(audio, local_condition_batch=lc,
                                  local_condition_offset=0))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    for _, spec in arms:
        timed(spec, a.warmup)
    ms = {k: [] for k, _ in arms}
    for _ in range(a.rounds):
        for k, spec in arms:
            ms[k].append(timed(spec, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines.append('training step 8 x 16000, Lc 80, scales 4,5,10, features '
                 'from the audio every step (median of %d rounds of %d '
                 'steps): raw %.3f ms, normalised %.3f ms (%+.3f ms)'
                 % (a.rounds, a.steps, med['raw'], med['normalised'],
                    med['normalised'] - med['raw']))
    for k, _ in arms:
        lines.append('%s rounds (ms): %s, spread %.3f'
                     % (k, [round(v, 3) for v in ms[k]],
                        max(ms[k]) - min(ms[k])))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
