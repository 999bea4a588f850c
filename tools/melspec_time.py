"""Cost of the log-mel front end (wn_melspec): microseconds per call at
8 x 16000 and 1 x 160000 samples (hop 256, n_fft 1024, 80 mels) beside a
torch.stft + matmul restatement on the same device (the yardstick), and the
default LC-upsampler training step (tools/lc_upsample_step_time.py's shape:
wavenet_params.json, 8 x 16000, Lc 80, scales 4,5,10) with the features
computed from the audio every step against precomputed frames, in interleaved
rounds of one process.  Reported, not gated.

    python tools/melspec_time.py [--iters 200] [--steps 20] [--rounds 5]
        [--out profiles/melspec_time.txt]
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


def per_call_us(fn, iters):
    for _ in range(10):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def stft_restatement(spec, device):
    """The same rule through torch.stft (centre padding by hand: zeros,
    shifted by hop // 2) and a matmul with the filterbank."""
    win = torch.from_numpy(spec.window).to(device)
    melw = torch.from_numpy(spec.melw).to(device)
    N, hop = spec.n_fft, spec.hop

    def run(x):
        F = -(-x.shape[1] // hop)
        left = N // 2 - hop // 2
        need = (F - 1) * hop + N
        xp = torch.nn.functional.pad(x, (left, max(0, need - left - x.shape[1])))
        st = torch.stft(xp, N, hop_length=hop, window=win, center=False,
                        return_complex=True)[:, :, :F]
        p = st.real ** 2 + st.imag ** 2
        return torch.log(torch.clamp(torch.matmul(melw, p), min=spec.floor)) \
            .transpose(1, 2)
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel, features, optimizer_factory
    dev = torch.device('cuda', 0)
    lines = ['device: %s' % torch.cuda.get_device_name(0)]
    spec = features.MelSpec(16000)
    ref = stft_restatement(spec, dev)
    rng = np.random.default_rng(0)
    for B, T in ((8, 16000), (1, 160000)):
        x = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)).to(dev)
        diff = float((spec(x) - ref(x)).abs().max())
        k = per_call_us(lambda: spec(x), a.iters)
        r = per_call_us(lambda: ref(x), a.iters)
        lines.append('%d x %d: wn_melspec %.1f us per call, torch.stft + matmul '
                     '%.1f us (max abs difference %.2g)' % (B, T, k, r, diff))
    # the training step
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    scales, B, T, Lc = (4, 5, 10), 8, 16000, 80
    spec = features.MelSpec(params['sample_rate'], hop=200, n_mels=Lc)
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
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T)).astype(np.float32)).to(dev)
    frames = spec(audio)

    def timed(fly, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            lc = net.local_condition_from_audio(spec, audio) if fly else frames
            opt.minimize(net.loss(audio, local_condition_batch=lc,
                                  local_condition_offset=0))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3
    for fly in (False, True):
        timed(fly, a.warmup)
    ms = {False: [], True: []}
    for _ in range(a.rounds):
        for fly in (False, True):
            ms[fly].append(timed(fly, a.steps))
    pre, fly = statistics.median(ms[False]), statistics.median(ms[True])
    lines.append('training step 8 x 16000, Lc 80, scales 4,5,10 (median of %d '
                 'rounds of %d steps): precomputed frames %.3f ms, features '
                 'from the audio every step %.3f ms (%+.1f %%)'
                 % (a.rounds, a.steps, pre, fly, 100 * (fly / pre - 1)))
    lines.append('rounds (ms): precomputed %s, on the fly %s'
                 % ([round(v, 3) for v in ms[False]], [round(v, 3) for v in ms[True]]))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
