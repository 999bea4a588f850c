"""Cost of the mel + F0 front end's assembly (wn_lc_frames) at 8 x 160000
samples, 16 kHz, 80 mels, hop 256 (625 frames per clip), in one process,
device events around warmed-up calls, the arms of a comparison alternating
round by round so that clock drift and the host's other work hit both alike:

  1. the wn_lc_frames launch (normalise the mels, F0 channel and voicing flag,
     one tensor [B, F, 82]) beside the composition it replaces on the same
     inputs: wn_feature_normalize + PitchTracker.channels (torch ops in
     float64) + torch.cat;
  2. the whole front end from the audio: `mel` (wn_melspec + normalise)
     against `mel+f0` with the tracker, and with the Viterbi path;
  3. the training step of the default model (wavenet_params.json, batch 8 x
     16000 samples) with 82 local-conditioning channels against 80, by
     tools/lc_step_time.py's method.

Reported per arm: the median over the rounds and the spread (max - min) of
the arm's own rounds.  Nothing is gated; where the fused launch is slower
than the composition by more than the spread, the file says so.

    python tools/lc_frames_time.py [--iters 200] [--rounds 5] [--steps 20]
        [--out profiles/lc_frames_time.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def per_call_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), \
        torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def rounds_of(arms, iters, rounds, warmup=10):
    """{name: [us per call, one per round]}, the arms alternating."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    got = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            got[k].append(per_call_us(fn, iters))
    return got


def line_of(name, us):
    return '%s: median %.2f us, rounds %s, spread %.2f us' % (
        name, statistics.median(us), ' '.join('%.2f' % v for v in us),
        max(us) - min(us))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import features, frontend, pitch
    dev = torch.device('cuda', 0)
    B, T, sr, M = 8, 160000, 16000, 80
    lines = ['device: %s' % torch.cuda.get_device_name(0)]
    rng = np.random.default_rng(0)
    # tools/pitch_time.py's audio: a harmonic glide per clip plus noise
    tt = np.arange(T) / sr
    x = np.stack([0.4 * np.sin(2 * np.pi * (110.0 + 20 * b + 30 * tt) * tt) *
                  (np.sin(2 * np.pi * 0.7 * tt + b) > -0.3) for b in range(B)])
    x = (x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
    x = torch.from_numpy(x).to(dev)
    norm = features.Normalizer.from_range(-23.0, 7.0, M)
    mel = features.MelSpec(sr, n_mels=M, normalizer=norm)
    t = pitch.PitchTracker(sr)
    path = pitch.PitchPath(t)
    specs = {'mel+f0, tracker': frontend.MelPitchSpec(mel, t),
             'mel+f0, path': frontend.MelPitchSpec(mel, t, path),
             'mel+f0, tracker, interpolated':
                 frontend.MelPitchSpec(mel, t, None, True)}
    F = mel.num_frames(T)
    raw = mel.with_normalizer(None)(x)
    p = t(x)
    lines.append('%d x %d samples at %d Hz, %d mels, hop %d: %d frames per '
                 'clip, %.1f %% voiced'
                 % (B, T, sr, M, mel.hop, F,
                    100 * float((p.f0 > 0).to(torch.float64).mean())))

    # 1. the launch beside the composition it replaces
    fused0, fused1 = specs['mel+f0, tracker'], \
        specs['mel+f0, tracker, interpolated']
    out = torch.empty((B, F, M + 2), dtype=torch.float32, device=dev)

    def composition():
        return torch.cat([norm(raw), t.channels(p)], -1)
    same = torch.equal(fused0.assemble(raw, p.f0)[..., :M],
                       composition()[..., :M])
    worst = float((fused0.assemble(raw, p.f0) - composition()).abs().max())
    got = rounds_of({
        'wn_lc_frames, mode 0': lambda: fused0.assemble(raw, p.f0, out=out),
        'wn_lc_frames, mode 1': lambda: fused1.assemble(raw, p.f0, out=out),
        'composition': composition}, a.iters, a.rounds)
    lines.append('1. one launch against wn_feature_normalize + '
                 'PitchTracker.channels + torch.cat (max |difference| of the '
                 'results %.3g%s):' % (worst, '' if same else
                                       '; THE MEL CHANNELS DIFFER'))
    lines += ['   ' + line_of(k, v) for k, v in got.items()]
    fu, co = got['wn_lc_frames, mode 0'], got['composition']
    gap = statistics.median(fu) - statistics.median(co)
    spread = max(max(fu) - min(fu), max(co) - min(co))
    if gap <= spread:
        lines.append('   the fused launch takes %.2f x the composition\'s '
                     'time' % (statistics.median(fu) / statistics.median(co)))
    else:
        lines.append('   THE FUSED LAUNCH IS SLOWER THAN THE COMPOSITION by '
                     '%.2f us, more than the spread of %.2f us: not the '
                     'intended state' % (gap, spread))

    # 2. the whole front end from the audio
    arms = {'mel': lambda: mel(x)}
    arms.update({k: (lambda s=s: s(x)) for k, s in specs.items()})
    got = rounds_of(arms, max(1, a.iters // 10), a.rounds, warmup=3)
    lines.append('2. the whole front end from the audio:')
    lines += ['   ' + line_of(k, v) for k, v in got.items()]

    # 3. the training step with Lc 82 against 80
    import lc_step_time as st
    from wavenet import optimizer_factory
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    Bs, Ts = 8, 16000
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (Bs, Ts)).astype(
        np.float32)).cuda()
    runs = {}
    for lc in (M, M + 2):
        net = st.build(params, Bs, lc)
        opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
        feats = torch.from_numpy(rng.standard_normal((Bs, Ts, lc)).astype(
            np.float32)).cuda()
        st.timed(net, opt, audio, feats, 5)
        runs[lc] = (net, opt, feats, [])
    for _ in range(a.rounds):
        for lc in (M, M + 2):
            net, opt, feats, ms = runs[lc]
            ms.append(st.timed(net, opt, audio, feats, a.steps))
    lines.append('3. the training step of wavenet_params.json, batch %d x %d, '
                 '%d steps per round:' % (Bs, Ts, a.steps))
    for lc in (M, M + 2):
        ms = runs[lc][3]
        lines.append('   Lc %d: median %.3f ms, rounds %s, spread %.3f ms'
                     % (lc, statistics.median(ms),
                        ' '.join('%.3f' % v for v in ms), max(ms) - min(ms)))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
