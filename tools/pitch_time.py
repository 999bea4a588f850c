"""Cost of the pitch tracker (wn_pitch_track): microseconds per launch and
nanoseconds per frame at 8 x 160000 samples, 16 kHz, hop 256 and the default
settings (window 1024, lags 32 .. 267), beside wn_melspec on the same audio and
beside a torch restatement of the rule on the same device -- the frames as an
`unfold` view of the padded audio, d one lag after the other in float32, the
prefix in float64, c', the first lag under the threshold and the minimum; the
walk down the slope and the interpolation are left out of it.  Device events
around warmed-up launches.  Reported, not gated, but for one condition: the
kernel must not be slower than the restatement; otherwise the file says so.

    python tools/pitch_time.py [--iters 500] [--ref_iters 3]
        [--out profiles/pitch_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def per_call_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def torch_restatement(t):
    """x [B, T] -> (c' [B, F, tau_max + 1] float32, lag [B, F], voiced)."""
    W, hop, tmax, tmin = t.window, t.hop, t.tau_max, t.tau_min
    N = W + tmax

    def run(x):
        B, T = x.shape
        F = -(-T // hop)
        left = N // 2 - hop // 2
        need = (F - 1) * hop + N
        xp = torch.nn.functional.pad(x, (left, max(0, need - left - T)))
        y = xp.unfold(1, N, hop)[:, :F]                 # [B, F, N], a view
        head = y[..., :W]
        d = torch.zeros((B, F, tmax + 1), dtype=torch.float32, device=x.device)
        for tau in range(1, tmax + 1):
            v = head - y[..., tau:tau + W]
            d[..., tau] = (v * v).sum(-1)
        S = torch.cumsum(d.to(torch.float64), -1)
        lags = torch.arange(tmax + 1, device=x.device, dtype=torch.float64)
        c = torch.where(S > 0, d.to(torch.float64) * lags / S,
                        torch.ones_like(S)).to(torch.float32)
        c[..., 0] = 1.0
        silent = (head * head).sum(-1) <= t.silence * W
        c = torch.where(silent[..., None], torch.ones_like(c), c)
        r = c[..., tmin:tmax]
        under = r < t.threshold
        voiced = under.any(-1) & ~silent
        lag = torch.where(voiced, under.to(torch.int8).argmax(-1),
                          r.argmin(-1)) + tmin
        return c, lag, voiced
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=500)
    ap.add_argument('--ref_iters', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import features, pitch
    dev = torch.device('cuda', 0)
    B, T, sr = 8, 160000, 16000
    lines = ['device: %s' % torch.cuda.get_device_name(0)]
    rng = np.random.default_rng(0)
    # a harmonic glide per clip plus noise: voiced and unvoiced frames
    tt = np.arange(T) / sr
    x = np.stack([0.4 * np.sin(2 * np.pi * (110.0 + 20 * b + 30 * tt) * tt) *
                  (np.sin(2 * np.pi * 0.7 * tt + b) > -0.3) for b in range(B)])
    x = (x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
    x = torch.from_numpy(x).to(dev)
    t = pitch.PitchTracker(sr)
    spec = features.MelSpec(sr)
    frames = B * t.num_frames(T)
    ref = torch_restatement(t)
    p = t(x, return_cmnd=True)
    c, lag, voiced = ref(x)
    diff = float((p.cmnd - c).abs().max())
    same = float(((p.f0 > 0) == voiced).to(torch.float64).mean())
    k = per_call_us(lambda: t(x), a.iters, 10)
    kc = per_call_us(lambda: t(x, return_cmnd=True), a.iters, 10)
    m = per_call_us(lambda: spec(x), a.iters, 10)
    r = per_call_us(lambda: ref(x), a.ref_iters, 1)
    lines.append('%d x %d samples at %d Hz, hop %d, window %d, lags %d .. %d: '
                 '%d frames, %.1f %% voiced'
                 % (B, T, sr, t.hop, t.window, t.tau_min, t.tau_max, frames,
                    100 * float((p.f0 > 0).to(torch.float64).mean())))
    lines.append('wn_pitch_track: %.1f us per launch, %.1f ns per frame '
                 '(with the cmnd output: %.1f us, %.1f ns per frame)'
                 % (k, 1e3 * k / frames, kc, 1e3 * kc / frames))
    lines.append('wn_melspec (n_fft 1024, 80 mels) on the same audio: %.1f us '
                 'per launch, %.1f ns per frame' % (m, 1e3 * m / frames))
    lines.append('torch restatement (unfold view, one lag after the other, '
                 'float32 d, float64 prefix): %.1f us per call, %.1f ns per '
                 'frame; max |c\' - kernel| %.2g, voicing agrees on %.2f %% of '
                 'the frames' % (r, 1e3 * r / frames, diff, 100 * same))
    if k <= r:
        lines.append('the kernel is %.0f x faster than the restatement'
                     % (r / k))
    else:
        lines.append('THE KERNEL IS SLOWER THAN THE TORCH RESTATEMENT (%.2f x):'
                     ' not the intended state; the launch is one workgroup '
                     'per frame and should be bound by its LDS reads'
                     % (k / r))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
