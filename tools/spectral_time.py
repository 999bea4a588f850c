"""Cost of the synthesis metrics at 8 x 160000 samples and the three default
resolutions (1024:120:600, 2048:240:1200, 512:50:240): microseconds for

  * the wn_stft_distance launches (StftDistance: per resolution the tiles'
    launch and the clips' sums), all three and each alone;
  * a torch restatement on the same device: torch.stft(center=False) on the two
    explicitly zero-padded signals per resolution, then the elementwise rule
    and the three sums per clip in float64;
  * two wn_melspec launches (80 mels) per resolution at the same (n_fft, hop),
    for scale;
  * wn_cepstral_distance (order 13) beside wn_feature_distance on [8, 625, 80].

Device events around warmed-up launches; the arms alternate inside one
process, --rounds rounds of --iters calls each; the median round and the
spread (min .. max) are reported.  Reported, not gated: where the kernel is
slower than the restatement the file says so in words.

    python tools/spectral_time.py [--iters 20] [--rounds 5]
        [--out profiles/spectral_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def per_call_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def alternate(arms, iters, rounds, warmup=3):
    """{name: (median, min, max)} us per call; the arms take turns."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(per_call_us(fn, iters))
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}


def torch_restatement(dist):
    """(g, o) [B, T] -> float64 [R, 3, B], the rule through torch.stft."""
    from wavenet import features
    tables = []
    for n_fft, hop, win in dist.resolutions:
        w = features.MelSpec(2.0, n_fft=n_fft, hop=hop, n_mels=1,
                             win_length=win).window
        tables.append((n_fft, hop, torch.from_numpy(w).cuda()))
    fl = dist.floor

    def run(g, o):
        T = g.shape[1]
        out = []
        for n_fft, hop, w in tables:
            F = -(-T // hop)
            left = n_fft // 2 - hop // 2
            right = (F - 1) * hop + n_fft - left - T
            p = []
            for x in (g, o):
                s = torch.stft(torch.nn.functional.pad(x, (left, right)),
                               n_fft, hop_length=hop, window=w, center=False,
                               return_complex=True)
                p.append((s.real * s.real + s.imag * s.imag).clamp_min(fl))
            mg, mo = p[0].sqrt(), p[1].sqrt()
            d = (mo - mg).double()
            l = ((p[1].log() - p[0].log()).abs() * 0.5).double()
            out.append(torch.stack([(d * d).sum((1, 2)),
                                    (mo.double() ** 2).sum((1, 2)),
                                    l.sum((1, 2))]))
        return torch.stack(out)
    return run


def row(name, v, unit='us'):
    return '%-58s %9.1f %s  (%.1f .. %.1f)' % (name, v[0], unit, v[1], v[2])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import features, spectral
    if not torch.cuda.is_available():
        raise SystemExit('spectral_time: no device; nothing is measured '
                         'without one')
    B, T = 8, 160000
    lines = ['device: %s' % torch.cuda.get_device_name(0),
             '%d x %d samples; median of %d rounds of %d calls (min .. max), '
             'the arms alternated' % (B, T, a.rounds, a.iters)]
    rng = np.random.default_rng(0)
    tt = np.arange(T) / 16000.0
    o = np.stack([0.4 * np.sin(2 * np.pi * (110.0 + 20 * b + 30 * tt) * tt)
                  for b in range(B)]) + 0.01 * rng.standard_normal((B, T))
    g = 0.8 * o + 0.03 * rng.standard_normal((B, T))
    g = torch.from_numpy(g.astype(np.float32)).cuda()
    o = torch.from_numpy(o.astype(np.float32)).cuda()

    dist = spectral.StftDistance()
    ref = torch_restatement(dist)
    got = torch.stack(list(dist(g, o))).permute(1, 0, 2)       # [R, 3, B]
    want = ref(g, o)
    rel = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
    lines.append('kernel against the torch restatement, largest relative '
                 'difference of a sum: %.2g' % rel)

    singles = [spectral.StftDistance((r,)) for r in dist.resolutions]
    mels = [features.MelSpec(16000, n_fft=r[0], hop=r[1], n_mels=80,
                             win_length=r[2]) for r in dist.resolutions]
    arms = {'kernel': lambda: dist(g, o), 'torch': lambda: ref(g, o),
            'melspec': lambda: [(m(g), m(o)) for m in mels]}
    for r, s in zip(dist.resolutions, singles):
        arms['kernel %d:%d:%d' % r] = (lambda s=s: s(g, o))
    for r, m in zip(dist.resolutions, mels):
        arms['melspec %d:%d:%d' % r] = (lambda m=m: (m(g), m(o)))
    t = alternate(arms, a.iters, a.rounds)
    lines.append(row('wn_stft_distance, three resolutions (six launches)',
                     t['kernel']))
    for r in dist.resolutions:
        lines.append(row('  %d:%d:%d alone' % r, t['kernel %d:%d:%d' % r]))
    lines.append(row('torch restatement (stft x 2 per resolution, '
                     'elementwise, sums)', t['torch']))
    lines.append(row('2 x wn_melspec (80 mels) per resolution, for scale',
                     t['melspec']))
    for r in dist.resolutions:
        lines.append(row('  %d:%d:%d alone' % r, t['melspec %d:%d:%d' % r]))
    k, r_ = t['kernel'][0], t['torch'][0]
    if k <= r_:
        lines.append('the kernel is %.1f x faster than the restatement'
                     % (r_ / k))
    else:
        lines.append('THE KERNEL IS SLOWER THAN THE TORCH RESTATEMENT '
                     '(%.2f x): not the intended state' % (k / r_))

    fa = torch.from_numpy(rng.uniform(-23, 7, (8, 625, 80))
                          .astype(np.float32)).cuda()
    fb = fa + torch.from_numpy(rng.normal(0, 1.5, (8, 625, 80))
                               .astype(np.float32)).cuda()
    t = alternate({'cep': lambda: spectral.cepstral_distance(fa, fb),
                   'feat': lambda: features.frame_distance(fa, fb)},
                  a.iters, a.rounds)
    lines.append('[8, 625, 80] log-mel frames:')
    lines.append(row('wn_cepstral_distance, order 13 (two launches)',
                     t['cep']))
    lines.append(row('wn_feature_distance (two launches)', t['feat']))
    lines.append('(every figure includes the Python wrapper: allocation of '
                 'the outputs and the scratch, the ctypes call)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
