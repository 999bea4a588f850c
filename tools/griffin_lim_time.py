"""Cost of the Griffin-Lim baseline at 8 x 160000 samples, 80 mels,
(n_fft, hop, win_length) = (1024, 256, 1024), 32 iterations: microseconds for

  * one iteration, split into wn_istft (two launches: the frames' inverse
    DFTs on the matrix cores, the gather) and wn_gl_project (one launch: the
    STFT and the projection fused);
  * a torch restatement of one iteration on the same device: torch.fft.irfft,
    the window, torch.nn.functional.fold and the division by the windows'
    squares (torch.istft refuses this grid: without centring the periodic
    Hann's zero makes the envelope vanish at the first sample), then torch.stft
    (center=False) on the explicitly zero-padded signal and the elementwise
    projection;
  * the whole call (mel inversion, starting spectrum, 32 iterations, the last
    inverse) through the Python wrapper;
  * wn_melspec on the same audio, for scale.

Device events around warmed-up launches; the arms alternate inside one
process, --rounds rounds of --iters calls each; the median round and the
spread (min .. max) are reported.  Reported, not gated: a direct DFT does
n_fft / log2(n_fft) times an FFT's arithmetic, and where the kernels are slower
than the restatement the file says so in words.

    python tools/griffin_lim_time.py [--iters 10] [--rounds 5]
        [--out profiles/griffin_lim_time.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectral_time import alternate, row  # noqa: E402


def torch_iteration(gl, T):
    """(c, A, t_prev) -> (x, t, c): one iteration through torch's FFTs."""
    N, hop = gl.n_fft, gl.hop
    F = -(-T // hop)
    w = torch.from_numpy(gl.spec.window).cuda()
    left = N // 2 - hop // 2
    total = (F - 1) * hop + N
    right = total - left - T
    env = torch.nn.functional.fold(
        (w * w)[None, :, None].expand(1, N, F).contiguous(), (1, total),
        (1, N), stride=(1, hop)).reshape(total)[left:left + T]
    ok = env > 1e-8
    env = torch.where(ok, env, torch.ones_like(env))
    alpha = float(np.float32(gl.momentum))

    def run(c, A, tp):
        y = torch.fft.irfft(c, n=N, dim=-1) * w                 # [B, F, N]
        x = torch.nn.functional.fold(y.transpose(1, 2), (1, total), (1, N),
                                     stride=(1, hop)).reshape(-1, total)
        x = torch.where(ok, x[:, left:left + T] / env, torch.zeros_like(env))
        s = torch.stft(torch.nn.functional.pad(x, (left, right)), N,
                       hop_length=hop, window=w, center=False,
                       return_complex=True).transpose(1, 2)     # [B, F, nb]
        mag = s.abs()
        big = mag * mag > 1e-30
        t = torch.where(big, s * (A / torch.where(big, mag, torch.ones_like(mag))),
                        torch.complex(A, torch.zeros_like(A)))
        return x, t, t + alpha * (t - tp)
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import features, griffin_lim
    if not torch.cuda.is_available():
        raise SystemExit('griffin_lim_time: no device; nothing is measured '
                         'without one')
    B, T, ITER = 8, 160000, 32
    spec = features.MelSpec(16000, n_fft=1024, hop=256, n_mels=80)
    gl = griffin_lim.GriffinLim(spec, iterations=ITER)
    lines = ['device: %s' % torch.cuda.get_device_name(0),
             '%d x %d samples, %d mels, n_fft %d, hop %d, %d iterations; '
             'median of %d rounds of %d calls (min .. max), the arms '
             'alternated' % (B, T, spec.n_mels, spec.n_fft, spec.hop, ITER,
                             a.rounds, a.iters)]
    rng = np.random.default_rng(0)
    tt = np.arange(T) / 16000.0
    audio = np.stack([0.4 * np.sin(2 * np.pi * (110.0 + 20 * b + 30 * tt) * tt)
                      for b in range(B)]) + 0.01 * rng.standard_normal((B, T))
    audio = torch.from_numpy(audio.astype(np.float32)).cuda()
    frames = spec(audio)
    F = int(frames.shape[1])

    A = gl.magnitude(frames)
    c = torch.view_as_real(gl.initial(A)).contiguous()
    t = c.clone()
    x = torch.empty((B, T), dtype=torch.float32, device='cuda')
    scratch = gl._scratch(B, T, x.device)
    alpha = float(np.float32(gl.momentum))

    # one iteration both ways from the same state
    ref = torch_iteration(gl, T)
    c0, t0 = torch.view_as_complex(c.clone()), torch.view_as_complex(t.clone())
    gl._istft(c, None, scratch, x)
    gl._project(x, None, A, t, c, alpha, None, None)
    xr, tr, cr = ref(c0, A, t0)
    scale = float(xr.abs().max())
    lines.append('kernels against the torch restatement after one iteration, '
                 'largest difference: x %.2g of %.2g, t %.2g, c %.2g'
                 % (float((x - xr).abs().max()), scale,
                    float((torch.view_as_complex(t) - tr).abs().max()),
                    float((torch.view_as_complex(c) - cr).abs().max())))

    def k_istft():
        gl._istft(c, None, scratch, x)

    def k_project():
        gl._project(x, None, A, t, c, alpha, None, None)

    def k_iteration():
        k_istft()
        k_project()

    arms = {'istft': k_istft, 'project': k_project, 'iteration': k_iteration,
            'torch': lambda: ref(c0, A, t0), 'whole': lambda: gl(frames),
            'melspec': lambda: spec(audio)}
    r = alternate(arms, a.iters, a.rounds)
    lines.append(row('one iteration: wn_istft + wn_gl_project (three launches)',
                     r['iteration']))
    lines.append(row('  wn_istft alone (frames, gather)', r['istft']))
    lines.append(row('  wn_gl_project alone', r['project']))
    lines.append(row('torch restatement of one iteration (irfft, fold, stft, '
                     'elementwise)', r['torch']))
    lines.append(row('GriffinLim call, %d iterations, [%d, %d, %d] frames'
                     % (ITER, B, F, spec.n_mels), r['whole']))
    lines.append(row('wn_melspec on the same audio, for scale', r['melspec']))
    k, r_ = r['iteration'][0], r['torch'][0]
    if k <= r_:
        lines.append('the kernels are %.1f x faster than the restatement'
                     % (r_ / k))
    else:
        lines.append('THE KERNELS ARE SLOWER THAN THE TORCH RESTATEMENT '
                     '(%.2f x): a direct DFT against an FFT, n_fft / log2(n_fft)'
                     ' = %.0f times the arithmetic' % (k / r_, 1024 / 10.0))
    lines.append('(the kernel arms call the entries on preallocated buffers; '
                 'the whole call includes the Python wrapper and its '
                 'allocations)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
