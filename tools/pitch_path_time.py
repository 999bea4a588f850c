"""Cost of the pitch path (wn_pitch_path) at 8 x 160000 samples, 16 kHz, hop
256 and the default tracker (window 1024, lags 32 .. 267, so 235 voiced states
and 625 frames per clip), three arms in one process, device events around
warmed-up calls:

  1. wn_pitch_track with the cmnd output (what the path reads);
  2. wn_pitch_path on those rows -- per launch, and per frame of ONE clip's
     chain (a launch of one clip: the recurrence is serial in the frame);
  3. a torch restatement of the same recurrence on the same device: a Python
     loop over the frames with cummin for the two one-sided minima, the walk
     back as a loop of gathers.

Reported, not gated, but for one condition: the kernel must not be slower
than the restatement; otherwise the file says so.

    python tools/pitch_path_time.py [--iters 50] [--ref_iters 2]
        [--out profiles/pitch_path_time.txt]
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


def torch_restatement(path, device):
    """(cmnd [B, F, tau_max + 1], lag [B, F]) -> (lag [B, F], cost [B])."""
    t = path.tracker
    tmin, tmax, N = t.tau_min, t.tau_max, path.num_states
    pen, bias = (torch.from_numpy(v[tmin:tmax]).to(device)
                 for v in path.tables())
    sw, unv = path.switch, path.unvoiced

    def run(cmnd, lag):
        B, F, _ = cmnd.shape
        loc = cmnd[..., tmin:tmax] + bias
        lu = torch.where(lag == 0, torch.zeros_like(loc[..., 0]),
                         torch.full_like(loc[..., 0], unv))
        pred = torch.full((B, F, N + 1), N, dtype=torch.int64, device=device)
        cost = torch.zeros(B, dtype=torch.float64, device=device)
        V = U = None
        for f in range(F):
            if f == 0:
                nV, nU = loc[:, 0], lu[:, 0]
            else:
                ma, ia = torch.cummin(V - pen, -1)
                mb, ib = torch.cummin((V + pen).flip(-1), -1)
                mb, ib = mb.flip(-1), N - 1 - ib.flip(-1)
                L, Rr = ma + pen, mb - pen
                left = L <= Rr
                vv = torch.where(left, L, Rr)
                fu = (U + sw)[:, None]
                voiced = vv <= fu
                pred[:, f, :N] = torch.where(
                    voiced, torch.where(left, ia, ib), N)
                nV = torch.where(voiced, vv, fu) + loc[:, f]
                mv, kb = V.min(-1)
                fv = mv + sw
                stay = U <= fv
                pred[:, f, N] = torch.where(stay, N, kb)
                nU = torch.where(stay, U, fv) + lu[:, f]
            m = torch.minimum(nV.min(-1).values, nU)
            V, U = nV - m[:, None], nU - m
            cost += m.to(torch.float64)
        mv, kb = V.min(-1)
        st = torch.where(U <= mv, N, kb)
        out = torch.zeros((B, F), dtype=torch.int64, device=device)
        for f in range(F - 1, -1, -1):
            out[:, f] = torch.where(st < N, st + tmin, 0)
            st = pred[:, f].gather(1, st[:, None])[:, 0]
        return out, cost
    return run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--ref_iters', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import pitch
    dev = torch.device('cuda', 0)
    B, T, sr = 8, 160000, 16000
    lines = ['device: %s' % torch.cuda.get_device_name(0)]
    rng = np.random.default_rng(0)
    # tools/pitch_time.py's audio: a harmonic glide per clip plus noise
    tt = np.arange(T) / sr
    x = np.stack([0.4 * np.sin(2 * np.pi * (110.0 + 20 * b + 30 * tt) * tt) *
                  (np.sin(2 * np.pi * 0.7 * tt + b) > -0.3) for b in range(B)])
    x = (x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
    x = torch.from_numpy(x).to(dev)
    t = pitch.PitchTracker(sr)
    path = pitch.PitchPath(t)
    F = t.num_frames(T)
    raw = t(x, return_cmnd=True)
    one = (raw.cmnd[:1].contiguous(), raw.lag[:1].contiguous())
    p, cost = path.decode(raw.cmnd, raw.lag, return_cost=True)
    ref = torch_restatement(path, dev)
    rl, rc = ref(raw.cmnd, raw.lag)
    same = float((rl == p.lag).to(torch.float64).mean())
    dcost = float((rc - cost).abs().max())
    k1 = per_call_us(lambda: t(x, return_cmnd=True), a.iters, 5)
    k2 = per_call_us(lambda: path.decode(raw.cmnd, raw.lag), a.iters, 5)
    k2one = per_call_us(lambda: path.decode(*one), a.iters, 5)
    k3 = per_call_us(lambda: ref(raw.cmnd, raw.lag), a.ref_iters, 1)
    lines.append('%d x %d samples at %d Hz, hop %d, window %d, lags %d .. %d: '
                 '%d frames per clip, %d voiced states; raw track %.1f %% '
                 'voiced, path %.1f %%, %d frames differ'
                 % (B, T, sr, t.hop, t.window, t.tau_min, t.tau_max, F,
                    path.num_states,
                    100 * float((raw.f0 > 0).to(torch.float64).mean()),
                    100 * float((p.f0 > 0).to(torch.float64).mean()),
                    int((raw.lag * (raw.f0 > 0) != p.lag).sum())))
    lines.append('1. wn_pitch_track with the cmnd output: %.1f us per launch, '
                 '%.1f ns per frame' % (k1, 1e3 * k1 / (B * F)))
    lines.append('2. wn_pitch_path, %d clips: %.1f us per launch; one clip: '
                 '%.1f us per launch, %.2f us per frame of the chain'
                 % (B, k2, k2one, k2one / F))
    lines.append('3. torch restatement (a loop over the frames, cummin both '
                 'ways, gathers back), %d clips: %.0f us per call, %.1f us '
                 'per frame; its lags agree with the kernel\'s on %.2f %% of '
                 'the frames, max |cost - kernel| %.2g'
                 % (B, k3, k3 / F, 100 * same, dcost))
    if k2 <= k3:
        lines.append('the kernel is %.0f x faster than the restatement'
                     % (k3 / k2))
    else:
        lines.append('THE KERNEL IS SLOWER THAN THE TORCH RESTATEMENT (%.2f '
                     'x): not the intended state' % (k2 / k3))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
