"""Pitch on the device: F0, aperiodicity and voicing per frame of the
local-conditioning (LC) grid (csrc/wn_pitch.hip, include/wavenet_pitch.h), two
frame-rate conditioning channels built from them, and the F0 error of two
tracks.

The rule, a YIN-style tracker on the LC alignment of the log-mel front end --
frame f sits beside the samples f * hop .. f * hop + hop - 1 -- for a clip
x[0:n], with W = window:

    tau_min  = max(2, floor(sample_rate / fmax))
    tau_max  = ceil(sample_rate / fmin)        tau_min + 2 <= tau_max <= 1024
    F        = ceil(n / hop) frames
    c        = f * hop + hop // 2              the frame's centre
    y[j]     = x[c - (W + tau_max) // 2 + j],  j < W + tau_max; x = 0 outside [0, n)

    1. e = sum_{j < W} y[j]^2 (float32).  e <= silence * W: the frame is
       silent: f0 = 0, aper = 1, lag = 0, its cmnd row all 1.
    2. d[tau] = sum_{j < W} (y[j] - y[j + tau])^2, tau = 1 .. tau_max, float32,
       the direct form, one fixed summation order (wavenet_pitch.h).
    3. S[tau] = sum_{k = 1 .. tau} d[k] in float64, ascending;
       c'[tau] = float32(d[tau] * tau / S[tau]) where S[tau] > 0, else 1;
       c'[0] = 1.
    4. The first tau in [tau_min, tau_max - 1] with c'[tau] < threshold, then
       down the slope while tau + 1 <= tau_max - 1 and c'[tau + 1] < c'[tau]:
       voiced.  Without one: the smallest index of the minimum of c' over
       that range, unvoiced.
    5. lag = tau, aper = c'[tau].  Voiced: with a, b, g = c'[tau - 1],
       c'[tau], c'[tau + 1], den = (a - 2 b) + g,
       delta = den > 0 ? clamp(0.5 (a - g) / den, -0.5, 0.5) : 0,
       f0 = sample_rate / (tau + delta) in float32.  Unvoiced: f0 = 0.
       "Voiced" is f0 > 0 everywhere.
    6. Frames f >= ceil(n / hop) of a padded batch are exact zeros.

The lag range is computed in double from sample_rate, fmin and fmax rounded to
float32, as the library's wn_pitch_tau_min / wn_pitch_tau_max compute it.  No
smoothing across frames: a frame's bits depend on its own W + tau_max samples
and the settings alone.

`PitchTracker.reference` states the rule in numpy; `PitchTracker.channels`
and `f0_error` are plain torch ops on whatever device their input lives on.
"""
import collections
import math

import numpy as np

from . import _lib
from .features import _is_int, _is_num, check_lengths

WINDOW_MAX = 2048
HOP_MAX = 4096
TAU_MAX = 1024


class Pitch(collections.namedtuple('Pitch', 'f0 aper lag cmnd')):
    """What a PitchTracker returns: f0 (Hz, 0 where unvoiced), aper (c' at
    the lag) float32 and lag int32, [B, F] or [F]; cmnd float32
    [..., tau_max + 1] or None."""
    __slots__ = ()

    @property
    def voiced(self):
        return self.f0 > 0


def lag_range(sample_rate, fmin, fmax):
    """(tau_min, tau_max) of the module docstring."""
    sr = float(np.float32(sample_rate))
    return (max(2, int(math.floor(sr / float(np.float32(fmax))))),
            int(math.ceil(sr / float(np.float32(fmin)))))


class PitchTracker(object):
    """The tracker of one setting.  Calling it tracks audio on the device;
    every argument is checked here, before any library or device is
    touched."""

    def __init__(self, sample_rate, hop=256, fmin=60.0, fmax=500.0,
                 window=1024, threshold=0.15, silence=1e-7):
        if not _is_num(sample_rate) or not sample_rate > 0:
            raise ValueError('sample_rate must be a positive number, got %r'
                             % (sample_rate,))
        if not _is_int(hop) or not 1 <= hop <= HOP_MAX:
            raise ValueError('hop must be an int in [1, %d], got %r'
                             % (HOP_MAX, hop))
        if not _is_int(window) or not 64 <= window <= WINDOW_MAX or \
                window % 64:
            raise ValueError('window must be a multiple of 64 in [64, %d], '
                             'got %r' % (WINDOW_MAX, window))
        if not _is_num(fmin) or not _is_num(fmax) or not 0 < fmin < fmax:
            raise ValueError('0 < fmin < fmax is required, got fmin %r, fmax '
                             '%r' % (fmin, fmax))
        if not _is_num(threshold) or not 0 < threshold < 1 or \
                not 0 < float(np.float32(threshold)) < 1:
            raise ValueError('threshold must lie in (0, 1), got %r'
                             % (threshold,))
        if not _is_num(silence) or not silence >= 0:
            raise ValueError('silence must be a non-negative mean square, '
                             'got %r' % (silence,))
        with np.errstate(over='ignore'):
            finite = all(np.isfinite(np.float32(v)) and np.float32(v) > 0
                         for v in (sample_rate, fmin, fmax))
        if not finite:
            raise ValueError('sample_rate, fmin and fmax must be positive '
                             'float32 numbers, got %r, %r, %r'
                             % (sample_rate, fmin, fmax))
        tau_min, tau_max = lag_range(sample_rate, fmin, fmax)
        if not tau_min + 2 <= tau_max <= TAU_MAX:
            raise ValueError(
                'tau_min + 2 <= tau_max <= %d is required: sample_rate %r, '
                'fmin %r, fmax %r give the lags %d .. %d'
                % (TAU_MAX, sample_rate, fmin, fmax, tau_min, tau_max))
        self.sample_rate = sample_rate
        self.hop, self.window = int(hop), int(window)
        self.fmin, self.fmax = float(fmin), float(fmax)
        self.threshold, self.silence = float(threshold), float(silence)
        self.tau_min, self.tau_max = tau_min, tau_max

    def settings(self):
        """The constructor's keywords as a plain dict (`from_settings`
        inverts it exactly)."""
        return dict(sample_rate=self.sample_rate, hop=self.hop,
                    fmin=self.fmin, fmax=self.fmax, window=self.window,
                    threshold=self.threshold, silence=self.silence)

    @classmethod
    def from_settings(cls, d):
        if not isinstance(d, dict) or 'sample_rate' not in d:
            raise ValueError("pitch settings need 'sample_rate', got %r"
                             % (d,))
        return cls(**d)

    def num_frames(self, n):
        return -(-int(n) // self.hop)

    def __call__(self, audio, lengths=None, return_cmnd=False):
        """Track audio [B, T] or [T] (a float array or device tensor):
        Pitch(f0, aper, lag, cmnd) of device tensors [B, F] or [F], F =
        ceil(T / hop), cmnd [..., tau_max + 1] with return_cmnd else None,
        without waiting for the device.  lengths ([B] ints, 1 <= n[b] <= T):
        clip b has n[b] real samples; what lies behind them is not read, and
        frames f >= ceil(n[b] / hop) are zeros."""
        import torch
        if not isinstance(audio, torch.Tensor):
            audio = np.asarray(audio)
            if audio.dtype == object or \
                    not np.issubdtype(audio.dtype, np.floating):
                raise ValueError('pitch: audio must be a float array')
        elif not audio.is_floating_point():
            raise ValueError('pitch: audio must be floating point')
        one = audio.ndim == 1
        if audio.ndim not in (1, 2) or audio.shape[-1] < 1 or \
                (not one and audio.shape[0] < 1):
            raise ValueError('pitch: audio must have shape [B, T] or [T], '
                             'got %s' % (tuple(audio.shape),))
        B, T = (1 if one else int(audio.shape[0])), int(audio.shape[-1])
        if B > 65535 or T > 1 << 30:
            raise ValueError('pitch: B <= 65535 and T <= 2^30 are required, '
                             'got [%d, %d]' % (B, T))
        n = check_lengths(lengths, B, T, 'pitch')
        _lib.load()
        _lib.require_gpu()
        if isinstance(audio, torch.Tensor) and audio.device.type == 'cuda':
            device = audio.device
        else:
            device = torch.device('cuda', torch.cuda.current_device())
            if not isinstance(audio, torch.Tensor):
                audio = torch.from_numpy(np.ascontiguousarray(audio))
        a = audio.to(device=device, dtype=torch.float32).reshape(B, T) \
            .contiguous()
        F = self.num_frames(T)
        with torch.cuda.device(device):
            nd = None if n is None else torch.from_numpy(n).to(device)
            f0 = torch.empty((B, F), dtype=torch.float32, device=device)
            aper = torch.empty_like(f0)
            lag = torch.empty((B, F), dtype=torch.int32, device=device)
            cmnd = torch.empty((B, F, self.tau_max + 1), dtype=torch.float32,
                               device=device) if return_cmnd else None
            _lib.call('wn_pitch_track', _lib.ptr(a), _lib.ptr(nd), T, B, T,
                      self.hop, self.window, self.tau_min, self.tau_max,
                      self.threshold, self.silence, self.sample_rate,
                      _lib.ptr(f0), _lib.ptr(aper), _lib.ptr(lag),
                      _lib.ptr(cmnd), _lib.stream())
        if one:
            return Pitch(f0[0], aper[0], lag[0],
                         None if cmnd is None else cmnd[0])
        return Pitch(f0, aper, lag, cmnd)

    def reference(self, x, dtype=np.float64):
        """The rule in numpy for one clip x [n]: Pitch of numpy arrays [F]
        (cmnd [F, tau_max + 1]).  dtype float64: every sum and quotient in
        float64; float32: e, d, c' and the interpolation in float32 (numpy's
        summation order), S in float64."""
        dtype = np.dtype(dtype).type
        x = np.asarray(x, dtype).reshape(-1)
        n, W, hop = x.shape[0], self.window, self.hop
        tmin, tmax = self.tau_min, self.tau_max
        N, F = W + tmax, self.num_frames(n)
        pos = (np.arange(F) * hop + hop // 2 - N // 2)[:, None] + \
            np.arange(N)[None, :]
        ok = (pos >= 0) & (pos < n)
        y = np.where(ok, x[np.clip(pos, 0, n - 1)], dtype(0))
        head = y[:, :W]
        e = (head * head).sum(1, dtype=dtype)
        d = np.zeros((F, tmax + 1), dtype)
        for tau in range(1, tmax + 1):
            v = head - y[:, tau:tau + W]
            d[:, tau] = (v * v).sum(1, dtype=dtype)
        S = np.cumsum(d.astype(np.float64), axis=1)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = d.astype(np.float64) * np.arange(tmax + 1)[None, :] / S
        cm = np.where(S > 0, q, 1.0).astype(dtype)
        cm[:, 0] = 1
        thr = dtype(self.threshold)
        sr = dtype(np.float32(self.sample_rate))
        f0 = np.zeros(F, dtype)
        aper = np.ones(F, dtype)
        lag = np.zeros(F, np.int32)
        for f in range(F):
            if e[f] <= dtype(self.silence) * dtype(W):
                cm[f] = 1
                continue
            c = cm[f]
            under = np.nonzero(c[tmin:tmax] < thr)[0]
            if under.size:
                tau = tmin + int(under[0])
                while tau + 1 <= tmax - 1 and c[tau + 1] < c[tau]:
                    tau += 1
                a, b, g = c[tau - 1], c[tau], c[tau + 1]
                den = (a - dtype(2) * b) + g
                delta = dtype(0)
                if den > 0:
                    delta = min(max(dtype(0.5) * (a - g) / den, dtype(-0.5)),
                                dtype(0.5))
                f0[f] = sr / (dtype(tau) + delta)
            else:
                tau = tmin + int(np.argmin(c[tmin:tmax]))
            lag[f], aper[f] = tau, c[tau]
        return Pitch(f0, aper, lag, cm)

    def channels(self, pitch, nframes=None):
        """Two frame-rate conditioning channels of a Pitch (or an f0 tensor)
        [B, F] or [F]: float32 [B, F, 2] or [F, 2] on the input's device.
        Channel 0: log2(f0 / fmin) / log2(fmax / fmin) clamped to [0, 1] on
        voiced frames (computed in float64, rounded once), 0 elsewhere;
        channel 1: the voicing flag, 0.0 or 1.0.  nframes ([B] ints): frames
        at or behind nframes[b] are zeros (the tracker's padding frames are
        zeros already: f0 = 0 there).  Plain torch ops, no synchronisation.

        A model built with local_condition_channels = n_mels + 2 takes

            torch.cat([mel_frames, tracker.channels(p)], -1)

        as local_condition_batch, mel_frames [B, F, n_mels] being the log-mel
        front end's frames of the same audio at the same hop."""
        import torch
        f0 = pitch.f0 if isinstance(pitch, Pitch) else pitch
        if not isinstance(f0, torch.Tensor):
            f0 = torch.from_numpy(np.asarray(f0, np.float32))
        if f0.dim() not in (1, 2) or not f0.is_floating_point():
            raise ValueError('channels: f0 must be a float tensor [B, F] or '
                             '[F], got %s %s' % (f0.dtype, tuple(f0.shape)))
        voiced = _real(f0 > 0, nframes, 'channels')
        safe = torch.where(voiced, f0.to(torch.float64),
                           torch.full_like(f0, self.fmin, dtype=torch.float64))
        rel = torch.log2(safe / self.fmin) / math.log2(self.fmax / self.fmin)
        rel = torch.where(voiced, rel.clamp(0.0, 1.0), torch.zeros_like(rel))
        return torch.stack([rel.to(torch.float32),
                            voiced.to(torch.float32)], -1)


def _real(mask, nframes, what):
    """`mask` [B, F] or [F] and-ed with f < nframes[b] (None: as it is)."""
    import torch
    if nframes is None:
        return mask
    F = int(mask.shape[-1])
    B = 1 if mask.dim() == 1 else int(mask.shape[0])
    if hasattr(nframes, 'detach'):
        n = nframes.to(device=mask.device, dtype=torch.int64).reshape(-1)
    else:
        n = np.asarray(nframes)
        if n.dtype == object or n.dtype == np.bool_ or \
                not np.issubdtype(n.dtype, np.integer):
            raise ValueError('%s: nframes must be integers, got %s'
                             % (what, n.dtype))
        n = torch.from_numpy(n.astype(np.int64).reshape(-1)).to(mask.device)
    if int(n.shape[0]) != B:
        raise ValueError('%s: nframes must have shape [%d], got [%d]'
                         % (what, B, int(n.shape[0])))
    keep = torch.arange(F, device=mask.device)[None, :] < n[:, None]
    return mask & (keep[0] if mask.dim() == 1 else keep)


class F0Error(collections.namedtuple(
        'F0Error', 'frames both gross fine vuv sq_cents voiced_ref')):
    """What `f0_error` returns, per clip [B]: int64 counts frames, both,
    gross, fine, vuv, voiced_ref and the float64 sum sq_cents, on the inputs'
    device."""
    __slots__ = ()

    def summary(self):
        """Over all clips (one host wait):
            f0_rmse_cents     = sqrt(sum sq_cents / sum fine); None without
                                a fine frame
            gross_pitch_error = sum gross / sum both; None where no frame is
                                voiced on both sides
            vuv_error         = sum vuv / sum frames
            voiced_frames     = the reference's voiced frames
            frames"""
        import torch
        t = torch.stack([v.sum().to(torch.float64) for v in self]).cpu()
        frames, both, gross, fine, vuv, sq, vref = (float(v) for v in t)
        if frames < 1:
            raise ValueError('summary: no frames were counted')
        return {'f0_rmse_cents': math.sqrt(sq / fine) if fine else None,
                'gross_pitch_error': gross / both if both else None,
                'vuv_error': vuv / frames,
                'voiced_frames': int(vref), 'frames': int(frames)}


def f0_error(generated, original, nframes=None):
    """The F0 error of `generated` against `original`, two Pitch (or f0
    tensors) [B, F] or [F] of the same shape on one device -> F0Error of [B]
    tensors ([1] for [F]).  Over clip b's real frames (nframes: [B] ints;
    None: all F), with fa, fb the two f0, va = fa > 0, vb = fb > 0:
        frames, both = va & vb, gross = both & |fa / fb - 1| > 0.2,
        fine = both & ~gross, vuv = va ^ vb, voiced_ref = vb,
        sq_cents = sum over fine of (1200 log2(fa / fb))^2
    in float64 torch ops; no synchronisation."""
    import torch
    fa = generated.f0 if isinstance(generated, Pitch) else generated
    fb = original.f0 if isinstance(original, Pitch) else original
    for t in (fa, fb):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point() or \
                t.dim() not in (1, 2):
            raise ValueError('f0_error: two float tensors [B, F] or [F] (or '
                             'two Pitch) are required')
    if fa.shape != fb.shape or fa.device != fb.device:
        raise ValueError('f0_error: %s on %s against %s on %s'
                         % (tuple(fa.shape), fa.device, tuple(fb.shape),
                            fb.device))
    if fa.dim() == 1:
        fa, fb = fa[None], fb[None]
    real = _real(torch.ones_like(fa, dtype=torch.bool), nframes, 'f0_error')
    fa, fb = fa.to(torch.float64), fb.to(torch.float64)
    va, vb = (fa > 0) & real, (fb > 0) & real
    both = va & vb
    one = torch.ones_like(fa)
    ratio = torch.where(both, fa, one) / torch.where(both, fb, one)
    gross = both & ((ratio - 1.0).abs() > 0.2)
    fine = both & ~gross
    cents = 1200.0 * torch.log2(ratio)
    sq = torch.where(fine, cents * cents, torch.zeros_like(cents)).sum(1)

    def count(m):
        return m.sum(1, dtype=torch.int64)
    return F0Error(count(real), count(both), count(gross), count(fine),
                   count(va ^ vb), sq, count(vb))
