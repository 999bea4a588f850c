"""Log-mel features on the device: frame-rate local-conditioning (LC) input
computed from the audio itself (csrc/wn_features.hip).

The rule, aligned to the LC convention -- frame f sits beside the samples
f * hop .. f * hop + hop - 1 -- for a clip x[0:n]:

    F        = ceil(n / hop) frames
    c        = f * hop + hop // 2                      the frame's centre
    frame[j] = x[c - n_fft // 2 + j] * window[j]       x = 0 outside [0, n)
    P[k]     = |DFT(frame)[k]|^2, k = 0 .. n_fft // 2
    M[m]     = sum_k melw[m][k] P[k]
    out[f][m] = log(max(M[m], floor))                  natural log

window: a periodic Hann window of win_length, centred in the n_fft samples.
melw: n_mels triangles of peak 1 (no area normalisation) over the bin centre
frequencies, between n_mels + 2 points equally spaced on the HTK mel scale
2595 log10(1 + f / 700) from fmin to fmax.  There is no reflection at the
clip's edges.  The tables are computed once per MelSpec in float64 and rounded
to float32; `logmel_reference` states the same rule in numpy.

Normalisation.  log(max(M, floor)) spans about -23 .. +7: far outside what a
Xavier-initialised conditioning projection can take.  `FeatureStats` sums x
and x * x per channel over a corpus's frames on the device, in float64 and in
one fixed order (wn_feature_stats); `Normalizer` is the affine + clamp rule

    v   = (x - shift[c]) * scale[c]                    float32, two roundings
    out = v < lo ? lo : (v > hi ? hi : v)              (a NaN stays a NaN)

applied on the device to the real frames (wn_feature_normalize; padding
frames stay exact zeros).  A MelSpec with a normaliser applies it to what it
computes, and its constants travel in the checkpoint's 'lc_features' entry.

Distance.  `frame_distance(a, b, nframes)` sums |a - b|, (a - b)^2 and the
per-frame root mean square of a - b over each clip's real frames on the device
(wn_feature_distance: float32 subtraction, float64 sums, one fixed order);
`FrameDistance.summary` turns the sums of log-mel features into dB.
"""
import copy
import re

import numpy as np

from . import _lib

N_FFT_MAX = 2048
N_MELS_MAX = 128


def _is_int(v):
    return isinstance(v, (int, np.integer)) and \
        not isinstance(v, (bool, np.bool_))


def _is_num(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and \
        not isinstance(v, (bool, np.bool_)) and np.isfinite(v)


def hz_to_mel(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)


def mel_to_hz(m):
    return 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)


def check_lengths(lengths, B, T, what):
    """`lengths` as int32 numpy [B] with 1 <= n[b] <= T (None stays None)."""
    if lengths is None:
        return None
    if hasattr(lengths, 'detach'):
        lengths = lengths.detach().cpu().numpy()
    n = np.asarray(lengths)
    if n.dtype == object or n.dtype == np.bool_ or \
            not np.issubdtype(n.dtype, np.integer):
        raise ValueError('%s: lengths must be %d integers (dtype %s)'
                         % (what, B, n.dtype))
    if n.shape != (B,):
        raise ValueError('%s: lengths must have shape [%d], got %s'
                         % (what, B, list(n.shape)))
    if (n < 1).any() or (n > T).any():
        raise ValueError('%s: lengths must lie in [1, T] = [1, %d], got %s'
                         % (what, T, n.tolist()))
    return n.astype(np.int32)


class MelSpec(object):
    """The log-mel front end of one setting.  Calling it computes features on
    the device; every argument is checked here, before any library or device
    is touched."""

    def __init__(self, sample_rate, n_fft=1024, hop=256, n_mels=80,
                 win_length=None, fmin=0.0, fmax=None, floor=1e-10, *,
                 normalizer=None):
        if not _is_num(sample_rate) or not sample_rate > 0:
            raise ValueError('sample_rate must be a positive number, got %r'
                             % (sample_rate,))
        if not _is_int(n_fft) or not 64 <= n_fft <= N_FFT_MAX or n_fft % 64:
            raise ValueError('n_fft must be a multiple of 64 in [64, %d], '
                             'got %r' % (N_FFT_MAX, n_fft))
        if win_length is None:
            win_length = n_fft
        if not _is_int(hop) or not _is_int(win_length) or \
                not 1 <= hop <= win_length <= n_fft:
            raise ValueError('1 <= hop <= win_length <= n_fft = %d is '
                             'required, got hop %r, win_length %r'
                             % (n_fft, hop, win_length))
        if not _is_int(n_mels) or not 1 <= n_mels <= N_MELS_MAX:
            raise ValueError('n_mels must be an int in [1, %d], got %r'
                             % (N_MELS_MAX, n_mels))
        if fmax is None:
            fmax = sample_rate / 2.0
        if not _is_num(fmin) or not _is_num(fmax) or \
                not 0 <= fmin < fmax <= sample_rate / 2.0:
            raise ValueError('0 <= fmin < fmax <= sample_rate / 2 = %g is '
                             'required, got fmin %r, fmax %r'
                             % (sample_rate / 2.0, fmin, fmax))
        if not _is_num(floor) or not floor > 0:
            raise ValueError('floor must be positive, got %r' % (floor,))
        _check_normalizer(normalizer, n_mels)
        self.normalizer = normalizer
        self.sample_rate = sample_rate
        self.n_fft, self.hop, self.n_mels = int(n_fft), int(hop), int(n_mels)
        self.win_length = int(win_length)
        self.fmin, self.fmax, self.floor = float(fmin), float(fmax), float(floor)
        self.n_bins = self.n_fft // 2 + 1
        self._tables()
        self._dev = {}

    def settings(self):
        """The constructor's keywords (train.py stores them in every
        checkpoint under 'lc_features', beside 'kind': 'mel')."""
        d = dict(sample_rate=self.sample_rate, n_fft=self.n_fft,
                 hop=self.hop, n_mels=self.n_mels,
                 win_length=self.win_length, fmin=self.fmin,
                 fmax=self.fmax, floor=self.floor)
        if self.normalizer is not None:
            d['normalizer'] = self.normalizer.entry()
        return d

    def with_normalizer(self, normalizer):
        """A spec with this normaliser (None: without one) that shares the
        tables and the device cache with this one."""
        _check_normalizer(normalizer, self.n_mels)
        other = copy.copy(self)
        other.normalizer = normalizer
        return other

    def num_frames(self, n):
        return -(-int(n) // self.hop)

    @property
    def channels(self):
        """The channels of the frames: what the model's
        local_condition_channels must be."""
        return self.n_mels

    def _tables(self):
        """window [n_fft] and melw [n_mels][n_bins]: float64, and rounded to
        float32 as the device gets them."""
        N, W, nb = self.n_fft, self.win_length, self.n_bins
        win = np.zeros(N, np.float64)
        lo = (N - W) // 2
        win[lo:lo + W] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)
        pts = mel_to_hz(np.linspace(hz_to_mel(self.fmin), hz_to_mel(self.fmax),
                                    self.n_mels + 2))
        fk = np.arange(nb, dtype=np.float64) * self.sample_rate / N
        up = (fk[None, :] - pts[:-2, None]) / (pts[1:-1] - pts[:-2])[:, None]
        down = (pts[2:, None] - fk[None, :]) / (pts[2:] - pts[1:-1])[:, None]
        self.window64 = win
        self.melw64 = np.maximum(0.0, np.minimum(up, down))
        self.window = win.astype(np.float32)
        self.melw = self.melw64.astype(np.float32)

    def basis64(self):
        """(cos, sin) [n_fft][n_bins] of 2 pi j k / n_fft in float64 (the
        angle through (j k) mod n_fft: exact integers, no large arguments)."""
        N = self.n_fft
        jk = (np.arange(N, dtype=np.int64)[:, None] *
              np.arange(self.n_bins, dtype=np.int64)[None, :]) % N
        ang = 2.0 * np.pi * jk.astype(np.float64) / N
        return np.cos(ang), np.sin(ang)

    def device_tables(self, device):
        """(window, basis, melw) in the kernel's layouts (wavenet_hip.h) on
        `device`, uploaded once."""
        import torch
        key = str(device)
        if key not in self._dev:
            N, nb = self.n_fft, self.n_bins
            NC, MP = -(-nb // 32), -(-self.n_mels // 32) * 32
            cos, sin = self.basis64()
            basis = np.zeros((NC, N, 2, 32), np.float32)
            for c in range(NC):
                k1 = min(nb, 32 * c + 32)
                basis[c, :, 0, :k1 - 32 * c] = cos[:, 32 * c:k1]
                basis[c, :, 1, :k1 - 32 * c] = sin[:, 32 * c:k1]
            melw = np.zeros((32 * NC, MP), np.float32)
            melw[:nb, :self.n_mels] = self.melw.T
            self._dev[key] = tuple(
                torch.from_numpy(t).to(device)
                for t in (self.window, basis.reshape(-1), melw))
        return self._dev[key]

    def __call__(self, audio, lengths=None):
        """Features of audio [B, T] or [T] (a float array or device tensor):
        device float32 [B, F, n_mels] or [F, n_mels], F = ceil(T / hop),
        without waiting for the device.  lengths ([B] ints, 1 <= n[b] <= T):
        clip b has n[b] real samples; what lies behind them is not read, and
        frames f >= ceil(n[b] / hop) are zeros.  With a normaliser the real
        frames are normalised (one more launch), the zeros stay zeros."""
        import torch
        if not isinstance(audio, torch.Tensor):
            audio = np.asarray(audio)
            if audio.dtype == object or \
                    not np.issubdtype(audio.dtype, np.floating):
                raise ValueError('spec: audio must be a float array')
        one = audio.ndim == 1
        if audio.ndim not in (1, 2) or audio.shape[-1] < 1 or \
                (not one and audio.shape[0] < 1):
            raise ValueError('spec: audio must have shape [B, T] or [T], got '
                             '%s' % (tuple(audio.shape),))
        B, T = (1 if one else int(audio.shape[0])), int(audio.shape[-1])
        n = check_lengths(lengths, B, T, 'spec')
        if isinstance(audio, torch.Tensor) and not audio.is_floating_point():
            raise ValueError('spec: audio must be floating point')
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
        with torch.cuda.device(device):
            win, basis, melw = self.device_tables(device)
            nd = None if n is None else torch.from_numpy(n).to(device)
            F = self.num_frames(T)
            out = torch.empty((B, F, self.n_mels), dtype=torch.float32,
                              device=device)
            _lib.call('wn_melspec', _lib.ptr(a), T, B, T, _lib.ptr(nd),
                      _lib.ptr(win), _lib.ptr(basis), _lib.ptr(melw),
                      self.n_fft, self.hop, self.n_bins, self.n_mels,
                      self.floor, _lib.ptr(out), _lib.stream())
            if self.normalizer is not None:
                self.normalizer._launch(
                    out, out, None if n is None else -(-n // self.hop))
        return out[0] if one else out


def _check_normalizer(normalizer, n_mels):
    if normalizer is None:
        return
    if not isinstance(normalizer, Normalizer):
        raise ValueError('normalizer must be a features.Normalizer or None')
    if normalizer.n_channels != n_mels:
        raise ValueError('the normaliser has %d channels, the front end %r '
                         'mels' % (normalizer.n_channels, n_mels))


def _frames_arg(frames, C, what):
    """(frames, one, B, F): `frames` as it came, whether it was [F, C], and
    its shape; float32 [B, F, C] or [F, C] with C channels is required."""
    if hasattr(frames, 'detach'):
        ok = str(frames.dtype) == 'torch.float32'
    else:
        frames = np.asarray(frames)
        ok = frames.dtype == np.float32
    shape = tuple(int(v) for v in frames.shape)
    if not ok or len(shape) not in (2, 3) or shape[-1] != C or \
            min(shape) < 1:
        raise ValueError('%s: frames must be float32 [B, F, %d] or [F, %d], '
                         'got %s %s' % (what, C, C, frames.dtype, shape))
    one = len(shape) == 2
    B, F = (1, shape[0]) if one else shape[:2]
    if B * F > 2 ** 31 - 1:
        raise ValueError('%s: B * F = %d exceeds 2^31 - 1' % (what, B * F))
    return frames, one, B, F


def _nframes_arg(nframes, B, F, what):
    """`nframes` as int32 numpy [B] with 0 <= n[b] <= F (None stays None)."""
    if nframes is None:
        return None
    if hasattr(nframes, 'detach'):
        nframes = nframes.detach().cpu().numpy()
    n = np.asarray(nframes)
    if n.dtype == object or n.dtype == np.bool_ or \
            not np.issubdtype(n.dtype, np.integer) or n.shape != (B,):
        raise ValueError('%s: nframes must be %d integers, got %s %s'
                         % (what, B, n.dtype, list(n.shape)))
    if (n < 0).any() or (n > F).any():
        raise ValueError('%s: nframes must lie in [0, F] = [0, %d], got %s'
                         % (what, F, n.tolist()))
    return n.astype(np.int32)


def _to_device(frames, B, F, C):
    """float32 device tensor [B, F, C], contiguous (the library is loaded)."""
    import torch
    if isinstance(frames, torch.Tensor) and frames.device.type == 'cuda':
        t = frames
    else:
        if not isinstance(frames, torch.Tensor):
            # (a copy of a read-only array: torch wants a writable one)
            frames = torch.from_numpy(
                np.ascontiguousarray(frames) if frames.flags.writeable
                else np.array(frames))
        t = frames.to(torch.device('cuda', torch.cuda.current_device()))
    return t.reshape(B, F, C).contiguous()


class FeatureStats(object):
    """Per-channel sums of x and x * x over frames, in float64: `update` adds
    a tensor's real frames on the device (wn_feature_stats: one fixed
    summation order, no atomics) without waiting for it; the sums a host
    gives (`from_sums`, `merge`, `load`) are kept beside and added in
    `sums()`.  The frame count is the host's."""

    def __init__(self, n_channels):
        if not _is_int(n_channels) or not 1 <= n_channels <= 512:
            raise ValueError('n_channels must be an int in [1, 512], got %r'
                             % (n_channels,))
        self.n_channels = int(n_channels)
        self.count = 0
        self._s = np.zeros((2, self.n_channels), np.float64)
        self._acc = None            # device float64 [2, C]
        self._partials = None

    def update(self, frames, nframes=None):
        C = self.n_channels
        frames, one, B, F = _frames_arg(frames, C, 'FeatureStats.update')
        n = _nframes_arg(nframes, B, F, 'FeatureStats.update')
        import torch
        _lib.load()
        _lib.require_gpu()
        t = _to_device(frames, B, F, C)
        if self._acc is not None and self._acc.device != t.device:
            raise ValueError('FeatureStats.update: frames on %s, the sums so '
                             'far on %s' % (t.device, self._acc.device))
        with torch.cuda.device(t.device):
            if self._acc is None:
                parts = _lib.load().wn_feature_stats_partials_count()
                self._acc = torch.zeros((2, C), dtype=torch.float64,
                                        device=t.device)
                self._partials = torch.empty(parts * 2 * C,
                                             dtype=torch.float64,
                                             device=t.device)
            nd = None if n is None else torch.from_numpy(n).to(t.device)
            _lib.call('wn_feature_stats', _lib.ptr(t), B, F, C, _lib.ptr(nd),
                      _lib.ptr(self._acc), _lib.ptr(self._partials),
                      _lib.stream())
        self.count += B * F if n is None else int(n.sum())
        return self

    def sums(self):
        """(count, s1 float64 [C], s2 float64 [C]) on the host (waits for
        the device where `update` ran)."""
        s = self._s
        if self._acc is not None:
            s = s + self._acc.cpu().numpy()
        return self.count, s[0].copy(), s[1].copy()

    def mean(self):
        n, s1, _ = self.sums()
        if n == 0:
            raise ValueError('FeatureStats.mean: no frames were counted')
        return s1 / n

    def std(self):
        """The population value, sqrt(max(s2 / n - mean^2, 0))."""
        n, s1, s2 = self.sums()
        if n == 0:
            raise ValueError('FeatureStats.std: no frames were counted')
        m = s1 / n
        return np.sqrt(np.maximum(s2 / n - m * m, 0.0))

    @classmethod
    def from_sums(cls, count, s1, s2):
        s1, s2 = np.asarray(s1, np.float64), np.asarray(s2, np.float64)
        if s1.ndim != 1 or s1.shape != s2.shape or s1.shape[0] < 1:
            raise ValueError('from_sums: s1 and s2 must both be [C], got %s '
                             'and %s' % (s1.shape, s2.shape))
        if isinstance(count, np.ndarray) and count.shape == ():
            count = count.item()
        if isinstance(count, (float, np.floating)) and \
                float(count).is_integer():
            count = int(count)
        if not _is_int(count) or count < 0:
            raise ValueError('from_sums: count must be a non-negative int, '
                             'got %r' % (count,))
        self = cls(s1.shape[0])
        self.count = int(count)
        self._s = np.stack([s1, s2])
        return self

    def merge(self, other):
        """Add another's sums to this one's (host only)."""
        if not isinstance(other, FeatureStats) or \
                other.n_channels != self.n_channels:
            raise ValueError('merge: FeatureStats of %d channels is required'
                             % self.n_channels)
        n, s1, s2 = other.sums()
        self.count += n
        self._s = self._s + np.stack([s1, s2])
        return self

    def vector(self):
        """float64 [1 + 2 C]: count, s1, s2 (what an all-reduce sums)."""
        n, s1, s2 = self.sums()
        return np.concatenate([[float(n)], s1, s2])

    @classmethod
    def from_vector(cls, v):
        v = np.asarray(v, np.float64).reshape(-1)
        C = (v.shape[0] - 1) // 2
        if v.shape[0] != 1 + 2 * C or C < 1:
            raise ValueError('from_vector: 1 + 2 C values are required')
        return cls.from_sums(v[0], v[1:1 + C], v[1 + C:])

    def save(self, path):
        n, s1, s2 = self.sums()
        with open(path, 'wb') as f:       # (np.savez would append .npz)
            np.savez(f, count=np.int64(n), s1=s1, s2=s2)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls.from_sums(int(z['count']), z['s1'], z['s2'])


class Normalizer(object):
    """out = clamp((x - shift[c]) * scale[c], lo, hi) per channel (module
    docstring).  Calling it runs wn_feature_normalize on the device;
    `reference` is the same rule in numpy float32."""

    def __init__(self, shift, scale, lo=None, hi=None, count=None):
        shift, scale = np.asarray(shift), np.asarray(scale)
        for name, v in (('shift', shift), ('scale', scale)):
            if v.ndim != 1 or v.shape[0] < 1 or v.shape[0] > 512 or \
                    v.dtype == object or v.dtype == np.bool_ or \
                    not np.issubdtype(v.dtype, np.number):
                raise ValueError('Normalizer: %s must be [C] numbers, '
                                 '1 <= C <= 512, got %s %s'
                                 % (name, v.dtype, v.shape))
        if shift.shape != scale.shape:
            raise ValueError('Normalizer: shift has %d channels, scale %d'
                             % (shift.shape[0], scale.shape[0]))
        with np.errstate(over='ignore'):
            shift, scale = shift.astype(np.float32), scale.astype(np.float32)
        if not np.isfinite(shift).all() or not np.isfinite(scale).all():
            raise ValueError('Normalizer: shift and scale must be finite')
        if (scale == 0).any():
            raise ValueError('Normalizer: scale must not be zero')
        for name, v in (('lo', lo), ('hi', hi)):
            if v is not None and (
                    not isinstance(v, (int, float, np.integer, np.floating))
                    or isinstance(v, (bool, np.bool_)) or np.isnan(v)):
                raise ValueError('Normalizer: %s must be a number or None, '
                                 'got %r' % (name, v))
        self.lo = None if lo is None or lo == -np.inf else \
            float(np.float32(lo))
        self.hi = None if hi is None or hi == np.inf else \
            float(np.float32(hi))
        if self._lo() > self._hi():
            raise ValueError('Normalizer: lo %r > hi %r' % (lo, hi))
        if count is not None and (not _is_int(count) or count < 0):
            raise ValueError('Normalizer: count must be a non-negative int '
                             'or None, got %r' % (count,))
        self.shift, self.scale = shift, scale
        self.count = None if count is None else int(count)
        self.n_channels = int(shift.shape[0])
        self._dev = {}

    def _lo(self):
        return -np.inf if self.lo is None else self.lo

    def _hi(self):
        return np.inf if self.hi is None else self.hi

    @classmethod
    def from_stats(cls, stats, clip=None, min_std=1e-5):
        """shift = float32(mean), scale = float32(1 / max(std, min_std)),
        clamped to [-clip, clip] with a clip."""
        if not isinstance(stats, FeatureStats):
            raise ValueError('from_stats: a FeatureStats is required')
        if clip is not None and (not _is_num(clip) or not clip > 0):
            raise ValueError('from_stats: clip must be positive, got %r'
                             % (clip,))
        if not _is_num(min_std) or not min_std > 0:
            raise ValueError('from_stats: min_std must be positive, got %r'
                             % (min_std,))
        mean, std = stats.mean(), stats.std()
        return cls(mean.astype(np.float32),
                   (1.0 / np.maximum(std, float(min_std))).astype(np.float32),
                   None if clip is None else -float(clip),
                   None if clip is None else float(clip), count=stats.count)

    @classmethod
    def from_range(cls, lo, hi, n_channels):
        """The dB-range convention: (x - lo) / (hi - lo), clamped to [0, 1].
        No statistics."""
        if not _is_num(lo) or not _is_num(hi) or not lo < hi:
            raise ValueError('from_range: lo < hi is required, got %r, %r'
                             % (lo, hi))
        if not _is_int(n_channels) or not 1 <= n_channels <= 512:
            raise ValueError('from_range: n_channels must be an int in '
                             '[1, 512], got %r' % (n_channels,))
        return cls(np.full(n_channels, lo, np.float32),
                   np.full(n_channels, 1.0 / (float(hi) - float(lo)),
                           np.float32), 0.0, 1.0)

    def entry(self):
        """A plain dict for a checkpoint (`from_entry` inverts it bit for
        bit: a float32 is exactly a Python float)."""
        return dict(shift=[float(v) for v in self.shift],
                    scale=[float(v) for v in self.scale],
                    lo=self.lo, hi=self.hi, count=self.count)

    @classmethod
    def from_entry(cls, d):
        if not isinstance(d, dict) or 'shift' not in d or 'scale' not in d:
            raise ValueError("a normaliser entry needs 'shift' and 'scale', "
                             'got %r' % (d,))
        return cls(np.asarray(d['shift'], np.float64),
                   np.asarray(d['scale'], np.float64), d.get('lo'),
                   d.get('hi'), count=d.get('count'))

    def with_clip(self, clip):
        """The same shift and scale, clamped to [-clip, clip]."""
        if not _is_num(clip) or not clip > 0:
            raise ValueError('clip must be positive, got %r' % (clip,))
        return Normalizer(self.shift, self.scale, -float(clip), float(clip),
                          count=self.count)

    def reference(self, frames, nframes=None):
        """The rule in numpy float32: [B, F, C] or [F, C]."""
        x, one, B, F = _frames_arg(np.asarray(frames), self.n_channels,
                                   'Normalizer.reference')
        n = _nframes_arg(nframes, B, F, 'Normalizer.reference')
        x = x.reshape(B, F, self.n_channels)
        with np.errstate(all='ignore'):
            v = ((x - self.shift) * self.scale).astype(np.float32)
            lo, hi = np.float32(self._lo()), np.float32(self._hi())
            v = np.where(v < lo, lo, np.where(v > hi, hi, v))
        if n is not None:
            v = np.where(np.arange(F)[None, :, None] < n[:, None, None], v,
                         np.float32(0))
        v = v.astype(np.float32)
        return v[0] if one else v

    def invert(self, frames, nframes=None):
        """x = v / scale[c] + shift[c] of normalised frames v, float32
        [B, F, C] or [F, C] (an array or a tensor): a float32 torch tensor on
        the frames' device, from torch's elementwise operators (plumbing, no
        kernel of the library).  Frames at or behind nframes[b] stay zeros.
        Clamped values do not come back: a v at lo or hi returns the edge of
        the clamp, not what was there before it."""
        import torch
        C = self.n_channels
        frames, one, B, F = _frames_arg(frames, C, 'Normalizer.invert')
        n = _nframes_arg(nframes, B, F, 'Normalizer.invert')
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.array(frames))
        v = frames.reshape(B, F, C)
        shift = torch.from_numpy(self.shift).to(v.device)
        scale = torch.from_numpy(self.scale).to(v.device)
        x = v / scale + shift
        if n is not None:
            real = torch.arange(F, device=v.device)[None, :, None] < \
                torch.from_numpy(n).to(v.device)[:, None, None]
            x = torch.where(real, x, torch.zeros((), dtype=x.dtype,
                                                 device=v.device))
        return x[0] if one else x

    def device_tables(self, device):
        """(shift, scale) on `device`, uploaded once."""
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.shift).to(device),
                              torch.from_numpy(self.scale).to(device))
        return self._dev[key]

    def _launch(self, src, dst, n):
        """src -> dst, device float32 [B, F, C] contiguous; n: int32 numpy
        [B] or None.  On src's device, torch's current stream."""
        import torch
        shift, scale = self.device_tables(src.device)
        B, F, C = (int(v) for v in src.shape)
        nd = None if n is None else \
            torch.from_numpy(np.ascontiguousarray(n, np.int32)).to(src.device)
        _lib.call('wn_feature_normalize', _lib.ptr(src), _lib.ptr(dst), B, F,
                  C, _lib.ptr(nd), _lib.ptr(shift), _lib.ptr(scale),
                  self._lo(), self._hi(), _lib.stream())

    def __call__(self, frames, nframes=None, out=None):
        """Normalised frames, device float32 of frames' shape, without
        waiting for the device.  nframes ([B] ints in [0, F]): clip b has
        that many real frames; the others become zeros and are not read.
        out: a contiguous device float32 tensor of the same shape to write
        into (may be `frames` itself)."""
        C = self.n_channels
        frames, one, B, F = _frames_arg(frames, C, 'Normalizer')
        n = _nframes_arg(nframes, B, F, 'Normalizer')
        if out is not None:
            if not hasattr(out, 'detach') or \
                    str(out.dtype) != 'torch.float32' or \
                    tuple(out.shape) != tuple(frames.shape) or \
                    out.device.type != 'cuda' or not out.is_contiguous():
                raise ValueError('Normalizer: out must be a contiguous '
                                 'float32 device tensor of shape %s'
                                 % (tuple(frames.shape),))
        import torch
        _lib.load()
        _lib.require_gpu()
        src = _to_device(frames, B, F, C)
        if out is not None and out.device != src.device:
            raise ValueError('Normalizer: out on %s, frames on %s'
                             % (out.device, src.device))
        dst = torch.empty_like(src) if out is None else out.view(B, F, C)
        with torch.cuda.device(src.device):
            self._launch(src, dst, n)
        return out if out is not None else (dst[0] if one else dst)


DB_PER_NEPER = 10.0 / np.log(10.0)      # natural log of power -> dB


class FrameDistance(object):
    """What `frame_distance` returns: abs_sum, sq_sum, rms_sum, device
    float64 [B] each (the rule: `frame_distance`)."""

    def __init__(self, abs_sum, sq_sum, rms_sum):
        self.abs_sum, self.sq_sum, self.rms_sum = abs_sum, sq_sum, rms_sum

    def __iter__(self):
        return iter((self.abs_sum, self.sq_sum, self.rms_sum))

    def summary(self, nframes, C):
        """(log_mel_mae_db, log_mel_lsd_db) over all clips, for features that
        are natural logs of power (waits for the device):
            mae = (10 / ln 10) sum abs_sum / (sum nframes * C)
            lsd = (10 / ln 10) sum rms_sum / sum nframes
        nframes: the real frames per clip (ints, or one int for all)."""
        if not _is_int(C) or C < 1:
            raise ValueError('summary: C must be a positive int, got %r'
                             % (C,))
        B = int(self.abs_sum.shape[0])
        n = np.asarray(nframes)
        if n.dtype == object or n.dtype == np.bool_ or \
                not np.issubdtype(n.dtype, np.integer) or \
                n.shape not in ((), (B,)) or (n < 0).any():
            raise ValueError('summary: nframes must be %d non-negative '
                             'integers, got %r' % (B, nframes))
        total = int(n) * B if n.shape == () else int(n.sum())
        if total < 1:
            raise ValueError('summary: no frames were counted')
        a = float(self.abs_sum.sum().item())
        r = float(self.rms_sum.sum().item())
        return DB_PER_NEPER * a / (total * int(C)), DB_PER_NEPER * r / total


def frame_distance(a, b, nframes=None):
    """Distance of two feature tensors, float32 [B, F, C] or [F, C] of the
    same shape, 1 <= C <= 512, on the device (wn_feature_distance), without
    waiting for it.  With d = a - b in float32, widened to float64:
        abs_sum[b] = sum |d|, sq_sum[b] = sum d^2,
        rms_sum[b] = sum_f sqrt(mean_c d^2)
    over clip b's real frames (nframes: [B] ints in [0, F]; the others are
    not read).  One fixed summation order, no atomics: a clip's numbers do
    not depend on the batch.  Returns a FrameDistance of float64 [B] tensors
    ([1] for [F, C] inputs)."""
    what = 'frame_distance'
    shapes = []
    for t in (a, b):
        t = t if hasattr(t, 'detach') else np.asarray(t)
        shapes.append(tuple(int(v) for v in t.shape))
    if shapes[0] != shapes[1]:
        raise ValueError('%s: a and b must have the same shape, got %s and '
                         '%s' % (what, shapes[0], shapes[1]))
    if len(shapes[0]) not in (2, 3) or not 1 <= shapes[0][-1] <= 512:
        raise ValueError('%s: float32 [B, F, C] or [F, C] with 1 <= C <= 512 '
                         'is required, got %s' % (what, shapes[0]))
    C = shapes[0][-1]
    a, _, B, F = _frames_arg(a, C, what)
    b, _, _, _ = _frames_arg(b, C, what)
    n = _nframes_arg(nframes, B, F, what)
    import torch
    lib = _lib.load()
    _lib.require_gpu()
    ta = _to_device(a, B, F, C)
    tb = _to_device(b, B, F, C)
    if ta.device != tb.device:
        raise ValueError('%s: a on %s, b on %s' % (what, ta.device, tb.device))
    with torch.cuda.device(ta.device):
        nd = None if n is None else torch.from_numpy(n).to(ta.device)
        out = torch.empty((3, B), dtype=torch.float64, device=ta.device)
        parts = torch.empty(lib.wn_feature_distance_partials(B, F),
                            dtype=torch.float64, device=ta.device)
        _lib.call('wn_feature_distance', _lib.ptr(ta), _lib.ptr(tb), B, F, C,
                  _lib.ptr(nd), _lib.ptr(out[0]), _lib.ptr(out[1]),
                  _lib.ptr(out[2]), _lib.ptr(parts), _lib.stream())
    return FrameDistance(out[0], out[1], out[2])


def logmel_reference(x, spec, dtype=np.float64):
    """The rule above in numpy for one clip x [n]: [ceil(n / hop), n_mels].
    dtype float64: the float64 tables; float32: the rounded tables the device
    gets, and float32 arithmetic."""
    dtype = np.dtype(dtype).type
    x = np.asarray(x, dtype).reshape(-1)
    n, N, hop = x.shape[0], spec.n_fft, spec.hop
    F = spec.num_frames(n)
    pos = (np.arange(F) * hop + hop // 2 - N // 2)[:, None] + \
        np.arange(N)[None, :]
    ok = (pos >= 0) & (pos < n)
    cos, sin = spec.basis64()
    fr = np.where(ok, x[np.clip(pos, 0, n - 1)], dtype(0)) * \
        spec.window64.astype(dtype)[None, :]
    re = fr @ cos.astype(dtype)
    im = fr @ sin.astype(dtype)
    m = (re * re + im * im) @ spec.melw64.astype(dtype).T
    out = np.log(np.maximum(m, dtype(spec.floor)))
    if spec.normalizer is not None:
        out = spec.normalizer.reference(out.astype(np.float32)).astype(dtype)
    return out


def is_spec(obj):
    """Whether obj is a front end: a MelSpec, or the mel + F0 composite
    frontend.MelPitchSpec (which has what the package reads from a MelSpec:
    hop, sample_rate, num_frames, n_mels, channels, normalizer,
    with_normalizer, settings; calling it gives [B, F, channels])."""
    if isinstance(obj, MelSpec):
        return True
    from . import frontend           # (frontend imports pitch, pitch this)
    return isinstance(obj, frontend.MelPitchSpec)


def local_condition_from_audio(net, spec, audio, lengths=None):
    """WaveNetModel.local_condition_from_audio (model.py)."""
    import torch
    if not is_spec(spec):
        raise ValueError('local_condition_from_audio: spec must be a MelSpec '
                         'or a frontend.MelPitchSpec')
    if not net.Lc:
        raise ValueError('local_condition_from_audio: this model was built '
                         'without local conditioning')
    if spec.channels != net.Lc:
        raise ValueError('local_condition_from_audio: the front end has %d '
                         '%s, the model %d local-conditioning channels'
                         % (spec.channels, 'mels' if isinstance(spec, MelSpec)
                            else 'channels', net.Lc))
    if net.lc_up and spec.hop != net.lc_hop:
        raise ValueError('local_condition_from_audio: the front end has hop '
                         '%d, the model upsamples by %d'
                         % (spec.hop, net.lc_hop))
    fr = spec(audio, lengths)
    if net.lc_up:
        return fr
    one = fr.dim() == 2
    T = int((audio.shape if hasattr(audio, 'shape') else np.shape(audio))[-1])
    idx = torch.arange(T, device=fr.device) // spec.hop
    rows = fr.index_select(fr.dim() - 2, idx)
    return rows if one else rows.contiguous()


# ------------------------------------------------------------ command line
def add_cli_flags(p, also=''):
    """The front end's flags, shared by train.py, evaluate.py, generate.py
    and tools/make_lc_features.py."""
    p.add_argument('--lc_features', choices=['mel', 'mel+f0', 'none'],
                   default=None,
                   help='Local conditioning from the audio itself: log-mel '
                   'features computed on the device (wavenet/features.py), '
                   '--lc_channels mels at one frame per hop samples; frame f '
                   'sits beside samples f * hop .. f * hop + hop - 1.  No '
                   '<clip>.npy files are read.  The features are those of '
                   'the piece as dequeued: a piece\'s edges see zeros, not '
                   'the neighbouring samples of its file.  mel+f0: '
                   '--lc_channels - 2 mels, then an F0 channel and a voicing '
                   'flag from the device pitch tracker '
                   '(wavenet/frontend.py).' + also)
    p.add_argument('--lc_f0_fmin', type=float, default=None,
                   help='--lc_features mel+f0: lowest F0 in Hz (default 60)')
    p.add_argument('--lc_f0_fmax', type=float, default=None,
                   help='--lc_features mel+f0: highest F0 in Hz (default 500)')
    p.add_argument('--lc_f0_path', type=_bool_arg, default=None,
                   metavar='true|false',
                   help='--lc_features mel+f0: take the F0 track from the '
                   'Viterbi path over the frames (pitch.PitchPath) instead of '
                   'frame by frame (default false)')
    p.add_argument('--lc_f0_interpolate', type=_bool_arg, default=None,
                   metavar='true|false',
                   help='--lc_features mel+f0: fill the F0 channel of '
                   'unvoiced frames by linear interpolation between the '
                   'nearest voiced frames instead of 0 (default false)')
    p.add_argument('--lc_n_fft', type=int, default=None,
                   help='--lc_features: DFT size, a multiple of 64 in '
                   '[64, %d] (default 1024)' % N_FFT_MAX)
    p.add_argument('--lc_win_length', type=int, default=None,
                   help='--lc_features: Hann window length, hop <= it <= '
                   '--lc_n_fft (default --lc_n_fft)')
    p.add_argument('--lc_fmin', type=float, default=None,
                   help='--lc_features: lowest filter edge in Hz (default 0)')
    p.add_argument('--lc_fmax', type=float, default=None,
                   help='--lc_features: highest filter edge in Hz (default '
                   'sample_rate / 2)')


    p.add_argument('--lc_normalize', choices=['none', 'corpus', 'range'],
                   default=None,
                   help='--lc_features: normalise the features on the '
                   'device.  corpus: per channel to zero mean and unit '
                   'variance with the statistics of the training corpus '
                   '(--device_corpus true computes them at load, else '
                   '--lc_stats FILE); range: (x - LO) / (HI - LO) clamped to '
                   '[0, 1] with --lc_range LO,HI; none: off, whatever the '
                   'checkpoint says.  The constants are stored in every '
                   'checkpoint (default: the checkpoint\'s).')
    p.add_argument('--lc_norm_clip', type=float, default=None,
                   help='--lc_normalize corpus: clamp the normalised '
                   'features to [-C, C]')
    p.add_argument('--lc_range', type=str, default=None,
                   help='--lc_normalize range: LO,HI in log-mel units, e.g. '
                   '-23,7')
    # (argparse takes an argument that starts with '-' for a flag unless it
    # looks like a negative number; "-23,7" has to look like one too)
    num = r'(\d+\.?\d*|\.\d+)([eE][-+]?\d+)?'
    p._negative_number_matcher = re.compile(
        r'^-%s(,[-+]?%s)?$' % (num, num))
    p.add_argument('--lc_stats', type=str, default=None,
                   help='--lc_normalize corpus: an .npz of per-channel sums '
                   '(tools/make_lc_stats.py, or a run\'s lc_stats.npz)')


_CLI_KEYS = ('n_fft', 'win_length', 'fmin', 'fmax')
_NORM_KEYS = ('normalize', 'norm_clip', 'range', 'stats')
_F0_KEYS = ('f0_fmin', 'f0_fmax', 'f0_path', 'f0_interpolate')
KINDS = ('mel', 'mel+f0')        # the front ends --lc_features switches on
F0_CHANNELS_ERROR = ('--lc_features mel+f0 needs --lc_channels >= 3: two of '
                     'the channels are the F0 channel and the voicing flag, '
                     'the others are mels (got %r)')


def _bool_arg(text):
    if str(text).lower() not in ('true', 'false'):
        import argparse
        raise argparse.ArgumentTypeError('true or false is required, got %r'
                                         % (text,))
    return str(text).lower() == 'true'


def cli_flags_given(args):
    """The --lc_n_fft ... flags that were given, by name."""
    return ['--lc_' + k for k in _CLI_KEYS + _NORM_KEYS
            if getattr(args, 'lc_' + k, None) is not None]


def f0_flags_given(args):
    """The --lc_f0_... flags that were given, by name."""
    return ['--lc_' + k for k in _F0_KEYS
            if getattr(args, 'lc_' + k, None) is not None]


def f0_flags_refused(args, stored_may_decide=False):
    """One line where a --lc_f0_... flag was given without --lc_features
    mel+f0, or --lc_features mel+f0 with fewer than 3 --lc_channels; else
    None.  stored_may_decide: without --lc_features a checkpoint may still
    name the front end (evaluate.py, generate.py)."""
    kind = getattr(args, 'lc_features', None)
    given = f0_flags_given(args)
    if given and kind != 'mel+f0' and not (kind is None and stored_may_decide):
        return '%s needs --lc_features mel+f0' % given[0]
    ch = getattr(args, 'lc_channels', None)
    if kind == 'mel+f0' and ch is not None and ch < 3:
        return F0_CHANNELS_ERROR % (ch,)
    return None


def stored_channels(stored):
    """The local-conditioning channels of a model trained on the front end
    of a checkpoint's 'lc_features' entry (None where it names none)."""
    n = stored.get('n_mels')
    if n is not None and stored.get('kind') == 'mel+f0':
        n += 2
    return n


def parse_range(text):
    """(lo, hi) of --lc_range LO,HI."""
    try:
        lo, hi = (float(v) for v in str(text).split(','))
    except ValueError:
        raise ValueError('--lc_range must be LO,HI (two numbers), got %r'
                         % (text,))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError('--lc_range needs finite LO < HI, got %r' % (text,))
    return lo, hi


def normalize_flags(args, corpus=False):
    """ValueError where --lc_normalize, --lc_norm_clip, --lc_range and
    --lc_stats do not fit together.  corpus: a device corpus will compute
    the statistics."""
    mode = getattr(args, 'lc_normalize', None)
    clip = getattr(args, 'lc_norm_clip', None)
    rng = getattr(args, 'lc_range', None)
    stats = getattr(args, 'lc_stats', None)
    if clip is not None and (not np.isfinite(clip) or not clip > 0):
        raise ValueError('--lc_norm_clip must be positive, got %r' % (clip,))
    if rng is not None:
        if mode != 'range':
            raise ValueError('--lc_range needs --lc_normalize range')
        parse_range(rng)
    if mode == 'range' and rng is None:
        raise ValueError('--lc_normalize range needs --lc_range LO,HI')
    if stats is not None and mode != 'corpus':
        raise ValueError('--lc_stats needs --lc_normalize corpus')
    if clip is not None and mode in ('none', 'range'):
        raise ValueError('--lc_norm_clip does not go with --lc_normalize %s'
                         % mode)
    if mode == 'corpus' and stats is None and not corpus:
        raise ValueError('--lc_normalize corpus needs --device_corpus true '
                         'or --lc_stats FILE')


def normalizer_from_cli(args, n_mels, stored=None, corpus=False):
    """The Normalizer the flags ask for, or None.  stored: a checkpoint's
    normaliser entry, the default without --lc_normalize (--lc_norm_clip
    then replaces its clamp).  With --lc_normalize corpus and no --lc_stats
    the corpus supplies it later (corpus=True): None."""
    normalize_flags(args, corpus)
    mode = getattr(args, 'lc_normalize', None)
    clip = getattr(args, 'lc_norm_clip', None)
    if mode == 'none':
        return None
    if mode == 'range':
        return Normalizer.from_range(*parse_range(args.lc_range),
                                     n_channels=n_mels)
    if mode == 'corpus':
        if args.lc_stats is None:
            return None
        try:
            stats = FeatureStats.load(args.lc_stats)
        except (OSError, KeyError) as e:
            raise ValueError('--lc_stats %s: %s' % (args.lc_stats, e))
        if stats.n_channels != n_mels:
            raise ValueError('--lc_stats %s holds %d channels, the front end '
                             'has %d mels' % (args.lc_stats, stats.n_channels,
                                              n_mels))
        return Normalizer.from_stats(stats, clip)
    if stored is None:
        if clip is not None:
            raise ValueError('--lc_norm_clip needs --lc_normalize corpus')
        return None
    norm = Normalizer.from_entry(stored)
    return norm if clip is None else norm.with_clip(clip)


def same_kind(stored, kind):
    """Whether a checkpoint's entry names the front end `kind`."""
    return stored is not None and stored.get('kind') == kind


def spec_from_cli(args, sample_rate, n_mels, hop, stored=None, corpus=False):
    """The front end the flags ask for -- a MelSpec, or with --lc_features
    mel+f0 a frontend.MelPitchSpec -- or None without one (its normaliser:
    normalizer_from_cli).  `stored`:
    a checkpoint's 'lc_features' entry -- without --lc_features it switches
    the front end on (--lc_features none: off), and its settings are the
    defaults of the flags that are absent.  ValueError where the flags, the
    model (n_mels = --lc_channels: the model's channels, two more than the
    mels with mel+f0; hop) and the entry do not fit."""
    kind = args.lc_features
    if kind is None and stored is not None:
        kind = stored.get('kind')
    if kind in (None, 'none'):
        given = cli_flags_given(args)
        if given:
            raise ValueError('%s needs --lc_features mel' % given[0])
        if f0_flags_given(args):
            raise ValueError('%s needs --lc_features mel+f0'
                             % f0_flags_given(args)[0])
        return None
    if kind not in KINDS:
        raise ValueError('unknown front end %r in the checkpoint\'s '
                         "'lc_features'" % (kind,))
    composite = kind == 'mel+f0'
    if not composite and f0_flags_given(args):
        raise ValueError('%s needs --lc_features mel+f0'
                         % f0_flags_given(args)[0])
    if stored is not None and stored.get('kind') in KINDS and \
            stored.get('kind') != kind:
        raise ValueError("the checkpoint's 'lc_features' are %r, the command "
                         'line asks for --lc_features %s'
                         % (stored.get('kind'), kind))
    if composite and n_mels is not None:
        if n_mels < 3:
            raise ValueError(F0_CHANNELS_ERROR % (n_mels,))
        if same_kind(stored, kind) and 'n_mels' in stored and \
                stored['n_mels'] + 2 != n_mels:
            # (in the units of the flag: the model's channels)
            raise ValueError(
                "the checkpoint's 'lc_features' have %d channels (%d mels + "
                'F0 + voicing), the command line asks for --lc_channels %d'
                % (stored['n_mels'] + 2, stored['n_mels'], n_mels))
        n_mels -= 2
    same = same_kind(stored, kind)
    kw = {}
    if same:
        kw = {k: stored[k] for k in _CLI_KEYS + ('floor',) if k in stored}
        for name, mine in (('n_mels', n_mels), ('hop', hop),
                           ('sample_rate', sample_rate)):
            if name in stored and mine is not None and stored[name] != mine:
                raise ValueError(
                    "the checkpoint's 'lc_features' have %s %r, the command "
                    'line asks for %r' % (name, stored[name], mine))
        n_mels = stored.get('n_mels') if n_mels is None else n_mels
        hop = stored.get('hop') if hop is None else hop
    for k in _CLI_KEYS:
        if getattr(args, 'lc_' + k) is not None:
            kw[k] = getattr(args, 'lc_' + k)
    if n_mels is None:
        raise ValueError('--lc_features %s needs --lc_channels (the number '
                         'of mels%s)' % (kind, ' + 2' if composite else ''))
    if hop is None:
        raise ValueError('--lc_features %s needs --lc_hop or '
                         '--lc_upsample_scales (hop = their product)' % kind)
    entry = stored.get('normalizer') if same else None
    mel = MelSpec(sample_rate, hop=hop, n_mels=n_mels,
                  normalizer=normalizer_from_cli(args, n_mels, entry, corpus),
                  **kw)
    if not composite:
        return mel
    from . import frontend, pitch
    was = dict(stored.get('pitch') or {}) if same else {}
    path_kw = was.pop('path', None)
    interpolate = was.pop('interpolate', False)
    tkw = {k: v for k, v in was.items() if k not in ('sample_rate', 'hop')}
    for flag, name in (('lc_f0_fmin', 'fmin'), ('lc_f0_fmax', 'fmax')):
        if getattr(args, flag, None) is not None:
            tkw[name] = getattr(args, flag)
    tracker = pitch.PitchTracker(sample_rate, hop=hop, **tkw)
    want_path = getattr(args, 'lc_f0_path', None)
    if want_path is None:
        want_path = path_kw is not None
    path = pitch.PitchPath(tracker, **(path_kw or {})) if want_path else None
    if getattr(args, 'lc_f0_interpolate', None) is not None:
        interpolate = args.lc_f0_interpolate
    return frontend.MelPitchSpec(mel, tracker, path, bool(interpolate))


def checkpoint_entry(spec):
    """What train.py stores under 'lc_features'."""
    return dict(kind='mel' if isinstance(spec, MelSpec) else 'mel+f0',
                **spec.settings())
