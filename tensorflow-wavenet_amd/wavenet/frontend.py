"""The mel + F0 front end: log-mel frames with an F0 channel and a voicing
flag beside them, assembled on the device in one launch (csrc/
wn_lc_frames.hip, include/wavenet_lc_frames.h).

`MelPitchSpec(mel, tracker, path=None, interpolate=False)` is to the rest of
the package what a `features.MelSpec` is (`features.is_spec`): it has hop,
sample_rate, num_frames, n_mels (the mel part's), channels = n_mels + 2 (what
a model's local_condition_channels must be), normalizer / with_normalizer,
settings, and calling it computes frames [B, F, n_mels + 2] on the device:

    channels 0 .. n_mels - 1   the log-mel frames of `mel`, through its
                               normaliser where it has one
    channel  n_mels            the F0 channel, in [0, 1]
    channel  n_mels + 1        the voicing flag, 0.0 or 1.0

The F0 track is the tracker's, or with `path` (a pitch.PitchPath over that
tracker) the Viterbi path's.  On a voiced frame (f0 > 0, a real frame)

    r[f] = min(max(log2(f0 / fmin) / log2(fmax / fmin), 0), 1)     float64

goes, rounded once to float32, into the F0 channel.  On the other real frames
the channel is 0 (interpolate=False: the rule of PitchTracker.channels) or,
with interpolate=True, the continuous log-F0 of parametric vocoders: linear in
the frame index between the nearest voiced frames a < f < e,

    r[a] + (r[e] - r[a]) * ((f - a) / (e - a))                     float64

r[e] before the clip's first voiced frame, r[a] behind its last, 0 in a clip
without one -- so the channel has no step at a voicing edge; the flag still
tells the model where the voice is.  The normaliser acts on the mel channels
only (an n_mels-channel features.Normalizer): the pitch channels lie in [0, 1]
by construction and are never normalised or clamped.  Padding frames (behind
`lengths`) are exact zeros in every channel.
"""
import math

import numpy as np

from . import _lib
from . import features
from . import pitch as _pitch
from .features import check_lengths

MODES = ('zero', 'interp')


class MelPitchSpec(object):
    """The mel + F0 front end of one setting (module docstring).  Every
    argument is checked here, before any library or device is touched."""

    def __init__(self, mel, tracker, path=None, interpolate=False):
        if not isinstance(mel, features.MelSpec):
            raise ValueError('mel must be a features.MelSpec, got %r'
                             % (mel,))
        if not isinstance(tracker, _pitch.PitchTracker):
            raise ValueError('tracker must be a pitch.PitchTracker, got %r'
                             % (tracker,))
        if path is not None:
            if not isinstance(path, _pitch.PitchPath):
                raise ValueError('path must be a pitch.PitchPath or None, '
                                 'got %r' % (path,))
            if path.tracker is not tracker:
                raise ValueError('path must be a PitchPath over `tracker` '
                                 'itself')
        if not isinstance(interpolate, (bool, np.bool_)):
            raise ValueError('interpolate must be a bool, got %r'
                             % (interpolate,))
        if mel.hop != tracker.hop:
            raise ValueError('the mel front end has hop %d, the tracker %d'
                             % (mel.hop, tracker.hop))
        if mel.sample_rate != tracker.sample_rate:
            raise ValueError('the mel front end has sample rate %r, the '
                             'tracker %r' % (mel.sample_rate,
                                             tracker.sample_rate))
        self._mel = mel
        self.tracker, self.path = tracker, path
        self.interpolate = bool(interpolate)

    hop = property(lambda self: self._mel.hop)
    sample_rate = property(lambda self: self._mel.sample_rate)
    n_mels = property(lambda self: self._mel.n_mels)
    channels = property(lambda self: self._mel.n_mels + 2)
    normalizer = property(lambda self: self._mel.normalizer)
    mode = property(lambda self: 1 if self.interpolate else 0)

    @property
    def mel(self):
        """The mel part without its normaliser: the raw log-mel front end."""
        return self._mel.with_normalizer(None)

    @property
    def span(self):
        return math.log2(self.tracker.fmax / self.tracker.fmin)

    def num_frames(self, n):
        return self._mel.num_frames(n)

    def with_normalizer(self, normalizer):
        """A spec with this normaliser on its mel channels (None: without
        one) that shares the tables, the tracker and the path."""
        return MelPitchSpec(self._mel.with_normalizer(normalizer),
                            self.tracker, self.path, self.interpolate)

    def settings(self):
        """The mel part's settings (its normaliser's entry among them) and,
        under 'pitch', the tracker's, 'path' (the path's weights or None) and
        'interpolate' (`from_settings` inverts it exactly)."""
        path = None
        if self.path is not None:
            path = self.path.settings()
            del path['tracker']
        return dict(self._mel.settings(),
                    pitch=dict(self.tracker.settings(), path=path,
                               interpolate=self.interpolate))

    @classmethod
    def from_settings(cls, d):
        if not isinstance(d, dict) or not isinstance(d.get('pitch'), dict):
            raise ValueError("mel+f0 settings need 'pitch', got %r" % (d,))
        d = dict(d)
        d.pop('kind', None)
        p = dict(d.pop('pitch'))
        norm = d.pop('normalizer', None)
        path, interpolate = p.pop('path', None), p.pop('interpolate', False)
        tracker = _pitch.PitchTracker.from_settings(p)
        return cls(features.MelSpec(
            normalizer=None if norm is None else
            features.Normalizer.from_entry(norm), **d), tracker,
            None if path is None else _pitch.PitchPath(tracker, **path),
            interpolate)

    # ------------------------------------------------------------ the rule
    def reference_channels(self, f0, nframes=None, mode=None):
        """The two pitch channels of an F0 track in numpy: f0 [B, F] or [F]
        -> float32 [B, F, 2] or [F, 2]; nframes: [B] ints in [0, F] (None:
        F); mode: 0 / 1 (None: this spec's)."""
        mode = self.mode if mode is None else mode
        if mode not in (0, 1):
            raise ValueError('mode must be 0 or 1, got %r' % (mode,))
        f0 = np.asarray(f0)
        if f0.ndim not in (1, 2) or not np.issubdtype(f0.dtype, np.floating):
            raise ValueError('reference_channels: f0 must be a float array '
                             '[B, F] or [F], got %s %s' % (f0.dtype, f0.shape))
        one = f0.ndim == 1
        x = f0.reshape(-1, f0.shape[-1]).astype(np.float32)
        B, F = x.shape
        n = features._nframes_arg(nframes, B, F, 'reference_channels')
        n = np.full(B, F) if n is None else n
        idx = np.arange(F)[None, :]
        real = idx < n[:, None]
        with np.errstate(invalid='ignore'):
            voiced = real & (x > 0)
        fmin = self.tracker.fmin
        safe = np.where(voiced, x.astype(np.float64), fmin)
        with np.errstate(over='ignore'):
            r = np.minimum(np.maximum(np.log2(safe / fmin) / self.span, 0.0),
                           1.0)
        ch0 = np.where(voiced, r, 0.0)
        if mode == 1 and F:
            a = np.maximum.accumulate(np.where(voiced, idx, -1), axis=1)
            e = np.minimum.accumulate(np.where(voiced, idx, F)[:, ::-1],
                                      axis=1)[:, ::-1]
            has_a, has_e = a >= 0, e < F
            ra = np.take_along_axis(r, np.maximum(a, 0), 1)
            re = np.take_along_axis(r, np.minimum(e, F - 1), 1)
            both = has_a & has_e & ~voiced
            w = (idx - a).astype(np.float64) / \
                np.where(both, e - a, 1).astype(np.float64)
            fill = np.where(both, ra + (re - ra) * w,
                            np.where(has_e, re, np.where(has_a, ra, 0.0)))
            ch0 = np.where(voiced, r, np.where(real, fill, 0.0))
        out = np.stack([ch0.astype(np.float32), voiced.astype(np.float32)],
                       -1)
        return out[0] if one else out

    def reference(self, x, dtype=np.float64):
        """The rule in numpy for one clip x [n]: [ceil(n / hop), n_mels + 2]
        (features.logmel_reference, the tracker's float32 reference -- through
        the path's where there is one -- and reference_channels)."""
        mel = features.logmel_reference(x, self._mel, dtype)
        p = self.tracker.reference(x, np.float32)
        if self.path is not None:
            p = self.path.reference(p.cmnd, p.lag)[0]
        return np.concatenate(
            [mel, self.reference_channels(p.f0).astype(mel.dtype)], -1)

    # ---------------------------------------------------------- the device
    def assemble(self, mel, f0, nframes=None, out=None):
        """One wn_lc_frames launch on device tensors: mel float32 [B, F,
        n_mels] raw log-mel frames and f0 float32 [B, F] -> out float32 [B, F,
        n_mels + 2] (allocated unless given); nframes: a device int32 [B]
        tensor or None.  On mel's device, torch's current stream."""
        import torch
        B, F, M = (int(v) for v in mel.shape)
        if out is None:
            out = torch.empty((B, F, M + 2), dtype=torch.float32,
                              device=mel.device)
        launch(mel, M, M, self.normalizer, f0, self.mode, self.tracker.fmin,
               self.span, nframes, B, F, out, M + 2, M)
        return out

    def __call__(self, audio, lengths=None):
        """Frames of audio [B, T] or [T] (a float array or device tensor):
        device float32 [B, F, n_mels + 2] or [F, n_mels + 2], F = ceil(T /
        hop), without waiting for the device.  lengths ([B] ints, 1 <= n[b]
        <= T): clip b has n[b] real samples; frames f >= ceil(n[b] / hop) are
        zeros.  wn_melspec, the tracker (and the path), one wn_lc_frames."""
        import torch
        if not isinstance(audio, torch.Tensor):
            audio = np.asarray(audio)
            if audio.dtype == object or \
                    not np.issubdtype(audio.dtype, np.floating):
                raise ValueError('spec: audio must be a float array')
        elif not audio.is_floating_point():
            raise ValueError('spec: audio must be floating point')
        one = audio.ndim == 1
        if audio.ndim not in (1, 2) or audio.shape[-1] < 1 or \
                (not one and audio.shape[0] < 1):
            raise ValueError('spec: audio must have shape [B, T] or [T], got '
                             '%s' % (tuple(audio.shape),))
        B, T = (1 if one else int(audio.shape[0])), int(audio.shape[-1])
        if B > 65535 or T > 1 << 30:
            raise ValueError('spec: B <= 65535 and T <= 2^30 are required, '
                             'got [%d, %d]' % (B, T))
        n = check_lengths(lengths, B, T, 'spec')
        _lib.load()
        _lib.require_gpu()
        if isinstance(audio, torch.Tensor) and audio.device.type == 'cuda':
            device = audio.device
        else:
            device = torch.device('cuda', torch.cuda.current_device())
            if not isinstance(audio, torch.Tensor):
                audio = torch.from_numpy(np.ascontiguousarray(audio))
        a = audio.to(device=device, dtype=torch.float32).reshape(B, T)
        with torch.cuda.device(device):
            raw = self.mel(a, n)
            p = (self.path or self.tracker)(a, n)
            nd = None if n is None else torch.from_numpy(
                (-(-n // self.hop)).astype(np.int32)).to(device)
            out = self.assemble(raw, p.f0, nd)
        return out[0] if one else out


def launch(mel, ld_mel, M, normalizer, f0, mode, fmin, span, nframes, B, F,
           out, ld_out, c0):
    """wn_lc_frames on device tensors (mel, f0, nframes may be None; the
    header states the rule), on out's device and torch's current stream."""
    import torch
    shift = scale = None
    lo, hi = -np.inf, np.inf
    if normalizer is not None and mel is not None:
        shift, scale = normalizer.device_tables(out.device)
        lo, hi = normalizer._lo(), normalizer._hi()
    with torch.cuda.device(out.device):
        _lib.call('wn_lc_frames', _lib.ptr(mel), ld_mel, M, _lib.ptr(shift),
                  _lib.ptr(scale), lo, hi, _lib.ptr(f0), mode, float(fmin),
                  float(span), _lib.ptr(nframes), B, F, _lib.ptr(out), ld_out,
                  c0, _lib.stream())


def normalize_resident(frames, n_mels, normalizer):
    """The mel channels [0, n_mels) of resident frames, a contiguous device
    float32 [N, L] with L > n_mels, normalised in place: one wn_lc_frames
    launch without an f0 (one clip of N rows, which the entry splits over
    its workgroups)."""
    N, L = (int(v) for v in frames.shape)
    if N > 1 << 30:
        raise ValueError('the resident frames hold %d rows, wn_lc_frames '
                         'takes 2^30 at most' % N)
    launch(frames, L, n_mels, normalizer, None, 0, 1.0, 1.0, None, 1, N,
           frames, L, n_mels)
