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

`PitchPath` is the smoothing across frames, kept apart from the tracker: a
Viterbi path through the tracker's c' rows on the device (csrc/
wn_pitch_path.hip, include/wavenet_pitch_path.h), which takes the octave
slips of weak-fundamental frames out of the track.
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


def _interpolated_f0(c, tau, sr):
    """Step 5 of the module docstring in float32: f0 of the lag tau on the
    float32 row c."""
    f = np.float32
    a, b, g = c[tau - 1], c[tau], c[tau + 1]
    den = (a - f(2) * b) + g
    delta = f(0)
    if den > 0:
        delta = min(max(f(0.5) * (a - g) / den, f(-0.5)), f(0.5))
    return f(sr) / (f(tau) + delta)


class PitchPath(object):
    """A dynamic-programming (Viterbi) path through the tracker's lag
    candidates over the frames of a clip, on the device (csrc/
    wn_pitch_path.hip; include/wavenet_pitch_path.h states the rule operation
    by operation, `reference` restates it in numpy float32).

    Every frame's voiced state s = 0 .. N - 1 (the lag tau_min + s, N =
    tau_max - tau_min) costs c'[tau] + octave_bias * log2(tau / tau_min), the
    unvoiced state N costs `unvoiced` (0 on a frame the tracker calls
    silent); going from lag k to lag s costs jump * |log2 s - log2 k|, into
    or out of the unvoiced state `switch`.  The cheapest path is returned:
    Pitch(f0, aper, lag, None) like the tracker's, f0 = 0, lag = 0, aper = 1
    on its unvoiced frames.  A detour through unvoiced costs 2 * switch +
    unvoiced (>= jump with the defaults, which are design choices, not tuned
    on speech), and an isolated frame keeps the tracker's own voiced /
    unvoiced decision.

    Calling it tracks audio and decodes the path, in groups of clips so that
    the c' rows plus the predecessor workspace stay under `max_bytes`; clip
    b's bits do not depend on the grouping.  Every argument is checked here,
    before any library or device is touched."""

    def __init__(self, tracker, jump=0.3, octave_bias=0.05, switch=0.2,
                 unvoiced=None, max_bytes=1 << 30):
        if not isinstance(tracker, PitchTracker):
            raise ValueError('tracker must be a PitchTracker, got %r'
                             % (tracker,))
        if unvoiced is None:
            unvoiced = tracker.threshold
        for name, v in (('jump', jump), ('octave_bias', octave_bias),
                        ('switch', switch), ('unvoiced', unvoiced)):
            with np.errstate(over='ignore'):
                if not _is_num(v) or not v >= 0 or \
                        not np.isfinite(np.float32(v)):
                    raise ValueError('%s must be a finite non-negative '
                                     'float32 number, got %r' % (name, v))
        if not float(np.float32(unvoiced)) > 0:
            raise ValueError('unvoiced must be positive, got %r'
                             % (unvoiced,))
        if not _is_int(max_bytes) or max_bytes < 1:
            raise ValueError('max_bytes must be a positive int, got %r'
                             % (max_bytes,))
        self.tracker = tracker
        self.jump, self.octave_bias = float(jump), float(octave_bias)
        self.switch, self.unvoiced = float(switch), float(unvoiced)
        self.max_bytes = int(max_bytes)
        self.last_cost = None
        self._device_tables = {}

    hop = property(lambda self: self.tracker.hop)
    num_states = property(lambda self: self.tracker.tau_max -
                          self.tracker.tau_min)

    def settings(self):
        """The constructor's arguments as a plain dict, the tracker's
        settings under 'tracker' (`from_settings` inverts it exactly)."""
        return dict(tracker=self.tracker.settings(), jump=self.jump,
                    octave_bias=self.octave_bias, switch=self.switch,
                    unvoiced=self.unvoiced, max_bytes=self.max_bytes)

    @classmethod
    def from_settings(cls, d):
        if not isinstance(d, dict) or 'tracker' not in d:
            raise ValueError("pitch path settings need 'tracker', got %r"
                             % (d,))
        d = dict(d)
        return cls(PitchTracker.from_settings(d.pop('tracker')), **d)

    def tables(self):
        """(pen, bias): float32 [tau_max + 1], made in float64 and rounded
        once: pen[k] = jump * log2(max(k, 1)), bias[k] = octave_bias *
        (log2(max(k, 1)) - log2(tau_min)); bias[tau_min] is 0."""
        t = self.tracker
        lg = np.log2(np.maximum(np.arange(t.tau_max + 1), 1)
                     .astype(np.float64))
        return ((self.jump * lg).astype(np.float32),
                (self.octave_bias * (lg - lg[t.tau_min])).astype(np.float32))

    def clip_bytes(self, F):
        """Device bytes one clip of F frames needs: its c' rows and its
        predecessor workspace."""
        t = self.tracker
        return int(F) * (4 * (t.tau_max + 1) + 2 * (self.num_states + 1))

    def __call__(self, audio, lengths=None):
        """Track audio [B, T] or [T] with the tracker (return_cmnd=True) and
        decode the path: Pitch(f0, aper, lag, None) of device tensors [B, F]
        or [F], without waiting for the device.  `lengths` as the tracker
        takes them.  A clip that alone needs more than max_bytes is a
        ValueError naming both sizes, before any launch."""
        import torch
        t = self.tracker
        shape = tuple(getattr(audio, 'shape', None) or np.shape(audio))
        if len(shape) not in (1, 2) or not all(shape):
            t(audio, lengths)                   # (raises ValueError)
            raise ValueError('pitch: audio must have shape [B, T] or [T]')
        B = 1 if len(shape) == 1 else int(shape[0])
        F = t.num_frames(shape[-1])
        need = self.clip_bytes(F)
        if need > self.max_bytes:
            raise ValueError(
                'pitch path: one clip of %d frames needs %d bytes (c\' rows '
                'and predecessors), max_bytes is %d'
                % (F, need, self.max_bytes))
        n = check_lengths(lengths, B, int(shape[-1]), 'pitch')
        group = max(1, min(B, self.max_bytes // need))
        if len(shape) == 1 or group >= B:
            p = t(audio, n, return_cmnd=True)
            return self.decode(p.cmnd, p.lag,
                               None if n is None else -(-n // t.hop))
        parts, costs = [], []
        for g in range(0, B, group):
            ng = None if n is None else n[g:g + group]
            p = t(audio[g:g + group], ng, return_cmnd=True)
            parts.append(self.decode(p.cmnd, p.lag,
                                     None if ng is None else -(-ng // t.hop)))
            costs.append(self.last_cost)
        self.last_cost = torch.cat(costs)
        return Pitch(*(torch.cat(v) for v in list(zip(*parts))[:3]), None)

    path = __call__

    def decode(self, cmnd, lag, nframes=None, return_cost=False):
        """The path alone, on device tensors: cmnd float32 [B, F, tau_max +
        1] or [F, tau_max + 1] and lag int32 [B, F] or [F] as the tracker
        returned them; nframes ([B] ints in [0, F], or a device integer
        tensor, which the kernel clamps): clip b has nframes[b] real frames,
        the others are zeros in every output.  Returns Pitch(f0, aper, lag,
        None) (and with return_cost the float64 device tensor [B] of the
        paths' costs, which `last_cost` holds either way), without waiting
        for the device."""
        import torch
        t = self.tracker
        R, N = t.tau_max + 1, self.num_states
        if not isinstance(cmnd, torch.Tensor) or \
                cmnd.dtype != torch.float32 or cmnd.dim() not in (2, 3) or \
                int(cmnd.shape[-1]) != R or not all(cmnd.shape):
            raise ValueError('decode: cmnd must be a float32 tensor [B, F, '
                             '%d] or [F, %d]' % (R, R))
        if not isinstance(lag, torch.Tensor) or lag.dtype != torch.int32 or \
                lag.shape != cmnd.shape[:-1] or lag.device != cmnd.device:
            raise ValueError('decode: lag must be an int32 tensor %s on '
                             'cmnd\'s device' % (list(cmnd.shape[:-1]),))
        one = cmnd.dim() == 2
        B, F = (1 if one else int(cmnd.shape[0])), int(cmnd.shape[-2])
        if B > 65535 or F > 1 << 20:
            raise ValueError('decode: B <= 65535 and F <= 2^20 are required, '
                             'got [%d, %d]' % (B, F))
        nd = None
        if isinstance(nframes, torch.Tensor):
            if nframes.is_floating_point() or nframes.dtype == torch.bool \
                    or tuple(nframes.shape) != (B,):
                raise ValueError('decode: nframes must be %d integers' % B)
            nd = nframes
        elif nframes is not None:
            nf = np.asarray(nframes)
            if nf.dtype == object or nf.dtype == np.bool_ or \
                    not np.issubdtype(nf.dtype, np.integer) or \
                    nf.shape != (B,) or (nf < 0).any() or (nf > F).any():
                raise ValueError('decode: nframes must be %d integers in '
                                 '[0, %d], got %r' % (B, F, nframes))
            nd = torch.from_numpy(nf.astype(np.int32))
        if cmnd.device.type != 'cuda':
            raise ValueError('decode: cmnd and lag must be device tensors')
        _lib.load()
        _lib.require_gpu()
        device = cmnd.device
        with torch.cuda.device(device):
            if device not in self._device_tables:
                self._device_tables[device] = tuple(
                    torch.from_numpy(v).to(device) for v in self.tables())
            pen, bias = self._device_tables[device]
            if nd is not None:
                nd = nd.to(device=device, dtype=torch.int32).contiguous()
            cmnd, lag = cmnd.contiguous(), lag.contiguous()
            work = torch.empty(2 * B * F * (N + 1), dtype=torch.uint8,
                               device=device)
            f0 = torch.empty((B, F), dtype=torch.float32, device=device)
            aper = torch.empty_like(f0)
            out = torch.empty((B, F), dtype=torch.int32, device=device)
            cost = torch.empty(B, dtype=torch.float64, device=device)
            _lib.call('wn_pitch_path', _lib.ptr(cmnd), _lib.ptr(lag),
                      _lib.ptr(nd), B, F, t.tau_min, t.tau_max,
                      _lib.ptr(pen), _lib.ptr(bias), self.switch,
                      self.unvoiced, t.sample_rate, _lib.ptr(work),
                      _lib.ptr(f0), _lib.ptr(aper), _lib.ptr(out),
                      _lib.ptr(cost), _lib.stream())
        self.last_cost = cost
        p = Pitch(f0[0], aper[0], out[0], None) if one else \
            Pitch(f0, aper, out, None)
        return (p, cost) if return_cost else p

    def reference(self, cmnd, lag, return_vmax=False):
        """The rule of wavenet_pitch_path.h in numpy float32 for one clip:
        cmnd [F, tau_max + 1], lag [F] (the tracker's; 0: a silent frame) ->
        (Pitch of numpy arrays [F], cost as numpy float64); with return_vmax
        also the largest magnitude any intermediate took."""
        f32 = np.float32
        t = self.tracker
        tmin, tmax, N = t.tau_min, t.tau_max, self.num_states
        c = np.ascontiguousarray(cmnd, f32)
        lag_in = np.asarray(lag).reshape(-1)
        if c.ndim != 2 or c.shape[1] != tmax + 1 or \
                lag_in.shape[0] != c.shape[0]:
            raise ValueError('reference: cmnd [F, %d] and lag [F] are '
                             'required' % (tmax + 1))
        F = c.shape[0]
        pen, bias = self.tables()
        p, bs = pen[tmin:tmax], bias[tmin:tmax]
        sw, unv = f32(self.switch), f32(self.unvoiced)
        ar = np.arange(N)
        pred = np.zeros((F, N + 1), np.int64)
        cost, seen = np.float64(0), [0.0]

        def see(*values):
            with np.errstate(invalid='ignore'):
                seen[0] = max([seen[0]] + [float(np.max(np.abs(v)))
                                           for v in values])
        V = U = None
        with np.errstate(invalid='ignore', over='ignore'):
            for f in range(F):
                loc = c[f, tmin:tmax] + bs
                lu = f32(0) if lag_in[f] == 0 else unv
                if f == 0:
                    nV, nU = loc, lu
                else:
                    A, Bk = V - p, V + p
                    # the smallest index of the running minimum, from below
                    # and from above (min is exact: any scan gives these)
                    run = np.minimum.accumulate(A)
                    new = np.ones(N, bool)
                    new[1:] = A[1:] < run[:-1]
                    ia = np.maximum.accumulate(np.where(new, ar, 0))
                    run = np.minimum.accumulate(Bk[::-1])[::-1]
                    new = np.ones(N, bool)
                    new[:-1] = Bk[:-1] <= run[1:]
                    ib = np.minimum.accumulate(
                        np.where(new, ar, N)[::-1])[::-1]
                    L, Rr = A[ia] + p, Bk[ib] - p
                    left = L <= Rr
                    vv = np.where(left, L, Rr)
                    fu = U + sw
                    voiced = vv <= fu
                    pred[f, :N] = np.where(voiced, np.where(left, ia, ib), N)
                    nV = np.where(voiced, vv, fu) + loc
                    kb = int(np.argmin(V))
                    fv = V[kb] + sw
                    stay = U <= fv
                    pred[f, N] = N if stay else kb
                    nU = (U if stay else fv) + lu
                    see(A, Bk, L, Rr, fu, fv)
                see(loc, nV, nU)
                m = min(nV.min(), nU)
                V, U = nV - m, nU - m
                cost = cost + np.float64(m)
        f0 = np.zeros(F, f32)
        aper = np.ones(F, f32)
        out = np.zeros(F, np.int32)
        st = N if F == 0 or U <= V.min() else int(np.argmin(V))
        for f in range(F - 1, -1, -1):
            if st < N:
                tau = tmin + st
                out[f], aper[f] = tau, c[f, tau]
                with np.errstate(all='ignore'):
                    f0[f] = _interpolated_f0(c[f], tau,
                                             f32(t.sample_rate))
            st = int(pred[f, st])
        res = (Pitch(f0, aper, out, None), cost)
        return res + (seen[0],) if return_vmax else res


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
