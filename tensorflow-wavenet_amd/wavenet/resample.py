"""Sample-rate conversion on the device (csrc/wn_resample.hip, include/
wavenet_resample.h): a polyphase FIR resampler by the rational factor up / down
= rate_out / rate_in, reduced.

With m = max(up, down) and Hh = half_width * m the taps are, for i = -Hh .. Hh,

    g[i] = sinc(i / m) * I0(beta * sqrt(1 - (i / Hh)^2)) / I0(beta)
    h[i] = up * g[i] / sum(g)

computed here in float64 (np.sinc, np.i0) and rounded once to float32: a
Kaiser-windowed sinc of cutoff 1 / m, scipy.signal.resample_poly's own default
design (firwin(2 Hh + 1, 1 / m, window=('kaiser', beta)) * up).  A clip of n
samples gives out_length(n) = ceil(n up / down) samples,

    y[k] = sum_j h32[k down - j up] * x[j]

over 0 <= j < n with |k down - j up| <= Hh, j ascending, from +0, every
product rounded to float32 before it is added, no fused multiply-add.
`Resampler.reference` runs that loop in numpy float32; the device matches it
bit for bit.  The clip is taken as zero outside [0, n), as resample_poly takes
it, but a sample that does not exist is never multiplied: a NaN reaches the
outputs whose taps cover it and no other.

up == down (equal rates) is a copy: the windowed sinc is then a unit impulse
only up to rounding (np.sinc of an integer is 1e-17, not 0), and those side
taps would do nothing but carry a NaN to its 2 Hh neighbours.  The taps are
still computed, so `taps` always holds the design.

This is the converter of the metrics (wavenet/stoi.py is defined at 10 kHz).
audio_reader's host resampling stays scipy's: its floats are pinned.
"""
from math import gcd

import numpy as np

from . import _lib
from .emphasis import _audio_arg, _ld, _rows
from .features import _is_int, _is_num

RATIO_MAX = 1024
HALF_WIDTH_MAX = 32
BETA_MAX = 20.0
TAPS_MAX = 65537
B_MAX = 65535
T_MAX = 2 ** 30


def design(up, down, half_width, beta):
    """The float64 taps h[-Hh .. Hh] of the module docstring."""
    m = max(up, down)
    Hh = half_width * m
    i = np.arange(-Hh, Hh + 1, dtype=np.float64)
    arg = 1.0 - (i / Hh) ** 2
    g = np.sinc(i / m) * np.i0(beta * np.sqrt(np.maximum(arg, 0.0))) / \
        np.i0(beta)
    return up * g / g.sum()


def check_lengths(lengths, B, T, what):
    """`lengths` as int32 numpy [B] with 0 <= n[b] <= T (None stays None)."""
    if lengths is None:
        return None
    if hasattr(lengths, 'detach'):
        lengths = lengths.detach().cpu().numpy()
    n = np.asarray(lengths)
    if n.dtype == object or n.dtype == np.bool_ or \
            not np.issubdtype(n.dtype, np.integer) or n.shape != (B,):
        raise ValueError('%s: lengths must be %d integers, got %s %s'
                         % (what, B, n.dtype, list(n.shape)))
    if (n < 0).any() or (n > T).any():
        raise ValueError('%s: lengths must lie in [0, T] = [0, %d], got %s'
                         % (what, T, n.tolist()))
    return n.astype(np.int32)


class Resampler(object):
    """The converter of one pair of rates (module docstring).  Every argument
    is checked here, before any library or device is touched."""

    def __init__(self, rate_in, rate_out, half_width=10, beta=5.0):
        for name, v in (('rate_in', rate_in), ('rate_out', rate_out)):
            if not _is_int(v) or v < 1:
                raise ValueError('%s must be a positive int, got %r'
                                 % (name, v))
        if not _is_int(half_width) or not 1 <= half_width <= HALF_WIDTH_MAX:
            raise ValueError('half_width must be an int in [1, %d], got %r'
                             % (HALF_WIDTH_MAX, half_width))
        if not _is_num(beta) or not 0 <= beta <= BETA_MAX:
            raise ValueError('beta must lie in [0, %g], got %r'
                             % (BETA_MAX, beta))
        g = gcd(int(rate_in), int(rate_out))
        up, down = int(rate_out) // g, int(rate_in) // g
        if up > RATIO_MAX or down > RATIO_MAX:
            raise ValueError('rate_out / rate_in = %d / %d: up, down <= %d '
                             'is required' % (up, down, RATIO_MAX))
        Hh = int(half_width) * max(up, down)
        if 2 * Hh + 1 > TAPS_MAX:
            raise ValueError('2 * half_width * max(up, down) + 1 = %d taps: '
                             'at most %d' % (2 * Hh + 1, TAPS_MAX))
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        self.half_width, self.beta = int(half_width), float(beta)
        self.up, self.down, self.Hh = up, down, Hh
        self.taps64 = design(up, down, self.half_width, self.beta)
        self.taps = self.taps64.astype(np.float32)
        # the device's table (wavenet_resample.h): phase r at r * LPS
        self.LP = (2 * Hh + up) // up
        self.LPS = self.LP | 1
        tab = np.zeros((up, self.LPS), np.float32)
        for r in range(up):
            row = self.taps[r::up]
            tab[r, :row.shape[0]] = row
        self.table = tab
        self._dev = {}

    def __repr__(self):
        return 'Resampler(%d, %d, half_width=%d, beta=%r)' % (
            self.rate_in, self.rate_out, self.half_width, self.beta)

    def settings(self):
        return {'rate_in': self.rate_in, 'rate_out': self.rate_out,
                'half_width': self.half_width, 'beta': self.beta}

    @classmethod
    def from_settings(cls, d):
        keys = {'rate_in', 'rate_out', 'half_width', 'beta'}
        if not isinstance(d, dict) or set(d) != keys:
            raise ValueError('Resampler settings have the keys %s, got %r'
                             % (sorted(keys), d))
        return cls(**d)

    def out_length(self, n):
        """ceil(n up / down), of an int or an int array."""
        if isinstance(n, np.ndarray):
            return -(-n.astype(np.int64) * self.up // self.down)
        return -(-int(n) * self.up // self.down)

    def _shape(self, B, T, what):
        if B > B_MAX or T > T_MAX or self.out_length(T) > T_MAX:
            raise ValueError('%s: B <= 65535, T <= 2^30 and out_length(T) <= '
                             '2^30 are required, got B %d, T %d'
                             % (what, B, T))

    # ------------------------------------------------------ the rule, numpy
    def reference(self, audio, lengths=None):
        """`__call__` in numpy float32, bit for bit: [B, out_length(T)] or
        [out_length(T)]."""
        f32 = np.float32
        x, one, B, T = _audio_arg(np.asarray(audio), 'reference')
        self._shape(B, T, 'reference')
        n = check_lengths(lengths, B, T, 'reference')
        x = np.asarray(x, f32).reshape(B, T)
        up, down, Hh = self.up, self.down, self.Hh
        out = np.zeros((B, self.out_length(T)), f32)
        for b in range(B):
            nb = T if n is None else int(n[b])
            no = self.out_length(nb)
            if no == 0:
                continue
            if up == down:
                out[b, :no] = x[b, :nb]
                continue
            c = np.arange(no, dtype=np.int64) * down + Hh
            jh = c // up
            r = c - jh * up
            acc = np.zeros(no, f32)
            with np.errstate(all='ignore'):
                for t in range(self.LP - 1, -1, -1):       # j ascending
                    i, j = r + t * up, jh - t
                    ok = (i <= 2 * Hh) & (j >= 0) & (j < nb)
                    prod = (self.taps[np.minimum(i, 2 * Hh)] *
                            x[b, np.clip(j, 0, nb - 1)]).astype(f32)
                    acc = np.where(ok, (acc + prod).astype(f32), acc)
            out[b, :no] = acc
        return out[0] if one else out

    # ------------------------------------------------------------ the device
    @staticmethod
    def tile():
        """Outputs per workgroup of the kernel (loads the library; no
        device)."""
        return int(_lib.load().wn_resample_tile())

    def _table(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.table).to(device)
        return self._dev[key]

    def __call__(self, audio, lengths=None, out=None):
        """audio [B, T] or [T] (a float array or a device tensor) at rate_in
        -> device float32 [B, out_length(T)] or [out_length(T)] at rate_out,
        without waiting for the device.  lengths ([B] ints, 0 <= n[b] <= T):
        what lies at or behind n[b] is not read, and the outputs at or behind
        out_length(n[b]) are exact zeros.  out: a float32 device tensor of the
        result's shape to write into (unit stride inside a clip); it must not
        overlap audio."""
        import torch
        what = 'Resampler'
        audio, one, B, T = _audio_arg(audio, what)
        self._shape(B, T, what)
        To = self.out_length(T)
        shape = (To,) if one else (B, To)
        if out is not None and (
                not hasattr(out, 'detach') or
                str(out.dtype) != 'torch.float32' or
                tuple(out.shape) != shape or out.device.type != 'cuda'):
            raise ValueError('%s: out must be a float32 device tensor of '
                             'shape %s' % (what, shape))
        n = check_lengths(lengths, B, T, what)
        _lib.load()
        _lib.require_gpu()
        if isinstance(audio, torch.Tensor) and audio.device.type == 'cuda':
            device = audio.device
        else:
            device = out.device if out is not None else \
                torch.device('cuda', torch.cuda.current_device())
            if not isinstance(audio, torch.Tensor):
                audio = torch.from_numpy(np.ascontiguousarray(audio))
        src = audio.to(device=device, dtype=torch.float32).reshape(B, T)
        if not _rows(src):
            src = src.contiguous()
        if out is None:
            dst = torch.empty((B, To), dtype=torch.float32, device=device)
        else:
            if out.device != device:
                raise ValueError('%s: out on %s, audio on %s'
                                 % (what, out.device, device))
            dst = out.reshape(B, To) if one else out
            if not _rows(dst) or dst.data_ptr() != out.data_ptr():
                raise ValueError('%s: out needs unit stride inside a clip '
                                 'and clips at least out_length(T) apart'
                                 % what)
            lo_s, lo_d = src.data_ptr(), dst.data_ptr()
            hi_s = lo_s + 4 * ((B - 1) * _ld(src) + T)
            hi_d = lo_d + 4 * ((B - 1) * _ld(dst) + To)
            if lo_s < hi_d and lo_d < hi_s:
                raise ValueError('%s: out overlaps audio' % what)
        with torch.cuda.device(device):
            nd = None if n is None else torch.from_numpy(n).to(device)
            _lib.call('wn_resample', _lib.ptr(src), _ld(src), _lib.ptr(nd), B,
                      T, self.up, self.down, self.Hh,
                      _lib.ptr(self._table(device)), _lib.ptr(dst), _ld(dst),
                      _lib.stream())
        return out if out is not None else (dst[0] if one else dst)
