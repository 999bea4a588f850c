"""Pre-emphasis and de-emphasis on the device: first-order noise shaping for
the 8-bit mu-law signal path (csrc/wn_features.hip).

    pre:  e[t] = x[t] - float32(a * x[t - 1])        x[-1] = 0
    de:   y[t] = e[t] + a * y[t - 1]                  y[-1] = initial (0)

with a = float32(alpha).  The model sees and produces the emphasised signal
e; the quantisation noise of what it generates, white in e, is tilted down by
the inverse filter `de` (by up to 20 log10((1 + a) / (1 - a)) dB at low
frequencies).  Log-mel features are always those of the natural signal x.

`pre` is two float32 roundings per sample, bit for bit `reference_pre`.  `de`
is a blocked scan (one workgroup per clip, chunks of `chunk()` samples); it
agrees with the float64 recurrence within the bound of tests/emph_ref.py, and
a clip's bits depend on its own samples, alpha and `initial` alone.
`reference_de` is the plain sequential float32 loop.  alpha == 0 is the
identity in both.

With `lengths`, what lies at or behind n[b] is not read and comes out as
exact zeros.  train.py --preemphasis stores `entry()` in every checkpoint
under 'emphasis'; generate.py and evaluate.py read it from there.
"""
import numpy as np

from . import _lib
from .features import check_lengths


def _check_alpha(alpha):
    if isinstance(alpha, (bool, np.bool_)) or \
            not isinstance(alpha, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(alpha) < 1.0 or \
            not float(np.float32(alpha)) < 1.0:
        raise ValueError('alpha must be a number in [0, 1) (also as a '
                         'float32), got %r' % (alpha,))
    return float(alpha)


def _audio_arg(audio, what):
    """(audio, one, B, T): a float array or tensor [B, T] or [T]."""
    if hasattr(audio, 'detach'):
        ok = audio.is_floating_point()
    else:
        audio = np.asarray(audio)
        ok = audio.dtype != object and np.issubdtype(audio.dtype, np.floating)
    shape = tuple(int(v) for v in audio.shape)
    if not ok or len(shape) not in (1, 2) or min(shape + (1,)) < 1:
        raise ValueError('%s: audio must be a float array of shape [B, T] or '
                         '[T], got %s %s' % (what, audio.dtype, shape))
    one = len(shape) == 1
    return audio, one, (1 if one else shape[0]), shape[-1]


def _rows(t):
    """Whether the device tensor [B, T] can go to the kernel as it is: unit
    stride inside a clip, clips ld >= T apart."""
    B, T = t.shape
    return t.stride(1) == 1 and (B == 1 or t.stride(0) >= T)


def _ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def prepare(audio, lengths, out, what, alias_ok, checked=False):
    """Checks, then (src [B, T] on the device, dst [B, T], lengths on the
    device or None, one): what a filter over clips (here and in lpc.py) does
    with its audio, lengths and out arguments.  checked: `lengths` is
    check_lengths' result already."""
    audio, one, B, T = _audio_arg(audio, what)
    if out is not None:
        if out is audio and not alias_ok:
            raise ValueError('%s: out must not be audio itself (a '
                             'neighbour\'s input would be overwritten)'
                             % what)
        if not hasattr(out, 'detach') or \
                str(out.dtype) != 'torch.float32' or \
                tuple(out.shape) != tuple(audio.shape) or \
                out.device.type != 'cuda':
            raise ValueError('%s: out must be a float32 device tensor of '
                             'shape %s' % (what, tuple(audio.shape)))
    n = lengths if checked else check_lengths(lengths, B, T, what)
    import torch
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
        dst = torch.empty((B, T), dtype=torch.float32, device=device)
    else:
        if out.device != device:
            raise ValueError('%s: out on %s, audio on %s'
                             % (what, out.device, device))
        dst = out.reshape(B, T) if one else out
        if not _rows(dst) or dst.data_ptr() != out.data_ptr():
            raise ValueError('%s: out needs unit stride inside a clip '
                             'and clips at least T apart' % what)
    if not alias_ok or dst.data_ptr() != src.data_ptr() or \
            _ld(dst) != _ld(src):
        lo_s, lo_d = src.data_ptr(), dst.data_ptr()
        hi_s = lo_s + 4 * ((B - 1) * _ld(src) + T)
        hi_d = lo_d + 4 * ((B - 1) * _ld(dst) + T)
        if lo_s < hi_d and lo_d < hi_s:
            raise ValueError('%s: out overlaps audio' % what)
    nd = None if n is None else torch.from_numpy(n).to(device)
    return src, dst, nd, one


class Emphasis(object):
    """The filter pair of one alpha, 0 <= alpha < 1 (module docstring).
    Every argument is checked before the library or a device is touched."""

    def __init__(self, alpha):
        self.alpha = _check_alpha(alpha)
        self.alpha32 = np.float32(self.alpha)     # what both kernels use

    def __repr__(self):
        return 'Emphasis(%r)' % self.alpha

    def __eq__(self, other):
        return isinstance(other, Emphasis) and other.alpha == self.alpha

    def __ne__(self, other):
        return not self == other

    __hash__ = None

    # ------------------------------------------------------- checkpoint form
    def entry(self):
        """What checkpoints store under 'emphasis'."""
        return {'alpha': self.alpha}

    @classmethod
    def from_entry(cls, d):
        """The Emphasis of a checkpoint's entry; None for None."""
        if d is None:
            return None
        if not isinstance(d, dict) or 'alpha' not in d:
            raise ValueError("an emphasis entry needs 'alpha', got %r" % (d,))
        return cls(d['alpha'])

    @staticmethod
    def chunk():
        """Samples per workgroup iteration of the de-emphasis scan (loads
        the library; no device)."""
        return int(_lib.load().wn_emphasis_chunk())

    # ------------------------------------------------------ the rules, numpy
    def reference_pre(self, audio, lengths=None):
        """`pre` in numpy float32, bit for bit: [B, T] or [T]."""
        x, one, B, T = _audio_arg(np.asarray(audio), 'reference_pre')
        n = check_lengths(lengths, B, T, 'reference_pre')
        x = x.astype(np.float32).reshape(B, T)
        out = x.copy()
        if self.alpha32 != 0:
            prev = np.concatenate([np.zeros((B, 1), np.float32), x[:, :-1]], 1)
            with np.errstate(all='ignore'):
                out = (x - (self.alpha32 * prev).astype(np.float32)
                       ).astype(np.float32)
        if n is not None:
            out = np.where(np.arange(T)[None, :] < n[:, None], out,
                           np.float32(0))
        return out[0] if one else out

    def reference_de(self, audio, lengths=None, initial=None):
        """`de` as the plain sequential float32 loop: [B, T] or [T]."""
        e, one, B, T = _audio_arg(np.asarray(audio), 'reference_de')
        n = check_lengths(lengths, B, T, 'reference_de')
        e = e.astype(np.float32).reshape(B, T)
        y = np.zeros((B, T), np.float32)
        prev = np.zeros(B, np.float32) if initial is None else \
            np.asarray(initial, np.float32).reshape(B).copy()
        a = self.alpha32
        with np.errstate(all='ignore'):
            for t in range(T):
                prev = e[:, t] if a == 0 else \
                    (e[:, t] + (a * prev).astype(np.float32)
                     ).astype(np.float32)
                y[:, t] = prev
        if n is not None:
            y = np.where(np.arange(T)[None, :] < n[:, None], y, np.float32(0))
        return y[0] if one else y

    # ------------------------------------------------------------ the device
    def _prepare(self, audio, lengths, out, what, alias_ok):
        return prepare(audio, lengths, out, what, alias_ok)

    def pre(self, audio, lengths=None, out=None):
        """Pre-emphasised audio [B, T] or [T] (a float array or a device
        tensor): device float32 of the same shape, without waiting for the
        device.  lengths ([B] ints, 1 <= n[b] <= T): what lies at or behind
        n[b] is not read and comes out as zeros.  out: a float32 device
        tensor of audio's shape to write into (unit stride inside a clip);
        it must not be, or overlap, audio."""
        src, dst, nd, one = self._prepare(audio, lengths, out, 'pre', False)
        import torch
        with torch.cuda.device(src.device):
            _lib.call('wn_preemphasis', _lib.ptr(src), _lib.ptr(dst),
                      _ld(src), _ld(dst), int(src.shape[0]),
                      int(src.shape[1]), _lib.ptr(nd), float(self.alpha32),
                      _lib.stream())
        return out if out is not None else (dst[0] if one else dst)

    def de(self, audio, lengths=None, out=None, initial=None,
           return_last=False):
        """De-emphasised audio, as `pre` takes and returns it; out may be
        audio itself.  initial ([B] floats or a device tensor; one float for
        [T]): y[-1] of every clip, default 0.  return_last: also return
        y[n[b] - 1], device float32 [B] (a scalar tensor for [T]) -- the
        `initial` of the piece that follows."""
        shape = tuple(audio.shape) if hasattr(audio, 'shape') else \
            np.shape(audio)
        B = 1 if len(shape) == 1 else int(shape[0]) if shape else 0
        if initial is not None and not hasattr(initial, 'detach'):
            initial = np.asarray(initial)
            if initial.dtype == object or initial.dtype == np.bool_ or \
                    not np.issubdtype(initial.dtype, np.number) or \
                    initial.size != B:
                raise ValueError('de: initial must be %d numbers, got %r'
                                 % (B, initial))
            initial = initial.astype(np.float32).reshape(B)
        elif initial is not None and int(initial.numel()) != B:
            raise ValueError('de: initial must hold %d numbers, got shape %s'
                             % (B, tuple(initial.shape)))
        src, dst, nd, one = self._prepare(audio, lengths, out, 'de', True)
        import torch
        init = None
        if initial is not None:
            if not isinstance(initial, torch.Tensor):
                initial = torch.from_numpy(initial)
            init = initial.to(device=src.device, dtype=torch.float32) \
                .reshape(B).contiguous()
        last = torch.empty(B, dtype=torch.float32, device=src.device) \
            if return_last else None
        with torch.cuda.device(src.device):
            _lib.call('wn_deemphasis', _lib.ptr(src), _lib.ptr(dst),
                      _ld(src), _ld(dst), int(src.shape[0]),
                      int(src.shape[1]), _lib.ptr(nd), _lib.ptr(init),
                      _lib.ptr(last), float(self.alpha32), _lib.stream())
        res = out if out is not None else (dst[0] if one else dst)
        if return_last:
            return res, (last[0] if one else last)
        return res

    def de_ragged(self, waves):
        """De-emphasise a list of device float32 [n_u] clips as ONE ragged
        batch (zero padded, with lengths): a list of new [n_u] tensors."""
        import torch
        n = np.array([int(w.shape[0]) for w in waves], np.int64)
        buf = torch.zeros((len(waves), int(n.max())), dtype=torch.float32,
                          device=waves[0].device)
        for j, w in enumerate(waves):
            buf[j, :n[j]] = w
        self.de(buf, n, out=buf)
        return [buf[j, :n[j]] for j in range(len(waves))]


class DeStream(object):
    """De-emphasis of audio that grows: `feed(audio)` takes everything
    decoded so far (numpy float32 [n], each call a longer prefix-compatible
    array) and returns its de-emphasis as numpy.  What was filtered up to
    the last multiple of the scan's chunk is kept with its carry, so every
    call returns the bits that one call over the whole array gives."""

    def __init__(self, emphasis):
        self.emphasis = emphasis
        self.done = np.zeros(0, np.float32)
        self.last = None

    def feed(self, audio):
        audio = np.asarray(audio, np.float32).reshape(-1)
        k = self.done.shape[0]
        if audio.shape[0] <= k:
            return self.done[:audio.shape[0]].copy()
        y = self.emphasis.de(audio[k:], initial=self.last).cpu().numpy()
        out = np.concatenate([self.done, y])
        C = self.emphasis.chunk()
        keep = out.shape[0] // C * C
        if keep > k:
            self.done = out[:keep]
            self.last = out[keep - 1:keep]
        return out


# ------------------------------------------------------------ command line
def add_cli_flag(p, train=False):
    p.add_argument(
        '--preemphasis', type=float, default=None, metavar='A',
        help=('Train on the pre-emphasised signal e[t] = x[t] - A x[t - 1], '
              '0 <= A < 1 (e.g. 0.97); the features stay those of the '
              'natural signal.  Stored in every checkpoint (\'emphasis\'); '
              'generate.py and evaluate.py apply the inverse filter.  '
              'Default: off.') if train else
        ('The A of the checkpoint\'s pre-emphasis (train.py --preemphasis): '
         'what the model generates is run through the inverse filter '
         'y[t] = e[t] + A y[t - 1] on the device.  Default: the '
         'checkpoint\'s \'emphasis\' entry; 0 switches it off.'))


def from_cli(value, stored=None, continued=False):
    """The Emphasis of --preemphasis `value` (None: absent) and a
    checkpoint's 'emphasis' entry `stored`, or None.  The flag overrides the
    entry, 0 switches it off -- except for a run `continued` in its logdir,
    where a flag that differs from the entry is a ValueError naming both."""
    theirs = Emphasis.from_entry(stored)
    if value is None:
        return theirs
    mine = Emphasis(value)
    if continued:
        have = 0.0 if theirs is None else theirs.alpha
        if have != mine.alpha:
            raise ValueError(
                '--preemphasis %r does not match the checkpoint\'s %r: a run '
                'continued in its logdir keeps its pre-emphasis (start a new '
                'one with --restore_from)' % (mine.alpha, have))
    return mine if mine.alpha != 0 else None
