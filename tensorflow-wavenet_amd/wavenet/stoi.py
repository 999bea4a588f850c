"""STOI and ESTOI on the device (csrc/wn_stoi.hip, include/wavenet_stoi.h):
short-time objective intelligibility (Taal, Hendriks, Heusdens, Jensen 2011)
and its extended form (Jensen, Taal 2016) of a generated signal against the
original -- the correlation of the two signals' temporal envelopes in 15
third-octave bands over segments of 30 frames (384 ms), after the frames in
which the original is silent (40 dB below its loudest frame) were removed.

The rule, at 10 kHz (include/wavenet_stoi.h writes out every operation):

  1. both signals are resampled to 10 kHz (resample.Resampler; none at 10 kHz)
  2. frames of 256 samples, hop 128, window w[i] = sin^2(pi (i + 1) / 257)
  3. frame f of the ORIGINAL is kept iff its windowed energy E[f] > max E *
     1e-4; the kept frames of both signals are overlap-added into two
     compacted signals
  4. X[b][i]: the square root of the power of compacted frame i (windowed
     again, DFT length 512) in the bins [L_b, U_b) of band b; Y likewise
  5. per segment of 30 frames, in float64: STOI clips Y at (1 + 10^(15/20)) X
     after matching the band's energy, and averages the correlation
     coefficients of the 15 bands; ESTOI normalises rows, then columns, of the
     15 x 30 blocks and averages the 30 column products
  6. per clip the segments' values are summed; a clip's score is sum /
     segments, the corpus score the mean over the clips that have a segment.

Steps 2 - 4 run in float32, step 5 in float64.  `Stoi.reference` is the rule
for one clip pair in numpy; tests/stoi_ref.py restates it in float64 with
np.fft.rfft.  These are THIS tool's STOI on the stated rule: the resampler is
scipy.signal.resample_poly's design, not Octave's `resample` of the authors'
code, and the last full frame is included, so the third decimal need not match
other implementations.
"""
import numpy as np

from . import _lib, resample
from .emphasis import _audio_arg, _ld, _rows

RATE = 10000
FRAME, HOP, NFFT = 256, 128, 512
BANDS, SEGMENT = 15, 30
CLIP = 10.0 ** (15.0 / 20.0)
RANGE = np.float32(1e-4)                  # 40 dB
EPS = 2.0 ** -52
B_MAX, T_MAX = 65535, 2 ** 30


def band_edges():
    """int [16]: L_0 .. L_14 and U_14, the DFT bins nearest to the edges 150 *
    2^(b / 3) * 2^(-+1 / 6) Hz of the third-octave bands."""
    b = np.arange(BANDS + 1, dtype=np.float64)
    lo = 150.0 * 2.0 ** (b / 3.0) * 2.0 ** (-1.0 / 6.0)
    return np.round(lo * NFFT / RATE).astype(np.int64)


def window():
    i = np.arange(FRAME, dtype=np.float64)
    return (np.sin(np.pi * (i + 1.0) / (FRAME + 1.0)) ** 2).astype(np.float32)


def basis():
    """float32 [2, 512]: cos | sin of 2 pi q / 512."""
    q = np.arange(NFFT, dtype=np.float64)
    return np.stack([np.cos(2.0 * np.pi * q / NFFT),
                     np.sin(2.0 * np.pi * q / NFFT)]).astype(np.float32)


def frames_of(n):
    """Fs of n samples at 10 kHz (an int or an int array)."""
    n = np.asarray(n, np.int64)
    return np.where(n < FRAME, 0, (n - FRAME) // HOP + 1)


def segment_scores(X, Y):
    """Step 5 in float64 numpy: (stoi [S], estoi [S]) of the band amplitudes
    X, Y [15, M] (M >= 30)."""
    X = np.asarray(X).astype(np.float64)
    Y = np.asarray(Y).astype(np.float64)
    S = X.shape[1] - SEGMENT + 1
    st, es = np.zeros(S), np.zeros(S)

    def unit(v, axis):
        v = v - v.sum(axis=axis, keepdims=True) / v.shape[axis]
        return v / (np.sqrt((v * v).sum(axis=axis, keepdims=True)) + EPS)
    for s in range(S):
        x, y = X[:, s:s + SEGMENT], Y[:, s:s + SEGMENT]
        alpha = np.sqrt((x * x).sum(1, keepdims=True)) / \
            (np.sqrt((y * y).sum(1, keepdims=True)) + EPS)
        yc = np.minimum(alpha * y, (1.0 + CLIP) * x)
        st[s] = (unit(x, 1) * unit(yc, 1)).sum(1).sum() / BANDS
        es[s] = (unit(unit(x, 1), 0) * unit(unit(y, 1), 0)).sum() / SEGMENT
    return st, es


class StoiSums(object):
    """What Stoi returns: stoi_sum, estoi_sum (device float64 [B]), segments,
    kept (device int32 [B]); and `frames`, the host's count of frames per clip
    before the silent ones were removed (int64 numpy [B])."""

    def __init__(self, stoi_sum, estoi_sum, segments, kept, frames):
        self.stoi_sum, self.estoi_sum = stoi_sum, estoi_sum
        self.segments, self.kept = segments, kept
        self.frames = np.asarray(frames, np.int64).reshape(-1)

    def __iter__(self):
        return iter((self.stoi_sum, self.estoi_sum, self.segments, self.kept))

    @classmethod
    def cat(cls, parts):
        """The sums of several batches as one (clips in the given order)."""
        import torch
        parts = list(parts)
        if not parts:
            raise ValueError('StoiSums.cat: at least one batch is required')
        return cls(*(torch.cat(t) for t in zip(*parts)),
                   frames=np.concatenate([p.frames for p in parts]))

    def summary(self):
        """The corpus numbers (waits for the device): a clip's score is sum /
        segments, 'stoi' and 'estoi' the means over the clips with segments >
        0 in index order.  No such clip is a ValueError."""
        st, es, sg, kp = (t.detach().cpu().numpy() for t in self)
        keep = [b for b in range(sg.shape[0]) if sg[b] > 0]
        if not keep:
            raise ValueError('summary: no clip has a segment of %d kept '
                             'frames (%.0f ms at 10 kHz)'
                             % (SEGMENT, 1e3 * (HOP * (SEGMENT - 1) + FRAME) /
                                RATE))
        s = e = 0.0
        for b in keep:
            s += float(st[b]) / int(sg[b])
            e += float(es[b]) / int(sg[b])
        return {'stoi': s / len(keep), 'estoi': e / len(keep),
                'clips': len(keep), 'skipped_clips': int(sg.shape[0]) -
                len(keep), 'segments': int(sg.sum()),
                'kept_frames': int(kp.sum()), 'frames': int(self.frames.sum()),
                'sample_rate': RATE}


class Stoi(object):
    """The meter of one sample rate (module docstring).  Every argument is
    checked here, before any library or device is touched."""

    def __init__(self, sample_rate, half_width=10, beta=5.0):
        if not resample._is_int(sample_rate) or sample_rate < 1:
            raise ValueError('sample_rate must be a positive int, got %r'
                             % (sample_rate,))
        self.sample_rate = int(sample_rate)
        self.resampler = None if self.sample_rate == RATE else \
            resample.Resampler(self.sample_rate, RATE, half_width, beta)
        self.half_width, self.beta = int(half_width), float(beta)
        self.window, self.basis = window(), basis()
        self.edges = band_edges()
        self._dev = {}

    def __repr__(self):
        return 'Stoi(%d)' % self.sample_rate

    def settings(self):
        return {'sample_rate': self.sample_rate,
                'half_width': self.half_width, 'beta': self.beta}

    @classmethod
    def from_settings(cls, d):
        keys = {'sample_rate', 'half_width', 'beta'}
        if not isinstance(d, dict) or set(d) != keys:
            raise ValueError('Stoi settings have the keys %s, got %r'
                             % (sorted(keys), d))
        return cls(**d)

    def length10(self, n):
        """Samples at 10 kHz of n samples at sample_rate."""
        return n if self.resampler is None else self.resampler.out_length(n)

    # ------------------------------------------------------ the rule, numpy
    def reference_bands(self, generated, original):
        """Steps 1 - 4 for one clip pair in numpy float32: (X, Y, keep) with X
        (the original's), Y float32 [15, M] and keep bool [Fs]."""
        f32 = np.float32
        g = np.asarray(generated, f32).reshape(-1)
        o = np.asarray(original, f32).reshape(-1)
        if g.shape != o.shape:
            raise ValueError('reference: generated and original must have '
                             'one length, got %d and %d'
                             % (g.shape[0], o.shape[0]))
        if self.resampler is not None and g.shape[0]:
            g, o = self.resampler.reference(g), self.resampler.reference(o)
        w = self.window
        Fs = int(frames_of(o.shape[0]))
        idx = HOP * np.arange(Fs)[:, None] + np.arange(FRAME)[None, :]
        with np.errstate(all='ignore'):
            E = np.zeros(Fs, f32)
            for i in range(FRAME):
                p = (w[i] * o[idx[:, i]]).astype(f32)
                E = (E + (p * p).astype(f32)).astype(f32)
            emax = np.fmax.reduce(E, initial=f32(0)) if Fs else f32(0)
            keep = E > f32(emax * RANGE)
            k = np.nonzero(keep)[0]
            M = k.shape[0]
            out = []
            for sig in (o, g):
                fr = (w[None, :] * sig[idx[k]]).astype(f32)    # [M, 256]
                c = np.zeros((M, FRAME), f32)
                # the earlier frame's addend first
                c[1:, :HOP] = (c[1:, :HOP] + fr[:-1, HOP:]).astype(f32)
                c[:, :HOP] = (c[:, :HOP] + fr[:, :HOP]).astype(f32)
                c[:, HOP:] = (c[:, HOP:] + fr[:, HOP:]).astype(f32)
                c[:-1, HOP:] = (c[:-1, HOP:] + fr[1:, :HOP]).astype(f32)
                v = (c * w[None, :]).astype(f32)
                kb = np.arange(self.edges[0], self.edges[-1])
                re = np.zeros((M, kb.shape[0]), f32)
                im = np.zeros_like(re)
                for jj in range(FRAME):
                    q = (kb * jj) % NFFT
                    re = (re + (self.basis[0, q][None, :] * v[:, jj, None]
                                ).astype(f32)).astype(f32)
                    im = (im + (self.basis[1, q][None, :] * v[:, jj, None]
                                ).astype(f32)).astype(f32)
                P = ((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)
                A = np.zeros((BANDS, M), f32)
                for b in range(BANDS):
                    acc = np.zeros(M, f32)
                    for kk in range(self.edges[b], self.edges[b + 1]):
                        acc = (acc + P[:, kk - self.edges[0]]).astype(f32)
                    A[b] = np.sqrt(acc)
                out.append(A)
        return out[0], out[1], keep

    def reference(self, generated, original):
        """The rule for one clip pair (float [n] each, at sample_rate) in
        numpy: {'stoi_sum', 'estoi_sum', 'segments', 'kept', 'frames'}."""
        X, Y, keep = self.reference_bands(generated, original)
        M = int(keep.sum())
        if M < SEGMENT:
            return {'stoi_sum': 0.0, 'estoi_sum': 0.0, 'segments': 0,
                    'kept': M, 'frames': int(keep.shape[0])}
        st, es = segment_scores(X, Y)
        return {'stoi_sum': float(st.sum()), 'estoi_sum': float(es.sum()),
                'segments': M - SEGMENT + 1, 'kept': M,
                'frames': int(keep.shape[0])}

    # ------------------------------------------------------------ the device
    def _tables(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.window).to(device),
                              torch.from_numpy(self.basis).to(device))
        return self._dev[key]

    def __call__(self, generated, original, lengths=None):
        """generated, original: [B, T] or [T] each (float arrays or device
        tensors at sample_rate, one shape) -> StoiSums, without waiting for
        the device.  lengths ([B] ints, 0 <= n[b] <= T): what lies at or
        behind n[b] is not read."""
        import torch
        what = 'Stoi'
        generated, one, B, T = _audio_arg(generated, what)
        original, _, Bo, To = _audio_arg(original, what)
        if tuple(generated.shape) != tuple(original.shape):
            raise ValueError('%s: generated and original must have one shape, '
                             'got %s and %s' % (what, tuple(generated.shape),
                                                tuple(original.shape)))
        if B > B_MAX or T > T_MAX:
            raise ValueError('%s: B <= 65535 and T <= 2^30 are required, got '
                             'B %d, T %d' % (what, B, T))
        n = resample.check_lengths(lengths, B, T, what)
        lib = _lib.load()
        _lib.require_gpu()
        if self.resampler is not None:
            g10 = self.resampler(generated, n).reshape(B, -1)
            o10 = self.resampler(original, n).reshape(B, -1)
        else:
            g10, o10 = (self._on_device(t, B, T) for t in (generated,
                                                           original))
        device = o10.device
        if g10.device != device:
            raise ValueError('%s: generated on %s, original on %s'
                             % (what, g10.device, device))
        T10 = int(o10.shape[1])
        n10 = None if n is None else \
            np.asarray(self.length10(n.astype(np.int64)), np.int64)
        frames = frames_of(np.full(B, T10) if n10 is None else n10)
        with torch.cuda.device(device):
            nd = None if n10 is None else \
                torch.from_numpy(n10.astype(np.int32)).to(device)
            win, bas = self._tables(device)
            scratch = torch.empty(int(lib.wn_stoi_scratch_bytes(B, T10)) // 8,
                                  dtype=torch.float64, device=device)
            st = torch.empty(B, dtype=torch.float64, device=device)
            es = torch.empty(B, dtype=torch.float64, device=device)
            sg = torch.empty(B, dtype=torch.int32, device=device)
            kp = torch.empty(B, dtype=torch.int32, device=device)
            _lib.call('wn_stoi', _lib.ptr(g10), _ld(g10), _lib.ptr(o10),
                      _ld(o10), _lib.ptr(nd), B, T10, _lib.ptr(win),
                      _lib.ptr(bas), _lib.ptr(scratch), _lib.ptr(st),
                      _lib.ptr(es), _lib.ptr(sg), _lib.ptr(kp), _lib.stream())
        return StoiSums(st, es, sg, kp, frames)

    @staticmethod
    def _on_device(t, B, T):
        import torch
        if not isinstance(t, torch.Tensor):
            t = torch.from_numpy(np.ascontiguousarray(t))
        if t.device.type != 'cuda':
            t = t.to(torch.device('cuda', torch.cuda.current_device()))
        t = t.to(dtype=torch.float32).reshape(B, T)
        return t if _rows(t) else t.contiguous()
