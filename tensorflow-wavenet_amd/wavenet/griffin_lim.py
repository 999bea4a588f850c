"""Griffin-Lim baseline on the device (csrc/wn_griffin_lim.hip, include/
wavenet_griffin_lim.h): a complex STFT on the log-mel front end's frame grid,
its least-squares inverse, mel inversion and the Fast Griffin-Lim loop.

The grid is features.MelSpec's: F = ceil(n / hop) frames for a clip of n
samples, frame f centred at f * hop + hop // 2, zeros outside [0, n), a periodic
Hann window of win_length centred in n_fft samples.  No reflection at the
edges: the numbers differ from torch.stft(center=True)'s there.

    S = stft(x)           [F, n_fft // 2 + 1] complex, the e^{-i} DFT
    x = istft(S)          (sum_f w y_f) / (sum_f w^2), y_f the inverse DFT of
                          frame f; zero where sum w^2 <= 1e-8
    A = sqrt(max(pinv(melw) @ exp(logmel), 0))

pinv-and-clip is NOT a non-negative least squares solution: mel(A^2) differs
from the mel frames that went in, so the baseline's own log-mel error is not
zero even where the loop has converged.

The loop (Perraudin, Balazs, Sondergaard 2013), alpha = momentum:

    c_0 = A * exp(i phi),  t_0 = c_0
    x   = istft(c_{i-1})
    S   = stft(x);  t_i = A * S / |S|  (A where |S|^2 <= 1e-30)
    c_i = t_i + alpha * (t_i - t_{i-1})          i = 1 .. iterations
    result = istft(t_N)

alpha = 0 is plain Griffin-Lim.  phi is 2 pi p / 1024 with p a counter-based
draw from (seed, the clip's key, frame, bin), zero at bin 0 and at the Nyquist
bin: a clip's waveform does not depend on the batch it is run in.
"""
import numpy as np

from . import _lib, features
from .spectral import _lengths_arg, _signal_arg

ITERATIONS_MAX = 4096
PHASES = 1024
SEED_XOR = 0x6772696666696E4C
DEN_FLOOR = 1e-8
M2_FLOOR = 1e-30
INITS = ('random', 'zero')
KEY_MAX = 1 << 24
_M64 = (1 << 64) - 1


def phase_table():
    """float32 [1024, 2]: (cos, sin) of 2 pi p / 1024, rounded from float64."""
    ang = 2.0 * np.pi * np.arange(PHASES, dtype=np.float64) / PHASES
    tab = np.stack([np.cos(ang), np.sin(ang)], -1)
    tab[0] = (1.0, 0.0)
    return tab.astype(np.float32)


def _splitmix64(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def phase_indices(seed, key, F, n_bins, init='random'):
    """int [F, n_bins]: wn_gl_init's p (draw_bits of csrc/wn_common.h in
    uint64 numpy; bin 0 and the Nyquist bin get 0)."""
    p = np.zeros((F, n_bins), np.int64)
    if init == 'random':
        with np.errstate(over='ignore'):
            ctr = np.uint64((int(key) << 40) & _M64) | \
                np.arange(F * n_bins, dtype=np.uint64)
            bits = _splitmix64(np.uint64((int(seed) ^ SEED_XOR) & _M64) ^
                               _splitmix64(ctr))
        p = (bits & np.uint64(PHASES - 1)).astype(np.int64).reshape(F, n_bins)
        p[:, 0] = p[:, -1] = 0
    return p


def mel_pinv(spec):
    """(pinv64, pinv): the float64 pseudo-inverse [n_bins][n_mels] of the
    spec's own filterbank, and the same rounded to float32 as the device gets
    it (mel inversion here and in lpc.py)."""
    pinv64 = np.linalg.pinv(spec.melw64)
    return pinv64, np.ascontiguousarray(pinv64.astype(np.float32))


class GriffinLim(object):
    """The Griffin-Lim baseline of one front-end setting.  Every argument is
    checked here, before any library or device is touched."""

    def __init__(self, spec, iterations=32, momentum=0.99, seed=0,
                 init='random', max_bytes=1 << 30):
        if not isinstance(spec, features.MelSpec):
            raise ValueError('GriffinLim: spec must be a features.MelSpec '
                             "(for a MelPitchSpec pass its .mel), got %r"
                             % (type(spec).__name__,))
        if not features._is_int(iterations) or \
                not 0 <= iterations <= ITERATIONS_MAX:
            raise ValueError('iterations must be an int in [0, %d], got %r'
                             % (ITERATIONS_MAX, iterations))
        if not features._is_num(momentum) or not 0 <= momentum < 1 or \
                not np.float32(momentum) < 1:
            raise ValueError('momentum must lie in [0, 1), got %r'
                             % (momentum,))
        if not features._is_int(seed) or not 0 <= seed <= _M64:
            raise ValueError('seed must be an int in [0, 2^64), got %r'
                             % (seed,))
        if init not in INITS:
            raise ValueError('init must be one of %s, got %r'
                             % (', '.join(INITS), init))
        if not features._is_int(max_bytes) or max_bytes < 1:
            raise ValueError('max_bytes must be a positive int, got %r'
                             % (max_bytes,))
        self.spec = spec
        self.iterations, self.momentum = int(iterations), float(momentum)
        self.seed, self.init, self.max_bytes = int(seed), init, int(max_bytes)
        self.n_fft, self.hop, self.n_bins = spec.n_fft, spec.hop, spec.n_bins
        self.n_mels = spec.n_mels
        self.pinv64, self.pinv = mel_pinv(spec)
        self.tab = phase_table()
        self.last_trace = None
        self._dev = {}

    def settings(self):
        spec = self.spec.with_normalizer(None).settings()
        return dict(spec=spec, iterations=self.iterations,
                    momentum=self.momentum, seed=self.seed, init=self.init,
                    max_bytes=self.max_bytes)

    @classmethod
    def from_settings(cls, d):
        keys = {'spec', 'iterations', 'momentum', 'seed', 'init', 'max_bytes'}
        if not isinstance(d, dict) or set(d) != keys or \
                not isinstance(d['spec'], dict):
            raise ValueError('GriffinLim settings have the keys %s, got %r'
                             % (sorted(keys), d))
        d = dict(d)
        return cls(features.MelSpec(**d.pop('spec')), **d)

    def bytes_per_clip(self, F):
        """Device bytes one clip of F frames takes in a run: A, c, t and the
        inverse's scratch."""
        return F * (self.n_bins * (4 + 8 + 8) + self.n_fft * 4)

    # ---- device plumbing -------------------------------------------------
    def _tables(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.pinv).to(device),
                              torch.from_numpy(self.tab).to(device))
        return self._dev[key]

    def _grid(self, B, T, what):
        if B > 65535 or T > 2 ** 30:
            raise ValueError('%s: B <= 65535 and T <= 2^30 are required, got '
                             'B %d, T %d' % (what, B, T))

    @staticmethod
    def _device_of(t):
        import torch
        if isinstance(t, torch.Tensor) and t.device.type == 'cuda':
            return t.device
        return torch.device('cuda', torch.cuda.current_device())

    def _stft(self, x, nd, out):
        B, T = (int(v) for v in x.shape)
        win, basis, _ = self.spec.device_tables(x.device)
        _lib.call('wn_stft', _lib.ptr(x), int(x.stride(0)), B, T, _lib.ptr(nd),
                  _lib.ptr(win), _lib.ptr(basis), self.n_fft, self.hop,
                  self.n_bins, _lib.ptr(out), _lib.stream())

    def _istft(self, c, nd, scratch, x):
        B, T = (int(v) for v in x.shape)
        win, basis, _ = self.spec.device_tables(x.device)
        _lib.call('wn_istft', _lib.ptr(c), B, T, _lib.ptr(nd), _lib.ptr(win),
                  _lib.ptr(basis), self.n_fft, self.hop, self.n_bins,
                  _lib.ptr(scratch), _lib.ptr(x), int(x.stride(0)),
                  _lib.stream())

    def _project(self, x, nd, A, t, c, alpha, trace, parts):
        B, T = (int(v) for v in x.shape)
        win, basis, _ = self.spec.device_tables(x.device)
        _lib.call('wn_gl_project', _lib.ptr(x), int(x.stride(0)), B, T,
                  _lib.ptr(nd), _lib.ptr(win), _lib.ptr(basis), self.n_fft,
                  self.hop, self.n_bins, _lib.ptr(A), _lib.ptr(t), alpha,
                  _lib.ptr(t), _lib.ptr(c), _lib.ptr(trace),
                  None if trace is None else _lib.ptr(parts), _lib.stream())

    def _scratch(self, B, T, device):
        import torch
        lib = _lib.load()
        nbytes = lib.wn_istft_scratch_bytes(B, T, self.n_fft, self.hop)
        return torch.empty(nbytes // 4, dtype=torch.float32, device=device)

    # ---- the primitives --------------------------------------------------
    def stft(self, audio, lengths=None):
        """complex64 device tensor [B, F, n_bins] ([F, n_bins] for [T]) of
        audio [B, T] or [T], F = ceil(T / hop), without waiting for the
        device.  lengths ([B] ints in [0, T]): what lies behind them is not
        read, frames behind ceil(n[b] / hop) are zeros."""
        import torch
        what = 'stft'
        a = _signal_arg(audio, what)
        one = a.ndim == 1
        B, T = (1 if one else int(a.shape[0])), int(a.shape[-1])
        self._grid(B, T, what)
        n = _lengths_arg(lengths, B, T, what)
        _lib.load()
        _lib.require_gpu()
        device = self._device_of(a)
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(a))
        x = a.to(device=device, dtype=torch.float32).reshape(B, T).contiguous()
        with torch.cuda.device(device):
            nd = None if n is None else torch.from_numpy(n).to(device)
            F = self.spec.num_frames(T)
            out = torch.empty((B, F, self.n_bins, 2), dtype=torch.float32,
                              device=device)
            self._stft(x, nd, out)
        out = torch.view_as_complex(out)
        return out[0] if one else out

    def _spec_arg(self, spec, what):
        import torch
        if not isinstance(spec, torch.Tensor):
            spec = np.asarray(spec)
            if spec.dtype.kind != 'c':
                raise ValueError('%s: a complex array is required, got %s'
                                 % (what, spec.dtype))
            spec = torch.from_numpy(np.ascontiguousarray(
                spec.astype(np.complex64)))
        elif not spec.is_complex():
            raise ValueError('%s: a complex tensor is required, got %s'
                             % (what, spec.dtype))
        if spec.ndim not in (2, 3) or spec.shape[-1] != self.n_bins or \
                min(spec.shape) < 1:
            raise ValueError('%s: [B, F, %d] or [F, %d] is required, got %s'
                             % (what, self.n_bins, self.n_bins,
                                tuple(spec.shape)))
        return spec

    def istft(self, spec, lengths=None):
        """float32 device tensor [B, T] ([T] for [F, n_bins]), T = F * hop cut
        to max(lengths), of a complex spectrogram, without waiting for the
        device: the least-squares inverse of `stft` (module docstring)."""
        import torch
        what = 'istft'
        s = self._spec_arg(spec, what)
        one = s.ndim == 2
        B, F = (1 if one else int(s.shape[0])), int(s.shape[-2])
        T = F * self.hop
        self._grid(B, T, what)
        n = _lengths_arg(lengths, B, T, what)
        _lib.load()
        _lib.require_gpu()
        device = self._device_of(s)
        s = torch.view_as_real(s.to(device=device, dtype=torch.complex64)
                               .reshape(B, F, self.n_bins).contiguous())
        with torch.cuda.device(device):
            nd = None if n is None else torch.from_numpy(n).to(device)
            x = torch.empty((B, T), dtype=torch.float32, device=device)
            self._istft(s, nd, self._scratch(B, T, device), x)
        if n is not None:
            x = x[:, :max(int(n.max()), 1)]
        return x[0] if one else x

    def magnitude(self, frames, nframes=None):
        """float32 device tensor [B, F, n_bins] ([F, n_bins]) of linear
        magnitudes from RAW log-mel frames (natural log of power, MelSpec's
        output without a normaliser), without waiting for the device."""
        import torch
        what = 'magnitude'
        frames, one, B, F = features._frames_arg(frames, self.n_mels, what)
        n = features._nframes_arg(nframes, B, F, what)
        if B > 65535:
            raise ValueError('%s: B <= 65535 is required, got %d' % (what, B))
        _lib.load()
        _lib.require_gpu()
        src = features._to_device(frames, B, F, self.n_mels)
        with torch.cuda.device(src.device):
            nd = None if n is None else torch.from_numpy(n).to(src.device)
            out = torch.empty((B, F, self.n_bins), dtype=torch.float32,
                              device=src.device)
            self._magnitude(src, nd, out)
        return out[0] if one else out

    def _magnitude(self, src, nd, out):
        B, F = int(src.shape[0]), int(src.shape[1])
        pinv, _ = self._tables(src.device)
        _lib.call('wn_mel_to_magnitude', _lib.ptr(src), B, F, self.n_mels,
                  _lib.ptr(nd), _lib.ptr(pinv), self.n_bins, _lib.ptr(out),
                  _lib.stream())

    def initial(self, A, keys=None):
        """complex64 device tensor of A's shape: the starting spectrum of A
        (device float32 [B, F, n_bins]) under this seed and init."""
        import torch
        B, F = int(A.shape[0]), int(A.shape[1])
        k = self._keys_arg(keys, B, 'initial')
        _lib.load()
        _lib.require_gpu()
        with torch.cuda.device(A.device):
            c = torch.empty((B, F, self.n_bins, 2), dtype=torch.float32,
                            device=A.device)
            self._init(A.contiguous(), torch.from_numpy(k).to(A.device), c)
        return torch.view_as_complex(c)

    def _init(self, A, kd, c):
        B, F = int(A.shape[0]), int(A.shape[1])
        _, tab = self._tables(A.device)
        _lib.call('wn_gl_init', _lib.ptr(A), B, F, self.n_bins, _lib.ptr(kd),
                  self.seed, INITS.index(self.init), _lib.ptr(tab),
                  _lib.ptr(c), _lib.stream())

    @staticmethod
    def _keys_arg(keys, B, what):
        if keys is None:
            return np.arange(B, dtype=np.int64)
        k = np.asarray(keys)
        if k.dtype == object or k.dtype == np.bool_ or \
                not np.issubdtype(k.dtype, np.integer) or k.shape != (B,) or \
                (k < 0).any() or (k >= KEY_MAX).any():
            raise ValueError('%s: keys must be %d integers in [0, 2^24), got '
                             '%r' % (what, B, keys))
        return k.astype(np.int64)

    # ---- the loop --------------------------------------------------------
    def __call__(self, frames, lengths=None, nframes=None, keys=None,
                 return_trace=False):
        """Waveforms, device float32 [B, T] ([T] for [F, n_mels] frames), from
        RAW log-mel frames [B, F, n_mels] or [F, n_mels], without waiting for
        the device.  T = F * hop, cut to max(lengths) when lengths ([B] ints in
        [0, F * hop]) are given; nframes ([B] ints in [0, F]) alone stands for
        lengths = nframes * hop, and with lengths it must be their
        ceil(lengths / hop).  keys ([B] ints in [0, 2^24), default the clip's
        index in the call) name the clips' phase draws.  Clips run in groups
        that keep A, c, t and the scratch under max_bytes; a clip's bits do
        not depend on the grouping.  max_bytes does not bound the call's whole
        device memory: the frames and the [B, T] result of all clips lie
        outside it.  With return_trace the result is (waves,
        trace) and `last_trace` is set: device float64 [iterations + 1, B, 2],
        per clip (sum (|S_i| - A)^2, sum A^2) with S_i the STFT of
        istft(c_i), entry `iterations` that of the result."""
        import torch
        what = 'griffin_lim'
        frames, one, B, F = features._frames_arg(frames, self.n_mels, what)
        T = F * self.hop
        self._grid(B, T, what)
        n = _lengths_arg(lengths, B, T, what)
        nf = features._nframes_arg(nframes, B, F, what)
        if n is None and nf is not None:
            n = (nf.astype(np.int64) * self.hop).astype(np.int32)
        if n is not None and nf is not None and \
                (nf != -(-n // self.hop)).any():
            raise ValueError('%s: nframes %s are not ceil(lengths / hop) = %s'
                             % (what, nf.tolist(),
                                (-(-n // self.hop)).tolist()))
        if n is not None:
            nf = (-(-n // self.hop)).astype(np.int32)
        k = self._keys_arg(keys, B, what)
        per = self.bytes_per_clip(F)
        if per > self.max_bytes:
            raise ValueError('%s: one clip of %d frames takes %d bytes, '
                             'max_bytes is %d' % (what, F, per,
                                                  self.max_bytes))
        G = min(B, self.max_bytes // per)
        lib = _lib.load()
        _lib.require_gpu()
        src = features._to_device(frames, B, F, self.n_mels)
        device = src.device
        N = self.iterations
        alpha = float(np.float32(self.momentum))
        with torch.cuda.device(device):
            x = torch.empty((B, T), dtype=torch.float32, device=device)
            trace = torch.empty((N + 1, B, 2), dtype=torch.float64,
                                device=device) if return_trace else None
            nd = None if n is None else torch.from_numpy(n).to(device)
            nfd = None if nf is None else torch.from_numpy(nf).to(device)
            kd = torch.from_numpy(k).to(device)
            A = torch.empty((G, F, self.n_bins), dtype=torch.float32,
                            device=device)
            c = torch.empty((G, F, self.n_bins, 2), dtype=torch.float32,
                            device=device)
            t = torch.empty_like(c)
            scratch = self._scratch(G, T, device)
            parts = torch.empty(lib.wn_gl_project_partials(G, T, self.hop),
                                dtype=torch.float64, device=device) \
                if return_trace else None
            for g0 in range(0, B, G):
                g1 = min(B, g0 + G)
                g = g1 - g0
                Ag, cg, tg, xg = A[:g], c[:g], t[:g], x[g0:g1]
                ng = None if nd is None else nd[g0:g1]
                self._magnitude(src[g0:g1], None if nfd is None
                                else nfd[g0:g1], Ag)
                self._init(Ag, kd[g0:g1], cg)
                tg.copy_(cg)
                for i in range(N):
                    self._istft(cg, ng, scratch, xg)
                    self._project(xg, ng, Ag, tg, cg, alpha,
                                  None if trace is None else trace[i, g0:g1],
                                  parts)
                self._istft(tg, ng, scratch, xg)
                if trace is not None:
                    # (c and t are free now: the result's own numbers)
                    self._project(xg, ng, Ag, tg, cg, 0.0, trace[N, g0:g1],
                                  parts)
        if n is not None:
            x = x[:, :max(int(n.max()), 1)]
        x = x[0] if one else x
        if return_trace:
            self.last_trace = trace
            return x, trace
        return x

    # ---- the rule in numpy float32 -----------------------------------------
    def _ref_frames(self, n):
        N, hop = self.n_fft, self.hop
        Fb = self.spec.num_frames(n)
        pos = (np.arange(Fb) * hop + hop // 2 - N // 2)[:, None] + \
            np.arange(N)[None, :]
        return pos, (pos >= 0) & (pos < n)

    def _ref_basis(self):
        if not hasattr(self, '_basis32'):
            cos, sin = (t.astype(np.float32) for t in self.spec.basis64())
            cos[:, -1] = np.where(np.arange(self.n_fft) % 2, -1.0, 1.0)
            self._basis32 = (cos, sin)
        return self._basis32

    def reference_stft(self, x):
        """(re, im) float32 [Fb, n_bins] of ONE clip x [n]: wn_stft's rule."""
        f32 = np.float32
        x = np.asarray(x, f32).reshape(-1)
        n = x.shape[0]
        pos, ok = self._ref_frames(n)
        cos, sin = self._ref_basis()
        fr = np.where(ok, x[np.clip(pos, 0, max(n - 1, 0))] if n else f32(0),
                      f32(0)).astype(f32) * self.spec.window[None, :]
        re, im = fr @ cos, -(fr @ sin)
        im[:, 0] = im[:, -1] = 0
        return re.astype(f32), im.astype(f32)

    def reference_istft(self, re, im, n):
        """float32 [n] from (re, im) [Fb, n_bins]: wn_istft's rule."""
        f32 = np.float32
        N, hop, h = self.n_fft, self.hop, self.n_fft // 2
        re, im = np.asarray(re, f32), np.asarray(im, f32)
        cos, sin = self._ref_basis()
        win = self.spec.window
        a = re[:, :h].copy()
        a[:, 0] *= f32(0.5)
        b = -im[:, :h]
        b[:, 0] = f32(0.5) * re[:, h]
        s = sin[:, :h].copy()
        s[:, 0] = cos[:, -1]
        y = ((a @ cos[:, :h].T + b @ s.T).astype(f32) * f32(2.0 / N)) \
            .astype(f32)
        v = y * win[None, :]
        pos, ok = self._ref_frames(n)
        num, den = np.zeros(n, f32), np.zeros(n, f32)
        w2 = win * win
        for f in range(pos.shape[0]):
            m = ok[f]
            num[pos[f][m]] += v[f][m]
            den[pos[f][m]] += w2[m]
        with np.errstate(all='ignore'):
            return np.where(den > f32(DEN_FLOOR), num / den, f32(0)) \
                .astype(f32)

    def reference_magnitude(self, frames):
        """float32 [F, n_bins] from raw log-mel [F, n_mels]."""
        f32 = np.float32
        with np.errstate(all='ignore'):
            M = np.exp(np.asarray(frames, f32))
            P = (M @ self.pinv.T).astype(f32)
            return np.sqrt(np.where(P < 0, f32(0), P)).astype(f32)

    def reference_initial(self, A, key=0):
        """(re, im) float32 of the starting spectrum of ONE clip's A: bit for
        bit the device's."""
        A = np.asarray(A, np.float32)
        p = phase_indices(self.seed, key, A.shape[0], self.n_bins, self.init)
        return A * self.tab[p, 0], A * self.tab[p, 1]

    def reference_project(self, x, A, tre, tim, alpha=None):
        """((t_re, t_im), (c_re, c_im), (err, a2)) of one clip: wn_gl_project's
        rule."""
        f32 = np.float32
        alpha = f32(self.momentum if alpha is None else alpha)
        A = np.asarray(A, f32)
        re, im = self.reference_stft(x)
        with np.errstate(all='ignore'):
            m2 = re * re + im * im
            big = m2 > f32(M2_FLOOR)
            r = A / np.sqrt(np.where(big, m2, f32(1)))
            ntre = np.where(big, re * r, A).astype(f32)
            ntim = np.where(big, im * r, f32(0)).astype(f32)
            cre = ntre + alpha * (ntre - tre)
            cim = ntim + alpha * (ntim - tim)
            g = (np.sqrt(m2) - A).astype(np.float64)
        return (ntre, ntim), (cre.astype(f32), cim.astype(f32)), \
            (float((g * g).sum()), float((A.astype(np.float64) ** 2).sum()))

    def reference(self, frames, n, key=0, return_trace=False):
        """The whole rule for ONE clip in numpy float32 (the tables rounded
        from float64, as the device gets them): float32 [n] from raw log-mel
        [F, n_mels], F >= ceil(n / hop).  With return_trace also float64
        [iterations + 1, 2]."""
        frames = np.asarray(frames, np.float32)
        Fb = self.spec.num_frames(n)
        if frames.ndim != 2 or frames.shape[1] != self.n_mels or \
                frames.shape[0] < Fb:
            raise ValueError('reference: [F, %d] frames with F >= %d are '
                             'required, got %s' % (self.n_mels, Fb,
                                                   frames.shape))
        A = self.reference_magnitude(frames[:Fb])
        cre, cim = self.reference_initial(A, key)
        tre, tim = cre, cim
        trace = []
        for _ in range(self.iterations):
            x = self.reference_istft(cre, cim, n)
            (tre, tim), (cre, cim), tr = self.reference_project(x, A, tre, tim)
            trace.append(tr)
        x = self.reference_istft(tre, tim, n)
        if return_trace:
            trace.append(self.reference_project(x, A, tre, tim, 0.0)[2])
            return x, np.asarray(trace, np.float64)
        return x
