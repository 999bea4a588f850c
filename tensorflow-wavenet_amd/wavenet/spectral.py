"""Synthesis metrics on the device (csrc/wn_spectral.hip, include/
wavenet_spectral.h): the multi-resolution STFT distance of two signals and the
mel-cepstral distortion of two log-mel tensors.

STFT distance (the Parallel WaveGAN definition, on THIS project's frame grid).
At one resolution (n_fft, hop, win_length), for a clip of n samples: F =
ceil(n / hop) frames, frame f centred at f * hop + hop // 2, zeros outside
[0, n) -- no reflection at the clip's edges, so the numbers differ from
torch.stft(center=True)'s at the edges -- a periodic Hann window of win_length
centred in the n_fft samples.  With Pg, Po the float32 power spectra of the
generated and the original frame (features.MelSpec's window and basis tables):

    mg = sqrt(max(Pg, floor)),  mo = sqrt(max(Po, floor))
    sc_num = sum (mo - mg)^2,   sc_den = sum mo^2
    log_sum = sum |log max(Po, floor) - log max(Pg, floor)| / 2

over the clip's frames and the n_fft // 2 + 1 bins, every float32 term widened
to float64 and added in one fixed order (wavenet_spectral.h writes it down):
a clip's three numbers do not depend on the batch.  Then

    spectral_convergence = sqrt(sc_num / sc_den)
    log_stft_magnitude   = log_sum / (F * n_bins)

per clip, averaged over clips, then over resolutions.

Mel-cepstral distortion, MFCC style: the DCT-II of the difference of two RAW
log-mel spectra (natural log of power), coefficients 1 .. order (c0 excluded),

    mcd_sum = sum_f sqrt(0.5 * sum_n e[n]^2)
    mcd_db  = (10 / ln 10) * sum mcd_sum / sum frames

(the cepstrum of log amplitude is half that of log power, so this is the usual
(10 / ln 10) sqrt(2 sum dc^2)).  It is comparable between runs of this tool,
NOT to SPTK / WORLD mel-generalised-cepstrum MCDs.
"""
import numpy as np

from . import _lib, features

RESOLUTIONS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
FLOOR = 1e-7
MAX_RESOLUTIONS = 8
ORDER = 13
ORDER_MAX = 64
DB_PER_NEPER = features.DB_PER_NEPER


def _lengths_arg(lengths, B, T, what):
    """`lengths` as int32 numpy [B] with 0 <= n[b] <= T (None stays None; one
    int stands for every clip)."""
    if lengths is None:
        return None
    if hasattr(lengths, 'detach'):
        lengths = lengths.detach().cpu().numpy()
    n = np.asarray(lengths)
    if n.dtype == object or n.dtype == np.bool_ or \
            not np.issubdtype(n.dtype, np.integer) or \
            n.shape not in ((), (B,)):
        raise ValueError('%s: lengths must be %d integers, got %s %s'
                         % (what, B, n.dtype, list(n.shape)))
    n = np.broadcast_to(n, (B,))
    if (n < 0).any() or (T is not None and (n > T).any()):
        raise ValueError('%s: lengths must lie in [0, T]%s, got %s'
                         % (what, '' if T is None else ' = [0, %d]' % T,
                            n.tolist()))
    return n.astype(np.int32)


def _signal_arg(x, what):
    import torch
    if not isinstance(x, torch.Tensor):
        x = np.asarray(x)
        if x.dtype == object or not np.issubdtype(x.dtype, np.floating):
            raise ValueError('%s: the signals must be float arrays' % what)
    elif not x.is_floating_point():
        raise ValueError('%s: the signals must be floating point' % what)
    if x.ndim not in (1, 2) or min(x.shape) < 1:
        raise ValueError('%s: the signals must have shape [B, T] or [T], got '
                         '%s' % (what, tuple(x.shape)))
    return x


class StftSums(object):
    """What StftDistance returns: sc_num, sc_den, log_sum, device float64
    [R, B] each, for the R resolutions of `resolutions`."""

    def __init__(self, sc_num, sc_den, log_sum, resolutions):
        self.sc_num, self.sc_den, self.log_sum = sc_num, sc_den, log_sum
        self.resolutions = tuple(tuple(r) for r in resolutions)

    def __iter__(self):
        return iter((self.sc_num, self.sc_den, self.log_sum))

    @classmethod
    def cat(cls, parts):
        """The sums of several batches as one (clips in the given order)."""
        import torch
        parts = list(parts)
        if not parts or any(p.resolutions != parts[0].resolutions
                            for p in parts):
            raise ValueError('StftSums.cat: batches of one set of resolutions '
                             'are required')
        return cls(*(torch.cat(t, dim=1) for t in zip(*parts)),
                   resolutions=parts[0].resolutions)

    def summary(self, lengths):
        """The metrics over all clips (waits for the device).  lengths: the
        samples per clip ([B] ints, or one int for all).  Per resolution and
        clip sc = sqrt(sc_num / sc_den), lm = log_sum / (Fb * n_bins); the
        means over the clips in index order, then over the resolutions.  A
        clip of length 0 is left out; no clip at all is a ValueError."""
        B = int(self.sc_num.shape[1])
        n = _lengths_arg(lengths, B, None, 'summary')
        if n is None:
            raise ValueError('summary: lengths are required')
        keep = [b for b in range(B) if n[b] > 0]
        if not keep:
            raise ValueError('summary: no clip has a sample')
        num, den, lg = (t.detach().cpu().numpy() for t in self)
        per = []
        for r, (n_fft, hop, win) in enumerate(self.resolutions):
            sc = lm = 0.0
            for b in keep:
                frames = -(-int(n[b]) // hop)
                sc += float(np.sqrt(num[r, b] / den[r, b]))
                lm += float(lg[r, b]) / (frames * (n_fft // 2 + 1))
            per.append({'n_fft': n_fft, 'hop': hop, 'win_length': win,
                        'spectral_convergence': sc / len(keep),
                        'log_stft_magnitude': lm / len(keep)})
        return {
            'spectral_convergence':
                sum(p['spectral_convergence'] for p in per) / len(per),
            'log_stft_magnitude':
                sum(p['log_stft_magnitude'] for p in per) / len(per),
            'per_resolution': per}


class StftDistance(object):
    """The multi-resolution STFT distance of one setting.  Calling it runs one
    launch per resolution on the device; every argument is checked here,
    before any library or device is touched."""

    def __init__(self, resolutions=RESOLUTIONS, floor=FLOOR):
        try:
            res = [tuple(r) for r in resolutions]
        except TypeError:
            raise ValueError('resolutions must be (n_fft, hop, win_length) '
                             'triples, got %r' % (resolutions,))
        if not 1 <= len(res) <= MAX_RESOLUTIONS:
            raise ValueError('1 to %d resolutions are required, got %d'
                             % (MAX_RESOLUTIONS, len(res)))
        for r in res:
            if len(r) != 3 or not all(features._is_int(v) for v in r):
                raise ValueError('a resolution is three ints (n_fft, hop, '
                                 'win_length), got %r' % (r,))
            n_fft, hop, win = r
            if not 64 <= n_fft <= features.N_FFT_MAX or n_fft % 64:
                raise ValueError('n_fft must be a multiple of 64 in [64, %d], '
                                 'got %r' % (features.N_FFT_MAX, n_fft))
            if not 1 <= hop <= win <= n_fft:
                raise ValueError('1 <= hop <= win_length <= n_fft = %d is '
                                 'required, got hop %r, win_length %r'
                                 % (n_fft, hop, win))
        if not features._is_num(floor) or not floor > 0 or \
                not np.float32(floor) > 0:
            raise ValueError('floor must be positive, got %r' % (floor,))
        self.resolutions = tuple(tuple(int(v) for v in r) for r in res)
        self.floor = float(floor)
        # the window and basis tables are the log-mel front end's (one mel:
        # the filterbank is not used)
        self._specs = [features.MelSpec(2.0, n_fft=n_fft, hop=hop, n_mels=1,
                                        win_length=win)
                       for n_fft, hop, win in self.resolutions]

    def settings(self):
        return dict(resolutions=[list(r) for r in self.resolutions],
                    floor=self.floor)

    @classmethod
    def from_settings(cls, d):
        if not isinstance(d, dict) or set(d) != {'resolutions', 'floor'}:
            raise ValueError('StftDistance settings have the keys '
                             '"resolutions" and "floor", got %r' % (d,))
        return cls(**d)

    def __call__(self, generated, original, lengths=None):
        """StftSums of generated against original, [B, T] or [T] float arrays
        or device tensors of the same shape (and device), without waiting for
        the device.  lengths ([B] ints in [0, T]): clip b has n[b] samples;
        what lies behind them is not read."""
        import torch
        what = 'stft distance'
        g, o = _signal_arg(generated, what), _signal_arg(original, what)
        if tuple(g.shape) != tuple(o.shape):
            raise ValueError('%s: the signals must have the same shape, got '
                             '%s and %s' % (what, tuple(g.shape),
                                            tuple(o.shape)))
        one = g.ndim == 1
        B, T = (1 if one else int(g.shape[0])), int(g.shape[-1])
        if B > 65535 or T > 2 ** 30:
            raise ValueError('%s: B <= 65535 and T <= 2^30 are required, got '
                             '%s' % (what, tuple(g.shape)))
        n = _lengths_arg(lengths, B, T, what)
        gt, ot = (isinstance(t, torch.Tensor) and t.device.type == 'cuda'
                  for t in (g, o))
        if gt and ot and g.device != o.device:
            raise ValueError('%s: generated on %s, original on %s'
                             % (what, g.device, o.device))
        lib = _lib.load()
        _lib.require_gpu()
        device = g.device if gt else o.device if ot else \
            torch.device('cuda', torch.cuda.current_device())

        def dev(t):
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(np.ascontiguousarray(t))
            return t.to(device=device, dtype=torch.float32).reshape(B, T) \
                .contiguous()
        g, o = dev(g), dev(o)
        R = len(self.resolutions)
        with torch.cuda.device(device):
            nd = None if n is None else torch.from_numpy(n).to(device)
            out = torch.empty((3, R, B), dtype=torch.float64, device=device)
            for r, spec in enumerate(self._specs):
                win, basis, _ = spec.device_tables(device)
                parts = torch.empty(
                    lib.wn_stft_distance_partials(B, T, spec.hop),
                    dtype=torch.float64, device=device)
                _lib.call('wn_stft_distance', _lib.ptr(g), T, _lib.ptr(o), T,
                          B, T, _lib.ptr(nd), _lib.ptr(win), _lib.ptr(basis),
                          spec.n_fft, spec.hop, spec.n_bins, self.floor,
                          _lib.ptr(out[0, r]), _lib.ptr(out[1, r]),
                          _lib.ptr(out[2, r]), _lib.ptr(parts), _lib.stream())
        return StftSums(out[0], out[1], out[2], self.resolutions)

    def reference(self, g, o):
        """The rule for ONE clip in numpy float32 (the tables rounded from
        float64, as the device gets them): float64 [R, 3], the rows (sc_num,
        sc_den, log_sum) of the resolutions."""
        f32 = np.float32
        g = np.asarray(g, f32).reshape(-1)
        o = np.asarray(o, f32).reshape(-1)
        if g.shape != o.shape:
            raise ValueError('reference: two clips of one length are required')
        n = g.shape[0]
        fl = f32(self.floor)
        out = np.zeros((len(self._specs), 3), np.float64)
        for r, spec in enumerate(self._specs):
            N, hop = spec.n_fft, spec.hop
            F = spec.num_frames(n)
            pos = (np.arange(F) * hop + hop // 2 - N // 2)[:, None] + \
                np.arange(N)[None, :]
            ok = (pos >= 0) & (pos < n)
            at = np.clip(pos, 0, max(n - 1, 0))
            cos, sin = (t.astype(f32) for t in spec.basis64())
            p = []
            for x in (g, o):
                fr = np.where(ok, x[at] if n else f32(0), f32(0)) * \
                    spec.window[None, :]
                re, im = fr @ cos, fr @ sin
                # (bin 0 and the Nyquist bin are real: the table's
                # sin(pi j) = 1.2e-16 is not used)
                im[:, 0] = im[:, -1] = 0
                p.append(np.maximum(re * re + im * im, fl))
            pg, po = p
            mg, mo = np.sqrt(pg), np.sqrt(po)
            d = (mo - mg).astype(np.float64)
            l = np.abs(np.log(po) - np.log(pg)) * f32(0.5)
            assert mo.dtype == f32 and l.dtype == f32
            out[r] = ((d * d).sum(), (mo.astype(np.float64) ** 2).sum(),
                      l.astype(np.float64).sum())
        return out


def dct_table(C, K):
    """float64 [K][C]: dct[n - 1][m] = sqrt(2 / C) cos(pi n (m + 1/2) / C),
    n = 1 .. K (the orthonormal DCT-II without c0)."""
    n = np.arange(1, K + 1, dtype=np.float64)[:, None]
    m = np.arange(C, dtype=np.float64)[None, :]
    return np.sqrt(2.0 / C) * np.cos(np.pi * n * (m + 0.5) / C)


def _order_arg(order, C, what):
    if not features._is_int(order) or not 1 <= order <= min(C - 1, ORDER_MAX):
        raise ValueError('%s: order must be an int in [1, min(C - 1, %d)] = '
                         '[1, %d], got %r' % (what, ORDER_MAX,
                                              min(C - 1, ORDER_MAX), order))
    return int(order)


def _pair_shape(a, b, what):
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
    return shapes[0][-1]


_dct_dev = {}


def cepstral_distance(a, b, nframes=None, order=ORDER):
    """mcd_sum, device float64 [B] ([1] for [F, C] inputs), of two RAW log-mel
    tensors, float32 [B, F, C] or [F, C] of the same shape, on the device
    (wn_cepstral_distance) without waiting for it: per clip the sum over its
    real frames (nframes: [B] ints in [0, F]; the others are not read) of
    sqrt(0.5 sum_n e[n]^2), e the DCT-II coefficients 1 .. order of a - b.
    One fixed summation order: a clip's number does not depend on the
    batch."""
    what = 'cepstral_distance'
    C = _pair_shape(a, b, what)
    K = _order_arg(order, C, what)
    a, _, B, F = features._frames_arg(a, C, what)
    b, _, _, _ = features._frames_arg(b, C, what)
    n = features._nframes_arg(nframes, B, F, what)
    import torch
    lib = _lib.load()
    _lib.require_gpu()
    ta = features._to_device(a, B, F, C)
    tb = features._to_device(b, B, F, C)
    if ta.device != tb.device:
        raise ValueError('%s: a on %s, b on %s' % (what, ta.device, tb.device))
    with torch.cuda.device(ta.device):
        key = (C, K, str(ta.device))
        if key not in _dct_dev:
            _dct_dev[key] = torch.from_numpy(dct_table(C, K)).to(ta.device)
        nd = None if n is None else torch.from_numpy(n).to(ta.device)
        out = torch.empty(B, dtype=torch.float64, device=ta.device)
        parts = torch.empty(lib.wn_cepstral_distance_partials(B, F),
                            dtype=torch.float64, device=ta.device)
        _lib.call('wn_cepstral_distance', _lib.ptr(ta), _lib.ptr(tb), B, F, C,
                  _lib.ptr(nd), _lib.ptr(_dct_dev[key]), K, _lib.ptr(out),
                  _lib.ptr(parts), _lib.stream())
    return out


def cepstral_reference(a, b, nframes=None, order=ORDER):
    """cepstral_distance's rule in numpy: float64 [B]."""
    what = 'cepstral_reference'
    C = _pair_shape(a, b, what)
    K = _order_arg(order, C, what)
    a, _, B, F = features._frames_arg(np.asarray(a), C, what)
    b, _, _, _ = features._frames_arg(np.asarray(b), C, what)
    n = features._nframes_arg(nframes, B, F, what)
    d = (a.reshape(B, F, C) - b.reshape(B, F, C)).astype(np.float64)
    e = d @ dct_table(C, K).T
    r = np.sqrt(0.5 * (e * e).sum(-1))
    return np.array([r[i, :F if n is None else n[i]].sum() for i in range(B)],
                    np.float64)


def mcd_db(mcd_sum, nframes):
    """(10 / ln 10) sum mcd_sum / sum nframes: the mel-cepstral distortion in
    dB over all clips (waits for the device).  nframes: the real frames per
    clip (ints, or one int for all)."""
    s = mcd_sum.detach().cpu().numpy() if hasattr(mcd_sum, 'detach') \
        else np.asarray(mcd_sum, np.float64)
    B = int(s.shape[0])
    n = np.asarray(nframes)
    if n.dtype == object or n.dtype == np.bool_ or \
            not np.issubdtype(n.dtype, np.integer) or \
            n.shape not in ((), (B,)) or (n < 0).any():
        raise ValueError('mcd_db: nframes must be %d non-negative integers, '
                         'got %r' % (B, nframes))
    total = int(n) * B if n.shape == () else int(n.sum())
    if total < 1:
        raise ValueError('mcd_db: no frames were counted')
    return DB_PER_NEPER * float(s.sum()) / total
