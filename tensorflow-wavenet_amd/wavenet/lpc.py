"""Linear-prediction excitation on the device (csrc/wn_lpc.hip, include/
wavenet_lpc.h): an order-p predictor per frame from the raw log-mel frames,
the analysis filter that turns audio into its prediction residual and the
all-pole synthesis filter that puts the spectral envelope back.

    P = max(pinv(melw) @ exp(logmel), 0)          the frame's power spectrum
    r[i] = irfft(P)[i] * lagwin[i]                its autocorrelation, i <= p
    a    = Levinson-Durbin(r)                     x[t] ~ sum_i a_i x[t - i]

    analysis:   e[t] = (x[t] - sum_i a_i[f(t - i)] x[t - i]) * g
    synthesis:  y[t] = e[t] / g + sum_i a_i[f(t - i)] y[t - i]

f(u) = u // hop is the frame of sample u: a coefficient travels with the
sample it multiplies.  lagwin[i] = exp(-(2 pi lag_window i / sample_rate)^2 /
2) and lagwin[0] = 1 + noise (a Gaussian lag window and a white-noise floor),
g = float32(gain).  The sums run over i = order down to 1, one rounded
multiply and one rounded add per tap; include/wavenet_lpc.h states every
operation.  The model sees and produces the excitation e; the white
quantisation noise of what it generates is shaped by every frame's envelope.
The features are always those of the natural signal, and the coefficients
come from the features alone: generation from a feature file keeps working.

`reference_coefficients`, `reference_analysis` and `reference_synthesis` state
the three rules in numpy: the two filters in float32, bit for bit what the
device computes; the autocorrelation and the recursion in float64.  A frame
with r[0] <= 1e-30 (silence with -inf mels, a NaN frame) gets the identity
filter, all coefficients zero.  The recursion stops at the first reflection
coefficient that is not below 1 in modulus; the lower order's coefficients
stand, so every predictor is the polynomial of reflection coefficients below 1.

train.py --lpc_order stores `entry()` in every checkpoint under 'lpc';
generate.py and evaluate.py read it from there.
"""
import numpy as np

from . import _lib, features
from .emphasis import _ld, prepare
from .griffin_lim import mel_pinv

ORDER_MAX = 32
R0_FLOOR = 1e-30
GAIN_MIN, GAIN_MAX = 2.0 ** -10, 2.0 ** 10
HOP_MAX = 4096
AUTOCORR_PARTS = 8        # interleaved partial sums of r[i] (wavenet_lpc.h)


def check_values(order, noise, lag_window, gain, n_fft=None):
    """ValueError unless the four settings lie within their limits."""
    if not features._is_int(order) or not 1 <= order <= ORDER_MAX or \
            (n_fft is not None and order > n_fft // 2):
        raise ValueError('order must be an int in [1, %d] and at most n_fft '
                         '/ 2, got %r' % (ORDER_MAX, order))
    if not features._is_num(noise) or not 0 <= noise < 1:
        raise ValueError('noise must lie in [0, 1), got %r' % (noise,))
    if not features._is_num(lag_window) or not 0 <= lag_window:
        raise ValueError('lag_window must be a number of Hz >= 0, got %r'
                         % (lag_window,))
    if not features._is_num(gain) or not GAIN_MIN <= gain <= GAIN_MAX:
        raise ValueError('gain must lie in [2^-10, 2^10], got %r' % (gain,))


def levinson(r):
    """Levinson-Durbin on the autocorrelation r [p + 1] in float64, one
    rounded operation per operator: (a [p + 1] with a[0] = 1 and x[t] ~
    -sum_i a[i] x[t - i], the reflection coefficients taken, the final
    error).  Stops in front of the first reflection coefficient that is not
    below 1 in modulus: the higher a stay zero.  r[0] is taken as it is (the
    caller decides what an empty frame gets)."""
    r = [float(v) for v in np.asarray(r, np.float64).reshape(-1)]
    p = len(r) - 1
    a = [1.0] + [0.0] * p
    err, ks = r[0], []
    for i in range(1, p + 1):
        acc = r[i]
        for j in range(1, i):
            acc = acc + a[j] * r[i - j]
        if err == 0.0:
            break                       # (-acc / 0: never below 1)
        k = -acc / err
        if not abs(k) < 1.0:
            break
        a[1:i] = [a[j] + k * a[i - j] for j in range(1, i)]
        a[i] = k
        err = err * (1.0 - k * k)
        ks.append(k)
    return np.asarray(a, np.float64), np.asarray(ks, np.float64), err


class LinearPrediction(object):
    """The predictor and the filter pair of one front-end setting (module
    docstring).  Every argument is checked here, before any library or device
    is touched."""

    def __init__(self, spec, order=16, noise=1e-4, lag_window=40.0, gain=1.0):
        if not isinstance(spec, features.MelSpec):
            raise ValueError('LinearPrediction: spec must be a features.'
                             'MelSpec (for a MelPitchSpec pass its .mel), '
                             'got %r' % (type(spec).__name__,))
        check_values(order, noise, lag_window, gain, spec.n_fft)
        if spec.hop > HOP_MAX:
            raise ValueError('hop <= %d is required, got %d'
                             % (HOP_MAX, spec.hop))
        self.spec = spec
        self.order, self.noise = int(order), float(noise)
        self.lag_window, self.gain = float(lag_window), float(gain)
        self.n_fft, self.hop, self.n_bins = spec.n_fft, spec.hop, spec.n_bins
        self.n_mels = spec.n_mels
        self.gain32 = np.float32(self.gain)
        self.inv_gain32 = np.float32(1.0 / float(self.gain32))
        self.pinv64, self.pinv = mel_pinv(spec)
        # ctab [n_bins][order + 1]: w_k cos(2 pi i k / n_fft) / n_fft (the
        # angle through (i k) mod n_fft), lagwin [order + 1]
        N = self.n_fft
        i = np.arange(self.order + 1, dtype=np.int64)
        k = np.arange(self.n_bins, dtype=np.int64)
        w = np.full(self.n_bins, 2.0)
        w[0] = w[-1] = 1.0
        ang = 2.0 * np.pi * ((k[:, None] * i[None, :]) % N) / N
        self.ctab = np.ascontiguousarray(w[:, None] * np.cos(ang) / N)
        lw = np.exp(-0.5 * (2.0 * np.pi * self.lag_window *
                            i.astype(np.float64) / spec.sample_rate) ** 2)
        lw[0] = 1.0 + self.noise
        self.lagwin = lw
        self._dev = {}

    def __repr__(self):
        return 'LinearPrediction(order=%d, noise=%r, lag_window=%r, gain=%r)' \
            % (self.order, self.noise, self.lag_window, self.gain)

    # ------------------------------------------------- settings and entries
    def settings(self):
        spec = self.spec.with_normalizer(None).settings()
        return dict(spec=spec, **self.entry())

    @classmethod
    def from_settings(cls, d):
        keys = {'spec', 'order', 'noise', 'lag_window', 'gain'}
        if not isinstance(d, dict) or set(d) != keys or \
                not isinstance(d['spec'], dict):
            raise ValueError('LinearPrediction settings have the keys %s, '
                             'got %r' % (sorted(keys), d))
        d = dict(d)
        return cls(features.MelSpec(**d.pop('spec')), **d)

    def entry(self):
        """What checkpoints store under 'lpc'."""
        return {'order': self.order, 'noise': self.noise,
                'lag_window': self.lag_window, 'gain': self.gain}

    @classmethod
    def from_entry(cls, spec, d):
        """The LinearPrediction of a checkpoint's entry over `spec`; None for
        None."""
        if d is None:
            return None
        check_entry(d)
        return cls(spec, **d)

    # ---------------------------------------------------- the rules, numpy
    def reference_power(self, frames):
        """float32 [F, n_bins]: the clipped power spectrum of raw log-mel
        frames [F, n_mels], m ascending, every product rounded."""
        f32 = np.float32
        fr = np.asarray(frames, f32)
        with np.errstate(all='ignore'):
            M = np.exp(fr)
            P = np.zeros((fr.shape[0], self.n_bins), f32)
            for m in range(self.n_mels):
                P = P + (M[:, m, None] * self.pinv[None, :, m]).astype(f32)
            return np.where(P < 0, f32(0), P).astype(f32)

    def reference_autocorrelation(self, P):
        """float64 [F, order + 1] from the float32 power spectrum: eight
        partial sums over the bins q, q + 8, ... ascending (every product
        rounded), added in the order of q, then the lag window."""
        P = np.asarray(P, np.float32).astype(np.float64)
        Q, nb = AUTOCORR_PARTS, self.n_bins
        part = np.zeros((P.shape[0], Q, self.order + 1), np.float64)
        with np.errstate(all='ignore'):
            for k0 in range(0, nb, Q):
                w = min(Q, nb - k0)
                part[:, :w] = part[:, :w] + self.ctab[None, k0:k0 + w, :] * \
                    P[:, k0:k0 + w, None]
            r = part[:, 0]
            for q in range(1, Q):
                r = r + part[:, q]
            return r * self.lagwin[None, :]

    def reference_coefficients(self, frames, nframes=None):
        """`coefficients` in numpy: float32 [B, F, order] or [F, order]."""
        frames, one, B, F = features._frames_arg(
            np.asarray(frames), self.n_mels, 'reference_coefficients')
        n = features._nframes_arg(nframes, B, F, 'reference_coefficients')
        fr = frames.reshape(B, F, self.n_mels)
        out = np.zeros((B, F, self.order), np.float32)
        for b in range(B):
            Fb = F if n is None else int(n[b])
            if Fb == 0:
                continue
            r = self.reference_autocorrelation(self.reference_power(fr[b, :Fb]))
            for f in range(Fb):
                if not r[f, 0] > R0_FLOOR:
                    continue
                a = levinson(r[f])[0]
                out[b, f] = (-a[1:]).astype(np.float32)
        return out[0] if one else out

    def _ref_args(self, audio, coeffs, lengths, what):
        from .emphasis import _audio_arg
        x, one, B, T = _audio_arg(np.asarray(audio), what)
        n = features.check_lengths(lengths, B, T, what)
        c = np.asarray(coeffs, np.float32)
        c = c.reshape((B,) + c.shape[-2:])
        nn = np.full(B, T, np.int64) if n is None else n.astype(np.int64)
        self._check_frames(c.shape[1], c.shape[2], nn, what)
        t = np.arange(T)
        x = np.where(t[None, :] < nn[:, None],
                     x.astype(np.float32).reshape(B, T), np.float32(0))
        return x.astype(np.float32), c, nn, one, B, T

    def _check_frames(self, F, order, n, what):
        need = int(-(-int(np.max(n)) // self.hop))
        if order != self.order or F < need:
            raise ValueError('%s: coeffs must be [B, F, %d] with F >= '
                             'ceil(n / hop) = %d, got F %d, order %d'
                             % (what, self.order, need, F, order))

    def reference_analysis(self, audio, coeffs, lengths=None):
        """`analysis` in numpy float32, bit for bit: [B, T] or [T]."""
        f32 = np.float32
        x, c, n, one, B, T = self._ref_args(audio, coeffs, lengths,
                                            'reference_analysis')
        t = np.arange(T)
        acc = np.zeros((B, T), f32)
        rows = np.arange(B)[:, None]
        with np.errstate(all='ignore'):
            for i in range(self.order, 0, -1):
                u = t - i
                ok = u >= 0
                uc = np.maximum(u, 0)
                f = np.minimum(uc // self.hop, c.shape[1] - 1)
                prod = (c[rows, f[None, :], i - 1] * x[:, uc]).astype(f32)
                acc = np.where(ok[None, :], (acc + prod).astype(f32), acc)
            e = ((x - acc).astype(f32) * self.gain32).astype(f32)
        e = np.where(t[None, :] < n[:, None], e, f32(0)).astype(f32)
        return e[0] if one else e

    def reference_synthesis(self, excitation, coeffs, lengths=None):
        """`synthesis` in numpy float32, bit for bit (the transposed direct
        form, one elementwise step over the taps per sample): [B, T] or
        [T]."""
        f32 = np.float32
        e, c, n, one, B, T = self._ref_args(excitation, coeffs, lengths,
                                            'reference_synthesis')
        p = self.order
        y = np.zeros((B, T), f32)
        s = np.zeros((B, p + 1), f32)              # s[:, i - 1] = s_i
        with np.errstate(all='ignore'):
            eg = (e * self.inv_gain32).astype(f32)
            for t in range(int(n.max())):
                f = min(t // self.hop, c.shape[1] - 1)
                yt = (eg[:, t] + s[:, 0]).astype(f32)
                y[:, t] = yt
                s[:, :p] = (s[:, 1:] + (c[:, f, :] * yt[:, None]).astype(f32)
                            ).astype(f32)
        y = np.where(np.arange(T)[None, :] < n[:, None], y, f32(0)).astype(f32)
        return y[0] if one else y

    # ------------------------------------------------------------ the device
    def _tables(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            # (the pseudo-inverse transposed: a wave reads whole rows)
            self._dev[key] = tuple(
                torch.from_numpy(t).to(device) for t in
                (np.ascontiguousarray(self.pinv.T), self.ctab, self.lagwin))
        return self._dev[key]

    def coefficients(self, frames, nframes=None):
        """Predictor coefficients, device float32 [B, F, order] ([F, order]
        for [F, n_mels]), from RAW log-mel frames (natural log of power,
        MelSpec's output without a normaliser), without waiting for the
        device.  nframes ([B] ints in [0, F]): the frames at or behind them
        are not read and get zeros."""
        import torch
        what = 'coefficients'
        frames, one, B, F = features._frames_arg(frames, self.n_mels, what)
        n = features._nframes_arg(nframes, B, F, what)
        if B > 65535:
            raise ValueError('%s: B <= 65535 is required, got %d' % (what, B))
        _lib.load()
        _lib.require_gpu()
        src = features._to_device(frames, B, F, self.n_mels)
        with torch.cuda.device(src.device):
            nd = None if n is None else torch.from_numpy(n).to(src.device)
            pinv, ctab, lagwin = self._tables(src.device)
            out = torch.empty((B, F, self.order), dtype=torch.float32,
                              device=src.device)
            _lib.call('wn_lpc_from_mel', _lib.ptr(src), B, F, self.n_mels,
                      _lib.ptr(nd), _lib.ptr(pinv), self.n_bins,
                      _lib.ptr(ctab), _lib.ptr(lagwin), self.order,
                      _lib.ptr(out), _lib.stream())
        return out[0] if one else out

    @staticmethod
    def analysis_tile():
        """Samples per workgroup of the analysis kernel (loads the library;
        no device)."""
        return int(_lib.load().wn_lpc_analysis_tile())

    def _filter(self, entry, audio, coeffs, lengths, out, g, alias_ok):
        import torch
        what = entry[len('wn_lpc_'):]
        shape = tuple(int(v) for v in np.shape(audio)) \
            if not hasattr(audio, 'shape') else tuple(audio.shape)
        B = 1 if len(shape) == 1 else (shape[0] if shape else 0)
        T = shape[-1] if shape else 0
        if not hasattr(coeffs, 'detach'):
            coeffs = np.asarray(coeffs)
            ok = coeffs.dtype == np.float32
        else:
            ok = str(coeffs.dtype) == 'torch.float32'
        cs = tuple(int(v) for v in coeffs.shape)
        if not ok or len(cs) not in (2, 3) or \
                (cs[0] if len(cs) == 3 else 1) != B or min(cs + (1,)) < 1:
            raise ValueError('%s: coeffs must be float32 [%d, F, %d], got %s '
                             '%s' % (what, B, self.order, coeffs.dtype, cs))
        if B > 65535 or T > 2 ** 30:
            raise ValueError('%s: B <= 65535 and T <= 2^30 are required, got '
                             'B %d, T %d' % (what, B, T))
        n = features.check_lengths(lengths, B, T, what) if T else None
        self._check_frames(cs[-2], cs[-1], [T] if n is None else n, what)
        src, dst, nd, one = prepare(audio, n, out, what, alias_ok,
                                    checked=True)
        F = cs[-2]
        if not isinstance(coeffs, torch.Tensor):
            coeffs = torch.from_numpy(np.ascontiguousarray(coeffs))
        cf = coeffs.to(src.device).reshape(B, F, self.order).contiguous()
        with torch.cuda.device(src.device):
            _lib.call(entry, _lib.ptr(src), _ld(src), _lib.ptr(cf), F,
                      self.order, self.hop, _lib.ptr(nd), B, T, float(g),
                      _lib.ptr(dst), _ld(dst), _lib.stream())
        return out if out is not None else (dst[0] if one else dst)

    def analysis(self, audio, coeffs, lengths=None, out=None):
        """The excitation of audio [B, T] or [T] (a float array or a device
        tensor) under coeffs (float32 [B, F, order] or [F, order], F >=
        ceil(n / hop)): device float32 of audio's shape, without waiting for
        the device.  lengths ([B] ints, 1 <= n[b] <= T): what lies at or
        behind n[b] is not read and comes out as zeros.  out: a float32
        device tensor of audio's shape to write into (unit stride inside a
        clip); it must not be, or overlap, audio."""
        return self._filter('wn_lpc_analysis', audio, coeffs, lengths, out,
                            self.gain32, False)

    def synthesis(self, excitation, coeffs, lengths=None, out=None):
        """The inverse of `analysis`, as it takes and returns things; out may
        be the excitation itself."""
        return self._filter('wn_lpc_synthesis', excitation, coeffs, lengths,
                            out, self.inv_gain32, True)

    def synthesis_ragged(self, waves, coeffs_list):
        """`synthesis` of a list of device float32 [n_u] clips with their
        coefficients (float32 [F_u, order] each, on the device) as ONE ragged
        batch (zero padded, with lengths): a list of new [n_u] tensors."""
        import torch
        n = np.array([int(w.shape[0]) for w in waves], np.int64)
        F = max(max(int(c.shape[0]) for c in coeffs_list),
                -(-int(n.max()) // self.hop))
        buf = torch.zeros((len(waves), int(n.max())), dtype=torch.float32,
                          device=waves[0].device)
        cf = torch.zeros((len(waves), F, self.order), dtype=torch.float32,
                         device=waves[0].device)
        for j, (w, c) in enumerate(zip(waves, coeffs_list)):
            if int(c.shape[0]) < -(-int(n[j]) // self.hop):
                raise ValueError('synthesis_ragged: clip %d of %d samples '
                                 'has %d frames of coefficients'
                                 % (j, n[j], c.shape[0]))
            buf[j, :n[j]] = w
            cf[j, :c.shape[0]] = c
        self.synthesis(buf, cf, n, out=buf)
        return [buf[j, :n[j]] for j in range(len(waves))]

    # ------------------------------------------------- from audio or files
    def raw_frames(self, audio, lengths=None):
        """The RAW log-mel frames of audio on the device: the spec without
        its normaliser."""
        return self.spec.with_normalizer(None)(audio, lengths)

    def coefficients_of(self, audio, lengths=None):
        """The coefficients of audio's own raw log-mel frames, [B, F, order]
        or [F, order]."""
        n = None if lengths is None else \
            -(-np.asarray(lengths, np.int64) // self.hop)
        return self.coefficients(self.raw_frames(audio, lengths), n)


def frames_of_file(feats, spec):
    """The RAW log-mel frames behind a feature file's frames `feats`
    [F, channels] of the front end `spec` (a MelSpec, or a MelPitchSpec,
    whose mel columns are those in front): the mel columns with the front
    end's normaliser inverted (Normalizer.invert: what it clamped stays
    clamped), float32 [F, n_mels] as a CPU tensor or array -- or None where
    the file does not hold them.  The normaliser is the front end's own:
    a MelPitchSpec's `.mel` carries none."""
    feats = np.asarray(feats)
    n_mels = spec.n_mels
    if feats.ndim != 2 or feats.shape[0] == 0 or feats.shape[1] < n_mels:
        return None
    mel = np.ascontiguousarray(feats[:, :n_mels].astype(np.float32))
    norm = spec.normalizer
    return mel if norm is None else norm.invert(mel)


# ---------------------------------------------------------- checkpoint form
ENTRY_KEYS = ('order', 'noise', 'lag_window', 'gain')


def check_entry(d):
    if not isinstance(d, dict) or set(d) != set(ENTRY_KEYS):
        raise ValueError("an lpc entry has the keys %s, got %r"
                         % (sorted(ENTRY_KEYS), d))
    check_values(d['order'], d['noise'], d['lag_window'], d['gain'])


# ------------------------------------------------------------ command line
VALUE_FLAGS = ('lpc_gain', 'lpc_noise', 'lpc_lag_window')


def add_cli_flags(p, train=False):
    p.add_argument(
        '--lpc_order', type=int, default=None, metavar='P',
        help=('Train on the linear-prediction excitation: an order-P '
              'predictor per frame (1 <= P <= 32) from the raw log-mel of '
              'the batch, e[t] = (x[t] - sum_i a_i x[t - i]) * gain; the '
              'features stay those of the natural signal.  Needs '
              '--lc_features mel or mel+f0.  Stored in every checkpoint '
              '(\'lpc\'); generate.py and evaluate.py run what the model '
              'generates through the all-pole filter.  Default: off.')
        if train else
        ('The order of the checkpoint\'s linear prediction (train.py '
         '--lpc_order): what the model generates is run through the '
         'all-pole filter of every frame on the device; the coefficients '
         'come from the raw log-mel frames that condition the run (for '
         'generate.py --lc_path the checkpoint\'s normaliser is inverted: '
         'what it clamped stays clamped; of a mel+f0 file the mel columns '
         'are used).  Default: the checkpoint\'s \'lpc\' entry; 0 switches '
         'it off.'))
    p.add_argument('--lpc_gain', type=float, default=None, metavar='G',
                   help='The excitation is scaled by G, 2^-10 <= G <= 2^10, '
                   'before the mu-law encoder (which clips what leaves '
                   '[-1, 1]).  Default: %s.' %
                   ('1' if train else "the checkpoint's"))
    p.add_argument('--lpc_noise', type=float, default=None, metavar='X',
                   help='White-noise floor: r[0] is multiplied by 1 + X, '
                   '0 <= X < 1.  Default: %s.' %
                   ('1e-4' if train else "the checkpoint's"))
    p.add_argument('--lpc_lag_window', type=float, default=None, metavar='HZ',
                   help='Gaussian lag window of HZ Hertz (0: none).  '
                   'Default: %s.' % ('40' if train else "the checkpoint's"))


DEFAULTS = {'noise': 1e-4, 'lag_window': 40.0, 'gain': 1.0}


def flag_error(args, tool):
    """What is wrong with the --lpc_* flags of train.py, evaluate.py or
    generate.py (`tool`) among the other flags, as a message that names the
    flags, or None.  Only the command line is looked at."""
    order = args.lpc_order
    given = [k for k in VALUE_FLAGS if getattr(args, k) is not None]
    if order is None or order == 0:
        if given:
            return '--%s needs --lpc_order P with P >= 1' % given[0]
        return None
    vals = dict(DEFAULTS)
    for k in given:
        vals[k[len('lpc_'):]] = getattr(args, k)
    try:
        check_values(order, vals['noise'], vals['lag_window'], vals['gain'])
    except ValueError as e:
        return '--lpc_order / --lpc_gain / --lpc_noise / --lpc_lag_window: ' \
            '%s' % e
    if getattr(args, 'preemphasis', None):
        return '--lpc_order and --preemphasis are two shaping filters: ' \
            'choose one'
    if tool == 'train':
        if getattr(args, 'lc_features', None) not in features.KINDS:
            return '--lpc_order needs --lc_features mel or mel+f0 (the raw ' \
                'log-mel must come from the audio)'
        if getattr(args, 'lc_feature_context', None) == 'utterance':
            return '--lpc_order does not go with --lc_feature_context ' \
                'utterance (the resident frames are normalised in place)'
    if tool == 'generate' and getattr(args, 'wav_seed', None):
        return '--lpc_order does not go with --wav_seed (a seed has no ' \
            'frames to take its filter from)'
    return None


def from_cli(args, spec, stored=None, continued=False):
    """The LinearPrediction of the --lpc_* flags and a checkpoint's 'lpc'
    entry `stored` over the MelSpec `spec`, or None.  The flags override the
    entry value by value, --lpc_order 0 switches it off -- except for a run
    `continued` in its logdir, where flags that differ from the entry are a
    ValueError naming both.  spec None with linear prediction on: a
    ValueError."""
    if stored is not None:
        check_entry(stored)
    order = args.lpc_order
    if order is None and stored is None:
        return None
    mine = dict(DEFAULTS if stored is None else
                {k: stored[k] for k in DEFAULTS})
    mine['order'] = stored['order'] if order is None else order
    for k in VALUE_FLAGS:
        if getattr(args, k) is not None:
            mine[k[len('lpc_'):]] = getattr(args, k)
    on = mine['order'] != 0
    if continued:
        if (mine if on else None) != stored and \
                (order is not None or stored is not None):
            raise ValueError(
                '--lpc_order: the settings %r do not match the checkpoint\'s '
                '%r: a run continued in its logdir keeps its linear '
                'prediction (start a new one with --restore_from)'
                % (mine if on else None, stored))
    if not on:
        return None
    if spec is None:
        raise ValueError('linear prediction (--lpc_order, or the '
                         'checkpoint\'s \'lpc\' entry) needs log-mel frames: '
                         '--lc_features mel or mel+f0')
    return LinearPrediction(getattr(spec, 'mel', spec), **mine)
