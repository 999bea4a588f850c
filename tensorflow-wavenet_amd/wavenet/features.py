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
"""
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
                 win_length=None, fmin=0.0, fmax=None, floor=1e-10):
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
        return dict(sample_rate=self.sample_rate, n_fft=self.n_fft,
                    hop=self.hop, n_mels=self.n_mels,
                    win_length=self.win_length, fmin=self.fmin,
                    fmax=self.fmax, floor=self.floor)

    def num_frames(self, n):
        return -(-int(n) // self.hop)

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
        frames f >= ceil(n[b] / hop) are zeros."""
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
        return out[0] if one else out


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
    return np.log(np.maximum(m, dtype(spec.floor)))


def local_condition_from_audio(net, spec, audio, lengths=None):
    """WaveNetModel.local_condition_from_audio (model.py)."""
    import torch
    if not isinstance(spec, MelSpec):
        raise ValueError('local_condition_from_audio: spec must be a MelSpec')
    if not net.Lc:
        raise ValueError('local_condition_from_audio: this model was built '
                         'without local conditioning')
    if spec.n_mels != net.Lc:
        raise ValueError('local_condition_from_audio: the front end has %d '
                         'mels, the model %d local-conditioning channels'
                         % (spec.n_mels, net.Lc))
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
    p.add_argument('--lc_features', choices=['mel', 'none'], default=None,
                   help='Local conditioning from the audio itself: log-mel '
                   'features computed on the device (wavenet/features.py), '
                   '--lc_channels mels at one frame per hop samples; frame f '
                   'sits beside samples f * hop .. f * hop + hop - 1.  No '
                   '<clip>.npy files are read.  The features are those of '
                   'the piece as dequeued: a piece\'s edges see zeros, not '
                   'the neighbouring samples of its file.' + also)
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


_CLI_KEYS = ('n_fft', 'win_length', 'fmin', 'fmax')


def cli_flags_given(args):
    """The --lc_n_fft ... flags that were given, by name."""
    return ['--lc_' + k for k in _CLI_KEYS
            if getattr(args, 'lc_' + k) is not None]


def spec_from_cli(args, sample_rate, n_mels, hop, stored=None):
    """The MelSpec the flags ask for, or None without a front end.  `stored`:
    a checkpoint's 'lc_features' entry -- without --lc_features it switches
    the front end on (--lc_features none: off), and its settings are the
    defaults of the flags that are absent.  ValueError where the flags, the
    model (n_mels = --lc_channels, hop) and the entry do not fit."""
    kind = args.lc_features
    if kind is None and stored is not None:
        kind = stored.get('kind')
    if kind in (None, 'none'):
        given = cli_flags_given(args)
        if given:
            raise ValueError('%s needs --lc_features mel' % given[0])
        return None
    if kind != 'mel':
        raise ValueError('unknown front end %r in the checkpoint\'s '
                         "'lc_features'" % (kind,))
    kw = {}
    if stored is not None and stored.get('kind') == 'mel':
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
        raise ValueError('--lc_features mel needs --lc_channels (the number '
                         'of mels)')
    if hop is None:
        raise ValueError('--lc_features mel needs --lc_hop or '
                         '--lc_upsample_scales (hop = their product)')
    return MelSpec(sample_rate, hop=hop, n_mels=n_mels, **kw)


def checkpoint_entry(spec):
    """What train.py stores under 'lc_features'."""
    return dict(kind='mel', **spec.settings())
