"""Float64 numpy oracle of the log-mel front end (wavenet/features.py,
csrc/wn_features.hip).  It shares no code with the package: the frames are
cut out explicitly with zero padding and transformed with np.fft.rfft, the
filterbank is built here from the formulas.

    F = ceil(n / hop); frame f is centred at c = f * hop + hop // 2 and holds
    x[c - n_fft // 2 + j], j < n_fft, zeros outside [0, n); times a periodic
    Hann window of win_length centred in the frame; power spectrum; HTK-mel
    triangles of peak 1; log(max(., floor)).
"""
import math

import numpy as np

# (sample_rate, n_fft, hop, win_length, n_mels) of the test shapes
# Largest absolute error of logmel_f32_matmul (float32 tables, the DFT as a
# float32 matmul, float32 log) against logmel over the clips of make_audio,
# per shape, measured on a CPU (BLAS summation orders differ a little between
# hosts); the device kernel is held to MEL_TOL_FACTOR x the largest of them.
MEL_F32_ERR_BY_SHAPE = {'a': 4.2e-7, 'b': 6.8e-7, 'c': 9.2e-6}
MEL_F32_ERR = max(MEL_F32_ERR_BY_SHAPE.values())
MEL_TOL_FACTOR = 4.0
MEL_TOL = MEL_TOL_FACTOR * MEL_F32_ERR

SHAPES = {
    'a': dict(sample_rate=8000, n_fft=64, hop=16, win_length=64, n_mels=10),
    'b': dict(sample_rate=8000, n_fft=128, hop=24, win_length=96, n_mels=8),
    'c': dict(sample_rate=16000, n_fft=1024, hop=256, win_length=1024,
              n_mels=80),
}
# (B, T, lengths)
CLIPS = {
    'a': (3, 100, (5, 100, 33)),
    'b': (1, 24 * 33 + 7, None),
    'c': (2, 16000, None),
}


def mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_inv(m):
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


def filterbank(sample_rate, n_fft, n_mels, fmin=0.0, fmax=None):
    """[n_mels][n_fft // 2 + 1] float64, written out element by element."""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    m0, m1 = mel(fmin), mel(fmax)
    edge = [mel_inv(m0 + (m1 - m0) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    w = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        lo, mid, hi = edge[m], edge[m + 1], edge[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sample_rate / n_fft
            if lo < f <= mid:
                w[m, k] = (f - lo) / (mid - lo)
            elif mid < f < hi:
                w[m, k] = (hi - f) / (hi - mid)
    return w


def hann(n_fft, win_length):
    w = np.zeros(n_fft)
    lo = (n_fft - win_length) // 2
    for i in range(win_length):
        w[lo + i] = 0.5 * (1.0 - math.cos(2.0 * math.pi * i / win_length))
    return w


def frames(x, n_fft, hop):
    """[ceil(n / hop)][n_fft] float64 frames of clip x, zero padded."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    F = -(-n // hop)
    padded = np.concatenate([np.zeros(n_fft), x, np.zeros(n_fft + hop)])
    out = np.empty((F, n_fft))
    for f in range(F):
        start = f * hop + hop // 2 - n_fft // 2 + n_fft
        out[f] = padded[start:start + n_fft]
    return out


def mel_energy(x, sample_rate, n_fft, hop, win_length, n_mels, fmin=0.0,
               fmax=None):
    fr = frames(x, n_fft, hop) * hann(n_fft, win_length)[None, :]
    p = np.abs(np.fft.rfft(fr, axis=1)) ** 2
    return p @ filterbank(sample_rate, n_fft, n_mels, fmin, fmax).T


def logmel(x, sample_rate, n_fft, hop, win_length, n_mels, fmin=0.0,
           fmax=None, floor=1e-10):
    """Oracle features of ONE clip x [n]: [ceil(n / hop)][n_mels] float64."""
    return np.log(np.maximum(
        mel_energy(x, sample_rate, n_fft, hop, win_length, n_mels, fmin, fmax),
        floor))


def logmel_batch(audio, lengths, F=None, **kw):
    """[B][F][n_mels]: clip b cut to lengths[b], zero rows behind its frames."""
    audio = np.asarray(audio)
    B, T = audio.shape
    hop = kw['hop']
    F = -(-T // hop) if F is None else F
    out = np.zeros((B, F, kw['n_mels']))
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        out[b, :-(-n // hop)] = logmel(audio[b, :n], **kw)
    return out


def logmel_f32_matmul(x, sample_rate, n_fft, hop, win_length, n_mels,
                      floor=1e-10):
    """The kernel's rule restated in float32 numpy: float32 tables (rounded
    from float64), the DFT as a float32 matmul with the cos | sin basis,
    re^2 + im^2, a float32 matmul with the filterbank, float32 log.  Its
    error against `logmel` is what float32 arithmetic in some summation order
    costs: the yardstick of the GPU test's tolerance."""
    fr = (frames(x, n_fft, hop).astype(np.float32) *
          hann(n_fft, win_length).astype(np.float32)[None, :])
    j = np.arange(n_fft)[:, None]
    k = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((j * k) % n_fft) / n_fft
    re = fr @ np.cos(ang).astype(np.float32)
    im = fr @ np.sin(ang).astype(np.float32)
    p = re * re + im * im
    m = p @ filterbank(sample_rate, n_fft, n_mels).astype(np.float32).T
    return np.log(np.maximum(m, np.float32(floor)))


def make_audio(name):
    """Seeded white noise of amplitude 0.1 plus two sinusoids, float32
    [B][T]; and the lengths (None: whole clips)."""
    B, T, lengths = CLIPS[name]
    sr = SHAPES[name]['sample_rate']
    rng = np.random.default_rng({'a': 11, 'b': 12, 'c': 13}[name])
    t = np.arange(T) / sr
    x = rng.uniform(-0.1, 0.1, (B, T))
    x += 0.3 * np.sin(2 * np.pi * 0.055 * sr * t)[None, :]
    x += 0.2 * np.sin(2 * np.pi * 0.21 * sr * t + 1.0)[None, :]
    return x.astype(np.float32), lengths
