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

# The shapes that reach the rest of the kernel (csrc/wn_features.hip: STAGE on
# or off x one to four mel fragments, the bank pad of an even hop, the 16-byte
# or scalar epilogue, the chunk count against the eight waves):
#   d  hop 1 (odd: no pad), a second tile of 8 rows, one mel
#   e  n_fft no power of two (4 bin chunks), odd hop, odd window and odd
#      n_fft - win_length, two mel fragments + scalar epilogue, a one-sample
#      clip, band limits
#   f  hop = win_length = n_fft, two fragments + 16-byte epilogue, the second
#      clip ends on the tile boundary (32 of 34 frames)
#   g  the largest staged launch (16340 of 16384 staged floats), odd hop, four
#      fragments + 16-byte epilogue, 33 chunks: wave 0 takes five
#   h  one hop further: 16406 floats, so the samples are read from memory; four
#      fragments + scalar epilogue, win_length < n_fft, a short second clip
#   i  a clip shorter than one hop: one frame, four output floats
# and the pairs either side of the staging limit on the same audio:
#   gm  (g) at hop 462: memory            (g itself, hop 461: staged)
#   gp  (g) at hop 460, even: staged with its pad floats, 16344 floats --
#      16 bytes more than (g), the most on-chip memory any setting asks for
#   ks, km  n_fft 1024, 80 mels (three fragments) at hop 494: 16372 staged
#      floats; at hop 496: memory
SHAPES.update({
    'd': dict(sample_rate=8000, n_fft=64, hop=1, win_length=64, n_mels=1),
    'e': dict(sample_rate=8000, n_fft=192, hop=25, win_length=75, n_mels=33,
              fmin=300.0, fmax=3400.0),
    'f': dict(sample_rate=8000, n_fft=320, hop=320, win_length=320,
              n_mels=64),
    'g': dict(sample_rate=16000, n_fft=2048, hop=461, win_length=2048,
              n_mels=128, fmin=50.0, fmax=7600.0),
    'h': dict(sample_rate=16000, n_fft=2048, hop=462, win_length=1200,
              n_mels=97),
    'i': dict(sample_rate=8000, n_fft=128, hop=7, win_length=128, n_mels=4),
    'gm': dict(sample_rate=16000, n_fft=2048, hop=462, win_length=2048,
               n_mels=128, fmin=50.0, fmax=7600.0),
    'gp': dict(sample_rate=16000, n_fft=2048, hop=460, win_length=2048,
               n_mels=128, fmin=50.0, fmax=7600.0),
    'ks': dict(sample_rate=16000, n_fft=1024, hop=494, win_length=1024,
               n_mels=80),
    'km': dict(sample_rate=16000, n_fft=1024, hop=496, win_length=1024,
               n_mels=80),
})
CLIPS.update({
    'd': (1, 40, None),
    'e': (3, 1003, (1003, 1, 650)),
    'f': (2, 10720, (10720, 10240)),
    'g': (1, 15218, None),
    'h': (2, 15251, (15251, 700)),
    'i': (1, 5, None),
    'gm': (1, 15218, None),
    'gp': (1, 15218, None),
    'ks': (1, 16001, None),
    'km': (1, 16001, None),
})
NEW_SHAPES = ('d', 'e', 'f', 'g', 'h', 'i')
LIMIT_PAIRS = (('g', 'gm'), ('ks', 'km'))      # (staged, memory), same audio
# make_audio's seeds ('gm' and 'gp' have (g)'s audio, 'km' has 'ks''s)
SEEDS = {'a': 11, 'b': 12, 'c': 13, 'd': 14, 'e': 15, 'f': 16, 'g': 17,
         'h': 18, 'i': 19, 'gm': 17, 'gp': 17, 'ks': 20, 'km': 20}

# The yardstick of a new shape, measured on a CPU over the clips of make_audio:
# the largest of (matmul) the error of logmel_f32_matmul against logmel,
# (sequential) the error of logmel_f32_sequential against logmel, and (ulp)
# 2^-23 max |logmel| over the real frames -- one float32 unit in the last
# place at the largest output, which neither a float32 restatement nor a
# float32 log can be asked to beat.  Two summation orders, because on the
# small shapes they differ by up to a factor of 3.  The device kernel is held
# to MEL_TOL_FACTOR x its shape's own yardstick.  MEL_F32_ERR and MEL_TOL above
# stay derived from (a) - (c) alone.
#            matmul    sequential  ulp
MEL_F32_MEASURED = {
    'd': (3.3e-7, 3.4e-7, 3.8e-7),
    'e': (2.8e-6, 2.9e-6, 6.7e-7),
    'f': (6.5e-6, 8.9e-6, 7.6e-7),
    'g': (1.2e-5, 5.2e-6, 1.2e-6),
    'h': (5.0e-6, 4.0e-6, 1.1e-6),
    'i': (1.4e-7, 2.4e-7, 1.7e-7),
    'gm': (6.6e-6, 6.4e-6, 1.2e-6),
    'gp': (9.8e-6, 4.3e-6, 1.2e-6),
    'ks': (6.5e-6, 4.1e-6, 1.1e-6),
    'km': (5.9e-6, 4.8e-6, 1.1e-6),
}
MEL_YARDSTICK_BY_SHAPE = {k: max(v) for k, v in MEL_F32_MEASURED.items()}


def shape_tol(name):
    """The device bound of a new shape: MEL_TOL_FACTOR x its own yardstick."""
    return MEL_TOL_FACTOR * MEL_YARDSTICK_BY_SHAPE[name]


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
                      fmin=0.0, fmax=None, floor=1e-10):
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
    m = p @ filterbank(sample_rate, n_fft, n_mels, fmin,
                       fmax).astype(np.float32).T
    return np.log(np.maximum(m, np.float32(floor)))


def logmel_f32_sequential(x, sample_rate, n_fft, hop, win_length, n_mels,
                          fmin=0.0, fmax=None, floor=1e-10):
    """logmel_f32_matmul with both contractions summed in another order: one
    float32 rank-1 update per sample j = 0, 1, ... of the DFT, then one per
    bin k = 0, 1, ... of the filterbank, every product and every sum rounded
    to float32."""
    f32 = np.float32
    fr = (frames(x, n_fft, hop).astype(f32) *
          hann(n_fft, win_length).astype(f32)[None, :])
    j = np.arange(n_fft)[:, None]
    k = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((j * k) % n_fft) / n_fft
    cos, sin = np.cos(ang).astype(f32), np.sin(ang).astype(f32)
    re = np.zeros((fr.shape[0], n_fft // 2 + 1), f32)
    im = np.zeros_like(re)
    for s in range(n_fft):
        re += fr[:, s:s + 1] * cos[s][None, :]
        im += fr[:, s:s + 1] * sin[s][None, :]
    p = re * re + im * im
    w = filterbank(sample_rate, n_fft, n_mels, fmin, fmax).astype(f32)
    m = np.zeros((fr.shape[0], n_mels), f32)
    for b in range(n_fft // 2 + 1):
        m += p[:, b:b + 1] * w[:, b][None, :]
    assert re.dtype == f32 and m.dtype == f32
    return np.log(np.maximum(m, f32(floor)))


def yardstick_terms(name):
    """(matmul, sequential, ulp) of shape `name` on this host: what
    MEL_F32_MEASURED records."""
    x, lengths = make_audio(name)
    kw = SHAPES[name]
    t = [0.0, 0.0, 0.0]
    for b in range(x.shape[0]):
        clip = x[b, :x.shape[1] if lengths is None else lengths[b]]
        ref = logmel(clip, **kw)
        t[0] = max(t[0], float(np.abs(logmel_f32_matmul(clip, **kw) - ref).max()))
        t[1] = max(t[1], float(np.abs(logmel_f32_sequential(clip, **kw) -
                                      ref).max()))
        t[2] = max(t[2], float(2.0 ** -23 * np.abs(ref).max()))
    return tuple(t)


def make_audio(name):
    """Seeded white noise of amplitude 0.1 plus two sinusoids, float32
    [B][T]; and the lengths (None: whole clips)."""
    B, T, lengths = CLIPS[name]
    sr = SHAPES[name]['sample_rate']
    return signal(SEEDS[name], sr, B, T), lengths


def signal(seed, sr, B, T):
    """make_audio's signal, float32 [B][T]."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / sr
    x = rng.uniform(-0.1, 0.1, (B, T))
    x += 0.3 * np.sin(2 * np.pi * 0.055 * sr * t)[None, :]
    x += 0.2 * np.sin(2 * np.pi * 0.21 * sr * t + 1.0)[None, :]
    return x.astype(np.float32)
