"""Feature normalisation restated on its own: float64 / float32 numpy, no code
shared with the package (wavenet/features.py: FeatureStats, Normalizer;
csrc/wn_features.hip).

    s1[c] = sum x,  s2[c] = sum x * x      over the real frames, in float64
    mean  = s1 / n,  std = sqrt(max(s2 / n - mean^2, 0))
    shift = float32(mean),  scale = float32(1 / max(std, min_std))
    v     = (x - shift) * scale            float32, each operation rounded
    out   = v < lo ? lo : (v > hi ? hi : v);  zeros on the padding frames
"""
import numpy as np


def real_mask(B, F, nframes):
    """bool [B, F]: frame f of clip b is real."""
    if nframes is None:
        return np.ones((B, F), bool)
    n = np.clip(np.asarray(nframes, np.int64), 0, F)
    return np.arange(F)[None, :] < n[:, None]


def sums(x, nframes=None):
    """(count, s1, s2, a1, a2): the sums of x and x^2 over the real frames of
    x [B, F, C] in float64, and of |x| and x^2 for the error bound."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    m = real_mask(x.shape[0], x.shape[1], nframes)
    rows = x[m].astype(np.float64)            # [n, C]: only the real frames
    sq = rows * rows
    return (int(m.sum()), rows.sum(0), sq.sum(0), np.abs(rows).sum(0),
            sq.sum(0))


def sum_bound(n, a):
    """|S - S'| for two float64 summation orders of n terms with sum of
    magnitudes a: each order errs by at most (n - 1) u a to first order,
    u = 2^-53; 2 n u a bounds their difference."""
    return 2.0 * n * 2.0 ** -53 * np.asarray(a, np.float64)


def mean_std(count, s1, s2):
    mean = np.asarray(s1, np.float64) / count
    var = np.asarray(s2, np.float64) / count - mean * mean
    return mean, np.sqrt(np.maximum(var, 0.0))


def shift_scale(count, s1, s2, min_std=1e-5):
    mean, std = mean_std(count, s1, s2)
    return mean.astype(np.float32), \
        (1.0 / np.maximum(std, min_std)).astype(np.float32)


def normalize(x, shift, scale, lo=-np.inf, hi=np.inf, nframes=None):
    """float32 [B, F, C], element by element."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3
    shift = np.asarray(shift, np.float32)
    scale = np.asarray(scale, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all='ignore'):
        d = np.subtract(x, shift[None, None, :], dtype=np.float32)
        v = np.multiply(d, scale[None, None, :], dtype=np.float32)
        low, high = v < lo, v > hi            # (both false for a NaN)
        out = v.copy()
        out[high] = hi
        out[low] = lo
    out[~real_mask(x.shape[0], x.shape[1], nframes)] = np.float32(0)
    return out


def motivation_clip(rate=16000, n=16000, seed=0):
    """A 0.1-amplitude tone plus noise between two stretches of silence."""
    rng = np.random.default_rng(seed)
    x = np.zeros(n, np.float32)
    lo, hi = n // 4, 3 * n // 4
    t = np.arange(hi - lo)
    x[lo:hi] = (0.1 * np.sin(2 * np.pi * 440.0 * t / rate) +
                0.01 * rng.standard_normal(hi - lo)).astype(np.float32)
    return x


def xavier(rows, cols, seed=0):
    lim = np.sqrt(6.0 / (rows + cols))
    return np.random.default_rng(seed).uniform(-lim, lim, (rows, cols))
