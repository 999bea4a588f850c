"""An independent float64 restatement of the synthesis metrics of
include/wavenet_spectral.h (wavenet/spectral.py): the STFT distance with
explicit zero padding and np.fft.rfft, the cepstral distance with a DCT table
written out by Python loops; the test signals and kernel shapes of
tests/test_gpu_spectral.py; and the yardstick its tolerances come from.  None
of it uses the package."""
import math

import numpy as np

FLOOR = 1e-7
TOL_FACTOR = 4.0

# name -> (n_fft, hop, win_length, T, lengths or None); B = 4 clips everywhere
SHAPES = {
    'tiles': (64, 1, 64, 100, None),          # four tiles, the last partial
    'idle': (192, 24, 192, 900, None),        # 4 bin chunks for 8 waves
    'oddhop': (320, 25, 300, 1000, None),     # odd hop: no LDS pad
    'nooverlap': (320, 320, 320, 11000, None),
    'r512': (512, 50, 240, 1700, None),       # 34 frames: a tile of two
    'r1024': (1024, 120, 600, 4000, None),
    'r2048': (2048, 240, 1200, 8000, (8000, 7441, 241, 1)),
    # either side of the LDS staging edge (wn_stft_distance_staged)
    'e2048s': (2048, 263, 2048, 9001, None),
    'e2048m': (2048, 264, 2048, 9001, None),
    'e1024s': (1024, 329, 1024, 11300, None),
    'e1024m': (1024, 330, 1024, 11300, None),
}
STAGED = {'e2048s': 1, 'e2048m': 0, 'e1024s': 1, 'e1024m': 0}
SEEDS = {k: 101 + i for i, k in enumerate(sorted(SHAPES))}
OUTPUTS = ('sc_num', 'sc_den', 'log_sum')

# The yardstick (the practice of tests/mel_ref.py).  Per shape and output, over
# the clips of make_pair, the largest RELATIVE error against stft_sums of two
# float32 restatements that differ in summation order -- (matmul) the DFT as a
# float32 matmul with the cos | sin basis, (sequential) one float32 rank-1
# update per sample -- and (ulp) one float32 unit in the last place, 2^-23.
# "Relative" is to the clip's own scale: the value itself for sc_num and
# sc_den, sum (|log Po| + |log Pg|) / 2 for log_sum (its terms are differences
# of logs, so its error does not shrink with its value).  The device is held,
# clip by clip, to TOL_FACTOR x the largest of the three terms x the clip's
# scale; yardstick_terms(name) reproduces a row on a CPU.  No figure here comes
# from the device.
#                      matmul   sequential  ulp
STFT_F32_MEASURED = {
    'tiles': {'sc_num': (7.3e-08, 7.3e-08, 1.2e-07),
        'sc_den': (2.3e-08, 2.4e-08, 1.2e-07),
        'log_sum': (1.3e-08, 1.1e-08, 1.2e-07)},
    'idle': {'sc_num': (2.9e-07, 2.4e-07, 1.2e-07),
        'sc_den': (8.8e-08, 6.9e-08, 1.2e-07),
        'log_sum': (2e-08, 1.4e-08, 1.2e-07)},
    'oddhop': {'sc_num': (1.7e-07, 2.2e-07, 1.2e-07),
        'sc_den': (5e-08, 4.8e-08, 1.2e-07),
        'log_sum': (2e-08, 1.6e-08, 1.2e-07)},
    'nooverlap': {'sc_num': (4.8e-07, 5.1e-07, 1.2e-07),
        'sc_den': (1.1e-07, 1.2e-07, 1.2e-07),
        'log_sum': (6.3e-08, 6.7e-08, 1.2e-07)},
    'r512': {'sc_num': (8.9e-08, 3.2e-07, 1.2e-07),
        'sc_den': (3e-08, 6.3e-08, 1.2e-07),
        'log_sum': (1.2e-08, 1.3e-08, 1.2e-07)},
    'r1024': {'sc_num': (3e-07, 4.6e-07, 1.2e-07),
        'sc_den': (4.6e-08, 1.1e-07, 1.2e-07),
        'log_sum': (1.6e-08, 1.1e-08, 1.2e-07)},
    'r2048': {'sc_num': (3.2e-07, 4e-07, 1.2e-07),
        'sc_den': (7.3e-08, 7.3e-08, 1.2e-07),
        'log_sum': (1.8e-08, 4e-08, 1.2e-07)},
    'e2048s': {'sc_num': (3.6e-07, 8.7e-07, 1.2e-07),
        'sc_den': (6e-08, 1.4e-07, 1.2e-07),
        'log_sum': (2e-08, 1.4e-08, 1.2e-07)},
    'e2048m': {'sc_num': (1.3e-07, 1.1e-06, 1.2e-07),
        'sc_den': (3.6e-08, 2.8e-07, 1.2e-07),
        'log_sum': (2.4e-08, 1.5e-08, 1.2e-07)},
    'e1024s': {'sc_num': (2.3e-07, 2.8e-07, 1.2e-07),
        'sc_den': (3.4e-08, 7.9e-08, 1.2e-07),
        'log_sum': (1.9e-08, 2e-08, 1.2e-07)},
    'e1024m': {'sc_num': (2.9e-07, 4.3e-07, 1.2e-07),
        'sc_den': (6.7e-08, 2e-07, 1.2e-07),
        'log_sum': (5.8e-08, 3e-08, 1.2e-07)},
}


def hann(n_fft, win_length):
    w = np.zeros(n_fft)
    lo = (n_fft - win_length) // 2
    for i in range(win_length):
        w[lo + i] = 0.5 * (1.0 - math.cos(2.0 * math.pi * i / win_length))
    return w


def padded(x, n_fft, hop):
    """x between explicit zeros, so that frame f of the project's grid (centre
    f * hop + hop // 2, zeros outside the clip) is padded[f * hop : f * hop +
    n_fft] for f < ceil(n / hop): what torch.stft(center=False) frames."""
    x = np.asarray(x)
    n = x.shape[0]
    F = -(-n // hop)
    left = n_fft // 2 - hop // 2
    total = (F - 1) * hop + n_fft
    return np.concatenate([np.zeros(left, x.dtype), x,
                           np.zeros(total - left - n, x.dtype)])


def frames(x, n_fft, hop):
    """[ceil(n / hop)][n_fft] frames of clip x (its dtype), zero padded."""
    n = np.asarray(x).shape[0]
    F = -(-n // hop)
    p = padded(x, n_fft, hop)
    out = np.empty((F, n_fft), p.dtype)
    for f in range(F):
        out[f] = p[f * hop:f * hop + n_fft]
    return out


def power(x, n_fft, hop, win_length):
    """|STFT|^2 of ONE clip in float64: [F][n_fft // 2 + 1]."""
    fr = frames(np.asarray(x, np.float64), n_fft, hop) * \
        hann(n_fft, win_length)[None, :]
    s = np.fft.rfft(fr, axis=1)
    return s.real ** 2 + s.imag ** 2


def _sums(pg, po, floor):
    pg, po = np.maximum(pg, floor), np.maximum(po, floor)
    mg, mo = np.sqrt(pg), np.sqrt(po)
    return (float(((mo - mg) ** 2).sum()), float((mo ** 2).sum()),
            float((np.abs(np.log(po) - np.log(pg)) * 0.5).sum()))


def stft_sums(g, o, n_fft, hop, win_length, floor=FLOOR):
    """(sc_num, sc_den, log_sum) of ONE clip pair in float64."""
    return _sums(power(g, n_fft, hop, win_length),
                 power(o, n_fft, hop, win_length), floor)


def scales(g, o, n_fft, hop, win_length, floor=FLOOR):
    """What a clip's three errors are relative to (see above)."""
    pg = np.maximum(power(g, n_fft, hop, win_length), floor)
    po = np.maximum(power(o, n_fft, hop, win_length), floor)
    s = _sums(pg, po, floor)
    return (s[0], s[1],
            float(((np.abs(np.log(po)) + np.abs(np.log(pg))) * 0.5).sum()))


def metrics(g, o, n_fft, hop, win_length, floor=FLOOR):
    """(spectral convergence, log STFT magnitude) of ONE clip pair."""
    num, den, lg = stft_sums(g, o, n_fft, hop, win_length, floor)
    F = -(-np.asarray(g).shape[0] // hop)
    return math.sqrt(num / den), lg / (F * (n_fft // 2 + 1))


# ------------------------------------------------------ float32 restatements
def _basis32(n_fft):
    j = np.arange(n_fft)[:, None]
    k = np.arange(n_fft // 2 + 1)[None, :]
    ang = 2.0 * np.pi * ((j * k) % n_fft) / n_fft
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _sums32(pg, po, floor):
    f32 = np.float32
    assert pg.dtype == f32 and po.dtype == f32
    pg, po = np.maximum(pg, f32(floor)), np.maximum(po, f32(floor))
    mg, mo = np.sqrt(pg), np.sqrt(po)
    d = (mo - mg).astype(np.float64)
    l = np.abs(np.log(po) - np.log(pg)) * f32(0.5)
    assert l.dtype == f32 and mo.dtype == f32
    return (float((d * d).sum()), float((mo.astype(np.float64) ** 2).sum()),
            float(l.astype(np.float64).sum()))


def stft_f32_matmul(g, o, n_fft, hop, win_length, floor=FLOOR):
    """The kernel's rule in float32 numpy: float32 tables (rounded from
    float64), the DFT as a float32 matmul, float32 sqrt and log, the terms
    summed in float64."""
    f32 = np.float32
    cos, sin = _basis32(n_fft)
    w = hann(n_fft, win_length).astype(f32)[None, :]
    p = []
    for x in (g, o):
        fr = frames(np.asarray(x, f32), n_fft, hop) * w
        re, im = fr @ cos, fr @ sin
        p.append(re * re + im * im)
    return _sums32(p[0], p[1], floor)


def stft_f32_sequential(g, o, n_fft, hop, win_length, floor=FLOOR):
    """stft_f32_matmul with the DFT summed in another order: one float32
    rank-1 update per sample j = 0, 1, ..."""
    f32 = np.float32
    cos, sin = _basis32(n_fft)
    w = hann(n_fft, win_length).astype(f32)[None, :]
    p = []
    for x in (g, o):
        fr = frames(np.asarray(x, f32), n_fft, hop) * w
        re = np.zeros((fr.shape[0], n_fft // 2 + 1), f32)
        im = np.zeros_like(re)
        for s in range(n_fft):
            re += fr[:, s:s + 1] * cos[s][None, :]
            im += fr[:, s:s + 1] * sin[s][None, :]
        p.append(re * re + im * im)
    return _sums32(p[0], p[1], floor)


def yardstick_terms(name):
    """{output: (matmul, sequential, ulp)} of shape `name` on this host: what
    STFT_F32_MEASURED records."""
    n_fft, hop, win, T, lengths = SHAPES[name]
    g, o = make_pair(name)
    t = np.zeros((3, 3))
    t[:, 2] = 2.0 ** -23
    for b in range(g.shape[0]):
        n = T if lengths is None else lengths[b]
        gb, ob = g[b, :n], o[b, :n]
        ref = stft_sums(gb, ob, n_fft, hop, win)
        sc = scales(gb, ob, n_fft, hop, win)
        for col, fn in enumerate((stft_f32_matmul, stft_f32_sequential)):
            got = fn(gb, ob, n_fft, hop, win)
            for k in range(3):
                t[k, col] = max(t[k, col], abs(got[k] - ref[k]) / sc[k])
    return {OUTPUTS[k]: tuple(float(v) for v in t[k]) for k in range(3)}


def rel_tol(name, output):
    """The device's relative bound for an output of a shape: TOL_FACTOR x the
    largest recorded term."""
    return TOL_FACTOR * max(STFT_F32_MEASURED[name][output])


# ------------------------------------------------------------------ signals
def original(rng, T, f0=0.011):
    """Harmonics + noise, float64 [T]."""
    t = np.arange(T)
    x = 0.01 * rng.standard_normal(T)
    for h, a in ((1, 0.3), (2, 0.2), (3, 0.1), (7, 0.05)):
        x += a * np.sin(2 * np.pi * f0 * h * t + rng.uniform(0, 2 * np.pi))
    return x


def generated(rng, x, gain=0.8, snr_db=20.0):
    """gain * x + white noise at snr_db below gain * x."""
    y = gain * x
    rms = math.sqrt(float(np.mean(y * y))) if y.size else 0.0
    return y + rms * 10.0 ** (-snr_db / 20.0) * rng.standard_normal(x.shape[0])


def make_pair(name):
    """(generated, original), float32 [4][T] each, seeded: clip 0 the plain
    pair; clip 1 the pair with a shared stretch of zeros in the middle; clip 2
    a silent generated clip against a loud original; clip 3 another plain
    pair (other pitch, 6 dB quieter)."""
    T = SHAPES[name][3]
    rng = np.random.default_rng(SEEDS[name])
    o = np.stack([original(rng, T), original(rng, T, 0.017),
                  original(rng, T, 0.023), 0.5 * original(rng, T, 0.031)])
    g = np.stack([generated(rng, o[b]) for b in range(4)])
    lo, hi = T // 3, T // 3 + max(1, T // 4)
    o[1, lo:hi] = 0.0
    g[1, lo:hi] = 0.0
    g[2] = 0.0
    return g.astype(np.float32), o.astype(np.float32)


# ----------------------------------------------------------------- cepstra
def dct_table(C, K):
    """[K][C] float64, element by element: sqrt(2 / C) cos(pi n (m + 1/2) / C),
    n = 1 .. K."""
    t = np.zeros((K, C))
    for n in range(1, K + 1):
        for m in range(C):
            t[n - 1, m] = math.sqrt(2.0 / C) * math.cos(
                math.pi * n * (m + 0.5) / C)
    return t


def mcd_sums(a, b, nframes, order):
    """(mcd_sum [B], bound [B]) of float32 [B][F][C] raw log-mel tensors in
    float64: per real frame d = a - b (ONE float32 subtraction, the rule's),
    e = dct d, r = sqrt(0.5 sum e^2), summed over the clip's real frames.

    The bound, for a device that follows the rule in float64 in ANY order.
    Two float64 evaluations of e[n], a sum of C products, differ by at most
    2 gamma_C sum_m |dct[n][m] d[m]| with gamma_C ~ C 2^-53, and the two
    tables by an ulp per entry, (1 + 2) 2^-53 more per product: taken together
    de[n] <= 2 C 2^-52 sum_m |dct[n][m] d[m]|.  r = |e| / sqrt 2 is Lipschitz
    in e with constant 1 / sqrt 2, so dr <= sqrt(0.5 sum de[n]^2), plus the
    roundings of the K squares and their sum, the product and the square root:
    (K + 4) 2^-53 r each side.  The F additions of the frames add F 2^-53
    mcd_sum each side.  bound = sum_f sqrt(0.5 sum_n de[n]^2) +
    (F + K + 4) 2^-52 mcd_sum."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    B, F, C = a.shape
    t = dct_table(C, order)
    d = (a - b).astype(np.float64)
    out, bound = np.zeros(B), np.zeros(B)
    for i in range(B):
        n = F if nframes is None else int(nframes[i])
        for f in range(n):
            e = t @ d[i, f]
            de = 2.0 * C * 2.0 ** -52 * (np.abs(t) @ np.abs(d[i, f]))
            out[i] += math.sqrt(0.5 * float((e * e).sum()))
            bound[i] += math.sqrt(0.5 * float((de * de).sum()))
        bound[i] += (F + order + 4) * 2.0 ** -52 * out[i]
    return out, bound


def mcd_db(a, b, nframes, order):
    s, _ = mcd_sums(a, b, nframes, order)
    n = a.shape[0] * a.shape[1] if nframes is None else int(np.sum(nframes))
    return 10.0 / math.log(10.0) * float(s.sum()) / n


def logmel_pair(seed, B, F, C):
    """Two raw log-mel-like float32 tensors [B][F][C] in the range of
    log(max(M, 1e-10))."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-23.0, 7.0, (B, F, C))
    b = a + rng.normal(0.0, 1.5, (B, F, C))
    return a.astype(np.float32), b.astype(np.float32)
