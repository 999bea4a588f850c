"""Float64 oracle of the pitch tracker (wavenet/pitch.py, csrc/wn_pitch.hip,
include/wavenet_pitch.h).  It shares no code with the package: frames are cut
out of an explicitly zero-padded copy, the sums are plain numpy or loops.

    tau_min = max(2, floor(sr / fmax)), tau_max = ceil(sr / fmin)
    F = ceil(n / hop); frame f is centred at c = f * hop + hop // 2 and holds
    y[j] = x[c - (W + tau_max) // 2 + j], j < W + tau_max, zeros outside [0, n)
    e = sum_{j<W} y[j]^2; e <= silence * W: silent (f0 0, aper 1, lag 0, c' 1)
    d[tau] = sum_{j<W} (y[j] - y[j + tau])^2, S[tau] = d[1] + .. + d[tau]
    c'[tau] = d[tau] tau / S[tau] where S[tau] > 0 else 1; c'[0] = 1
    pick: the first tau in [tau_min, tau_max - 1] under the threshold, then
    down the slope (voiced); else the first minimum of that range (unvoiced)
    voiced: f0 = sr / (tau + delta), the parabola through c'[tau - 1 .. tau + 1]

and, besides the oracle: two float32 restatements of d (the yardstick of the
device's tolerance), `decisive` (the frames whose pick no error of that size
can change), the derived F0 tolerance, the test signals and shapes, and numpy
statements of pitch.f0_error and PitchTracker.channels.
"""
import math

import numpy as np

DEFAULTS = dict(hop=256, fmin=60.0, fmax=500.0, window=1024, threshold=0.15,
                silence=1e-7)

# ---- the GPU test's shapes (settings; B, T, lengths)
#   a  the defaults at 16 kHz; three clips, one cut inside a frame, one shorter
#      than two hops: 24 frames, lags 32 .. 267 (67 lag groups: one wave and
#      three lanes of the second per segment)
#   b  hop 1, the smallest window, lags 2 .. 9 (two lag groups, pad lags 9 ..
#      12 computed and dropped): 70 frames
#   c  the largest on-chip footprint: window 2048, tau_max 1024 (an exact
#      division), odd hop
#   d1 tau_min = 2 (fmax = sr / 2) with tau_max 267, d2 with tau_max 65:
#      neither a multiple of 4 nor of 64
#   e1 one sample; e2 a clip shorter than one hop; e3 hop 4096 > window
SHAPES = {
    'a': dict(sample_rate=16000),
    'b': dict(sample_rate=8000, hop=1, window=64, fmin=900.0, fmax=4000.0),
    'c': dict(sample_rate=48000, hop=461, window=2048, fmin=46.875,
              fmax=500.0),
    'd1': dict(sample_rate=16000, hop=100, window=128, fmin=60.0,
               fmax=8000.0),
    'd2': dict(sample_rate=8000, hop=100, window=128, fmin=124.0,
               fmax=4000.0),
    'e1': dict(sample_rate=16000),
    'e2': dict(sample_rate=16000),
    'e3': dict(sample_rate=16000, hop=4096),
}
CLIPS = {
    'a': (3, 6000, (6000, 4097, 300)),
    'b': (1, 70, None),
    'c': (1, 5000, None),
    'd1': (2, 1500, (1500, 777)),
    'd2': (1, 1500, None),
    'e1': (1, 1, None),
    'e2': (1, 100, None),
    'e3': (1, 9000, None),
}
SEEDS = {'a': 31, 'b': 32, 'c': 33, 'd1': 34, 'd2': 35, 'e1': 36, 'e2': 37,
         'e3': 38}
LAGS = {'a': (32, 267), 'b': (2, 9), 'c': (96, 1024), 'd1': (2, 267),
        'd2': (2, 65), 'e1': (32, 267), 'e2': (32, 267), 'e3': (32, 267)}

# The yardstick of a shape, measured on a CPU over the clips of make_audio
# (yardstick_terms): the largest error on c' of (sequential) cmnd_f32 with d
# summed in float32 one j after the other, and of (pairwise) cmnd_f32 with
# numpy's pairwise float32 sum, S in float64 both times, against cmnd64; and
# 2^-23.  The device is held to PITCH_TOL_FACTOR x the largest of the three,
# the project's usual margin over its float32 yardstick (tests/mel_ref.py).
#              sequential  pairwise  2^-23
PITCH_F32_MEASURED = {
    'a': (3.0e-6, 1.3e-6, 2.0 ** -23),
    'b': (2.0e-7, 1.4e-7, 2.0 ** -23),
    'c': (5.6e-6, 3.8e-7, 2.0 ** -23),
    'd1': (9.4e-7, 2.5e-7, 2.0 ** -23),
    'd2': (8.1e-7, 3.0e-7, 2.0 ** -23),
    'e1': (0.0, 0.0, 2.0 ** -23),
    'e2': (4.8e-7, 1.7e-7, 2.0 ** -23),
    'e3': (2.0e-6, 3.1e-7, 2.0 ** -23),
}
PITCH_TOL_FACTOR = 4.0

# Steady three-harmonic tones at 16 kHz with the defaults: the largest
# |f0 / f - 1| of the oracle over the interior frames (tone_error), measured
# here; the test holds the oracle and the package's reference to TONE_BOUND.
TONES = (62.0, 80.0, 123.4, 220.0, 440.0, 495.0)
TONE_ERR_MEASURED = {62.0: 8.8e-6, 80.0: 1.9e-5, 123.4: 2.2e-5, 220.0: 7.6e-5,
                     440.0: 3.0e-4, 495.0: 4.4e-4}
TONE_BOUND = 5e-4           # the largest of them (495 Hz), rounded up

# Inputs whose rows are ties: every c' of a frame equal to 1, so that no pick
# is decisive although the device's values are exact (d = 0 throughout, or
# d[tau] = 2 v^2 for every tau: S[tau] = tau d exactly in float64, c' = 1).
# The GPU test asserts those frames exactly: c' all 1, unvoiced, lag tau_min.
#   one      a clip of one sample
#   constant 0.25 throughout: the frames clear of the clip's edges
TIES = {'one': np.full(1, 0.3, np.float32),
        'constant': np.full(3000, 0.25, np.float32)}


def shape_tol(name):
    """The device's bound on c' for shape `name`, and the m of `decisive`."""
    return PITCH_TOL_FACTOR * max(PITCH_F32_MEASURED[name])


def settings(name):
    return dict(DEFAULTS, **SHAPES[name])


def lag_range(sample_rate, fmin, fmax):
    return (max(2, int(math.floor(sample_rate / fmax))),
            int(math.ceil(sample_rate / fmin)))


def frames(x, hop, window, tau_max, dtype=np.float64):
    """[ceil(n / hop)][window + tau_max] frames of clip x, zero padded."""
    x = np.asarray(x, dtype)
    n = x.shape[0]
    N = window + tau_max
    F = -(-n // hop)
    padded = np.concatenate([np.zeros(N, dtype), x, np.zeros(N + hop, dtype)])
    out = np.empty((F, N), dtype)
    for f in range(F):
        start = f * hop + hop // 2 - N // 2 + N
        out[f] = padded[start:start + N]
    return out


def _normalise(d, e, window, silence):
    """c' [F][tau_max + 1] float64 from d [F][tau_max + 1] (d[:, 0] unused)
    and the frames' energies; silent rows are all 1."""
    F, n1 = d.shape
    c = np.ones((F, n1))
    for f in range(F):
        if e[f] <= silence * window:
            continue
        s = 0.0
        for tau in range(1, n1):
            s += float(d[f, tau])
            if s > 0:
                c[f, tau] = float(d[f, tau]) * tau / s
    return c


def cmnd64(x, sample_rate, hop, fmin, fmax, window, threshold, silence):
    """(c' float64 [F][tau_max + 1], e float64 [F]) of ONE clip x [n]."""
    _, tau_max = lag_range(sample_rate, fmin, fmax)
    y = frames(x, hop, window, tau_max)
    e = (y[:, :window] ** 2).sum(1)
    d = np.zeros((y.shape[0], tau_max + 1))
    for tau in range(1, tau_max + 1):
        d[:, tau] = ((y[:, :window] - y[:, tau:tau + window]) ** 2).sum(1)
    return _normalise(d, e, window, silence), e


def cmnd_f32(x, order, sample_rate, hop, fmin, fmax, window, threshold,
             silence):
    """c' with e and d summed in float32 -- order 'sequential': one j after
    the other, every product and sum rounded; 'pairwise': numpy's sum -- and
    S and the quotient in float64, rounded to float32 once."""
    f32 = np.float32
    _, tau_max = lag_range(sample_rate, fmin, fmax)
    y = frames(x, hop, window, tau_max, f32)
    F = y.shape[0]
    d = np.zeros((F, tau_max + 1), f32)
    if order == 'sequential':
        e = np.zeros(F, f32)
        for j in range(window):
            v = y[:, j:j + 1] - y[:, j + 1:j + 1 + tau_max]
            d[:, 1:] += v * v
            e += y[:, j] * y[:, j]
    else:
        e = (y[:, :window] * y[:, :window]).sum(1, dtype=f32)
        for tau in range(1, tau_max + 1):
            v = y[:, :window] - y[:, tau:tau + window]
            d[:, tau] = (v * v).sum(1, dtype=f32)
    assert d.dtype == f32 and e.dtype == f32
    return _normalise(d, e, window, f32(silence)).astype(f32)


def pick(c, tau_min, tau_max, threshold):
    """(lag, voiced, comparisons) of one row c'[0 .. tau_max]; comparisons:
    the (tau, tau + 1) pairs the walk down the slope compared."""
    for tau in range(tau_min, tau_max):
        if c[tau] < threshold:
            seen = []
            while tau + 1 <= tau_max - 1:
                seen.append((tau, tau + 1))
                if not c[tau + 1] < c[tau]:
                    break
                tau += 1
            return tau, True, seen
    best = tau_min
    for tau in range(tau_min, tau_max):
        if c[tau] < c[best]:
            best = tau
    return best, False, []


def parabola(c, tau):
    """(delta, den) of a voiced pick."""
    a, b, g = c[tau - 1], c[tau], c[tau + 1]
    den = a - 2.0 * b + g
    if not den > 0:
        return 0.0, den
    return min(max(0.5 * (a - g) / den, -0.5), 0.5), den


def track(x, **kw):
    """The oracle of ONE clip x [n]: dict of f0, aper float64 [F], lag int
    [F], voiced bool [F], silent bool [F], cmnd [F][tau_max + 1], den [F]
    (the parabola's, voiced frames), e [F]."""
    tau_min, tau_max = lag_range(kw['sample_rate'], kw['fmin'], kw['fmax'])
    c, e = cmnd64(x, **kw)
    F = c.shape[0]
    out = dict(f0=np.zeros(F), aper=np.ones(F), lag=np.zeros(F, np.int64),
               voiced=np.zeros(F, bool), cmnd=c, den=np.zeros(F), e=e,
               silent=e <= kw['silence'] * kw['window'])
    for f in range(F):
        if out['silent'][f]:
            continue
        tau, voiced, _ = pick(c[f], tau_min, tau_max, kw['threshold'])
        out['lag'][f], out['aper'][f], out['voiced'][f] = tau, c[f, tau], voiced
        if voiced:
            delta, out['den'][f] = parabola(c[f], tau)
            out['f0'][f] = kw['sample_rate'] / (tau + delta)
    return out


def decisive(c, m, tau_min, tau_max, threshold):
    """True where no perturbation of every value of the row c'[0 .. tau_max]
    by at most m can change (lag, voiced).  Conservative -- true only when
    all of these hold: the picks at threshold - m and threshold + m agree
    with the pick at threshold; every comparison of the walk down the slope
    has a gap > 2 m; a voiced frame's two neighbours exceed its minimum by
    > 2 m and 3 m / den <= 0.25; an unvoiced frame's minimum is below every
    other value of the range by > 2 m (the adjacent ones included: the lag is
    asserted exactly)."""
    tau, voiced, seen = pick(c, tau_min, tau_max, threshold)
    for t in (threshold - m, threshold + m):
        if pick(c, tau_min, tau_max, t)[:2] != (tau, voiced):
            return False
    for i, j in seen:
        if not abs(c[j] - c[i]) > 2 * m:
            return False
    if voiced:
        if not (c[tau - 1] - c[tau] > 2 * m and c[tau + 1] - c[tau] > 2 * m):
            return False
        den = parabola(c, tau)[1]
        return bool(den > 0 and 3 * m / den <= 0.25)
    others = [c[i] for i in range(tau_min, tau_max) if i != tau]
    return bool(min(others) - c[tau] > 2 * m)


def decisive_frames(ref, m, **kw):
    """bool [F] over a `track` result: `decisive` rows that are also clear of
    the silence decision (e <= half or e >= twice silence * window)."""
    tau_min, tau_max = lag_range(kw['sample_rate'], kw['fmin'], kw['fmax'])
    lim = kw['silence'] * kw['window']
    out = np.zeros(ref['lag'].shape[0], bool)
    for f in range(out.shape[0]):
        if ref['silent'][f]:
            out[f] = ref['e'][f] <= 0.5 * lim
        else:
            out[f] = ref['e'][f] >= 2.0 * lim and decisive(
                ref['cmnd'][f], m, tau_min, tau_max, kw['threshold'])
    return out


def f0_tol(ref, m, sample_rate):
    """Per frame, for the voiced frames of a `track` result: with every c'
    off by at most m, the parabola's numerator 0.5 (a - g) moves by at most
    m and its denominator by at most 4 m, so to first order, for |delta| <=
    1 / 2, |d delta| <= 3 m / den (`decisive` requires 3 m / den <= 1 / 4),
    hence
        |d f0| <= f0 (3 m / den) / (tau + delta) + 4 ulp(f0)
    the ulps for the float32 interpolation and division.  (1 / (tau + delta)
    is f0 / sample_rate.)"""
    f0 = ref['f0']
    den = np.where(ref['den'] > 0, ref['den'], 1.0)
    ulp = np.spacing(f0.astype(np.float32)).astype(np.float64)
    return f0 * (3 * m / den) * (f0 / sample_rate) + 4 * ulp


# ---------------------------------------------------------------- signals
def signal(seed, sr, B, T, hop, window, fmin, fmax):
    """Seeded, float32 [B][T], five stretches:
      glide     a three-harmonic glide from 0.5 fmax upwards, plus noise of
                amplitude 1e-3, over the first 35 % and behind the constant
      noise     amplitude 0.1, the next 12 %
      zeros     exact, up to the constant stretch
      constant  0.25 over window + tau_min - 1 samples (at most 19 % of the
                clip) from the first frame start at or behind 68 %: a frame
                there has d[tau] = 0 and S[tau] = 0, so c'[tau] = 1, for
                every tau < tau_min, and no frame is constant throughout
                (all c' equal: no pick is decisive)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    tau_min, tau_max = lag_range(sr, fmin, fmax)
    N = window + tau_max
    a, b, c = int(0.35 * T), int(0.47 * T), int(0.68 * T)
    length = min(window + tau_min - 1, int(0.19 * T))
    if length == window + tau_min - 1:
        f = max(0, -(-(c - hop // 2 + N // 2) // hop))
        c = f * hop + hop // 2 - N // 2         # that frame's first sample
    x = np.zeros((B, T))
    for i in range(B):
        f = fmax * (0.5 + 0.1 * t / max(T, 2) + 0.02 * i)
        ph = 2 * np.pi * np.cumsum(f) / sr
        x[i] = 0.4 * np.sin(ph) + 0.2 * np.sin(2 * ph + 1.0) + \
            0.1 * np.sin(3 * ph + 2.0) + rng.uniform(-1e-3, 1e-3, T)
        x[i, a:b] = rng.uniform(-0.1, 0.1, b - a)
        x[i, b:c] = 0.0
        x[i, c:c + length] = 0.25
    return x.astype(np.float32)


def make_audio(name):
    """(audio float32 [B][T], lengths or None) of shape `name`."""
    B, T, lengths = CLIPS[name]
    kw = settings(name)
    x = signal(SEEDS[name], kw['sample_rate'], B, T, kw['hop'], kw['window'],
               kw['fmin'], kw['fmax'])
    if T == 1:
        # one sample v gives d[tau] = 2 v^2 for every tau: c' = 1 throughout,
        # a tie that no pick decides (TIES holds that input, checked exactly);
        # the one-sample clip of the shapes is the silent one
        x[:] = 0
    return x, lengths


def clips(name):
    """The clips of make_audio cut to their lengths."""
    x, lengths = make_audio(name)
    return [x[b, :x.shape[1] if lengths is None else lengths[b]]
            for b in range(x.shape[0])]


def yardstick_terms(name):
    """(sequential, pairwise, 2^-23) of shape `name` on this host: what
    PITCH_F32_MEASURED records."""
    kw = settings(name)
    t = [0.0, 0.0, 2.0 ** -23]
    for clip in clips(name):
        ref = cmnd64(clip, **kw)[0]
        for k, order in enumerate(('sequential', 'pairwise')):
            got = cmnd_f32(clip, order, **kw).astype(np.float64)
            t[k] = max(t[k], float(np.abs(got - ref).max()))
    return tuple(t)


def tone(f, sr=16000, T=8000):
    """A steady three-harmonic tone, float32 [T]."""
    ph = 2 * np.pi * f * np.arange(T) / sr
    return (0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 0.7) +
            0.125 * np.sin(3 * ph + 1.9)).astype(np.float32)


def interior(F, T, hop, window, tau_max):
    """The frames whose window + tau_max samples lie inside [0, T)."""
    N = window + tau_max
    return [f for f in range(F)
            if f * hop + hop // 2 - N // 2 >= 0 and
            f * hop + hop // 2 - N // 2 + N <= T]


def tone_error(f, sr=16000):
    """The largest |f0 / f - 1| of the oracle over the interior frames of
    tone(f) with the defaults (inf where one of them is unvoiced)."""
    kw = dict(DEFAULTS, sample_rate=sr)
    x = tone(f, sr)
    ref = track(x, **kw)
    _, tau_max = lag_range(sr, kw['fmin'], kw['fmax'])
    idx = interior(ref['f0'].shape[0], x.shape[0], kw['hop'], kw['window'],
                   tau_max)
    assert idx
    if not ref['voiced'][idx].all():
        return float('inf')
    return float(np.abs(ref['f0'][idx] / f - 1.0).max())


# ---------------------------------------------------- f0_error / channels
def f0_error(fa, fb, nframes=None):
    """numpy statement of pitch.f0_error: dict of per-clip arrays."""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    B, F = fa.shape
    out = {k: np.zeros(B, np.int64) for k in
           ('frames', 'both', 'gross', 'fine', 'vuv', 'voiced_ref')}
    out['sq_cents'] = np.zeros(B)
    for b in range(B):
        n = F if nframes is None else int(nframes[b])
        for f in range(n):
            a, r = fa[b, f], fb[b, f]
            out['frames'][b] += 1
            out['voiced_ref'][b] += r > 0
            out['vuv'][b] += (a > 0) != (r > 0)
            if a > 0 and r > 0:
                out['both'][b] += 1
                if abs(a / r - 1.0) > 0.2:
                    out['gross'][b] += 1
                else:
                    out['fine'][b] += 1
                    out['sq_cents'][b] += (1200.0 * math.log2(a / r)) ** 2
    return out


def f0_summary(e):
    tot = {k: float(v.sum()) for k, v in e.items()}
    return {'f0_rmse_cents': math.sqrt(tot['sq_cents'] / tot['fine'])
            if tot['fine'] else None,
            'gross_pitch_error': tot['gross'] / tot['both']
            if tot['both'] else None,
            'vuv_error': tot['vuv'] / tot['frames'],
            'voiced_frames': int(tot['voiced_ref']),
            'frames': int(tot['frames'])}


def channels(f0, fmin, fmax, nframes=None):
    """numpy statement of PitchTracker.channels: float32 [B][F][2]."""
    f0 = np.asarray(f0, np.float64)
    B, F = f0.shape
    out = np.zeros((B, F, 2), np.float32)
    for b in range(B):
        n = F if nframes is None else int(nframes[b])
        for f in range(n):
            if f0[b, f] > 0:
                v = math.log2(f0[b, f] / fmin) / math.log2(fmax / fmin)
                out[b, f, 0] = np.float32(min(max(v, 0.0), 1.0))
                out[b, f, 1] = 1.0
    return out
