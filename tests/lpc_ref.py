"""Linear prediction restated independently of wavenet/lpc.py, in float64, and
the fixtures its tests share (16 kHz).

The restatement shares no code path with the rule it checks:
  * the autocorrelation is an explicit np.fft.irfft of the clipped power
    spectrum, not a table of cosines summed bin by bin;
  * the coefficients are np.linalg.solve of the Toeplitz normal equations
    R a = r[1:], not Levinson-Durbin -- so it checks Levinson-Durbin;
  * the two filters are Python loops in the defining direct form, the
    coefficient of tap i taken from the frame of sample t - i.
Only the tables (the float32 pseudo-inverse, the lag window) are the rule's.
"""
import functools

import numpy as np

SR = 16000
R0_FLOOR = 1e-30

# (name, order, n_mels, n_fft, hop): the shapes of the coefficient tests.
# Orders 1, 2, 15, 16, 17, 32; n_mels 8, 80, 128; n_fft 64, 1024, 2048.
CASES = [('o1', 1, 80, 1024, 256), ('o2m8', 2, 8, 64, 16),
         ('o15', 15, 80, 1024, 256), ('o16', 16, 80, 1024, 256),
         ('o17m128', 17, 128, 2048, 512), ('o32', 32, 80, 1024, 256),
         ('o32m8', 32, 8, 64, 16), ('o16m128', 16, 128, 2048, 512)]
CASE = {c[0]: c for c in CASES}
FRAMES = 24                     # frames per coefficient case


def make_lp(order=16, n_mels=80, n_fft=1024, hop=256, **kw):
    from wavenet import features, lpc
    return lpc.LinearPrediction(
        features.MelSpec(SR, n_fft=n_fft, hop=hop, n_mels=n_mels),
        order=order, **kw)


def case_lp(name):
    return make_lp(*CASE[name][1:])


# ------------------------------------------------------------------ fixtures
def _resonate(x):
    """x through four two-pole resonators (a vowel's formants)."""
    y = np.asarray(x, np.float64)
    for fc, bw in ((700.0, 80.0), (1200.0, 100.0), (2600.0, 150.0),
                   (3500.0, 200.0)):
        r = np.exp(-np.pi * bw / SR)
        a1, a2 = -2.0 * r * np.cos(2.0 * np.pi * fc / SR), r * r
        out = np.zeros_like(y)
        p1 = p2 = 0.0
        for t in range(y.shape[0]):
            v = y[t] - a1 * p1 - a2 * p2
            out[t] = v
            p2, p1 = p1, v
        y = out
    return y


# the 2 s fixture's stretches, in samples
VOICED = (0, 12800)
UNVOICED = (12800, 19200)
SILENT = (19200, 24000)
QUIET = (24000, 32000)


@functools.lru_cache(maxsize=None)
def vowel():
    """float32 [32000]: a 125 Hz pulse train plus noise through four
    resonators (0 - 0.8 s), noise alone through them (- 1.2 s), exact zeros
    (- 1.5 s), the voiced signal again at 1e-3 of the amplitude (- 2 s);
    max |x| = 0.5."""
    rng = np.random.default_rng(20240917)
    n = 32000
    src = np.zeros(n)
    src[::128] = 1.0
    src += 0.01 * rng.standard_normal(n)
    src[UNVOICED[0]:UNVOICED[1]] = 0.05 * rng.standard_normal(
        UNVOICED[1] - UNVOICED[0])
    y = _resonate(src)
    y *= 0.5 / np.abs(y[:VOICED[1]]).max()
    y[UNVOICED[0]:UNVOICED[1]] *= 0.5
    y[SILENT[0]:SILENT[1]] = 0.0
    y[QUIET[0]:QUIET[1]] = 1e-3 * y[:QUIET[1] - QUIET[0]]
    out = y.astype(np.float32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def white():
    """float32 [8000]: white Gaussian noise, sigma 0.1."""
    out = (0.1 * np.random.default_rng(7).standard_normal(8000)
           ).astype(np.float32)
    out.setflags(write=False)
    return out


def logmel(x, lp):
    """Raw log-mel frames float32 [F, n_mels] of x under lp's front end, from
    the float64 rule of the front end."""
    from wavenet import features
    return features.logmel_reference(
        x, lp.spec.with_normalizer(None), np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def vowel_frames():
    """The default front end's (80 mels, n_fft 1024, hop 256) raw log-mel
    frames of `vowel`, float32 [125, 80]."""
    out = logmel(vowel(), make_lp())
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def white_frames():
    out = logmel(white(), make_lp())
    out.setflags(write=False)
    return out


NAN_FRAME, INF_FRAME = 3, 6


@functools.lru_cache(maxsize=None)
def broken_frames():
    """float32 [10, 80]: frames of the vowel with one frame holding a NaN mel
    (frame 3) and one of -inf mels (frame 6)."""
    fr = np.array(vowel_frames()[20:30])
    fr[NAN_FRAME, 11] = np.nan
    fr[INF_FRAME, :] = -np.inf
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def case_frames(name):
    """float32 [FRAMES, n_mels]: raw log-mel frames of the vowel fixture under
    the case's front end, FRAMES of them spread evenly over the clip (voiced,
    unvoiced, silent and quiet stretches all occur)."""
    lp = case_lp(name)
    fr = logmel(vowel(), lp)
    pick = np.linspace(0, fr.shape[0] - 1, FRAMES).round().astype(int)
    out = np.ascontiguousarray(fr[pick])
    out.setflags(write=False)
    return out


# ------------------------------------------------- the float64 restatement
def power64(lp, frames):
    """float64 [F, n_bins]: max(pinv @ exp(frames), 0) with the float32 table
    the device gets, everything else float64."""
    with np.errstate(all='ignore'):
        M = np.exp(np.asarray(frames, np.float32).astype(np.float64))
        P = M @ lp.pinv.astype(np.float64).T
        return np.where(P < 0, 0.0, P)


def autocorrelation64(lp, P):
    """float64 [F, order + 1]: irfft of the power spectrum, lag-windowed."""
    with np.errstate(all='ignore'):
        r = np.fft.irfft(np.asarray(P, np.float64), n=lp.n_fft, axis=-1)
        return r[..., :lp.order + 1] * lp.lagwin


def solve64(r):
    """The predictor of the autocorrelation r [p + 1]: a [p] with x[t] ~
    sum_i a[i - 1] x[t - i], from the Toeplitz normal equations."""
    r = np.asarray(r, np.float64)
    p = r.shape[0] - 1
    idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
    return np.linalg.solve(r[idx], r[1:])


def toeplitz_cond(r):
    r = np.asarray(r, np.float64)
    p = r.shape[0] - 1
    idx = np.abs(np.arange(p)[:, None] - np.arange(p)[None, :])
    return float(np.linalg.cond(r[idx]))


def coefficients_from_power(lp, P):
    """float64 [F, order] from a power spectrum [F, n_bins] (any float type):
    irfft, lag window, Toeplitz solve; zeros where !(r[0] > 1e-30)."""
    r = autocorrelation64(lp, np.asarray(P).astype(np.float64))
    out = np.zeros((r.shape[0], lp.order))
    for f in range(r.shape[0]):
        if r[f, 0] > R0_FLOOR and np.isfinite(r[f]).all():
            out[f] = solve64(r[f])
    return out


def coefficients64(lp, frames):
    return coefficients_from_power(lp, power64(lp, frames))


def power32_matmul(lp, frames):
    """float32 restatement one: P as one float32 matmul."""
    with np.errstate(all='ignore'):
        M = np.exp(np.asarray(frames, np.float32))
        P = (M @ lp.pinv.T).astype(np.float32)
        return np.where(P < 0, np.float32(0), P)


def power32_rank1(lp, frames):
    """float32 restatement two: rank-1 updates, the mels in DESCENDING
    order."""
    f32 = np.float32
    with np.errstate(all='ignore'):
        M = np.exp(np.asarray(frames, f32))
        P = np.zeros((M.shape[0], lp.n_bins), f32)
        for m in range(lp.n_mels - 1, -1, -1):
            P = (P + (M[:, m, None] * lp.pinv[None, :, m]).astype(f32)
                 ).astype(f32)
        return np.where(P < 0, f32(0), P)


def yardstick(lp, frames):
    """(c64 [F, order], tol [F]): the float64 coefficients and what a float32
    implementation of the power spectrum may differ from them by, per frame:
    four times (the larger error of the two float32 restatements over the
    case's frames + one float32 ulp of the frame's largest coefficient)."""
    c64 = coefficients64(lp, frames)
    err = max(np.abs(coefficients_from_power(lp, power32_matmul(lp, frames))
                     - c64).max(),
              np.abs(coefficients_from_power(lp, power32_rank1(lp, frames))
                     - c64).max())
    ulp = np.spacing(np.abs(c64).max(axis=1).astype(np.float32)
                     ).astype(np.float64)
    return c64, 4.0 * (err + ulp)


# ------------------------------------------------------------- the filters
def analysis64(x, coeffs, hop, gain=1.0):
    """e[t] = (x[t] - sum_{i=1..p, t-i>=0} c[(t-i)//hop][i-1] x[t-i]) gain,
    float64, a loop over the samples."""
    x = np.asarray(x, np.float64)
    c = np.asarray(coeffs, np.float64)
    p = c.shape[1]
    e = np.zeros_like(x)
    for t in range(x.shape[0]):
        acc = 0.0
        for i in range(min(p, t), 0, -1):
            acc += c[(t - i) // hop, i - 1] * x[t - i]
        e[t] = (x[t] - acc) * gain
    return e


def synthesis64(e, coeffs, hop, gain=1.0):
    """y[t] = e[t] / gain + sum_{i=1..p, t-i>=0} c[(t-i)//hop][i-1] y[t-i]."""
    e = np.asarray(e, np.float64)
    c = np.asarray(coeffs, np.float64)
    p = c.shape[1]
    y = np.zeros_like(e)
    for t in range(e.shape[0]):
        acc = 0.0
        for i in range(min(p, t), 0, -1):
            acc += c[(t - i) // hop, i - 1] * y[t - i]
        y[t] = e[t] / gain + acc
    return y


def analysis32_direct(x, coeffs, hop, gain=1.0):
    """The analysis rule in float32 as the header writes it, sample by sample
    and tap by tap (slow; for short clips)."""
    f32 = np.float32
    x = np.asarray(x, f32)
    c = np.asarray(coeffs, f32)
    e = np.zeros_like(x)
    with np.errstate(all='ignore'):
        for t in range(x.shape[0]):
            acc = f32(0)
            for i in range(min(c.shape[1], t), 0, -1):
                acc = f32(acc + f32(c[(t - i) // hop, i - 1] * x[t - i]))
            e[t] = f32(f32(x[t] - acc) * f32(gain))
    return e


def synthesis32_direct(e, coeffs, hop, gain=1.0):
    """The synthesis rule in float32 in the DIRECT form of the header (the
    kernel and reference_synthesis run the transposed form, the same chain of
    operations)."""
    f32 = np.float32
    e = np.asarray(e, f32)
    c = np.asarray(coeffs, f32)
    inv = f32(1.0 / float(f32(gain)))
    y = np.zeros_like(e)
    with np.errstate(all='ignore'):
        for t in range(e.shape[0]):
            acc = f32(0)
            for i in range(min(c.shape[1], t), 0, -1):
                acc = f32(acc + f32(c[(t - i) // hop, i - 1] * y[t - i]))
            y[t] = f32(f32(e[t] * inv) + acc)
    return y


def round_trip_bound(x, coeffs, hop, gain=1.0, probes=4):
    """What synthesis(analysis(x)) in float32 may differ from x by.  Each
    filter commits per sample at most g = (order + 2) 2^-24 times the sum of
    the magnitudes it adds, d[t] = g (|x[t]| + sum_i |c_i x[t - i]|); both
    filters' errors enter the all-pole recursion as a perturbation of the
    excitation of at most 2 d[t], and the recursion is linear, so what comes
    out is that perturbation through the float64 synthesis loop.  The signs of
    the roundings are unknown: `probes` random sign patterns of the worst-case
    magnitudes are run and four times the largest response is taken."""
    x = np.asarray(x, np.float64)
    c = np.abs(np.asarray(coeffs, np.float64))
    p = c.shape[1]
    g = (p + 2) * 2.0 ** -24
    d = np.zeros_like(x)
    ax = np.abs(x)
    for t in range(x.shape[0]):
        acc = ax[t]
        for i in range(min(p, t), 0, -1):
            acc += c[(t - i) // hop, i - 1] * ax[t - i]
        d[t] = 2.0 * g * acc
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(probes):
        s = rng.choice([-1.0, 1.0], size=x.shape[0])
        worst = max(worst, np.abs(synthesis64(s * d, coeffs, hop)).max())
    return 4.0 * worst
