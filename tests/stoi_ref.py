"""STOI / ESTOI restated in float64 from the rule of include/wavenet_stoi.h,
written independently of wavenet/stoi.py: explicit loops, np.fft.rfft for the
spectra.  Also the fixtures of the STOI tests (seeded; every frame decisively
on one side of the keep threshold) and a SECOND float32 evaluation of steps 3
- 4 with other summation orders, for the tests' bound."""
import math

import numpy as np

import resample_ref

RATE = 10000
L = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
U = L[1:] + [219]
C = 10.0 ** (15.0 / 20.0)
EPS = 2.0 ** -52


def window64():
    return np.array([math.sin(math.pi * (i + 1) / 257.0) ** 2
                     for i in range(256)])


def window32():
    return window64().astype(np.float32).astype(np.float64)


def to_10k(x, rs):
    """x at the rate of `rs` (a wavenet.resample.Resampler, or None at 10
    kHz) -> float64 at 10 kHz, with rs's float32 taps widened."""
    x = np.asarray(x, np.float64).reshape(-1)
    if rs is None:
        return x
    return resample_ref.resample64(x, rs.up, rs.down,
                                   rs.taps.astype(np.float64))


def energies(x10, w):
    Fs = (len(x10) - 256) // 128 + 1 if len(x10) >= 256 else 0
    E = np.zeros(Fs)
    for f in range(Fs):
        E[f] = np.sum((w * x10[128 * f:128 * f + 256]) ** 2)
    return E


def keep_of(x10, w):
    """(keep [Fs] bool, margin [Fs] = E / (Emax * 1e-4), or inf where Emax is
    not above zero)."""
    E = energies(x10, w)
    emax = E.max() if len(E) else 0.0
    if not emax > 0.0:
        return np.zeros(len(E), bool), np.full(len(E), np.inf)
    thr = emax * float(np.float32(1e-4))
    return E > thr, E / thr


def compact(x10, keep, w):
    k = np.nonzero(keep)[0]
    out = np.zeros(128 * (len(k) - 1) + 256 if len(k) else 0)
    for i, f in enumerate(k):
        out[128 * i:128 * i + 256] += w * x10[128 * f:128 * f + 256]
    return out


def bands(xc, M, w):
    A = np.zeros((15, M))
    for i in range(M):
        P = np.abs(np.fft.rfft(xc[128 * i:128 * i + 256] * w, 512)) ** 2
        for b in range(15):
            A[b, i] = math.sqrt(sum(P[k] for k in range(L[b], U[b])))
    return A


def _unit(v):
    v = v - sum(v) / len(v)
    return v / (math.sqrt(sum(v * v)) + EPS)


def scores(X, Y):
    """(stoi [S], estoi [S]) of band amplitudes [15, M], float64."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    M = X.shape[1]
    st, es = [], []
    for s in range(M - 29):
        x, y = X[:, s:s + 30], Y[:, s:s + 30]
        d = 0.0
        for b in range(15):
            alpha = math.sqrt(sum(x[b] ** 2)) / (math.sqrt(sum(y[b] ** 2)) +
                                                 EPS)
            yc = np.minimum(alpha * y[b], (1.0 + C) * x[b])
            d += sum(_unit(x[b]) * _unit(yc))
        st.append(d / 15.0)
        xr = np.stack([_unit(x[b]) for b in range(15)])
        yr = np.stack([_unit(y[b]) for b in range(15)])
        e = 0.0
        for m in range(30):
            e += sum(_unit(xr[:, m]) * _unit(yr[:, m]))
        es.append(e / 30.0)
    return np.array(st), np.array(es)


def stoi64(generated, original, rs=None, wide_window=False):
    """The rule for one clip pair in float64: a dict with stoi_sum, estoi_sum,
    segments, kept, frames, keep, margin, and stoi / estoi (sum / segments, or
    None).  The window is the rule's float32 window widened (wide_window: the
    float64 one, for closed forms)."""
    w = window64() if wide_window else window32()
    y10, x10 = to_10k(generated, rs), to_10k(original, rs)
    assert y10.shape == x10.shape
    keep, margin = keep_of(x10, w)
    M = int(keep.sum())
    res = {'kept': M, 'frames': len(keep), 'keep': keep, 'margin': margin,
           'segments': max(M - 29, 0), 'stoi_sum': 0.0, 'estoi_sum': 0.0,
           'stoi': None, 'estoi': None}
    if M >= 30:
        X = bands(compact(x10, keep, w), M, w)
        Y = bands(compact(y10, keep, w), M, w)
        st, es = scores(X, Y)
        res.update(stoi_sum=float(st.sum()), estoi_sum=float(es.sum()),
                   stoi=float(st.mean()), estoi=float(es.mean()), X=X, Y=Y)
    return res


def decisive(margin):
    """Whether every frame's E / (Emax * 1e-4) lies outside [1 - 1e-3, 1 +
    1e-3]."""
    m = np.asarray(margin)
    return bool(np.all((m < 1.0 - 1e-3) | (m > 1.0 + 1e-3)))


def corpus(results):
    """The corpus mean of stoi64 results: the clips with segments > 0."""
    ok = [r for r in results if r['segments'] > 0]
    return {'stoi': sum(r['stoi'] for r in ok) / len(ok),
            'estoi': sum(r['estoi'] for r in ok) / len(ok),
            'clips': len(ok), 'skipped_clips': len(results) - len(ok),
            'segments': sum(r['segments'] for r in ok),
            'kept_frames': sum(r['kept'] for r in results),
            'frames': sum(r['frames'] for r in results),
            'sample_rate': RATE}


# ----------------------------------------------- a second float32 evaluation
def bands32_alt(x10, keep):
    """Steps 3 (overlap-add) and 4 in float32 with OTHER summation orders than
    the rule's: the later frame's addend first, the DFT sums with j
    descending, the band sums with k descending.  x10: float32 at 10 kHz."""
    f32 = np.float32
    x = np.asarray(x10, f32)
    w = window64().astype(f32)
    q = np.arange(512, dtype=np.float64)
    cs = np.cos(2 * np.pi * q / 512).astype(f32)
    sn = np.sin(2 * np.pi * q / 512).astype(f32)
    k = np.nonzero(keep)[0]
    M = len(k)
    idx = 128 * k[:, None] + np.arange(256)[None, :]
    fr = (w[None, :] * x[idx]).astype(f32)
    c = np.zeros((M, 256), f32)
    c[:-1, 128:] = (c[:-1, 128:] + fr[1:, :128]).astype(f32)
    c[:, 128:] = (c[:, 128:] + fr[:, 128:]).astype(f32)
    c[:, :128] = (c[:, :128] + fr[:, :128]).astype(f32)
    c[1:, :128] = (c[1:, :128] + fr[:-1, 128:]).astype(f32)
    v = (c * w[None, :]).astype(f32)
    kb = np.arange(L[0], U[-1])
    re = np.zeros((M, len(kb)), f32)
    im = np.zeros_like(re)
    for j in range(255, -1, -1):
        t = (kb * j) % 512
        re = (re + (cs[t][None, :] * v[:, j, None]).astype(f32)).astype(f32)
        im = (im + (sn[t][None, :] * v[:, j, None]).astype(f32)).astype(f32)
    P = ((re * re).astype(f32) + (im * im).astype(f32)).astype(f32)
    A = np.zeros((15, M), f32)
    for b in range(15):
        acc = np.zeros(M, f32)
        for kk in range(U[b] - 1, L[b] - 1, -1):
            acc = (acc + P[:, kk - L[0]]).astype(f32)
        A[b] = np.sqrt(acc)
    return A


def alt32(generated, original, rs, keep):
    """(stoi, estoi) per-clip scores of the second float32 evaluation: the
    resampler with j descending, then bands32_alt, then `scores`."""
    g = np.asarray(generated, np.float32).reshape(-1)
    o = np.asarray(original, np.float32).reshape(-1)
    if rs is not None:
        g, o = (resample_ref.reversed_order32(t, rs.up, rs.down, rs.taps)
                for t in (g, o))
    st, es = scores(bands32_alt(o, keep), bands32_alt(g, keep))
    return float(st.mean()), float(es.mean())


def bound(value64, others):
    """4 x the larger of the largest distance of `others` from value64 and one
    float32 ulp of the value."""
    ulp = float(np.spacing(np.float32(abs(value64))))
    return 4.0 * max([abs(o - value64) for o in others] + [ulp])


# ------------------------------------------------------------------ fixtures
def _voice(n, rate, seed):
    """A harmonic tone complex under a slow envelope plus noise at -30 dB."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / float(rate)
    f0 = 120.0 + 25.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / rate
    x = sum(np.sin(h * ph + h) / h for h in range(1, 31))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t + 0.3)
    x = 0.25 * env * x
    rms = np.sqrt(np.mean(x * x))
    return x + rms * 10 ** (-30 / 20.0) * rng.standard_normal(n)


_fixtures = {}


def fixture(M, rate=16000, seed=0):
    """float32 [n] at `rate` whose original keeps exactly M frames, every frame
    decisive: [exact zeros | voice | the voice scaled by 1e-3 | voice | exact
    zeros] -- removed frames at the start, in the middle and at the end, kept
    frames beside them.  The second voiced stretch is grown until M is hit."""
    key = (M, rate, seed)
    if key in _fixtures:
        return _fixtures[key]
    from wavenet import resample
    rs = None if rate == RATE else resample.Resampler(rate, RATE)
    unit = rate // 100                          # 10 ms
    lead, quiet, tail = 7 * unit, 9 * unit, 6 * unit
    first = (M // 3) * 128 * rate // RATE
    w = window32()
    for grow in range(0, 400):
        second = (M - M // 3) * 128 * rate // RATE - 20 * unit + grow * unit // 4
        if second < unit:
            continue
        n = lead + first + quiet + second + tail
        x = _voice(n, rate, seed)
        x[:lead] = 0.0
        x[lead + first:lead + first + quiet] *= 1e-3
        x[n - tail:] = 0.0
        x = x.astype(np.float32)
        keep, margin = keep_of(to_10k(x, rs), w)
        if int(keep.sum()) == M and decisive(margin) and \
                not keep[0] and not keep[-1] and \
                not keep[np.nonzero(keep)[0][0]:np.nonzero(keep)[0][-1]].all():
            _fixtures[key] = x
            return x
    raise AssertionError('no fixture with M = %d found' % M)


def degraded(x, sigma, seed=1):
    """x + sigma * rms(x) * white noise, float32."""
    rng = np.random.default_rng(seed)
    x = np.asarray(x, np.float64)
    rms = np.sqrt(np.mean(x * x))
    return (x + sigma * rms * rng.standard_normal(len(x))).astype(np.float32)
