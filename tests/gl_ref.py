"""An independent float64 restatement of the Griffin-Lim baseline of
include/wavenet_griffin_lim.h (wavenet/griffin_lim.py): the STFT with explicit
zero padding and np.fft.rfft, its least-squares inverse with np.fft.irfft and a
Python-loop overlap-add, mel inversion with np.linalg.pinv, the phase draw in
Python integers and the Fast Griffin-Lim loop; two float32 restatements of
every primitive that differ in summation order, which set each shape's
yardstick; and the shapes and signals of tests/test_gpu_griffin_lim.py.  None of
it uses the package."""
import functools
import math

import numpy as np

DEN_FLOOR = 1e-8
M2_FLOOR = 1e-30
TOL_FACTOR = 4.0
ULP32 = 2.0 ** -23
SEED_XOR = 0x6772696666696E4C
M64 = (1 << 64) - 1

# name -> (n_fft, hop, win_length, T, lengths); B = len(lengths) clips
SHAPES = {
    'ragged': (64, 16, 64, 257, (257, 40, 1)),     # idle waves, tiny clips
    'oddhop': (128, 25, 100, 700, (700, 333)),     # odd hop, win < n_fft
    'nooverlap': (64, 64, 64, 640, (640, 130)),    # hop == win_length
    'tile32': (256, 64, 256, 2048, (2048, 2048)),  # exactly 32 frames
    'tile33': (256, 64, 256, 2049, (2049, 1000)),  # a 33rd on a partial tile
    'r1024': (1024, 256, 1024, 3000, (3000, 2111)),  # two chunks per wave
    'r2048': (2048, 512, 1200, 3000, (3000, 517)),
}
SEEDS = {k: 301 + i for i, k in enumerate(sorted(SHAPES))}

# whole runs: (n_fft, hop, win_length), T, the ragged lengths of B = 3 clips
RUN = ((256, 64, 256), 4000, (4000, 3201, 1777))
RUN_MELS, RUN_RATE = 40, 16000.0


def hann(n_fft, win_length):
    """Periodic Hann of win_length centred in n_fft."""
    w = np.zeros(n_fft)
    lo = (n_fft - win_length) // 2
    for i in range(win_length):
        w[lo + i] = 0.5 - 0.5 * math.cos(2.0 * math.pi * i / win_length)
    return w


def num_frames(n, hop):
    return -(-n // hop)


def padded(x, n_fft, hop):
    """x between explicit zeros, and the index of frame 0's first sample."""
    n = len(x)
    F = num_frames(n, hop)
    left = n_fft // 2
    total = left + (F - 1) * hop + hop // 2 + n_fft // 2 + n_fft
    buf = np.zeros(max(total, left + n), np.float64)
    buf[left:left + n] = x
    return buf, left + hop // 2 - n_fft // 2


def stft(x, n_fft, hop, win_length):
    """complex128 [F, n_fft / 2 + 1] of one clip."""
    x = np.asarray(x, np.float64)
    buf, s0 = padded(x, n_fft, hop)
    w = hann(n_fft, win_length)
    F = num_frames(len(x), hop)
    out = np.zeros((F, n_fft // 2 + 1), np.complex128)
    for f in range(F):
        out[f] = np.fft.rfft(buf[s0 + f * hop:s0 + f * hop + n_fft] * w)
    return out


def window_square_sum(n, n_fft, hop, win_length):
    """sum_f w^2 at each of the n samples, over the frames of an n-sample
    clip."""
    buf, s0 = padded(np.zeros(n), n_fft, hop)
    w2 = hann(n_fft, win_length) ** 2
    for f in range(num_frames(n, hop)):
        buf[s0 + f * hop:s0 + f * hop + n_fft] += w2
    return buf[n_fft // 2:n_fft // 2 + n]


def istft(S, n, n_fft, hop, win_length):
    """float64 [n]: the least-squares inverse of `stft` (zero where the
    windows' squares sum to <= 1e-8)."""
    S = np.asarray(S, np.complex128)
    buf, s0 = padded(np.zeros(n), n_fft, hop)
    w = hann(n_fft, win_length)
    for f in range(num_frames(n, hop)):
        y = np.fft.irfft(S[f], n_fft)
        for j in range(n_fft):
            buf[s0 + f * hop + j] += w[j] * y[j]
    num = buf[n_fft // 2:n_fft // 2 + n]
    den = window_square_sum(n, n_fft, hop, win_length)
    out = np.zeros(n)
    ok = den > DEN_FLOOR
    out[ok] = num[ok] / den[ok]
    return out


def mel(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def mel_inv(m):
    return 700.0 * (10.0 ** (m / 2595.0) - 1.0)


def filterbank(sample_rate, n_fft, n_mels, fmin=0.0, fmax=None):
    """float64 [n_mels][n_fft / 2 + 1] triangles (the front end's)."""
    fmax = sample_rate / 2.0 if fmax is None else fmax
    lo, hi = mel(fmin), mel(fmax)
    pts = [mel_inv(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    out = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        for k in range(n_fft // 2 + 1):
            f = k * sample_rate / n_fft
            up = (f - pts[m]) / (pts[m + 1] - pts[m])
            down = (pts[m + 2] - f) / (pts[m + 2] - pts[m + 1])
            out[m, k] = max(0.0, min(up, down))
    return out


def magnitude(frames, melw):
    """float64 [F, n_bins] from raw log-mel [F, n_mels]."""
    P = np.exp(np.asarray(frames, np.float64)) @ np.linalg.pinv(melw).T
    return np.sqrt(np.maximum(P, 0.0))


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def phase_index(seed, key, f, k, n_bins):
    """wn_gl_init's p in Python integers."""
    if k == 0 or k == n_bins - 1:
        return 0
    ctr = ((key << 40) | (f * n_bins + k)) & M64
    return splitmix64(((seed ^ SEED_XOR) & M64) ^ splitmix64(ctr)) & 1023


def initial(A, seed, key, init='random'):
    """complex128 [F, n_bins]: A on the drawn phases 2 pi p / 1024."""
    F, nb = A.shape
    out = np.zeros((F, nb), np.complex128)
    for f in range(F):
        for k in range(nb):
            p = phase_index(seed, key, f, k, nb) if init == 'random' else 0
            out[f, k] = A[f, k] * complex(math.cos(2 * math.pi * p / 1024),
                                          math.sin(2 * math.pi * p / 1024))
    return out


def project(S, A, t_prev, alpha):
    """(t, c, (err, a2)) from the spectrum S of the current audio."""
    mag = np.abs(S)
    big = mag * mag > M2_FLOOR
    t = np.where(big, A * S / np.where(big, mag, 1.0), A + 0j)
    c = t + alpha * (t - t_prev)
    return t, c, (float(((mag - A) ** 2).sum()), float((A * A).sum()))


def griffin_lim(A, n, res, iterations, alpha, seed=0, key=0, init='random'):
    """(x, trace [iterations + 1, 2]) of one clip in float64."""
    n_fft, hop, win = res
    c = initial(A, seed, key, init)
    t = c
    trace = []
    for _ in range(iterations):
        x = istft(c, n, n_fft, hop, win)
        t, c, tr = project(stft(x, n_fft, hop, win), A, t, alpha)
        trace.append(tr)
    x = istft(t, n, n_fft, hop, win)
    trace.append(project(stft(x, n_fft, hop, win), A, t, 0.0)[2])
    return x, np.asarray(trace)


def ratio(trace):
    """sqrt(sum (|S| - A)^2 / sum A^2) per trace entry."""
    trace = np.asarray(trace, np.float64)
    return np.sqrt(trace[..., 0] / trace[..., 1])


# ---- float32 restatements, two summation orders each ------------------------
def _tables32(n_fft, win_length):
    j = np.arange(n_fft, dtype=np.int64)[:, None]
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[None, :]
    ang = 2.0 * np.pi * ((j * k) % n_fft).astype(np.float64) / n_fft
    return (np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32),
            hann(n_fft, win_length).astype(np.float32))


def _frames32(x, n_fft, hop, win_length):
    buf, s0 = padded(np.asarray(x, np.float64), n_fft, hop)
    F = num_frames(len(x), hop)
    w = hann(n_fft, win_length).astype(np.float32)
    fr = np.stack([buf[s0 + f * hop:s0 + f * hop + n_fft] for f in range(F)])
    return fr.astype(np.float32) * w[None, :]


def stft_f32(x, n_fft, hop, win_length, order):
    """complex64-precision STFT: order 'matmul' (one float32 matmul) or
    'sequential' (one float32 rank-1 update per sample)."""
    cos, sin, _ = _tables32(n_fft, win_length)
    fr = _frames32(x, n_fft, hop, win_length)
    if order == 'matmul':
        re, im = fr @ cos, fr @ sin
    else:
        re = np.zeros((fr.shape[0], cos.shape[1]), np.float32)
        im = np.zeros_like(re)
        for j in range(n_fft):
            re += fr[:, j:j + 1] * cos[j:j + 1, :]
            im += fr[:, j:j + 1] * sin[j:j + 1, :]
    im = -im
    im[:, 0] = im[:, -1] = 0
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def istft_f32(S, n, n_fft, hop, win_length, order):
    """float32 inverse: order 'matmul' or 'sequential' (one float32 rank-1
    update per bin); the overlap-add in float32, frames ascending."""
    f32 = np.float32
    cos, sin, w = _tables32(n_fft, win_length)
    h = n_fft // 2
    S = np.asarray(S)[:num_frames(n, hop)]
    re, im = S.real.astype(f32), S.imag.astype(f32)
    sign = np.where(np.arange(n_fft) % 2, -1.0, 1.0).astype(f32)
    if order == 'matmul':
        y = f32(2.0) * (re[:, 1:h] @ cos[:, 1:h].T - im[:, 1:h] @ sin[:, 1:h].T)
        y = (y + re[:, :1] + re[:, h:h + 1] * sign[None, :]) * f32(1.0 / n_fft)
    else:
        y = np.zeros((re.shape[0], n_fft), f32)
        for k in range(1, h):
            y += re[:, k:k + 1] * cos[None, :, k] - im[:, k:k + 1] * sin[None, :, k]
        y = (f32(2.0) * y + re[:, :1] + re[:, h:h + 1] * sign[None, :]) / f32(n_fft)
    v = (y * w[None, :]).astype(f32)
    buf, s0 = padded(np.zeros(n), n_fft, hop)
    num, den = buf.astype(f32), buf.astype(f32)
    w2 = w * w
    for f in range(v.shape[0]):
        num[s0 + f * hop:s0 + f * hop + n_fft] += v[f]
        den[s0 + f * hop:s0 + f * hop + n_fft] += w2
    num, den = num[h:h + n], den[h:h + n]
    out = np.zeros(n, f32)
    ok = den > f32(DEN_FLOOR)
    out[ok] = num[ok] / den[ok]
    return out.astype(np.float64)


def magnitude_f32(frames, melw, order):
    f32 = np.float32
    pinv = np.linalg.pinv(melw).astype(f32)
    M = np.exp(np.asarray(frames, f32))
    if order == 'matmul':
        P = M @ pinv.T
    else:
        P = np.zeros((M.shape[0], pinv.shape[0]), f32)
        for m in range(M.shape[1]):
            P += M[:, m:m + 1] * pinv[None, :, m]
    return np.sqrt(np.maximum(P, f32(0))).astype(np.float64)


def project_f32(x, A, t_prev, alpha, res, order):
    """(t, c) as complex128 holding float32 values."""
    f32 = np.float32
    S = stft_f32(x, res[0], res[1], res[2], order)
    re, im = S.real.astype(f32), S.imag.astype(f32)
    A = np.asarray(A, f32)
    m2 = re * re + im * im
    big = m2 > f32(M2_FLOOR)
    r = A / np.sqrt(np.where(big, m2, f32(1)))
    tre = np.where(big, re * r, A).astype(f32)
    tim = np.where(big, im * r, f32(0)).astype(f32)
    pre, pim = t_prev.real.astype(f32), t_prev.imag.astype(f32)
    a = f32(alpha)
    cre, cim = tre + a * (tre - pre), tim + a * (tim - pim)
    g = (np.sqrt(m2) - A).astype(np.float64)
    return (tre.astype(np.float64) + 1j * tim, cre.astype(np.float64) + 1j * cim,
            (float((g * g).sum()), float((A.astype(np.float64) ** 2).sum())))


def griffin_lim_f32(A, n, res, iterations, alpha, seed=0, key=0,
                    order='matmul'):
    """The loop through the float32 restatements: (x, trace)."""
    n_fft, hop, win = res
    A = np.asarray(A, np.float32).astype(np.float64)
    c = initial(A, seed, key).astype(np.complex64).astype(np.complex128)
    t = c
    trace = []
    for _ in range(iterations):
        x = istft_f32(c, n, n_fft, hop, win, order)
        t, c, tr = project_f32(x, A, t, alpha, res, order)
        trace.append(tr)
    x = istft_f32(t, n, n_fft, hop, win, order)
    trace.append(project_f32(x, A, t, 0.0, res, order)[2])
    return x, np.asarray(trace)


def yardstick(ref64, restatements):
    """The largest of the float32 restatements' max errors against ref64 and
    one float32 ulp of ref64's scale."""
    ref64 = np.asarray(ref64)
    scale = float(np.abs(ref64).max()) if ref64.size else 0.0
    errs = [float(np.abs(np.asarray(r) - ref64).max()) if ref64.size else 0.0
            for r in restatements]
    return max(errs + [ULP32 * scale])


# ---- signals ----------------------------------------------------------------
def signal(seed, T, rate=16000.0):
    """A chirp plus a tone plus noise, float32 values in float64, |x| < 1."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / rate
    x = 0.4 * np.sin(2 * np.pi * (200.0 * t + 0.5 * 3000.0 * t * t / max(t[-1], 1e-9)))
    x += 0.3 * np.sin(2 * np.pi * 1234.5 * t + 1.0)
    x += 0.1 * rng.standard_normal(T)
    return x.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def make_audio(name):
    """float32 [B, T] Gaussian noise (no bin of its STFT vanishes)."""
    T, lengths = SHAPES[name][3:]
    rng = np.random.default_rng(SEEDS[name])
    return (0.5 * rng.standard_normal((len(lengths), T))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def make_spectrum(name):
    """complex64 [B, F, n_bins]: a random INCONSISTENT spectrum."""
    n_fft, hop, _, T, lengths = SHAPES[name]
    rng = np.random.default_rng(SEEDS[name] + 1000)
    shape = (len(lengths), num_frames(T, hop), n_fft // 2 + 1)
    return (rng.standard_normal(shape) +
            1j * rng.standard_normal(shape)).astype(np.complex64)


def logmel_frames(seed, B, F, C):
    """float32 [B, F, C] in the range of raw log-mel features."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-12.0, 3.0, (B, F, C)).astype(np.float32)
