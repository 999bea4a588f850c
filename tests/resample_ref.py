"""The sample-rate converter's rule restated in float64, written independently
of wavenet/resample.py: zero-stuff the clip by `up`, convolve with the taps
(np.convolve), keep every `down`-th sample from the filter's centre on.  The
taps are an argument: tests give it the float64 design or the float32 taps
widened."""
import numpy as np


def out_length(n, up, down):
    return (n * up + down - 1) // down


def resample64(x, up, down, taps):
    """float64 [ceil(n up / down)] from x [n] and taps [2 Hh + 1]."""
    x = np.asarray(x, np.float64).reshape(-1)
    h = np.asarray(taps, np.float64).reshape(-1)
    assert h.shape[0] % 2 == 1
    Hh = h.shape[0] // 2
    n = x.shape[0]
    if n == 0:
        return np.zeros(0, np.float64)
    stuffed = np.zeros(n * up, np.float64)
    stuffed[::up] = x
    full = np.convolve(stuffed, h)            # full[c + Hh]: centre at c
    k = np.arange(out_length(n, up, down))
    return full[k * down + Hh]


def reach(j, n, up, down, Hh):
    """The outputs k < out_length(n) whose taps cover sample j: |k down - j up|
    <= Hh."""
    k = np.arange(out_length(n, up, down))
    return k[np.abs(k * down - j * up) <= Hh]


def bound(x32, up, down, taps32, orders):
    """The tolerance of a float32 evaluation against resample64, per output
    (the scheme of tests/test_gpu_spectral*.py): 4 x the larger of the largest
    distance from float64 of the float32 evaluations `orders` (arrays [n_out])
    and one float32 ulp at the clip's largest |y|.  Returns (bound, y64)."""
    y64 = resample64(x32, up, down, np.asarray(taps32, np.float64))
    top = float(np.abs(y64).max()) if y64.size else 0.0
    ulp = float(np.spacing(np.float32(top)))
    d = max([float(np.abs(np.asarray(o, np.float64) - y64).max())
             for o in orders] + [ulp])
    return 4.0 * d, y64


def reversed_order32(x32, up, down, taps32):
    """The rule in float32 with j DEScending (the second summation order of
    the bound), by explicit loops over the taps, vectorised over outputs."""
    f32 = np.float32
    x = np.asarray(x32, f32).reshape(-1)
    h = np.asarray(taps32, f32)
    Hh = h.shape[0] // 2
    n = x.shape[0]
    no = out_length(n, up, down)
    k = np.arange(no, dtype=np.int64)
    acc = np.zeros(no, f32)
    j0 = -((-(k * down - Hh)) // up)          # ceil: the oldest sample
    steps = 2 * Hh // up + 1
    for s in range(steps, -1, -1):            # j descending
        j = j0 + s
        i = k * down - j * up + Hh
        ok = (i >= 0) & (i <= 2 * Hh) & (j >= 0) & (j < n)
        p = (h[np.clip(i, 0, 2 * Hh)] * x[np.clip(j, 0, n - 1)]).astype(f32)
        acc = np.where(ok, (acc + p).astype(f32), acc)
    return acc
