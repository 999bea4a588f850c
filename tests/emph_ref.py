"""Float64 restatement of the de-emphasis recurrence and its error bound,
written without looking at wavenet/emphasis.py's arithmetic.

    y[t] = e[t] + a * y[t - 1],  y[-1] = initial         a = float64(float32(alpha))

The bound.  In the float32 sequential order the input term e[t - k] passes
through at most k multiplications and k + 1 additions before it is part of
y[t]; a blocked scan passes it through fewer.  Every rounding changes the
term by at most 2^-24 of its size, so to first order

    |y_dev[t] - y_64[t]| <= 2^-24 * sum_k (2 k + 3) a^k |e[t - k]| + 2^-126

(the + 3 leaves room for the rounded table powers of a scan's fix-up; the
floor covers the subnormal tail of an impulse response).  `initial` counts
as the term k = t + 1.  The sum is two coupled recurrences:

    P[t] = |e[t]| + a P[t - 1]          = sum_k a^k |e[t - k]|
    Q[t] = a (Q[t - 1] + P[t - 1])      = sum_k k a^k |e[t - k]|
    bound[t] = 2^-24 (2 Q[t] + 3 P[t]) + 2^-126
"""
import numpy as np


def alpha64(alpha):
    """The alpha both kernels use, widened."""
    return float(np.float32(alpha))


def de64(e, alpha, lengths=None, initial=None):
    """(y, bound), float64 [B, T] each, of e [B, T] (or [T]); positions at or
    behind lengths[b] are zeros with bound zero."""
    e = np.asarray(e, np.float64)
    one = e.ndim == 1
    e = e.reshape(1, -1) if one else e
    B, T = e.shape
    a = alpha64(alpha)
    y = np.zeros((B, T))
    bound = np.zeros((B, T))
    prev = np.zeros(B) if initial is None else \
        np.asarray(initial, np.float64).reshape(B).copy()
    P, Q = np.abs(prev), np.zeros(B)
    for t in range(T):
        prev = e[:, t] + a * prev
        Q = a * (Q + P)
        P = np.abs(e[:, t]) + a * P
        y[:, t] = prev
        bound[:, t] = 2.0 ** -24 * (2.0 * Q + 3.0 * P) + 2.0 ** -126
    if lengths is not None:
        keep = np.arange(T)[None, :] < np.asarray(lengths)[:, None]
        y, bound = np.where(keep, y, 0.0), np.where(keep, bound, 0.0)
    return (y[0], bound[0]) if one else (y, bound)


def pre64(x, alpha):
    """e[t] = x[t] - a x[t - 1] in float64, x [T] or [B, T]."""
    x = np.asarray(x, np.float64)
    prev = np.concatenate([np.zeros(x.shape[:-1] + (1,)), x[..., :-1]], -1)
    return x - alpha64(alpha) * prev
