"""float64 restatement of global-norm clipping (tf.clip_by_global_norm) and
the EMA shadow weights (tf.train.ExponentialMovingAverage without num_updates)
on top of oracle.TFOptimizer:

    norm   = grad_scale * sqrt(sum g_i^2)          the norm before clipping
    factor = clip_norm / max(norm, clip_norm)      (NaN when norm is not finite)
    w'     = TFOptimizer.apply(w, g * grad_scale * factor + l2 * w * l2_mask)
    s'     = s - (1 - decay) * (s - w')            s_0 = w_0 (the weights before
                                                   the first update)

so that after k steps  s_k = decay^k w_0 + (1 - decay) sum_j decay^(k-j) w_j.
"""
import numpy as np

from util import O


def global_norm(g, grad_scale=1.0):
    g = np.asarray(g, np.float64).reshape(-1)
    return float(grad_scale) * float(np.sqrt(np.sum(g * g)))


def clip_factor(norm, clip_norm):
    if clip_norm is None:
        return 1.0
    if not np.isfinite(norm):
        return float('nan')
    return float(clip_norm) / max(float(norm), float(clip_norm))


class ClipEMAOptimizer(object):
    """O.TFOptimizer(kind, learning_rate, momentum) behind the clip, with the
    shadow; `apply(w, g)` returns the updated flat weights, `last_norm` is the
    norm before clipping and `shadow` the flat shadow (None without decay)."""

    def __init__(self, kind, learning_rate, momentum=0.9, clip_norm=None,
                 ema_decay=None):
        self.opt = O.TFOptimizer(kind, learning_rate, momentum)
        self.clip_norm, self.ema_decay = clip_norm, ema_decay
        self.shadow = None
        self.last_norm = None

    def apply(self, w, g, grad_scale=1.0, l2=0.0, l2_mask=None):
        w = np.asarray(w, np.float64)
        g = np.asarray(g, np.float64)
        if self.ema_decay is not None and self.shadow is None:
            self.shadow = w.copy()
        self.last_norm = global_norm(g, grad_scale)
        f = clip_factor(self.last_norm, self.clip_norm)
        g = g * (grad_scale * f)
        if l2 != 0.0:
            g = g + float(l2) * w * (1.0 if l2_mask is None else
                                     np.asarray(l2_mask, np.float64))
        w2 = self.opt.apply(w, g)
        if self.ema_decay is not None:
            self.shadow = self.shadow - (1.0 - self.ema_decay) * (
                self.shadow - w2)
        return w2
