"""Top-k and nucleus (top-p) truncation of the sampling draw, host side.

The device draw (csrc/wn_common.h: wave_trunc_cut) applies the rule below
between the temperature and the inverse CDF; this module states it in numpy
for the naive path of generate.py and for users who want to see what a
setting keeps.

    p     float32 probabilities (what predict_proba / proba_out return)
    tau   float32(temperature)
 1. top-k (skipped for top_k None or >= Q): with v the top_k-th largest value
    of p, keep the codes with p >= v.  A tie at the cut keeps its whole tie
    group, so the kept set does not depend on an order of equal values.
 2. temperature: w = p at tau == 1, else exp(log(p) / tau - max), p == 0
    weighted exactly 0; dropped codes weigh 0.
 3. nucleus (skipped for top_p None or 1): with total the float64 sum of the
    surviving w, walk the distinct values of p among the survivors from the
    largest down and keep the first prefix of whole tie groups whose w-mass is
    >= float64(float32(top_p)) * total.
A code outside the kept set is never drawn.
"""
import numpy as np


def check(top_k, top_p):
    """ValueError unless top_k is None or an int >= 1 (no bool) and top_p is
    None or a finite number in (0, 1]."""
    if top_k is not None:
        if isinstance(top_k, (bool, np.bool_)) or \
                not isinstance(top_k, (int, np.integer)) or int(top_k) < 1:
            raise ValueError('top_k must be None or an int >= 1, got %r'
                             % (top_k,))
    if top_p is not None:
        try:
            ok = not isinstance(top_p, (bool, np.bool_)) and \
                np.isfinite(float(top_p)) and 0.0 < float(top_p) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError('top_p must be None or a finite number in '
                             '(0, 1], got %r' % (top_p,))


def resolve(top_k, top_p, Q):
    """check(), then what the device gets: (top_k, float32 top_p) with 0 for
    "off" (None, top_k >= Q, top_p == 1)."""
    check(top_k, top_p)
    k = 0 if top_k is None or int(top_k) >= int(Q) else int(top_k)
    p = 0.0 if top_p is None else float(np.float32(top_p))
    return k, (0.0 if p >= 1.0 else p)


def _weights(p, tau):
    if tau == 1.0:
        return p.copy()
    with np.errstate(divide='ignore'):
        lp = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)) / tau, -np.inf)
    return np.exp(lp - lp.max())


def kept_mask(probs, temperature=1.0, top_k=None, top_p=None):
    """bool [..., Q]: the codes the draw keeps of float32 probabilities
    `probs` [..., Q] at `temperature` with top_k / top_p (rule above)."""
    check(top_k, top_p)
    p32 = np.asarray(probs, np.float32)
    Q = p32.shape[-1]
    k, P = resolve(top_k, top_p, Q)
    tau = float(np.float32(temperature))
    flat = p32.reshape(-1, Q)
    out = np.ones(flat.shape, bool)
    for row, keep in zip(flat, out):
        if k:
            keep &= row >= np.sort(row)[Q - k]
        if P:
            w = np.where(keep, _weights(row.astype(np.float64), tau), 0.0)
            bound = float(np.float32(P)) * w.sum()
            # distinct surviving values, largest first, and their w-mass
            vals = np.unique(row[keep])[::-1]
            mass = np.cumsum([w[keep & (row == v)].sum() for v in vals])
            cut = vals[int(np.argmax(mass >= bound))] if \
                (mass >= bound).any() else vals[-1]
            keep &= row >= cut
    return out.reshape(p32.shape)
