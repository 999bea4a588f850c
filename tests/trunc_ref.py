"""Host restatement of the truncated draw (top-k and nucleus / top-p), in
float64 numpy on top of tests/draw_ref.py and never through the library or
wavenet/sampling.py.  With p the float32 probabilities of a draw,
tau = float32(temperature), K = top_k and P = float32(top_p):

 1. top-k (skipped for K None or K >= Q): v = the K-th largest value of p,
    counting multiplicity; keep exactly the codes with p >= v (a tie at the
    cut keeps the whole tie group); dropped codes weigh exactly 0.
 2. temperature: draw_ref.weights(p, tau); dropped codes stay at 0.
 3. nucleus (skipped for P None or P == 1): total = the float64 sum of the
    surviving w; over the distinct values of p among the survivors, largest
    first, the kept set is the first prefix of whole tie groups whose w-mass
    is >= float64(P) * total; everything else weighs 0.
 4. the draw: draw_ref.pick(w, draw_ref.uniform(seed, counter)), unchanged.

The nucleus margin is the smallest |mass(prefix) - P * total| / total over the
prefixes: a device that adds the masses in another order decides every prefix
as this file does when the margin is far above float64 rounding."""
import numpy as np

import draw_ref as D


def truncate(p32, tau, top_k=None, top_p=None):
    """(w, keep, margin) of one row of float32 probabilities: the float64
    weights after truncation, the kept set (bool), the nucleus margin (inf
    without a nucleus step)."""
    p = np.asarray(p32, np.float32).reshape(-1)
    Q = p.size
    keep = np.ones(Q, bool)
    if top_k is not None and int(top_k) < Q:
        v = np.partition(p, Q - int(top_k))[Q - int(top_k)]
        keep = p >= v
    w = np.where(keep, D.weights(p, tau), 0.0)
    margin = np.inf
    if top_p is not None and float(np.float32(top_p)) != 1.0:
        total = w.sum()
        bound = float(np.float32(top_p)) * total
        vals = np.unique(p[keep])[::-1]            # distinct, largest first
        mass = np.array([w[p >= v].sum() for v in vals])
        margin = float(np.abs(mass - bound).min() / total)
        ok = np.nonzero(mass >= bound)[0]
        cut = vals[ok[0]] if ok.size else vals[-1]
        keep = keep & (p >= cut)
        w = np.where(keep, w, 0.0)
    return w, keep, margin


def check_draws(codes, probs, tau, top_k, top_p, seed, counters, max_ties=2,
                max_skipped=0, min_margin=1e-9, what=''):
    """draw_ref.check_draws for the truncated draw: codes[i] was drawn with
    counter counters[i] from the float32 probabilities probs[i] (or probs, one
    row for every draw).  No code outside the kept set, without tolerance;
    every code the restated one, but for draw_ref's summation-order tie (a
    code beside the boundary, at most max_ties).  A row whose nucleus margin
    is below min_margin is left out (at most max_skipped).  Returns (ties,
    rows left out, the kept sets [rows, Q])."""
    codes = np.asarray(codes).reshape(-1)
    counters = np.asarray(counters, np.int64).reshape(-1)
    probs = np.asarray(probs, np.float32)
    shared = probs.ndim == 1
    memo = {}                                  # (equal rows: one truncation)

    def trunc(r):
        key = r.tobytes()
        if key not in memo:
            memo[key] = truncate(r, tau, top_k, top_p)
        return memo[key]
    rows = [trunc(probs)] if shared else [trunc(r) for r in probs]
    assert len(counters) == len(codes) and (shared or len(rows) == len(codes))
    u = D.uniform(seed, counters)
    ties = skipped = 0
    for i, c in enumerate(codes):
        w, keep, m = rows[0 if shared else i]
        if m < min_margin:
            skipped += 1
            continue
        assert 0 <= c < w.size and keep[c] and w[c] > 0, \
            '%s: draw %d (counter %d) took code %d outside the kept set' % (
                what, i, counters[i], c)
        ref = int(D.pick(w, u[i]))
        if ref == c:
            continue
        mg, total = float(D.margin(w, u[i])), float(w.sum())
        near = D.boundary_codes(w, u[i])
        assert mg < D.TIE_REL * total and int(c) in near, \
            '%s: draw %d (counter %d, u = %.17g): device code %d, restated ' \
            'code %d (margin %.3g of total %.6g)' % (
                what, i, counters[i], u[i], c, ref, mg, total)
        ties += 1
    assert ties <= max_ties, '%s: %d summation-order ties' % (what, ties)
    assert skipped <= max_skipped, '%s: %d rows with a nucleus tie' % (what, skipped)
    return ties, skipped, np.array([r[1] for r in rows])
