"""Independent numpy restatements for wavenet/synthesis.py and
features.frame_distance: the rounds of the bulk path, and the three distance
sums (a float32 subtraction, then float64) with the bounds the device sums
are held to."""
import numpy as np


def plan_rounds(lengths, batch):
    """(rounds, steps, occupancy): the items longest first, ties by index,
    in consecutive groups of `batch`; a round runs its first item's length."""
    n = [int(v) for v in lengths]
    left = list(range(len(n)))
    rounds = []
    while left:
        # (selection, not a sort: the longest remaining item with the
        # smallest index, `batch` times)
        group = []
        while left and len(group) < batch:
            best = left[0]
            for u in left[1:]:
                if n[u] > n[best]:
                    best = u
            group.append(best)
            left.remove(best)
        rounds.append(group)
    steps = 0
    for g in rounds:
        steps += n[g[0]]
    return rounds, steps, sum(n) / float(batch * steps)


def real_mask(B, F, nframes):
    if nframes is None:
        return np.ones((B, F), bool)
    return np.arange(F)[None, :] < np.asarray(nframes)[:, None]


def distance(a, b, nframes=None):
    """abs_sum, sq_sum, rms_sum float64 [B] of float32 [B, F, C] inputs, and
    what the bounds need: per clip the number of terms n = nframes * C, the
    real frames, and max_f rms_f.  Frames behind nframes do not count,
    whatever they hold."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32
    B, F, C = a.shape
    m = real_mask(B, F, nframes)
    with np.errstate(invalid='ignore'):
        d = (a - b).astype(np.float32)             # the float32 subtraction
    d = np.where(m[:, :, None], d, np.float32(0)).astype(np.float64)
    sq_f = (d * d).sum(axis=2)
    rms_f = np.sqrt(sq_f / C)
    nf = m.sum(axis=1)
    return dict(abs_sum=np.abs(d).sum(axis=(1, 2)), sq_sum=sq_f.sum(axis=1),
                rms_sum=rms_f.sum(axis=1), terms=nf * C, frames=nf,
                rms_max=rms_f.max(axis=1))


def sum_bound(n, abs_terms):
    """|S_a - S_b| for two summation orders of the same n float64 terms:
    each is within (n - 1) u sum|term| of the exact sum to first order,
    u = 2^-53; 2 n u sum|term| covers both and the higher-order terms."""
    return 2.0 * np.asarray(n, np.float64) * 2.0 ** -53 * abs_terms


def rms_bound(ref):
    """rms_sum: the bound of two summation orders of its F terms, plus
    F * 2^-52 * max_f rms_f for the terms themselves (the square roots and
    the inner means, computed in another order)."""
    F = ref['frames'].astype(np.float64)
    return sum_bound(F, ref['rms_sum']) + F * 2.0 ** -52 * ref['rms_max']
