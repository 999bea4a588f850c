"""Host restatement of fast generation's sampling draw (generate.py:228-240:
log(p) / T, normalise, np.random.choice) with the device's random numbers, in
float64 numpy and never through the library.  The tests compare every code
the device draws with pick(weights(p, T), uniform(seed, counter)).

The random number.  Every draw site (fastgen_kernel, fg_draw_wave,
fg_draw_wg256<1|2> and fastgen_wide_kernel of csrc/wn_fastgen.hip,
fgb_draw_wave of csrc/wn_fastgen_batch.hip) takes the uniform of
csrc/wn_common.h (draw_uniform, or its halves draw_bits and draw_unit),
    r = splitmix64(seed ^ splitmix64(counter)),   u = (r >> 11) * 2**-53
and walks the inverse CDF of the weights at u * total.  All but fg_draw_wg256
draw with wave_draw_f64 of the same header.

The counter is the generator's absolute step count at the step that consumes
the code before the drawn one: `tpos` = cursors[0] + step in fastgen_kernel
and fastgen_wide_kernel, `steps_done` in fg_draw_wave, `base + i` (=
steps_done) in fg_draw_wg256 and `step` (the step that produced the logits,
per stream) in fgb_draw_wave.  After reset_generator(), output code k + 1 of
generate() (index k + 1 of the returned codes, seed samples included) is
drawn with counter k; prime_generator() leaves cursors[0] = len(seed) - 1,
which keeps that rule; continue_generation() goes on counting from where the
previous call stopped (its first new code: counter = steps so far).

The temperature.  WaveNetModel hands it to the device as float32, so compare
draws with tau = float(np.float32(T)).  At tau == 1 the weights are the
float32 probabilities themselves; otherwise exp(log p / tau - max), with a
probability of exactly 0 (float32 underflow) weighted exactly 0, as
np.log(0) = -inf makes it in the reference."""
import numpy as np

_MASK = (1 << 64) - 1
_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(x):
    """SplitMix64 (the state advances by the golden gamma, then the output
    mix): splitmix64(0) is the first output of the stream started at state 0.
    Python int or integer array; returns the same kind."""
    scalar = np.ndim(x) == 0
    v = np.uint64(int(x) & _MASK) if scalar else np.asarray(x).astype(np.uint64)
    with np.errstate(over='ignore'):
        v = v + _GAMMA
        v = (v ^ (v >> np.uint64(30))) * _M1
        v = (v ^ (v >> np.uint64(27))) * _M2
        v = v ^ (v >> np.uint64(31))
    return int(v) if scalar else v


def uniform(seed, counter):
    """The draw's uniform in [0, 1): 53 bits of
    splitmix64(seed ^ splitmix64(counter)).  `counter`: int or array."""
    s = np.uint64(int(seed) & _MASK)
    c = splitmix64(np.atleast_1d(np.asarray(counter, np.int64)))
    r = splitmix64(c ^ s) >> np.uint64(11)
    u = r.astype(np.float64) * 2.0 ** -53
    return float(u[0]) if np.ndim(counter) == 0 else u


def weights(p32, tau):
    """Unnormalised sampling weights of float32 probabilities p32 (last axis:
    the codes) at temperature tau, in float64."""
    p = np.asarray(p32, np.float32).astype(np.float64)
    if tau == 1.0:
        return p
    with np.errstate(divide='ignore'):
        lp = np.where(p > 0, np.log(np.where(p > 0, p, 1.0)) / tau, -np.inf)
    return np.exp(lp - lp.max(axis=-1, keepdims=True))


def _cdf(w, u):
    c = np.cumsum(w, axis=-1)
    return c, np.asarray(u, np.float64) * c[..., -1]


def pick(w, u):
    """The first code whose inclusive cumulative weight exceeds u * total
    (np.random.choice's inverse CDF with a known uniform).  w: [Q] or [N, Q]
    with u a scalar or [N]."""
    c, t = _cdf(w, u)
    return np.argmax(c > t[..., None], axis=-1)


def margin(w, u):
    """Distance of u * total from the nearest boundary between two codes of
    the cumulative weights (inf with a single code)."""
    c, t = _cdf(w, u)
    if c.shape[-1] < 2:
        return np.full(np.shape(t), np.inf)
    return np.abs(c[..., :-1] - t[..., None]).min(axis=-1)


def boundary_codes(w, u):
    """The two codes with weight > 0 on either side of the CDF boundary
    nearest to u * total (1-D w, scalar u)."""
    w = np.asarray(w, np.float64)
    c, t = _cdf(w, u)
    k = int(np.abs(c[:-1] - t).argmin())
    nz = np.nonzero(w > 0)[0]
    lo, hi = nz[nz <= k], nz[nz > k]
    return (int(lo[-1]) if lo.size else None, int(hi[0]) if hi.size else None)


TIE_REL = 1e-12    # a boundary this close (relative to the total) is a tie


def check_draws(codes, probs, tau, seed, counters, max_ties=2, what=''):
    """Every drawn code against the restatement.  codes[i] was drawn from the
    float32 probabilities probs[i] with counter counters[i] (one row per
    draw).  A code other than the restated one is accepted only at a
    summation-order tie (u * total within TIE_REL * total of a boundary) and
    only as one of the two codes beside that boundary; at most `max_ties` of
    them.  No code with probability 0 may be drawn.  Returns the number of
    ties."""
    codes = np.asarray(codes).reshape(-1)
    probs = np.asarray(probs, np.float32).reshape(len(codes), -1)
    counters = np.asarray(counters, np.int64).reshape(-1)
    assert len(counters) == len(codes)
    Q = probs.shape[1]
    assert codes.min() >= 0 and codes.max() < Q, (what, codes.min(), codes.max())
    zero = probs[np.arange(len(codes)), codes] == 0
    if zero.any():
        i = int(np.nonzero(zero)[0][0])
        raise AssertionError(
            '%s: %d of %d draws took a code of probability 0 (first: draw %d, '
            'counter %d, code %d)' % (what, int(zero.sum()), len(codes), i,
                                      counters[i], codes[i]))
    w = weights(probs, tau)
    u = uniform(seed, counters)
    ref = pick(w, u)
    bad = np.nonzero(ref != codes)[0]
    ties = 0
    for i in bad:
        m = float(margin(w[i], u[i]))
        total = float(w[i].sum())
        near = boundary_codes(w[i], u[i])
        if not (m < TIE_REL * total and int(codes[i]) in near):
            raise AssertionError(
                '%s: draw %d (counter %d, u = %.17g): device code %d, restated '
                'code %d (margin %.3g of total %.6g; %d of %d draws differ)'
                % (what, i, counters[i], u[i], codes[i], ref[i], m, total,
                   len(bad), len(codes)))
        ties += 1
    assert ties <= max_ties, '%s: %d summation-order ties (at most %d)' % (
        what, ties, max_ties)
    return ties
