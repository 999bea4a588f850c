"""An independent float64 oracle of the pitch path (include/
wavenet_pitch_path.h), in its direct O(N^2) form

    voiced s <- voiced k : V[k] + jump * |log2 tau_s - log2 tau_k|
    voiced s <- unvoiced : U + switch
    unvoiced <- voiced k : V[k] + switch
    unvoiced <- unvoiced : U

with the local costs c'[tau] + octave_bias * (log2 tau - log2 tau_min) for the
voiced lag tau and `unvoiced` (0 on a silent frame, lag[f] == 0) for the
unvoiced state.  No table, no one-sided minima, no normalisation: it shares no
code with the package.  Also the test signals of tests/test_pitch_path_host.py
and tests/test_gpu_pitch_path.py."""
import itertools
import math

import numpy as np

DEFAULTS = dict(jump=0.3, octave_bias=0.05, switch=0.2)


def _costs(cmnd, lag, tau_min, tau_max, jump, octave_bias, switch, unvoiced):
    """(loc [F, N + 1], trans [N + 1, N + 1]): trans[k, s] is the cost of
    going from state k to state s; state N is unvoiced."""
    c = np.asarray(cmnd, np.float64)
    N = tau_max - tau_min
    lg = np.array([math.log2(t) for t in range(tau_min, tau_max)])
    loc = np.empty((c.shape[0], N + 1))
    loc[:, :N] = c[:, tau_min:tau_max] + octave_bias * (lg - lg[0])[None, :]
    loc[:, N] = np.where(np.asarray(lag) == 0, 0.0, unvoiced)
    trans = np.full((N + 1, N + 1), float(switch))
    trans[:N, :N] = jump * np.abs(lg[None, :] - lg[:, None])
    trans[N, N] = 0.0
    return loc, trans


def solve(cmnd, lag, tau_min, tau_max, jump, octave_bias, switch, unvoiced):
    """(states [F], the optimum J*): a cheapest path and its cost."""
    loc, trans = _costs(cmnd, lag, tau_min, tau_max, jump, octave_bias,
                        switch, unvoiced)
    F = loc.shape[0]
    D = loc[0].copy()
    back = np.zeros((F, loc.shape[1]), np.int64)
    for f in range(1, F):
        through = D[:, None] + trans
        back[f] = through.argmin(0)
        D = through.min(0) + loc[f]
    states = np.zeros(F, np.int64)
    states[-1] = int(D.argmin())
    for f in range(F - 1, 0, -1):
        states[f - 1] = back[f, states[f]]
    return states, float(D.min())


def score(states, cmnd, lag, tau_min, tau_max, jump, octave_bias, switch,
          unvoiced):
    """The cost of the given path in float64."""
    loc, trans = _costs(cmnd, lag, tau_min, tau_max, jump, octave_bias,
                        switch, unvoiced)
    J = loc[0, states[0]]
    for f in range(1, len(states)):
        J += trans[states[f - 1], states[f]] + loc[f, states[f]]
    return float(J)


def brute(cmnd, lag, tau_min, tau_max, jump, octave_bias, switch, unvoiced):
    """The optimum by enumeration of every path (tiny N and F only)."""
    N, F = tau_max - tau_min, np.asarray(cmnd).shape[0]
    return min(score(path, cmnd, lag, tau_min, tau_max, jump, octave_bias,
                     switch, unvoiced)
               for path in itertools.product(range(N + 1), repeat=F))


def states_of(lag, tau_min, tau_max):
    """A Pitch's lag [F] as states: 0 -> N (unvoiced), tau -> tau - tau_min."""
    lag = np.asarray(lag, np.int64)
    return np.where(lag == 0, tau_max - tau_min, lag - tau_min)


# ------------------------------------------------------------------ inputs
def tracker_with_lags(pitch, tau_min=None, tau_max=None, **kw):
    """The default 16 kHz tracker, or one whose lag range is exactly
    tau_min .. tau_max (fmax just under 16000 / tau_min, fmin just over
    16000 / tau_max: the float32 rounding of neither can move a lag)."""
    if tau_min is None:
        return pitch.PitchTracker(16000, **kw)
    t = pitch.PitchTracker(16000, fmin=16000.0 / tau_max * (1 + 1e-6),
                           fmax=16000.0 / tau_min * (1 - 1e-6), **kw)
    assert (t.tau_min, t.tau_max) == (tau_min, tau_max)
    return t



def random_rows(seed, F, tau_max, silent=0.2, quantum=None):
    """(cmnd float32 [F, tau_max + 1] uniform in [0, 2) -- multiples of
    `quantum` with it -- with all-1 rows where lag is 0; lag int32 [F], 0 on
    about `silent` of the frames and 1 elsewhere (the path reads only
    lag == 0))."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 2.0, (F, tau_max + 1))
    if quantum:
        c = np.floor(c / quantum) * quantum
    c = c.astype(np.float32)
    lag = (rng.uniform(size=F) >= silent).astype(np.int32)
    c[lag == 0] = 1.0
    c[:, 0] = 1.0
    return c, lag


def octave_signal(sr=16000, n=16000):
    """A 100 Hz tone whose fundamental and third harmonic drop to a fifth in
    three stretches, under a steady second harmonic: the raw tracker reports
    lag 80 there instead of 160.  Silent from sample 14500 on."""
    t = np.arange(n) / float(sr)
    a1 = np.ones(n)
    for lo in (3000, 7000, 11000):
        a1[lo:lo + 2000] = 0.2
    x = 0.2 * (a1 * np.sin(2 * np.pi * 100 * t) +
               np.sin(2 * np.pi * 200 * t + 0.4) +
               0.3 * a1 * np.sin(2 * np.pi * 300 * t + 1.1))
    x[14500:] = 0.0
    return x


def harmonic_tone(f, sr=16000, n=16000):
    t = np.arange(n) / float(sr)
    return 0.3 * (np.sin(2 * np.pi * f * t) +
                  0.5 * np.sin(2 * np.pi * 2 * f * t + 0.7) +
                  0.25 * np.sin(2 * np.pi * 3 * f * t + 1.9))


def glide(sr=16000, n=16000):
    """110 -> 220 Hz, two harmonics."""
    t = np.arange(n) / float(sr)
    ph = 2 * np.pi * (110.0 * t + 55.0 * t * t)
    return 0.3 * (np.sin(ph) + 0.5 * np.sin(2 * ph + 0.3))


def noise(sr=16000, n=16000):
    return 0.1 * np.random.default_rng(5).standard_normal(n)
