"""An independent float64 restatement of include/wavenet_lc_frames.h in plain
Python loops (no numpy scans, nothing shared with wavenet/frontend.py): the
pitch channels of one clip's F0 track, the assembled frames of a batch, and
hand-made tracks for the tests."""
import math

import numpy as np


def rel(f0, fmin, fmax):
    """r of a voiced frame: min(max(log2(f0 / fmin) / log2(fmax / fmin), 0),
    1) in Python floats (float64)."""
    r = math.log2(float(f0) / fmin) / math.log2(fmax / fmin) \
        if not math.isinf(float(f0)) else math.inf
    return min(max(r, 0.0), 1.0)


def channels(f0, nframes, mode, fmin, fmax):
    """(ch0 float64 [F], flag float64 [F]) of one clip's track f0 [F] with
    `nframes` real frames: the F0 channel BEFORE its rounding to float32, and
    the voicing flag."""
    F = len(f0)
    n = min(max(int(nframes), 0), F)
    voiced = [f < n and bool(f0[f] > 0) for f in range(F)]    # (NaN > 0: False)
    r = [rel(f0[f], fmin, fmax) if voiced[f] else None for f in range(F)]
    # the nearest voiced frame at or before f, and at or behind it
    before, behind, last = [None] * F, [None] * F, None
    for f in range(n):
        last = f if voiced[f] else last
        before[f] = last
    last = None
    for f in range(n - 1, -1, -1):
        last = f if voiced[f] else last
        behind[f] = last
    ch0, flag = [0.0] * F, [0.0] * F
    for f in range(n):
        if voiced[f]:
            ch0[f], flag[f] = r[f], 1.0
            continue
        if mode == 0:
            continue
        a, e = before[f], behind[f]
        if a is not None and e is not None:
            ch0[f] = r[a] + (r[e] - r[a]) * (float(f - a) / float(e - a))
        elif e is not None:
            ch0[f] = r[e]
        elif a is not None:
            ch0[f] = r[a]
    return np.array(ch0, np.float64), np.array(flag, np.float64)


def batch_channels(f0, nframes, mode, fmin, fmax):
    """(ch0, flag) float64 [B, F] of f0 [B, F]; nframes [B] or None."""
    B, F = f0.shape
    n = [F] * B if nframes is None else nframes
    rows = [channels(f0[b], n[b], mode, fmin, fmax) for b in range(B)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def track(F, runs, hz=(80.0, 420.0), seed=0):
    """An F0 track float32 [F]: voiced on the half-open frame ranges `runs`
    (pitches drawn log-uniformly from `hz`), 0 elsewhere."""
    rng = np.random.default_rng(seed)
    f0 = np.zeros(F, np.float32)
    for lo, hi in runs:
        lo, hi = max(lo, 0), min(hi, F)
        if hi > lo:
            f0[lo:hi] = np.exp(rng.uniform(math.log(hz[0]), math.log(hz[1]),
                                           hi - lo)).astype(np.float32)
    return f0


def seam_tracks(F, CH):
    """Tracks [K, F] whose voiced runs and gaps end on, start on and span the
    chunk seams of a scan with CH frames per step, as far as F reaches; with
    leading-only and trailing-only voicing, one voiced frame at the first, a
    middle and the last position, an unvoiced clip and a fully voiced one."""
    s1, s2 = CH, 2 * CH
    spans = [
        [],                                         # all unvoiced
        [(0, F)],                                   # all voiced
        [(0, 1)], [(F // 2, F // 2 + 1)], [(F - 1, F)],
        [(0, 1), (F - 1, F)],                       # one gap of F - 2 frames
        [(0, s1)],                                  # a run that ends on a seam
        [(s1, F)],                                  # a run that starts on one
        [(s1 - 3, s1 + 3)],                         # a run that spans one
        [(0, s1 - 2), (s1 + 2, F)],                 # a gap that spans one
        [(0, s1 - 4), (s1, s1 + 1)],                # a gap that ends on one
        [(s1 - 1, s1), (s1 + 5, s1 + 6)],           # a gap that starts on one
        [(0, 2)],                                   # leading only, over seams
        [(F - 2, F)],                               # trailing only, over seams
        [(2, 3), (s2 + 1, F)],                      # a gap over two seams
        [(1, 2), (3, 4), (5, 9), (s1 + 1, s1 + 2), (s2 - 1, s2)],
    ]
    return np.stack([track(F, r, seed=10 + i) for i, r in enumerate(spans)])


def tone_with_gap(f, n=4000, gap=(1500, 2300), rate=16000.0, seed=0):
    """A harmonic tone of f Hz with a silent gap: float32 [n]."""
    rng = np.random.default_rng(seed)
    ph = 2 * np.pi * f * np.arange(n) / rate
    x = 0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 1.0) + \
        0.01 * rng.standard_normal(n)
    x[gap[0]:gap[1]] = 0.0
    return x.astype(np.float32)
