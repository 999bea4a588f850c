"""The device-resident corpus's rule, restated independently in numpy (it does
not import wavenet.corpus): splitmix64 in uint64, the epoch permutations, the
random starts, the plan of a batch, the gathers by plain slicing, the frames
windows."""
import numpy as np

M = 8                               # WaveNetModel.LC_CONTEXT_MAX
U64 = np.uint64


def splitmix64(x):
    x = np.atleast_1d(np.asarray(x, dtype=U64)).copy()
    with np.errstate(over='ignore'):
        x += U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U64(27))) * U64(0x94D049BB133111EB)
        x = x ^ (x >> U64(31))
    return x


def draw_bits(seed, c):
    return splitmix64(U64(seed) ^ splitmix64(c))


def splitmix64_int(x):
    """The same on Python ints (a check of the uint64 one)."""
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def make_items(lengths, sample_size, crop):
    """[(utterance, piece start)]"""
    items = []
    for u, n in enumerate(lengths):
        if n == 0:
            continue
        if crop == 'pieces' and sample_size:
            k = 0
            while k * sample_size < n:
                items.append((u, k * sample_size))
                k += 1
        else:
            items.append((u, 0))
    return items


def permutation(seed, e, P):
    keys = draw_bits(seed, np.arange(e * P, e * P + P, dtype=U64))
    return [i for _, i in sorted((int(k), i) for i, k in enumerate(keys))]


def plan(lengths, sample_size, crop, seed, step, B, category_ids=None,
         T=None):
    """Per slot (utterance, start, n, speaker id or None), and T."""
    items = make_items(lengths, sample_size, crop)
    P = len(items)
    slots = []
    for j in range(B):
        g = step * B + j
        e = g // P
        u, k = items[permutation(seed, e, P)[g % P]]
        nu = lengths[u]
        if crop == 'random':
            n = min(sample_size, nu)
            start = 0
            if nu > sample_size:
                start = int(draw_bits(seed ^ 0x63726f70, [g])[0]) % \
                    (nu - sample_size + 1)
        else:
            start = k
            n = nu - k if not sample_size else min(sample_size, nu - k)
        if T is not None:
            n = min(n, T)
        slots.append((u, start, n,
                      None if category_ids is None else category_ids[u]))
    return slots, (max(s[2] for s in slots) if T is None else T)


def gather(arrays, slots, T):
    """audio [B, T]: slices of the utterances, zeros behind them."""
    out = np.zeros((len(slots), T), np.float32)
    for j, (u, start, n, _) in enumerate(slots):
        out[j, :n] = arrays[u][start:start + n]
    return out


def window_frames(T, hop, m=M):
    return (T + hop - 2) // hop + 1 + 2 * m


def frame_windows(frames, slots, T, hop, m=M):
    """(window [B, Fw, Lc], offsets [B]) of per-utterance frames [F_u, Lc]."""
    Lc = frames[0].shape[1]
    out = np.zeros((len(slots), window_frames(T, hop, m), Lc), np.float32)
    offs = np.zeros(len(slots), np.int64)
    for j, (u, start, n, _) in enumerate(slots):
        f_lo = max(0, start // hop - m)
        f_hi = min(frames[u].shape[0], (start + n - 1) // hop + 1 + m)
        out[j, :f_hi - f_lo] = frames[u][f_lo:f_hi]
        offs[j] = start - f_lo * hop
    return out, offs


def frame_rows(frames, slots, T, hop):
    """rows [B, T, Lc]: row t is frame (start + t) // hop, zeros behind n."""
    Lc = frames[0].shape[1]
    out = np.zeros((len(slots), T, Lc), np.float32)
    for j, (u, start, n, _) in enumerate(slots):
        for t in range(n):
            out[j, t] = frames[u][(start + t) // hop]
    return out
