"""float64 restatement of what batched fast generation adds for mixture
models (test infrastructure only): the causal layer stepped over a 64-slot
history ring of levels, as include/wavenet_fastgen_mol.h states it."""
import numpy as np

SLOTS = 64
TOP = 65535


def centre32(j):
    """c(j) as the kernels form it: one rounded float32 division."""
    return float(np.float32(2 * int(j) - TOP) / np.float32(TOP))


def ring_causal(levels, W):
    """x [n, C] float64: step T consumes levels[T], which goes into slot
    T & 63 of a ring that starts empty (-1); the causal layer's output is
        x[T] = sum_k W[k] c(ring[(T - s_k) & 63]),
        s_k = (K0 - 1 - k) + (K0 - 1) // 2,
    k ascending from 0, a tap whose slot holds no level in 0 .. 65535
    skipped.  W: [K0, C]."""
    W = np.asarray(W, np.float64)
    K0 = W.shape[0]
    assert (K0 - 1) + (K0 - 1) // 2 < SLOTS
    ring = np.full(SLOTS, -1, np.int64)
    out = np.zeros((len(levels), W.shape[1]))
    for T, lv in enumerate(levels):
        ring[T & (SLOTS - 1)] = lv
        v = np.zeros(W.shape[1])
        for k in range(K0):
            j = ring[(T - ((K0 - 1 - k) + (K0 - 1) // 2)) & (SLOTS - 1)]
            if 0 <= j <= TOP:
                v = v + W[k] * centre32(j)
        out[T] = v
    return out
