"""Independent restatement of input noise (test infrastructure only; does not
import wavenet.input_noise): the rule in plain Python integers, one position
at a time, and a float64 loss with gradients for a pass whose network inputs
differ from its targets.

The rule (include/wavenet_hip.h): with thresh = int(prob * 2**24), w = width,

    c    = (key << 24) | t
    bits = splitmix64((seed ^ 0x6e6f697365) ^ splitmix64(c))
    hit  = (bits & 0xFFFFFF) < thresh
    d    = ((bits >> 24) & 0xFFFFF) % (w + 1) - ((bits >> 44) & 0xFFFFF) % (w + 1)
    q_in = clamp(q + d, 0, Q - 1) where hit, t < n and 0 <= q < Q, else q.

The loss: tests/lc_ref.py's network reads q_in; the labels are the CLEAN
codes shifted by one; lengths and history mask rows as tests/masked_ref.py
and tests/hist_ref.py state them (row t of clip b has a target iff
h[b] <= t + 1 < n[b]; row n[b] - 1 is TF's label-less last row; the mean over
D = sum(n - h), or B * T without lengths and history).
"""
import numpy as np
import torch
import torch.nn.functional as F

import lc_ref

M64 = (1 << 64) - 1
TAG = 0x6e6f697365


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def thresh(prob):
    return int(float(prob) * 16777216.0)


_BITS = {}


def bits_of(seed, key, n):
    """[bits of position t for t < n] of one clip (kept: the tests' grids
    ask for the same clips under many settings)."""
    have = _BITS.setdefault((seed, key), [])
    s = (seed ^ TAG) & M64
    for t in range(len(have), n):
        have.append(splitmix64(s ^ splitmix64(((key << 24) | t) & M64)))
    return have


def draw(seed, key, t, prob, width):
    """(hit, d) of one position."""
    bits = bits_of(int(seed), int(key), t + 1)[t]
    w1 = width + 1
    return ((bits & 0xFFFFFF) < thresh(prob),
            ((bits >> 24) & 0xFFFFF) % w1 - ((bits >> 44) & 0xFFFFF) % w1)


def codes_in(q, keys, lengths, Q, prob, width, seed):
    """q_in int32 [B, T] of codes q [B, T]; lengths B ints or None."""
    q = np.asarray(q)
    B, T = q.shape
    out = q.astype(np.int32).copy()
    th, w1 = thresh(prob), width + 1
    for b in range(B):
        n = T if lengths is None else max(0, min(T, int(lengths[b])))
        bits = bits_of(int(seed), int(keys[b]), n)
        row = q[b].tolist()
        for t in range(n):
            v, r = row[t], bits[t]
            if 0 <= v < Q and (r & 0xFFFFFF) < th:
                d = ((r >> 24) & 0xFFFFF) % w1 - ((r >> 44) & 0xFFFFF) % w1
                out[b, t] = min(max(v + d, 0), Q - 1)
    return out


# ---- the grid of shapes and settings both test files walk ------------------
SHAPES = [(1, 1), (2, 3), (1, 4), (3, 7), (2, 1024), (3, 1027), (2, 4099)]
SEEDS = (0, (1 << 63) + 12345)
PROBS = (0.0, 2.0 ** -24, 0.5, 1.0)
KEYS = (0, (1 << 40) - 1, 12345)


def length_sets(B, T):
    """None, all T, and a mix of 1 / an odd middle / T."""
    mid = max(1, min(T, (T // 2) | 1))
    return [None, [T] * B, [(1, mid, T)[(b + B) % 3] for b in range(B)]]


def grid():
    """Yields (audio [B, T], its mu-law codes q [B, T] by the project's
    oracle, keys [B], lengths, Q, prob, width, seed)."""
    from util import O
    rng = np.random.default_rng(24)
    for i, (B, T) in enumerate(SHAPES):
        keys = np.roll(np.array(KEYS, np.int64), i)[:B]
        for Q in (16, 256):
            audio = rng.uniform(-1, 1, (B, T)).astype(np.float32)
            q = np.asarray(O.mu_law_encode(audio, Q)).astype(np.int32)
            for lengths in length_sets(B, T):
                for width in (1, 3, Q - 1):
                    for prob in PROBS:
                        for seed in SEEDS:
                            yield (audio, q, keys, lengths, Q, prob, width,
                                   seed)


def _rows(raw, q_tgt, lengths, history, Q, quirk):
    """Per-row loss terms [B * T] of logits raw for the clean targets, and
    the denominator."""
    B, T = q_tgt.shape
    plain = lengths is None and history is None
    n = np.full(B, T, np.int64) if lengths is None else \
        np.asarray(lengths, np.int64).reshape(B)
    h = np.zeros(B, np.int64) if history is None else \
        np.broadcast_to(np.asarray(history, np.int64), (B,)).copy()
    nt, ht = torch.as_tensor(n).reshape(B, 1), torch.as_tensor(h).reshape(B, 1)
    t = torch.arange(T).reshape(1, T)
    has_label = ((t + 1 < nt) & (t + 1 >= ht)).reshape(-1)
    last = (t + 1 == nt).reshape(-1)
    enc = F.one_hot(q_tgt, Q).to(torch.float64)
    lab = F.pad(enc[:, 1:, :], (0, 0, 0, 1)).reshape(-1, Q)
    pred = raw.reshape(-1, Q)
    lse = torch.logsumexp(pred, -1)
    row = torch.where(has_label, lse - (lab * pred).sum(-1),
                      torch.zeros_like(lse))
    if quirk:
        row = torch.where(last, lse - lse.detach(), row)
    return row, float(B * T) if plain else float((n - h).sum())


def loss_and_grads(var, dilations, q_clean, q_in, lc=None, gc_ids=None,
                   lengths=None, history=None, use_biases=False,
                   quantization_channels=256, relu_masks=None,
                   residual_postproc=False, tf_xent_zero_label_quirk=True,
                   return_logits=False):
    """var, dilations, lc, gc_ids, relu_masks: as lc_ref.loss_and_grads.
    q_in int [B, T] is what the network reads, q_clean int [B, T] what the
    rows are labelled with.  Returns (loss, gradient tree[, float64 logits
    [B, T, Q]])."""
    v = lc_ref._to_torch(var)
    Q = quantization_channels
    qi = torch.as_tensor(np.asarray(q_in), dtype=torch.int64)
    qc = torch.as_tensor(np.asarray(q_clean), dtype=torch.int64)
    lct = None if lc is None else torch.as_tensor(np.asarray(lc, np.float64))
    raw, _ = lc_ref._forward(v, dilations, qi, lct, gc_ids, use_biases, Q,
                             relu_masks, residual_postproc)
    row, D = _rows(raw, qc, lengths, history, Q, tf_xent_zero_label_quirk)
    loss = row.sum() / D
    loss.backward()
    out = (float(loss.detach()), lc_ref._grads(v))
    if return_logits:
        out += (raw.detach().numpy(),)
    return out


def logits(var, dilations, q_in, lc=None, gc_ids=None, use_biases=False,
           quantization_channels=256, residual_postproc=False):
    """float64 logits [B, T, Q] of the network reading q_in."""
    return lc_ref.logits(var, dilations, q_in, lc, gc_ids, use_biases,
                         quantization_channels, residual_postproc)
