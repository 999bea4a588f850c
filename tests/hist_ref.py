"""float64 restatement of piece history (test infrastructure only): the
windowed loss and score of WaveNetModel.loss / score with `history`, and the
corpus's plan rule with history.  Built like tests/masked_ref.py and
tests/corpus_ref.py, on their layers (tests/lc_ref.py's network over
oracle/torch_graph.py's convolutions; tests/lc_up_ref.py's upsampler for
frames; tests/corpus_ref.py's plan).

The rule: clip b is the clip of n[b] samples fed alone; row t has a target
iff h[b] <= t + 1 < n[b]; rows with t + 1 < h[b] add nothing; row n[b] - 1 is
the label-less last row (TF's softmax / D backprop); the mean is taken over
D = sum(n - h).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import corpus_ref
import lc_ref
import lc_up_ref
import score_ref


def _bh(history, B):
    return np.broadcast_to(np.asarray(history, np.int64), (B,)).copy()


def loss_and_grads(var, dilations, codes, lengths, history, lc=None,
                   gc_ids=None, frames=None, offsets=None, scales=None,
                   use_biases=False, quantization_channels=256,
                   relu_masks=None, tf_xent_zero_label_quirk=True,
                   denominator=None):
    """var, dilations, codes [B, T], lc, gc_ids, relu_masks: as
    masked_ref.loss_and_grads, on the padded batch; lengths: B ints in [1, T]
    or None (T for every clip); history: B ints or one, 0 <= h <= n.  frames
    [B, F, Lc] at offsets [B] through the learned upsampler (scales) instead
    of lc rows: the gradient tree then includes 'lc_upsample'.  Returns
    (loss, gradient tree)."""
    v = lc_ref._to_torch(var)
    Q = quantization_channels
    q = torch.as_tensor(np.asarray(codes), dtype=torch.int64)
    B, T = q.shape
    n = np.full(B, T, np.int64) if lengths is None else \
        np.asarray(lengths, np.int64).reshape(B)
    h = _bh(history, B)
    assert (h >= 0).all() and (h <= n).all() and n.min() >= 1 and n.max() <= T
    lct = None if lc is None else torch.as_tensor(np.asarray(lc, np.float64))
    if frames is not None:
        up = v['lc_upsample']
        lct = lc_up_ref.rows(
            torch.as_tensor(np.asarray(frames, np.float64)),
            np.broadcast_to(np.asarray(offsets), (B,)), T, scales,
            [c['filter'] for c in up],
            [c['bias'] for c in up] if 'bias' in up[0] else None)
    raw, enc = lc_ref._forward(v, dilations, q, lct, gc_ids, use_biases, Q,
                               relu_masks, False)
    nt, ht = torch.as_tensor(n).reshape(B, 1), torch.as_tensor(h).reshape(B, 1)
    t = torch.arange(T).reshape(1, T)
    has_label = ((t + 1 < nt) & (t + 1 >= ht)).reshape(-1)
    last = (t + 1 == nt).reshape(-1)
    lab = F.pad(enc[:, 1:, :], (0, 0, 0, 1)).reshape(-1, Q)
    pred = raw.reshape(-1, Q)
    lse = torch.logsumexp(pred, -1)
    row = torch.where(has_label, lse - (lab * pred).sum(-1),
                      torch.zeros_like(lse))
    if tf_xent_zero_label_quirk:
        row = torch.where(last, lse - lse.detach(), row)
    D = float((n - h).sum()) if denominator is None else float(denominator)
    loss = row.sum() / D
    loss.backward()
    return float(loss.detach()), lc_ref._grads(v)


def rows(logits, codes, lengths, history, Q):
    """score_ref.rows with the history rows taken out: rows with
    t + 1 < h[b] have no target (nll 0, has / hit False)."""
    r = score_ref.rows(logits, codes, lengths, Q)
    B, T = np.asarray(codes).shape
    keep = np.arange(T)[None, :] + 1 >= _bh(history, B)[:, None]
    return dict(nll=np.where(keep, r['nll'], 0.0), has=r['has'] & keep,
                hit=r['hit'] & keep, margin=r['margin'])


def clips(r):
    """score_ref.clips: (nll float64 [B], count [B], correct [B])."""
    return score_ref.clips(r)


def denominator(lengths, history):
    n = np.asarray(lengths, np.int64)
    return float((n - _bh(history, n.shape[0])).sum())


def plan(lengths, sample_size, crop, seed, step, B, history,
         category_ids=None, T=None):
    """corpus_ref.plan with history H: per slot (utterance, start', n',
    speaker id or None), the slots' history h [B], T, and the slots' original
    starts.  h = min(H, start), start' = start - h, n' = n + h; then n' is cut
    to T (default max n') and h to n'."""
    slots, _ = corpus_ref.plan(lengths, sample_size, crop, seed, step, B,
                               category_ids)
    out, hist, orig = [], [], []
    for u, start, n, gc in slots:
        h = min(int(history), start)
        out.append([u, start - h, n + h, gc])
        hist.append(h)
        orig.append(start)
    if T is None:
        T = max(s[2] for s in out)
    for s in out:
        s[2] = min(s[2], T)
    hist = [min(h, s[2]) for h, s in zip(hist, out)]
    return [tuple(s) for s in out], hist, T, orig


def validation_pieces(n_file, sample_size, history):
    """[(first sample, end, h)] of a file of n_file samples cut into pieces
    of sample_size with history."""
    out = []
    for k in range(0, n_file, sample_size):
        h = min(history, k)
        out.append((k - h, min(k + sample_size, n_file), h))
    return out


def fsum(x):
    return math.fsum(np.asarray(x, np.float64).reshape(-1).tolist())
