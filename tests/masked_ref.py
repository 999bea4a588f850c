"""float64 reference of the masked loss (WaveNetModel.loss with `lengths`;
test infrastructure only).  Two routes to the same numbers:

  * loss_and_grads: tests/lc_ref.py's network on the PADDED batch, the
    cross-entropy rows masked as the model's docstring states them (clip b is
    a clip of T = lengths[b]: targets for t + 1 < lengths[b], the label-less
    row lengths[b] - 1 with TF's softmax / D backprop, nothing behind it, the
    mean over D = sum(lengths) rows), gradients by autograd;
  * assemble: sum_b lengths[b] * (L_b, g_b) / D from any trusted reference
    run on every clip ALONE and UNPADDED.  This is what the semantics mean,
    and it reaches the models lc_ref does not restate (scalar input, learned
    upsampling of frames with context).

tests/test_masked_loss_host.py holds the two against each other.
"""
import numpy as np
import torch
import torch.nn.functional as F

import lc_ref


def loss_and_grads(var, dilations, codes, lengths, lc=None, gc_ids=None,
                   use_biases=False, quantization_channels=256,
                   relu_masks=None, tf_xent_zero_label_quirk=True,
                   residual_postproc=False, denominator=None):
    """var, dilations, codes [B, T], lc, gc_ids, relu_masks: as
    lc_ref.loss_and_grads, on the padded batch.  lengths: B ints in [1, T].
    denominator: what the row sum is divided by (default sum(lengths)).
    Returns (loss, gradient tree)."""
    v = lc_ref._to_torch(var)
    Q = quantization_channels
    q = torch.as_tensor(np.asarray(codes), dtype=torch.int64)
    B, T = q.shape
    n = torch.as_tensor(np.asarray(lengths), dtype=torch.int64).reshape(B, 1)
    assert int(n.min()) >= 1 and int(n.max()) <= T
    lct = None if lc is None else torch.as_tensor(np.asarray(lc, np.float64))
    raw, enc = lc_ref._forward(v, dilations, q, lct, gc_ids, use_biases, Q,
                               relu_masks, residual_postproc)
    t = torch.arange(T).reshape(1, T)
    has_label = (t + 1 < n).reshape(-1)
    last = (t + 1 == n).reshape(-1)
    lab = F.pad(enc[:, 1:, :], (0, 0, 0, 1)).reshape(-1, Q)
    pred = raw.reshape(-1, Q)
    lse = torch.logsumexp(pred, -1)
    row = torch.where(has_label, lse - (lab * pred).sum(-1),
                      torch.zeros_like(lse))
    if tf_xent_zero_label_quirk:
        row = torch.where(last, lse - lse.detach(), row)
    D = float(n.sum()) if denominator is None else float(denominator)
    loss = row.sum() / D
    loss.backward()
    return float(loss.detach()), lc_ref._grads(v)


def _combine(trees, weights):
    first = trees[0]
    if isinstance(first, dict):
        return {k: _combine([t[k] for t in trees], weights) for k in first}
    if isinstance(first, list):
        return [_combine([t[i] for t in trees], weights)
                for i in range(len(first))]
    return sum(w * np.asarray(t, np.float64) for w, t in zip(weights, trees))


def assemble(per_clip, lengths, denominator=None):
    """per_clip: [(L_b, gradient tree g_b)] of every clip alone and unpadded
    (its first lengths[b] samples).  Returns (sum_b lengths[b] * L_b / D, the
    same combination of the trees)."""
    n = [int(x) for x in np.asarray(lengths).reshape(-1)]
    assert len(n) == len(per_clip)
    D = float(sum(n)) if denominator is None else float(denominator)
    w = [x / D for x in n]
    return (sum(wb * float(L) for wb, (L, _) in zip(w, per_clip)),
            _combine([g for _, g in per_clip], w))


def clip_masks(relu_masks, b, n):
    """The device's ReLU decisions of clip b's first n rows (or None)."""
    if relu_masks is None:
        return None
    return {k: m[b:b + 1, :n] for k, m in relu_masks.items()}


def clipwise(var, dilations, codes, lengths, lc=None, gc_ids=None,
             relu_masks=None, denominator=None, **kw):
    """assemble() over lc_ref.loss_and_grads of every clip alone."""
    per = []
    for b, n in enumerate(np.asarray(lengths).reshape(-1)):
        n = int(n)
        per.append(lc_ref.loss_and_grads(
            var, dilations, np.asarray(codes)[b:b + 1, :n],
            None if lc is None else np.asarray(lc)[b:b + 1, :n],
            gc_ids=None if gc_ids is None else np.asarray(gc_ids)[b:b + 1],
            relu_masks=clip_masks(relu_masks, b, n), **kw))
    return assemble(per, lengths, denominator)
