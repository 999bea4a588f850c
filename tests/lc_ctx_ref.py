"""float64 restatement of the frame-context convolution in front of the
learned local-conditioning upsampler (test infrastructure only):

    ctx[b][f][j] = sum_{k=0..2p} sum_c W[k][c][j] frames[b][f + k - p][c]

with frames outside [0, F) zero, W [2p + 1][Lc][Lc].  The upsampler
(tests/lc_up_ref.py) then runs on ctx in place of the frames, and its rows feed
tests/lc_ref.py's network; gradients by torch autograd on the CPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

import lc_ref
import lc_up_ref


def context(frames, W):
    """frames [B, F, Lc], W [2p + 1, Lc, Lc] (torch float64) -> ctx
    [B, F, Lc]."""
    K = W.shape[0]
    p = (K - 1) // 2
    nf = frames.shape[1]
    pad = F.pad(frames, (0, 0, p, p))
    out = 0
    for k in range(K):
        out = out + pad[:, k:k + nf, :] @ W[k]
    return out


def brute_force(frames, W):
    """One clip, one frame, one channel at a time (numpy float64)."""
    frames = np.asarray(frames, np.float64)
    W = np.asarray(W, np.float64)
    nf, Lc = frames.shape
    p = (W.shape[0] - 1) // 2
    out = np.zeros((nf, Lc))
    for f in range(nf):
        for j in range(Lc):
            a = 0.0
            for k in range(2 * p + 1):
                g = f + k - p
                if 0 <= g < nf:
                    for c in range(Lc):
                        a += W[k, c, j] * frames[g, c]
            out[f, j] = a
    return out


def rows_np(frames, offsets, T, scales, var):
    """The context convolution, then lc_up_ref.rows, on numpy: var is the
    model tree (its 'lc_context' and 'lc_upsample' keys)."""
    W = torch.as_tensor(np.asarray(var['lc_context']['filter'], np.float64))
    with torch.no_grad():
        ctx = context(torch.as_tensor(np.asarray(frames, np.float64)), W)
    return lc_up_ref.rows_np(ctx.numpy(), offsets, T, scales,
                             var['lc_upsample'])


def loss_and_grads(var, dilations, codes, frames, offsets, scales,
                   gc_ids=None, use_biases=False, quantization_channels=256,
                   relu_masks=None, tf_xent_zero_label_quirk=True):
    """lc_up_ref.loss_and_grads with the context convolution in front of the
    upsampler: the gradient tree includes 'lc_context'."""
    v = lc_ref._to_torch(var)
    Q = quantization_channels
    q = torch.as_tensor(np.asarray(codes), dtype=torch.int64)
    B, T = q.shape
    ctx = context(torch.as_tensor(np.asarray(frames, np.float64)),
                  v['lc_context']['filter'])
    up = v['lc_upsample']
    lct = lc_up_ref.rows(ctx, np.broadcast_to(np.asarray(offsets), (B,)), T,
                         scales, [c['filter'] for c in up],
                         [c['bias'] for c in up] if 'bias' in up[0] else None)
    raw, enc = lc_ref._forward(v, dilations, q, lct, gc_ids, use_biases, Q,
                               relu_masks, False)
    lab = F.pad(enc[:, 1:, :], (0, 0, 0, 1)).reshape(-1, Q)
    pred = raw.reshape(-1, Q)
    lse = torch.logsumexp(pred, -1)
    row = lse - (lab * pred).sum(-1)
    if tf_xent_zero_label_quirk:
        row = torch.where(lab.sum(-1) > 0, row, lse - lse.detach())
    loss = row.mean()
    loss.backward()
    return float(loss.detach()), lc_ref._grads(v)
