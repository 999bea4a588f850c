"""float64 restatement of the learned local-conditioning upsampler (test
infrastructure only).  Layer i (scale s_i) is a transposed convolution over
time with kernel = stride = s_i and a 3-tap kernel over the feature axis:

    out[c] = b_i + W_i[j][0] u[c-1] + W_i[j][1] u[c] + W_i[j][2] u[c+1]

(u[-1] = u[Lc] = 0) for output slot j of input row u.  Timeline position p
takes frame p // hop and the slot digits of p % hop (most significant first).
The rows feed tests/lc_ref.py's network, which ignores the variable tree's
'lc_upsample' key; gradients by torch autograd on the CPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

import lc_ref


def rows(frames, offsets, T, scales, filters, biases=None):
    """frames [B, F, Lc] and the layers' filters [s_i, 3] (biases [1] or
    None), torch float64 -> rows [B, T, Lc]; row t of clip b is timeline
    position offsets[b] + t."""
    B = frames.shape[0]
    hop = int(np.prod(scales))
    suf = [int(np.prod(scales[i + 1:])) for i in range(len(scales))]
    out = []
    for b in range(B):
        p = int(offsets[b]) + torch.arange(T)
        u = frames[b][p // hop]
        j = p % hop
        for i, s in enumerate(scales):
            w = filters[i][(j // suf[i]) % s]              # [T, 3]
            pad = F.pad(u, (1, 1))
            u = (w[:, 0:1] * pad[:, :-2] + w[:, 1:2] * pad[:, 1:-1] +
                 w[:, 2:3] * pad[:, 2:])
            if biases is not None:
                u = u + biases[i]
        out.append(u)
    return torch.stack(out)


def rows_np(frames, offsets, T, scales, var_up):
    """rows() on numpy: var_up is the model tree's 'lc_upsample' list."""
    fl = [torch.as_tensor(np.asarray(c['filter'], np.float64)) for c in var_up]
    bl = None
    if 'bias' in var_up[0]:
        bl = [torch.as_tensor(np.asarray(c['bias'], np.float64)) for c in var_up]
    with torch.no_grad():
        return rows(torch.as_tensor(np.asarray(frames, np.float64)),
                    offsets, T, scales, fl, bl).numpy()


def brute_force(frames, offset, T, scales, filters, biases=None):
    """One clip, one row, one channel at a time (numpy float64)."""
    frames = np.asarray(frames, np.float64)
    Lc = frames.shape[1]
    hop = int(np.prod(scales))
    out = np.zeros((T, Lc))
    for t in range(T):
        p = offset + t
        u = frames[p // hop].copy()
        rem, div = p % hop, hop
        for i, s in enumerate(scales):
            div //= s
            j, rem = rem // div, rem % div
            w = np.asarray(filters[i], np.float64)[j]
            v = np.zeros(Lc)
            for c in range(Lc):
                a = biases[i] if biases is not None else 0.0
                a += w[0] * (u[c - 1] if c > 0 else 0.0)
                a += w[1] * u[c]
                a += w[2] * (u[c + 1] if c + 1 < Lc else 0.0)
                v[c] = a
            u = v
        out[t] = u
    return out


def loss_and_grads(var, dilations, codes, frames, offsets, scales,
                   gc_ids=None, use_biases=False, quantization_channels=256,
                   relu_masks=None, tf_xent_zero_label_quirk=True):
    """lc_ref.loss_and_grads with the rows made by the upsampler from
    `frames` [B, F, Lc] at `offsets` [B]: the gradient tree includes
    'lc_upsample'."""
    v = lc_ref._to_torch(var)
    Q = quantization_channels
    q = torch.as_tensor(np.asarray(codes), dtype=torch.int64)
    B, T = q.shape
    up = v['lc_upsample']
    lct = rows(torch.as_tensor(np.asarray(frames, np.float64)),
               np.broadcast_to(np.asarray(offsets), (B,)), T, scales,
               [c['filter'] for c in up],
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
