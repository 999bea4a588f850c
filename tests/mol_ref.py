"""float64 restatement of the mixture-of-logistics head (test infrastructure
only, independent of wavenet/mol.py): the level rule in exact arithmetic, the
row loss from the NAIVE log(sigmoid(a) - sigmoid(b)) where that is well
conditioned and from the cancellation-free form elsewhere, gradients by
torch.autograd on the CPU, and a small whole network read from a model's
`variables`: scalar causal convolution, gated dilated stack with local and
global conditioning, skip sum, two 1x1 layers, mixture head.
"""
import numpy as np
import torch
import torch.nn.functional as F

import util  # noqa: F401  (puts the repository root on sys.path)
import lc_ctx_ref
import lc_ref
import lc_up_ref
from oracle.torch_graph import causal_conv

C = 65536
TOP = C - 1
H = 1.0 / TOP
NAIVE_MIN = 1e-3        # the naive difference is used above this


def levels(y):
    """Levels of float samples in float64: rint((clip(y) + 1) (C - 1) / 2).
    Equals the float32 rule wherever the sample is not within a float32
    rounding of a boundary."""
    y = np.clip(np.asarray(y, np.float64), -1.0, 1.0)
    return np.rint((y + 1.0) * (TOP / 2.0)).astype(np.int64)


def centres(j):
    return (2.0 * np.asarray(j, np.float64) - TOP) / TOP


def softplus(x):
    # (F.softplus goes linear above 20: 2e-9 off)
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def log_bin(j, mu, beta, form='auto'):
    """log P(level j) under a logistic(mu, e^beta), float64 torch, any
    broadcastable shapes (j int64).  form: 'naive' log(sigmoid(a) -
    sigmoid(b)) with the outer bins open, 'stable', or 'auto' (naive where
    the difference exceeds NAIVE_MIN)."""
    c = (2.0 * j.to(torch.float64) - TOP) / TOP
    is_ = torch.exp(-beta)
    a = (c + H - mu) * is_
    b = (c - H - mu) * is_
    lo, hi = j == 0, j == TOP
    one, zero = torch.ones_like(a), torch.zeros_like(a)
    up = torch.where(hi, one, torch.sigmoid(a))
    dn = torch.where(lo, zero, torch.sigmoid(b))
    diff = up - dn
    naive = torch.log(torch.clamp(diff, min=NAIVE_MIN if form == 'auto'
                                  else 1e-300))
    if form == 'naive':
        return naive
    D = 2.0 * H * is_
    mid = -softplus(-a) - softplus(b) + torch.log(-torch.expm1(-D))
    stable = torch.where(lo, -softplus(-a), torch.where(hi, -softplus(b),
                                                        mid))
    if form == 'stable':
        return stable
    return torch.where(diff > NAIVE_MIN, naive, stable)


def row_nll(logits, target, K, log_scale_min, form='auto'):
    """nll [N] (torch float64) of logits [N, >= 3 Kp] (torch) for the target
    levels [N]; the derivative through the scale clamp is 0 strictly below
    it and 1 from the clamp on (torch.maximum would halve it at the tie)."""
    Kp = (K + 3) // 4 * 4
    pi, mu = logits[:, :K], logits[:, Kp:Kp + K]
    braw = logits[:, 2 * Kp:2 * Kp + K]
    beta = torch.where(braw < float(log_scale_min),
                       torch.full_like(braw, float(log_scale_min)), braw)
    lp = log_bin(target.reshape(-1, 1), mu, beta, form)
    return -torch.logsumexp(torch.log_softmax(pi, -1) + lp, -1)


def loss_rows(logits, target, K, log_scale_min, inv=1.0):
    """(nll [N], d(sum(nll) * inv)/dlogits [N, W]) as numpy float64; target
    -1 marks a row without one: nll 0 and a zero gradient row."""
    lg = torch.tensor(np.asarray(logits, np.float64), requires_grad=True)
    t = np.asarray(target, np.int64)
    has = torch.as_tensor(t >= 0)
    nll = row_nll(lg, torch.as_tensor(np.where(t >= 0, t, 1)), K,
                  log_scale_min)
    nll = torch.where(has, nll, torch.zeros_like(nll))
    (nll.sum() * float(inv)).backward()
    return nll.detach().numpy(), lg.grad.numpy()


def params(row, K, log_scale_min):
    Kp = (K + 3) // 4 * 4
    r = np.asarray(row, np.float64)
    pi = r[:K]
    ls = pi - pi.max() - np.log(np.exp(pi - pi.max()).sum())
    return np.stack([ls, r[Kp:Kp + K],
                     np.maximum(r[2 * Kp:2 * Kp + K], log_scale_min)])


# ------------------------------------------------------------- the network
def targets(lv, lengths=None, history=None):
    """Target level of every row [B, T] (-1: none) of levels lv [B, T]."""
    B, T = lv.shape
    n = np.full(B, T) if lengths is None else np.asarray(lengths)
    h = np.zeros(B, np.int64) if history is None else \
        np.broadcast_to(np.asarray(history), (B,))
    t = np.arange(T)[None, :]
    has = (t + 1 < n[:, None]) & (t + 1 >= h[:, None])
    nxt = np.concatenate([lv[:, 1:], np.zeros((B, 1), lv.dtype)], 1)
    return np.where(has, nxt, -1)


def forward(v, dilations, x_in, lct, gc_ids, use_biases, relu_masks=None):
    """Head outputs [B, T, Q] (torch float64) of the torch tree `v` for the
    scalar input x_in [B, T]."""
    gce = None
    if gc_ids is not None:
        gce = v['embeddings']['gc_embedding'][
            torch.as_tensor(np.asarray(gc_ids), dtype=torch.int64)].unsqueeze(1)
    x = causal_conv(x_in.unsqueeze(-1), v['causal_layer']['filter'], 1)
    stack, total = v['dilated_stack'], 0
    for i, cur in enumerate(stack):
        d = int(dilations[i])
        cf = causal_conv(x, cur['filter'], d)
        cg = causal_conv(x, cur['gate'], d)
        if gce is not None:
            cf = cf + gce @ cur['gc_filtweights'][0]
            cg = cg + gce @ cur['gc_gateweights'][0]
        if lct is not None:
            cf = cf + lct @ cur['lc_filtweights']
            cg = cg + lct @ cur['lc_gateweights']
        if use_biases:
            cf = cf + cur['filter_bias']
            cg = cg + cur['gate_bias']
        out = torch.tanh(cf) * torch.sigmoid(cg)
        skip = out @ cur['skip'][0]
        if use_biases:
            skip = skip + cur['skip_bias']
        total = total + skip
        if i != len(stack) - 1:
            tr = out @ cur['dense'][0]
            if use_biases:
                tr = tr + cur['dense_bias']
            x = x + tr
    p = v['postprocessing']

    def relu(t, key):
        if relu_masks is None:
            return F.relu(t)
        return t * torch.as_tensor(relu_masks[key]).to(t.dtype)
    c1 = relu(total, 'total') @ p['postprocess1'][0]
    if use_biases:
        c1 = c1 + p['postprocess1_bias']
    raw = relu(c1, 'c1') @ p['postprocess2'][0]
    if use_biases:
        raw = raw + p['postprocess2_bias']
    return raw


def lc_rows(v, lc, B, T, scales=None, offsets=0):
    """The per-sample conditioning rows [B, T, Lc] (torch): rows as given, or
    frames through the context convolution and the learned upsampler."""
    if lc is None:
        return None
    t = torch.as_tensor(np.asarray(lc, np.float64))
    if scales is None:
        return t
    if 'lc_context' in v:
        t = lc_ctx_ref.context(t, v['lc_context']['filter'])
    up = v['lc_upsample']
    return lc_up_ref.rows(t, np.broadcast_to(np.asarray(offsets), (B,)), T,
                          scales, [c['filter'] for c in up],
                          [c['bias'] for c in up] if 'bias' in up[0] else None)


def network(var, dilations, x_in, target, den, head, lc=None, scales=None,
            gc_ids=None, use_biases=False, relu_masks=None, grads=True,
            offsets=0):
    """The float64 network on the scalar input x_in [B, T] (what the device
    network reads: the centres).  target int [B, T], -1 for a row without
    one; den: the mean's denominator; head: (K, log_scale_min); offsets: the
    timeline position of each clip's first sample (frames through `scales`).
    Returns (loss, gradient tree or None, head outputs [B, T, Q] numpy, row
    nll [B, T] numpy)."""
    v = lc_ref._to_torch(var)
    x = torch.as_tensor(np.asarray(x_in, np.float64))
    B, T = x.shape
    lct = lc_rows(v, lc, B, T, scales, offsets)
    raw = forward(v, dilations, x, lct, gc_ids, use_biases, relu_masks)
    t = np.asarray(target, np.int64).reshape(-1)
    has = torch.as_tensor(t >= 0)
    tt = torch.as_tensor(np.where(t >= 0, t, 1))
    pred = raw.reshape(B * T, -1)
    row = row_nll(pred, tt, head[0], head[1])
    row = torch.where(has, row, torch.zeros_like(row))
    loss = row.sum() / float(den)
    g = None
    if grads:
        loss.backward()
        g = lc_ref._grads(v)
    return (float(loss.detach()), g, raw.detach().numpy(),
            row.detach().numpy().reshape(B, T))
