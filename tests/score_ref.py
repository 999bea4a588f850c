"""float64 reference of WaveNetModel.score / wn_xent_score (test
infrastructure only).  Two parts:

  * rows / clips: from given logits, per-row negative log-likelihood, whether
    a row has a target, whether its arg-max hits the target, the top-two
    margin; per-clip sums (math.fsum), counts and hits -- numpy float64;
  * model_logits: the model's float64 logits from tests/lc_ref.py's network on
    lc_ref.model_tree(net) (no ReLU masks: the forward pass is continuous),
    behind tests/lc_ctx_ref.py's context + upsampler for frames, or from the
    project's float64 oracle for scalar input.
"""
import math

import numpy as np

import lc_ctx_ref
import lc_ref
import lc_up_ref


def rows(logits, codes, lengths, Q):
    """logits [B, T, >= Q] (columns >= Q ignored), codes int [B, T], lengths
    B ints or None.  Returns dict(nll float64 [B, T] (0 without target),
    has bool [B, T], hit bool [B, T], margin float64 [B, T] (top-two gap of
    the row, NaN where the row holds a NaN))."""
    x = np.asarray(logits)[..., :Q].astype(np.float64)
    codes = np.asarray(codes).astype(np.int64)
    B, T = codes.shape
    n = np.full(B, T) if lengths is None else \
        np.clip(np.asarray(lengths).astype(np.int64), 0, T)
    tgt = np.concatenate([codes[:, 1:], np.full((B, 1), -1)], 1)
    t = np.arange(T)[None, :]
    has = (t + 1 < n[:, None]) & (tgt >= 0) & (tgt < Q)
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.nanmax(np.where(np.isnan(x), -np.inf, x), -1, keepdims=True)
        lse = (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))[..., 0]
    own = np.take_along_axis(x, np.clip(tgt, 0, Q - 1)[..., None], -1)[..., 0]
    nll = np.where(has, lse - own, 0.0)
    bad = np.isnan(x).any(-1)
    hit = has & (np.argmax(x, -1) == tgt) & ~bad     # (lowest index on ties)
    top = np.sort(x, -1)
    return dict(nll=nll, has=has, hit=hit, margin=top[..., -1] - top[..., -2])


def clips(r):
    """(nll float64 [B] by math.fsum, count int [B], correct int [B]) of
    rows()'s result."""
    nll = np.array([math.fsum(row) if not np.isnan(row).any() else np.nan
                    for row in r['nll']])
    return nll, r['has'].sum(1), r['hit'].sum(1)


def model_logits(net, dilations, codes, lc=None, gc_ids=None, frames=None,
                 offsets=None, scales=None):
    """float64 logits [B, T, Q] of a one-hot-input model: lc rows [B, T, Lc],
    or frames [B, F, Lc] at offsets [B] through the model's (context and)
    upsampler."""
    var = lc_ref.model_tree(net)
    codes = np.asarray(codes)
    if frames is not None:
        B, T = codes.shape
        off = np.broadcast_to(np.asarray(offsets), (B,))
        if 'lc_context' in var:
            lc = lc_ctx_ref.rows_np(frames, off, T, scales, var)
        else:
            lc = lc_up_ref.rows_np(frames, off, T, scales, var['lc_upsample'])
    return lc_ref.logits(var, dilations, codes, lc, gc_ids=gc_ids,
                         use_biases=net.use_biases,
                         quantization_channels=net.Q)


def oracle_logits(cfg, var, audio, gc_ids=None):
    """float64 logits of the project's oracle (scalar input, any model it
    states): cfg needs 'batch_size' = audio's rows."""
    from util import O
    _, cache = O.loss(cfg, var, audio, gc_ids, None, np.float64, keep=True)
    return np.asarray(cache['logits'], np.float64)
