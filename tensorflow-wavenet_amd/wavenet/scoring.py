"""Scoring of held-out data, host side: the forward pass predict_proba makes,
then wn_xent_score on its logits (csrc/wn_loss.hip).  Functions take the model
first; WaveNetModel.score / score_from_codes call in here."""
import collections

import torch

from . import _lib
from . import local_condition as lcond
from . import mol
from . import train_pass

# nll float64 [B], count int32 [B], correct int32 [B] (device tensors, one
# entry per clip), per_sample float32 [B, T] or None.  correct is None for a
# mixture-of-logistics model: an arg-max is not defined for that head
Score = collections.namedtuple('Score', 'nll count correct per_sample')


def score(net, q, global_condition_batch, audio, lc, mask, per_sample,
          hist=None, q_in=None):
    """Score codes q [B, T] (any B >= 1) with the LC input checked
    (local_condition.check), the lengths (model.check_lengths) and the
    history (model.check_history).  q_in: the codes the network reads
    instead (q stays the target), or None.  Nothing here waits for the
    device."""
    B, T = q.shape
    ws = net._workspace(B, T, False)
    if net.mol_K:
        # (WaveNetModel.score quantised into ws.q and ws.audio: mol.stage)
        return _score_mixture(net, ws, global_condition_batch, lc, mask,
                              per_sample, hist)
    q_lab = train_pass.stage_codes(ws, q, q_in)
    if net.scalar_input:
        if audio is None:
            raise ValueError('scalar_input needs the float audio')
        ws.audio.copy_(audio.reshape(-1))
    ids = net._gc_ids(global_condition_batch, B)
    lcond.fill(net, lc, ws)
    train_pass.run_pass(net, 'fwd', ws, ids,
                        train_pass.step_path(net, ws, False))
    dev = net.device
    nll = torch.empty(B, dtype=torch.float64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    correct = torch.empty(B, dtype=torch.int32, device=dev)
    rows = torch.empty((B, T), dtype=torch.float32, device=dev) \
        if per_sample else None
    if getattr(ws, 'score_scratch', None) is None:
        ws.score_scratch = torch.empty(
            int(_lib.load().wn_xent_score_scratch_floats(B * T)),
            dtype=torch.float32, device=dev)
    lengths = None
    if mask is not None:
        # staged in the workspace like the masked loss's: the kernels read
        # them from device memory
        lengths = ws.xent_mask[:B]
        lengths.copy_(torch.from_numpy(mask[0]))
    if hist is None:
        _lib.call('wn_xent_score', _lib.ptr(ws.logits), net.Q,
                  _lib.ptr(q_lab), _lib.ptr(lengths), _lib.ptr(rows),
                  _lib.ptr(nll), _lib.ptr(count), _lib.ptr(correct),
                  _lib.ptr(ws.score_scratch), B, T, net.Q, _lib.stream())
    else:
        ws.xent_hist.copy_(torch.from_numpy(hist))
        _lib.call('wn_xent_score_window', _lib.ptr(ws.logits), net.Q,
                  _lib.ptr(q_lab), _lib.ptr(ws.xent_hist), _lib.ptr(lengths),
                  _lib.ptr(rows), _lib.ptr(nll), _lib.ptr(count),
                  _lib.ptr(correct), _lib.ptr(ws.score_scratch), B, T, net.Q,
                  _lib.stream())
    # 0, or NaN when a dependency wait of the forward stack launch expired
    # (as predict_proba): a wrong score is never returned silently
    return Score(nll + ws.loss_parts[0], count, correct, rows)


def _score_mixture(net, ws, global_condition_batch, lc, mask, per_sample,
                   hist):
    """score for a model built with output_mixture: the same pass, then
    wn_mol_score on the levels in ws.q (csrc/wn_mol.hip)."""
    B, T, dev = ws.B, ws.T, net.device
    ids = net._gc_ids(global_condition_batch, B)
    lcond.fill(net, lc, ws)
    train_pass.run_pass(net, 'fwd', ws, ids,
                        train_pass.step_path(net, ws, False))
    nll = torch.empty(B, dtype=torch.float64, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    rows = torch.empty((B, T), dtype=torch.float32, device=dev) \
        if per_sample else None
    lengths = None
    if mask is not None:
        lengths = ws.xent_mask[:B]
        lengths.copy_(torch.from_numpy(mask[0]))
    if hist is not None:
        ws.xent_hist.copy_(torch.from_numpy(hist))
    mol.score(net, ws, lengths, None if hist is None else ws.xent_hist, rows,
              nll, count)
    return Score(nll + ws.loss_parts[0], count, None, rows)
