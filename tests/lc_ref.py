"""float64 restatement of the network WITH local conditioning (test
infrastructure only): the reference graph's layers (oracle/torch_graph.py's
causal convolutions) plus, in every layer,

    filter[b, t] += lc[b, t, :] @ lc_filtweights,  gate[b, t] += lc[b, t, :] @ lc_gateweights

next to global conditioning's 1x1 conv of the embedding.  Gradients by torch
autograd on the CPU.  Works on the nested `variables` tree of a WaveNetModel
(numpy copies), so that the model's own views name every gradient.
"""
import numpy as np
import torch
import torch.nn.functional as F

import util  # noqa: F401  (puts the repository root on sys.path)
from oracle.torch_graph import causal_conv


def _to_torch(tree):
    if isinstance(tree, dict):
        return {k: _to_torch(v) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_to_torch(v) for v in tree]
    return torch.tensor(np.asarray(tree, dtype=np.float64), requires_grad=True)


def _grads(tree):
    if isinstance(tree, dict):
        return {k: _grads(v) for k, v in tree.items()}
    if isinstance(tree, list):
        return [_grads(v) for v in tree]
    g = tree.grad
    return np.zeros(tuple(tree.shape)) if g is None else g.numpy()


def flatten(tree, prefix=''):
    """[(path, array)] in a fixed order."""
    if isinstance(tree, dict):
        out = []
        for k in sorted(tree):
            out += flatten(tree[k], prefix + '/' + k)
        return out
    if isinstance(tree, list):
        out = []
        for i, v in enumerate(tree):
            out += flatten(v, '%s/%d' % (prefix, i))
        return out
    return [(prefix, np.asarray(tree))]


def _forward(v, dilations, q, lct, gc_ids, use_biases, Q, relu_masks,
             residual_postproc):
    """Logits [B, T, Q] of the torch tree `v` (float64)."""
    enc = F.one_hot(q, Q).to(torch.float64)
    gce = None
    if gc_ids is not None:
        gce = v['embeddings']['gc_embedding'][
            torch.as_tensor(np.asarray(gc_ids), dtype=torch.int64)].unsqueeze(1)
    x = causal_conv(enc, v['causal_layer']['filter'], 1)
    stack = v['dilated_stack']
    total = 0
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
    h2 = relu(c1, 'c1')
    if residual_postproc:
        h2 = h2 + total            # (the pre-ReLU skip sum)
    raw = h2 @ p['postprocess2'][0]
    if use_biases:
        raw = raw + p['postprocess2_bias']
    return raw, enc


def _leaves(tree, name=''):
    """[(last key, tensor)] of a torch tree."""
    if isinstance(tree, dict):
        return [x for k in sorted(tree) for x in _leaves(tree[k], k)]
    if isinstance(tree, list):
        return [x for t in tree for x in _leaves(t, name)]
    return [(name, tree)]


def loss_and_grads(var, dilations, codes, lc=None, gc_ids=None, use_biases=False,
                   quantization_channels=256, relu_masks=None,
                   tf_xent_zero_label_quirk=True, residual_postproc=False,
                   l2=None, tf_bias_name_quirk=True, return_logits=False):
    """var: the model's `variables` tree as numpy (model_tree); dilations:
    one per layer; codes int [B, T]; lc float
    [B, T, Lc] or None.  relu_masks: optional dict(total=, c1=) of bool
    [B, T, S] -- the device's ReLU decisions, used in place of the float64
    ones (they can differ only where a pre-activation rounds across zero).
    residual_postproc: the pre-ReLU skip sum is added to the post-ReLU c1.
    l2: lam of the L2 term lam * sum(w^2) / 2 over every variable, or (with
    tf_bias_name_quirk False) over those whose name does not say 'bias'.
    Returns (loss, gradient tree shaped like `var`), and with return_logits
    the float64 logits [B, T, Q] as a third item."""
    v = _to_torch(var)
    Q = quantization_channels
    q = torch.as_tensor(np.asarray(codes), dtype=torch.int64)
    lct = None if lc is None else torch.as_tensor(np.asarray(lc, np.float64))
    raw, enc = _forward(v, dilations, q, lct, gc_ids, use_biases, Q,
                        relu_masks, residual_postproc)
    lab = F.pad(enc[:, 1:, :], (0, 0, 0, 1)).reshape(-1, Q)
    pred = raw.reshape(-1, Q)
    lse = torch.logsumexp(pred, -1)
    row = lse - (lab * pred).sum(-1)
    if tf_xent_zero_label_quirk:
        # TF's fused softmax cross-entropy: the all-zero-label last row of a
        # clip adds 0 to the loss but its softmax to the gradient
        row = torch.where(lab.sum(-1) > 0, row, lse - lse.detach())
    loss = row.mean()
    if l2 is not None:
        loss = loss + float(l2) * sum(
            (w * w).sum() / 2 for n, w in _leaves(v)
            if tf_bias_name_quirk or 'bias' not in n)
    loss.backward()
    out = (float(loss.detach()), _grads(v))
    if return_logits:
        out += (raw.detach().numpy(),)
    return out


def logits(var, dilations, codes, lc=None, gc_ids=None, use_biases=False,
           quantization_channels=256, residual_postproc=False):
    """The float64 logits [B, T, Q] alone (no gradients)."""
    with torch.no_grad():
        raw, _ = _forward(
            _to_torch(var), dilations,
            torch.as_tensor(np.asarray(codes), dtype=torch.int64),
            None if lc is None else torch.as_tensor(np.asarray(lc, np.float64)),
            gc_ids, use_biases, quantization_channels, None, residual_postproc)
    return raw.numpy()


def model_tree(net, grads=False):
    """The model's variables (or, grads=True, its gradients) as numpy
    float64, nested like `variables`."""
    from util import tree_to_numpy
    return tree_to_numpy(net.gradients if grads else net.variables)


def device_relu_masks(net, B, T):
    """The ReLU decisions of the model's last training forward pass."""
    ws = [w for w in net._ws.values() if w.T == T and w.training][0]
    S = net.S
    # (with residual_postproc h2 = relu(c1) + total: c1 is kept on its own)
    c1 = ws.c1 if net.residual_postproc else ws.h2
    return dict(total=(ws.h1 > 0).cpu().numpy().reshape(B, T, S),
                c1=(c1 > 0).cpu().numpy().reshape(B, T, S))
