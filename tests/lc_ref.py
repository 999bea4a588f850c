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


def loss_and_grads(var, dilations, codes, lc=None, gc_ids=None, use_biases=False,
                   quantization_channels=256, relu_masks=None,
                   tf_xent_zero_label_quirk=True):
    """var: the model's `variables` tree as numpy (model_tree); dilations:
    one per layer; codes int [B, T]; lc float
    [B, T, Lc] or None.  relu_masks: optional dict(total=, c1=) of bool
    [B, T, S] -- the device's ReLU decisions, used in place of the float64
    ones (they can differ only where a pre-activation rounds across zero).
    Returns (loss, gradient tree shaped like `var`)."""
    v = _to_torch(var)
    Q = quantization_channels
    q = torch.as_tensor(np.asarray(codes), dtype=torch.int64)
    B, T = q.shape
    enc = F.one_hot(q, Q).to(torch.float64)
    lct = None if lc is None else torch.as_tensor(np.asarray(lc, np.float64))
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
    raw = relu(c1, 'c1') @ p['postprocess2'][0]
    if use_biases:
        raw = raw + p['postprocess2_bias']
    lab = F.pad(enc[:, 1:, :], (0, 0, 0, 1)).reshape(-1, Q)
    pred = raw.reshape(-1, Q)
    lse = torch.logsumexp(pred, -1)
    row = lse - (lab * pred).sum(-1)
    if tf_xent_zero_label_quirk:
        # TF's fused softmax cross-entropy: the all-zero-label last row of a
        # clip adds 0 to the loss but its softmax to the gradient
        row = torch.where(lab.sum(-1) > 0, row, lse - lse.detach())
    loss = row.mean()
    loss.backward()
    return float(loss.detach()), _grads(v)


def model_tree(net, grads=False):
    """The model's variables (or, grads=True, its gradients) as numpy
    float64, nested like `variables`."""
    from util import tree_to_numpy
    return tree_to_numpy(net.gradients if grads else net.variables)


def device_relu_masks(net, B, T):
    """The ReLU decisions of the model's last training forward pass."""
    ws = [w for w in net._ws.values() if w.T == T and w.training][0]
    S = net.S
    return dict(total=(ws.h1 > 0).cpu().numpy().reshape(B, T, S),
                c1=(ws.h2 > 0).cpu().numpy().reshape(B, T, S))
