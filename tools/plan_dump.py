"""What a training step launches, as data: for one named configuration run
three `loss` calls (eager, recorded, replayed) and one `predict_proba`, and
write as JSON
  * every recorded launch plan of every workspace (`ws.plans`), each launch as
    [entry point, arguments]: a non-pointer argument is its value, a pointer
    argument is null or the workspace buffer (or `params` / `grads`) it points
    into and its offset, anything else 'other';
  * the launches the third `loss` call issues outside a plan (`_lib.record`
    around it: the loss kernels, and the whole backward where it is eager);
  * the three losses (repr) and the SHA-256 of the gradient bucket and of the
    probabilities.
Two trees launch the same and compute the same bits exactly when their files
are equal.  It reads public names, `net._ws`, `ws.plans` and `_lib` only.

    python tools/plan_dump.py --list
    python tools/plan_dump.py NAME --out FILE     # one process per NAME
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

# name -> (batch, samples, constructor keywords, model attributes, loss
# keywords); every StepPath value a call can take today is in here
LC = dict(local_condition_channels=20)
UP = dict(LC, local_condition_upsample_scales=(4, 5))
CONFIGS = {
    'default_b8': (8, 16000, {}, {}, {}),          # stack / stack
    'default_b4': (4, 8000, {}, {}, {}),           # side-stream TN, all splits
    'default_b1': (1, 16000, {}, {}, {}),          # stack_skip, fewer splits
    'per_layer': (2, 8000, {}, dict(stack_fwd=False, stack_bwd=False), {}),
    'generic_layers': (2, 8000, {}, dict(generic_layers=True), {}),
    'filter3': (2, 8000, dict(filter_width=3), {}, {}),
    'blocked64': (2, 8000, dict(residual_channels=64, dilation_channels=64),
                  {}, {}),
    'scalar_input': (2, 8000, dict(scalar_input=True), {}, {}),
    'onehot512': (2, 8000, dict(quantization_channels=512), {}, {}),
    'global_condition': (2, 8000, dict(global_condition_channels=16,
                                       global_condition_cardinality=4), {},
                         {}),
    'residual_postproc': (2, 8000, dict(residual_postproc=True), {}, {}),
    'no_biases': (2, 8000, dict(use_biases=False), {}, {}),
    'bf16x6': (2, 8000, {}, dict(gemm_mode='bf16x6'), {}),
    'lc_rows': (2, 8000, LC, {}, {}),
    'lc_upsample': (2, 8000, UP, {}, {}),
    'lc_context': (2, 8000, dict(UP, local_condition_context=2), {}, {}),
    'masked': (2, 8000, {}, {}, dict(lengths=[8000, 5000])),
    'l2': (2, 8000, {}, {}, dict(l2_regularization_strength=1e-3)),
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()


def buffers(net):
    """(first address, end, name) of params, grads and every tensor of every
    workspace; aliases keep the first name in sorted order."""
    out = {}
    named = [('params', net.params), ('grads', net.grads)]
    for ws in net._ws.values():
        named += sorted((k, v) for k, v in vars(ws).items()
                        if isinstance(v, torch.Tensor))
    for name, t in named:
        if t.numel():
            lo = t.data_ptr()
            out.setdefault(lo, (lo + t.numel() * t.element_size(), name))
    return sorted((lo, hi, name) for lo, (hi, name) in out.items())


def describe(plan, bufs, sigs):
    def pointer(a):
        if not a:
            return None
        for lo, hi, name in bufs:
            if lo <= a < hi:
                return '%s+%d' % (name, a - lo)
        return 'other'
    out = []
    for fn, args, name, flops in plan:
        if name == 'py':                 # a stream fork / join
            out.append(['py', []])
            continue
        types = sigs[name][1]
        out.append([name, [pointer(a) if t is ctypes.c_void_p else a
                           for a, t in zip(args, types)]])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('name', nargs='?')
    ap.add_argument('--list', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    if a.list or a.name is None:
        print(' '.join(CONFIGS))
        return 0
    from wavenet import WaveNetModel, _lib
    B, T, ctor, attrs, call = CONFIGS[a.name]
    p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    kw = {k: v for k, v in p.items() if k != 'sample_rate'}
    kw.update(ctor)
    net = WaveNetModel(batch_size=B, seed=0, **kw)
    for k, v in attrs.items():
        setattr(net, k, v)
    rng = np.random.default_rng(7)
    audio = rng.uniform(-0.9, 0.9, (B, T)).astype(np.float32)
    Tp = 2000
    codes = rng.integers(0, net.quantization_channels, (B, Tp))
    ids = [b % 4 for b in range(B)] if net.global_condition_channels else None
    call, proba = dict(call), {}
    if net.local_condition_channels:
        Lc = net.local_condition_channels
        hop = 20 if net.local_condition_upsample_scales else 1
        call['local_condition_batch'] = rng.standard_normal(
            (B, (T + hop - 1) // hop, Lc)).astype(np.float32)
        proba['local_condition'] = rng.standard_normal(
            (B, Tp, Lc)).astype(np.float32)
    losses = []
    for i in range(3):
        if i < 2:
            loss = net.loss(audio, ids, **call)
        else:
            with _lib.record() as rec:
                loss = net.loss(audio, ids, **call)
        losses.append(repr(float(loss)))
    grads = sha(net.grads)
    pr = net.predict_proba(codes, ids, **proba)
    torch.cuda.synchronize()
    bufs = buffers(net)
    plans = {}
    for (b, t, training), ws in sorted(net._ws.items()):
        for key, plan in ws.plans.items():
            tag, path, has_ids = key[0], list(key[1]), key[2]
            plans[json.dumps([b, t, training, tag, path, has_ids])] = \
                None if not plan else describe(plan, bufs, _lib.SIGNATURES)
    out = dict(name=a.name, losses=losses, grads_sha256=grads,
               proba_sha256=sha(pr), plans=plans,
               third_call=describe(rec.plan, bufs, _lib.SIGNATURES))
    text = json.dumps(out, indent=0, sort_keys=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    print('%s: losses %s grads %s proba %s, %d plans, %d launches' % (
        a.name, ' '.join(losses), grads[:16], out['proba_sha256'][:16],
        len(plans), sum(len(v or []) for v in plans.values())))
    return 0


if __name__ == '__main__':
    sys.exit(main())
