"""Cost of the frame-context convolution in front of the learned
local-conditioning upsampler: the training step of the default model
(wavenet_params.json, batch 8 x 16000 samples, Lc = 80, scales 4,5,10 = hop
200, per-clip offsets) with context P = 2 against the same model without
context, in one process.

Four models, timed in interleaved rounds (each round runs `--steps` steps,
loss + Adam update, of one model after `--warmup` untimed ones), so that
clock and thermal drift hit all alike:
  up_dev    frames [B, F, Lc] + offsets already on the device, no context
  ctx_dev   the same with the context convolution
  up_host   the same frames handed over from host memory every step
  ctx_host  the same with the context convolution
The host pair is what train.py does: its reader yields host arrays.  Prints
one JSON line of per-step medians.

    python tools/lc_context_step_time.py [--context 2] [--steps 20]
        [--rounds 5] [--models ctx_dev] [--out FILE]

(--models: a comma-separated subset, e.g. for one model under rocprofv3.)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(net, opt, audio, frames, off, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = net.loss(audio, local_condition_batch=frames,
                        local_condition_offset=off)
        opt.minimize(loss)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lc', type=int, default=80)
    ap.add_argument('--scales', default='4,5,10')
    ap.add_argument('--context', type=int, default=2)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--models', default='up_dev,ctx_dev,up_host,ctx_host')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import WaveNetModel, optimizer_factory
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    scales = tuple(int(s) for s in a.scales.split(','))
    hop = int(np.prod(scales))
    B, T = a.batch, a.samples
    rng = np.random.default_rng(0)
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T)).astype(
        np.float32)).cuda()
    offs = rng.integers(0, 4 * hop, B)
    F = (int(offs.max()) + T - 1) // hop + 1
    frames = rng.standard_normal((B, F, a.lc)).astype(np.float32)
    inputs = {'up_dev': (torch.from_numpy(frames).cuda(), None),
              'ctx_dev': (torch.from_numpy(frames).cuda(), a.context),
              'up_host': (frames, None),
              'ctx_host': (frames, a.context)}
    inputs = {k: inputs[k] for k in a.models.split(',')}
    runs = {}
    for name, (x, p) in inputs.items():
        net = WaveNetModel(
            batch_size=B, dilations=params['dilations'],
            filter_width=params['filter_width'],
            residual_channels=params['residual_channels'],
            dilation_channels=params['dilation_channels'],
            skip_channels=params['skip_channels'],
            quantization_channels=params['quantization_channels'],
            use_biases=params['use_biases'],
            scalar_input=params['scalar_input'],
            initial_filter_width=params['initial_filter_width'],
            local_condition_channels=a.lc,
            local_condition_upsample_scales=scales,
            local_condition_context=p)
        opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
        timed(net, opt, audio, x, offs, a.warmup)
        runs[name] = (net, opt, x, [])
    for _ in range(a.rounds):
        for name in inputs:
            net, opt, x, ms = runs[name]
            ms.append(timed(net, opt, audio, x, offs, a.steps))
    med = {k: statistics.median(v[3]) for k, v in runs.items()}
    out = dict(config='wavenet_params.json', batch=B, samples=T, lc=a.lc,
               scales=list(scales), hop=hop, context=a.context,
               steps=a.steps, rounds=a.rounds)
    for k in inputs:
        out[k + '_ms'] = round(med[k], 3)
    for kind in ('dev', 'host'):
        if 'up_' + kind in med and 'ctx_' + kind in med:
            u, c = med['up_' + kind], med['ctx_' + kind]
            out['ctx_vs_up_%s_pct' % kind] = round(100 * (c / u - 1), 1)
    out['rounds_ms'] = {k: [round(v, 3) for v in runs[k][3]] for k in inputs}
    out['device'] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
