"""Cost of local conditioning: the training step of the default model
(wavenet_params.json, batch 8 x 16000 samples) with Lc = 80 local-conditioning
channels against the same model without LC, in one process.

Both models take the same random audio; each timed round runs `--steps`
steps (loss + Adam update) of one model after `--warmup` untimed ones, and
the rounds alternate A / B / A / B ... so that clock and thermal drift hit
both alike.  Prints one JSON line: per-step medians over the rounds, the
difference, and the LC model's variant word (it always takes the 32-row stack
launches).

    python tools/lc_step_time.py [--lc 80] [--steps 20] [--rounds 5] [--out FILE]
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


def build(params, B, lc):
    from wavenet import WaveNetModel
    return WaveNetModel(
        batch_size=B, dilations=params['dilations'],
        filter_width=params['filter_width'],
        residual_channels=params['residual_channels'],
        dilation_channels=params['dilation_channels'],
        skip_channels=params['skip_channels'],
        quantization_channels=params['quantization_channels'],
        use_biases=params['use_biases'], scalar_input=params['scalar_input'],
        initial_filter_width=params['initial_filter_width'],
        local_condition_channels=lc)


def timed(net, opt, audio, lc, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = net.loss(audio, local_condition_batch=lc)
        opt.minimize(loss)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--lc', type=int, default=80)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from wavenet import optimizer_factory
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    B, T = a.batch, a.samples
    rng = np.random.default_rng(0)
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T)).astype(
        np.float32)).cuda()
    feats = torch.from_numpy(rng.standard_normal((B, T, a.lc)).astype(
        np.float32)).cuda()
    runs = {}
    for name, lc in (('plain', None), ('lc', a.lc)):
        net = build(params, B, lc)
        opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
        x = feats if lc else None
        timed(net, opt, audio, x, a.warmup)
        runs[name] = (net, opt, x, [])
    for _ in range(a.rounds):
        for name in ('plain', 'lc'):
            net, opt, x, ms = runs[name]
            ms.append(timed(net, opt, audio, x, a.steps))
    med = {k: statistics.median(v[3]) for k, v in runs.items()}
    ws = [w for w in runs['lc'][0]._ws.values() if w.training][0]
    out = dict(config='wavenet_params.json', batch=B, samples=T, lc=a.lc,
               steps=a.steps, rounds=a.rounds,
               plain_ms=round(med['plain'], 3), lc_ms=round(med['lc'], 3),
               extra_ms=round(med['lc'] - med['plain'], 3),
               extra_pct=round(100 * (med['lc'] / med['plain'] - 1), 1),
               plain_rounds_ms=[round(v, 3) for v in runs['plain'][3]],
               lc_rounds_ms=[round(v, 3) for v in runs['lc'][3]],
               lc_stack_variant=ws.stack_variant,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
