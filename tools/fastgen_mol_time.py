"""Step time of batched fast generation for a mixture-of-logistics model:
  python tools/fastgen_mol_time.py [--steps N] [--rounds R] [--out FILE]
The default stack (wavenet_params.json) with scalar input and K = 10
components (generate_mixture_batch) beside the one-hot default stack
(generate_batch) in the same process, at B = 1, 32, 256: after a warm-up call
of each shape the two models alternate, round by round, each call timed with
device events; reported are the median us per lock-step step, the fastest and
slowest round, and the mixture / one-hot ratio.  Then the naive path
(predict_mixture + mol.sample) per sample, on a 1-sample window and on a
receptive-field window.  Nothing asserts a time; --out also writes the
report to a file (profiles/fastgen_mol_time.txt)."""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import WaveNetModel, mol  # noqa: E402
from util import model_kwargs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=2000)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--components', type=int, default=10)
ap.add_argument('--out', type=str, default=None)
args = ap.parse_args()
n, K = args.steps, args.components

p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
cfg = {k: p[k] for k in p if k != 'sample_rate'}
cfg['batch_size'] = 1
onehot = WaveNetModel(seed=0, **model_kwargs(cfg))
kw = model_kwargs(dict(cfg, scalar_input=True))
mix = WaveNetModel(seed=0, output_mixture=K, **kw)
with torch.no_grad():
    # (scales round e^-4 of full scale, so that the streams move)
    mix.variables['postprocessing']['postprocess2_bias'][
        2 * mix.mol_Kp:2 * mix.mol_Kp + K] -= 4.0

lines = []


def say(s):
    print(s)
    lines.append(s)


def once(fn):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out          # us


res = {'steps': n, 'rounds': args.rounds, 'components': K,
       'initial_filter_width': mix.initial_filter_width, 'batch': {},
       'naive': {}}
say('default stack, %d lock-step steps a call, %d alternating rounds; '
    'mixture: scalar input, initial_filter_width %d, K = %d'
    % (n, args.rounds, mix.initial_filter_width, K))
for B in (1, 32, 256):
    seeds = [2 + b for b in range(B)]
    calls = dict(
        mixture=lambda: mix.generate_mixture_batch(n, seeds),
        onehot=lambda: onehot.generate_batch(n, seeds))
    ts = {k: [] for k in calls}
    sums = {}
    for k, fn in calls.items():                   # warm-up: graphs, buffers
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k, fn in calls.items():
            us, out = once(fn)
            ts[k].append(us / n)
            sums[k] = int(out.cpu().numpy().astype(np.int64).sum())
    r = {k: dict(us_per_step=float(np.median(v)), fastest=min(v),
                 slowest=max(v), checksum=sums[k]) for k, v in ts.items()}
    r['ratio'] = r['mixture']['us_per_step'] / r['onehot']['us_per_step']
    res['batch'][B] = r
    say('B = %3d: mixture %7.2f us/step (%.2f .. %.2f)   one-hot %7.2f us/step '
        '(%.2f .. %.2f)   ratio %.3f   checksums %d %d'
        % (B, r['mixture']['us_per_step'], r['mixture']['fastest'],
           r['mixture']['slowest'], r['onehot']['us_per_step'],
           r['onehot']['fastest'], r['onehot']['slowest'], r['ratio'],
           sums['mixture'], sums['onehot']))

for name, T in (('1-sample window', 1),
                ('receptive-field window', mix.receptive_field)):
    wave = mol.centres(np.random.default_rng(0).integers(
        0, mol.LEVELS, T)).astype(np.float32)

    def naive():
        params = mix.predict_mixture(wave)
        return mol.sample(params[None], [2], [0], 1.0)[0]
    naive()
    torch.cuda.synchronize()
    v = [once(naive)[0] for _ in range(max(5, args.rounds))]
    res['naive'][T] = dict(us_per_sample=float(np.median(v)), fastest=min(v),
                           slowest=max(v))
    say('naive path, %s (%d samples): %9.1f us/sample (%.1f .. %.1f)'
        % (name, T, np.median(v), min(v), max(v)))
say(json.dumps(res))
if args.out:
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
