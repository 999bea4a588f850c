"""Step time of two checkouts of this repository against each other, for a
change that must not move it (same library build: WN_LIB_PATH).

Measuring (no --trees): the default model (wavenet_params.json) at --batch x
--samples in the tree this file sits in; prints one JSON line with the time
per training step (loss + Adam update, launch plans replayed) and the host
time to ISSUE one eager step (use_launch_plans = False, no device sync: what
tools/host_overhead.py prints as `launch plans False`).

Comparing (--trees A B): runs itself in tree A and tree B alternately, one
fresh process per measurement, --rounds rounds for each shape of --shapes,
so that clock and thermal drift hit both alike; stops at the first process
that fails.  Writes one JSON object: per shape and tree the rounds, their
median, A's spread (max - min) and whether B's median lies between A's
fastest and slowest round.

    python tools/step_time_ab.py --trees ../parent . --out FILE
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(a):
    sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
    import numpy as np
    import torch
    from wavenet import WaveNetModel, optimizer_factory
    p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    kw = {k: v for k, v in p.items() if k != 'sample_rate'}
    net = WaveNetModel(batch_size=a.batch, seed=0, **kw)
    opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
    audio = torch.from_numpy(np.random.default_rng(0).uniform(
        -0.9, 0.9, (a.batch, a.samples)).astype(np.float32)).cuda()

    def run(n):
        t0 = time.perf_counter()
        for _ in range(n):
            opt.minimize(net.loss(audio))
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) / n * 1e3, (time.perf_counter() - t0) / n * 1e3

    run(a.warmup)
    step = run(a.steps)[1]
    net.use_launch_plans = False
    run(a.warmup)
    issue = run(a.steps)[0]
    print(json.dumps(dict(step_ms=round(step, 4),
                          eager_issue_ms=round(issue, 4),
                          device=torch.cuda.get_device_name(0))))
    return 0


def compare(a):
    shapes = [tuple(int(x) for x in s.split('x')) for s in a.shapes.split(',')]
    out = dict(trees=a.trees, steps=a.steps, warmup=a.warmup,
               rounds=a.rounds, shapes={})
    for B, T in shapes:
        ms = [dict(step_ms=[], eager_issue_ms=[]) for _ in a.trees]
        for _ in range(a.rounds):
            for i, tree in enumerate(a.trees):
                r = subprocess.run(
                    [sys.executable, os.path.join(tree, 'tools',
                                                  os.path.basename(__file__)),
                     '--batch', str(B), '--samples', str(T), '--steps',
                     str(a.steps), '--warmup', str(a.warmup)],
                    stdout=subprocess.PIPE, timeout=a.timeout)
                if r.returncode != 0:
                    print('%s failed at %d x %d: exit %d'
                          % (tree, B, T, r.returncode))
                    return 1
                got = json.loads(r.stdout.decode().strip().splitlines()[-1])
                out['device'] = got.pop('device')
                for k, v in got.items():
                    ms[i][k].append(v)
                print(B, T, tree, got, flush=True)
        res = {}
        for k in ('step_ms', 'eager_issue_ms'):
            med = [statistics.median(m[k]) for m in ms]
            res[k] = dict(
                a_rounds=ms[0][k], b_rounds=ms[1][k],
                a_median=round(med[0], 4), b_median=round(med[1], 4),
                a_spread=round(max(ms[0][k]) - min(ms[0][k]), 4),
                b_median_within_a_rounds=bool(
                    min(ms[0][k]) <= med[1] <= max(ms[0][k])))
        out['shapes']['%dx%d' % (B, T)] = res
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--trees', nargs=2, default=None, metavar=('A', 'B'))
    ap.add_argument('--shapes', default='8x16000,1x16000')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--timeout', type=int, default=120)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    return measure(a) if a.trees is None else compare(a)


if __name__ == '__main__':
    sys.exit(main())
