"""What piece history costs, timed: the training step of the default model
(wavenet_params.json, batch 8 x 16000 samples, net.loss + minimize) fed from a
DeviceCorpus two ways in one process --

    history 0   the pieces as cut (train.py without --piece_history): the
                launches of tools/corpus_step_time.py's `corpus` arm
    history rf  every piece behind up to net.receptive_field samples of its
                left context (train.py --piece_history rf): T = 16000 + rf,
                the loss with lengths and history

The tool writes tools/corpus_step_time.py's wav tree to a temporary directory
first.  Each timed round runs `--steps` steps of one arm after `--warmup`
untimed ones of every arm, and the rounds alternate 0 / rf / 0 ... so that
clock and thermal drift hit both arms alike.  Prints one JSON line -- per-step
medians over the rounds, each arm's rounds and their spread, the predicted
(target) samples per step and per second -- and, with --out, writes it there
behind two plain lines (and a third with --baseline FILE, the JSON line of
tools/corpus_step_time.py run on the same box: its `corpus` arm against the
`history 0` arm).

    python tools/history_step_time.py [--steps 20] [--rounds 5]
        [--baseline FILE] [--out profiles/history_step_time.txt]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--speakers', type=int, default=8)
    ap.add_argument('--clips', type=int, default=8)
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--baseline', default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from clip_step_time import build
    from corpus_step_time import SILENCE_THRESHOLD, write_tree
    from wavenet import optimizer_factory
    from wavenet.corpus import DeviceCorpus
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    rate, B, size = params['sample_rate'], a.batch, a.samples
    tree = tempfile.mkdtemp(prefix='history_step_time_')
    try:
        write_tree(tree, a.speakers, a.clips, a.seconds, rate, a.seed)
        net = build(params, B)
        rf = net.receptive_field
        opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
        arms = []
        for name, H in (('history_0', 0), ('history_rf', rf)):
            corpus = DeviceCorpus(tree, rate, False, sample_size=size,
                                  silence_threshold=SILENCE_THRESHOLD,
                                  history=H)
            arms.append(dict(name=name, corpus=corpus, T=size + H, step=0,
                             targets=[], ms=[]))

        def one_step(arm):
            arm['step'] += 1
            # (T given: the shape stays [B, T] whatever the pieces' lengths)
            b = arm['corpus'].batch(arm['step'], B, T=arm['T'])
            if arm['corpus'].index.history:
                # (as train.py --piece_history: lengths and history)
                loss = net.loss(b.audio, lengths=b.lengths, history=b.history)
                arm['targets'].append(int((b.lengths - b.history).sum()))
            else:
                loss = net.loss(b.audio)
                arm['targets'].append(int(b.lengths.sum()))
            opt.minimize(loss)

        def timed(arm, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one_step(arm)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        for arm in arms:
            timed(arm, a.warmup)
            arm['targets'] = []
        for _ in range(a.rounds):
            for arm in arms:
                arm['ms'].append(timed(arm, a.steps))
        out = dict(config='wavenet_params.json', batch=B, samples=size,
                   receptive_field=rf, steps=a.steps, rounds=a.rounds,
                   device=torch.cuda.get_device_name(0))
        for arm in arms:
            k, ms = arm['name'], statistics.median(arm['ms'])
            per_step = float(np.mean(arm['targets']))
            out[k + '_T'] = arm['T']
            out[k + '_ms'] = round(ms, 3)
            out[k + '_rounds_ms'] = [round(v, 3) for v in arm['ms']]
            out[k + '_spread_ms'] = round(max(arm['ms']) - min(arm['ms']), 3)
            out[k + '_targets_per_step'] = round(per_step, 1)
            out[k + '_targets_per_s'] = round(per_step / ms * 1e3)
        out['rf_over_0_ms'] = round(out['history_rf_ms'] / out['history_0_ms'],
                                    3)
        out['rf_over_0_T'] = round((size + rf) / float(size), 3)
    finally:
        shutil.rmtree(tree, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    lines = [
        'history 0:  %.3f ms/step (rounds spread %.3f ms), T = %d, '
        '%d target samples/s' % (out['history_0_ms'],
                                 out['history_0_spread_ms'], out['history_0_T'],
                                 out['history_0_targets_per_s']),
        'history rf: %.3f ms/step (rounds spread %.3f ms), T = %d, '
        '%d target samples/s; %.3f x the history 0 step, beside T\'s ratio '
        '%.3f' % (out['history_rf_ms'], out['history_rf_spread_ms'],
                  out['history_rf_T'], out['history_rf_targets_per_s'],
                  out['rf_over_0_ms'], out['rf_over_0_T'])]
    if a.baseline:
        base = json.loads(open(a.baseline).read().strip().splitlines()[-1])
        lines.append(
            'tools/corpus_step_time.py on the same box, corpus arm: %.3f '
            'ms/step (rounds spread %.3f ms); history 0 minus it: %+.3f ms'
            % (base['corpus_ms'], base['corpus_spread_ms'],
               out['history_0_ms'] - base['corpus_ms']))
    for text in lines:
        print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n' + line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
