"""Where the training batches come from, timed: the training step of the
default model (wavenet_params.json, batch 8 x 16000 samples, net.loss +
minimize) fed three ways in one process --

    resident  one synthetic batch that stays on the device (bench.py's step)
    reader    AudioReader on a wav tree: its thread, dequeue's numpy padding
              and the training loop's copy on a side stream
              (wavenet/training.py, StageIn)
    corpus    DeviceCorpus.batch: the batch cut on the device by the kernel

The tool writes a VCTK-shaped tree of 16 kHz wavs (p<id>/p<id>_<n>.wav, a few
hundred pieces of 16000 samples) to a temporary directory first.  Each timed
round runs `--steps` steps of one arm after `--warmup` untimed ones of every
arm, and the rounds go resident / reader / corpus / resident ... so that
clock and thermal drift hit all arms alike.  The gather launch alone is timed
between device events (one pair per launch, nothing else on the stream), and
batch()'s host time per call without waiting for the device.
Prints one JSON line: per-step medians over the rounds, each arm's rounds and
their spread (the noise differences have to be read against), the gather's
microseconds per launch and its bytes per second (read + written).

    python tools/corpus_step_time.py [--steps 20] [--rounds 5] [--out FILE]
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

SILENCE_THRESHOLD = 0.3        # train.py's


def write_tree(root, speakers, clips, seconds, rate, seed):
    """speakers x clips wavs of about `seconds` each: a loud tone plus noise
    (the trimming keeps nearly all of it)."""
    from scipy.io import wavfile
    rng = np.random.default_rng(seed)
    for s in range(speakers):
        d = os.path.join(root, 'p%d' % (225 + s))
        os.makedirs(d)
        for c in range(clips):
            n = int(rate * seconds * rng.uniform(0.8, 1.2))
            f = 110.0 * 2 ** (rng.integers(0, 36) / 12.0)
            x = 0.6 * np.sin(2 * np.pi * f * np.arange(n) / rate) + \
                0.05 * rng.standard_normal(n)
            wavfile.write(os.path.join(d, 'p%d_%03d.wav' % (225 + s, c + 1)),
                          rate, (np.clip(x, -1, 1) * 32767).astype(np.int16))


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
    ap.add_argument('--gather_launches', type=int, default=200)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    from clip_step_time import build
    from wavenet import AudioReader, optimizer_factory
    from wavenet.audio_reader import Coordinator
    from wavenet.corpus import DeviceCorpus
    from wavenet.training import StageIn
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    rate, B, T = params['sample_rate'], a.batch, a.samples
    tree = tempfile.mkdtemp(prefix='corpus_step_time_')
    coord = Coordinator()
    threads = []
    try:
        write_tree(tree, a.speakers, a.clips, a.seconds, rate, a.seed)
        net = build(params, B)
        opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)
        rng = np.random.default_rng(a.seed)
        resident = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T)).astype(
            np.float32)).cuda()
        t0 = time.perf_counter()
        corpus = DeviceCorpus(tree, rate, False, sample_size=T,
                              silence_threshold=SILENCE_THRESHOLD)
        torch.cuda.synchronize()
        load_s = time.perf_counter() - t0
        reader = AudioReader(tree, coord, sample_rate=rate, gc_enabled=False,
                             sample_size=T,
                             silence_threshold=SILENCE_THRESHOLD, seed=0)
        threads = reader.start_threads()
        stage_in = StageIn(net.device)

        def from_reader():
            while True:             # (eight short last pieces: next batch)
                host = reader.dequeue(B)
                if host.shape[1] == T:
                    return stage_in(host.reshape(B, -1))

        step = [0]

        def from_corpus():
            step[0] += 1
            # (T given: the shape stays [B, T] whatever the pieces' lengths)
            return corpus.batch(step[0], B, T=T).audio

        arms = (('resident', lambda: resident), ('reader', from_reader),
                ('corpus', from_corpus))

        def timed(batch, steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                opt.minimize(net.loss(batch()))
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3

        for _, fn in arms:
            timed(fn, a.warmup)
        ms = {k: [] for k, _ in arms}
        for _ in range(a.rounds):
            for k, fn in arms:
                ms[k].append(timed(fn, a.steps))
        # the gather alone: one launch between two events on an idle stream
        # (its plan arguments prepared before), and batch()'s host time
        us, out_buf = [], torch.empty((B, T), dtype=torch.float32,
                                      device=net.device)
        for k in range(a.gather_launches):
            args = corpus.plan_args(k, B)
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            corpus.gather(k, B, out_buf, args)
            e.record()
            e.synchronize()
            us.append(s.elapsed_time(e) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.gather_launches):
            from_corpus()
        host_us = (time.perf_counter() - t0) / a.gather_launches * 1e6
        torch.cuda.synchronize()
        gather_us = statistics.median(us)
        moved = 2 * 4 * B * T
        out = dict(config='wavenet_params.json', batch=B, samples=T,
                   steps=a.steps, rounds=a.rounds,
                   files=a.speakers * a.clips, pieces=len(corpus.items),
                   corpus_samples=int(corpus.flat.numel()),
                   corpus_load_s=round(load_s, 3),
                   device=torch.cuda.get_device_name(0))
        for k, _ in arms:
            out[k + '_ms'] = round(statistics.median(ms[k]), 3)
            out[k + '_rounds_ms'] = [round(v, 3) for v in ms[k]]
            out[k + '_spread_ms'] = round(max(ms[k]) - min(ms[k]), 3)
        for k in ('reader', 'corpus'):
            out[k + '_minus_resident_ms'] = round(
                out[k + '_ms'] - out['resident_ms'], 3)
        out.update(batch_host_us=round(host_us, 1),
                   gather_us=round(gather_us, 2),
                   gather_min_us=round(min(us), 2),
                   gather_bytes=moved,
                   gather_gb_per_s=round(moved / gather_us * 1e-3, 2))
    finally:
        coord.request_stop()
        coord.join(threads)
        shutil.rmtree(tree, ignore_errors=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
