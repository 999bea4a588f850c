"""Cost of the mixture-of-logistics head, two comparisons in one process:

  loss  wn_mol_loss (K = 10, 36 columns) beside wn_xent (Q = 256), each with
        its gradient written in place, on --batch x --samples rows of random
        logits (levels cycling through the edges and the interior);
  step  the training step (loss + Adam update) of the default model of
        wavenet_params.json with scalar_input switched on, once with the
        softmax head and once with output_mixture = 10.

Both are timed with device events.  A round times `--steps` repetitions of one
kind after `--warmup` untimed ones of both; the rounds alternate softmax /
mixture / softmax ... so that clock and thermal drift hit both alike.  Prints
one JSON line: per-repetition medians over the rounds, every round, and the
spread of each kind's rounds (the noise a difference has to be read against).

    python tools/mol_step_time.py [--steps 20] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

K = 10


def events_ms(fn, reps):
    """Milliseconds per call of fn over `reps` calls, by device events."""
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(kinds, warmup, rounds, steps):
    """{name: [ms per repetition of every round]} of the (name, fn) pairs."""
    for _, fn in kinds:
        events_ms(fn, warmup)
    ms = {k: [] for k, _ in kinds}
    for _ in range(rounds):
        for k, fn in kinds:
            ms[k].append(events_ms(fn, steps))
    return ms


def report(ms, unit=1.0, digits=3):
    out = {}
    for k, v in ms.items():
        out[k] = dict(median=round(statistics.median(v) * unit, digits),
                      rounds=[round(x * unit, digits) for x in v],
                      spread=round((max(v) - min(v)) * unit, digits))
    return out


def loss_kinds(B, T, seed):
    from wavenet import _lib, mol
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    N, Kp = B * T, mol.padded(K)
    st = torch.cuda.current_stream().cuda_stream
    parts = torch.empty(lib.wn_xent_partials(N), device='cuda')
    # softmax: logits [N, 256], codes
    x_logits = torch.from_numpy(
        rng.normal(0, 2, (N, 256)).astype(np.float32)).cuda()
    x_work = torch.empty_like(x_logits)
    codes = torch.from_numpy(rng.integers(0, 256, N).astype(np.int32)).cuda()
    # mixture: [pi | mu | beta_raw], means near the targets, scales e^-9 .. e^-3
    lv = rng.integers(0, 65536, N)
    lv[::97], lv[1::97] = 0, 65535
    c = mol.centres(np.roll(lv, -1)).astype(np.float64)[:, None]
    beta = rng.uniform(-9, -3, (N, K))
    m = np.zeros((N, 3 * Kp), np.float32)
    m[:, :K] = rng.normal(0, 2, (N, K))
    m[:, Kp:Kp + K] = c + rng.normal(0, 2, (N, K)) * np.exp(beta)
    m[:, 2 * Kp:2 * Kp + K] = beta
    m_logits = torch.from_numpy(m).cuda()
    m_work = torch.empty_like(m_logits)
    levels = torch.from_numpy(lv.astype(np.int32)).cuda()

    def xent():
        x_work.copy_(x_logits)
        _lib.call('wn_xent', x_work.data_ptr(), 256, codes.data_ptr(),
                  x_work.data_ptr(), parts.data_ptr(), B, T, 256, 1, st)

    def mixture():
        m_work.copy_(m_logits)
        _lib.call('wn_mol_loss', m_work.data_ptr(), 3 * Kp, levels.data_ptr(),
                  None, None, None, m_work.data_ptr(), parts.data_ptr(), B, T,
                  K, -14.0, st)

    def xent_copy():
        x_work.copy_(x_logits)

    def mixture_copy():
        m_work.copy_(m_logits)
    # (the logits are rewritten before every call: in place, the second call
    # would read gradients; the copies alone are timed beside them)
    return (('xent', xent), ('mixture', mixture), ('xent_copy', xent_copy),
            ('mixture_copy', mixture_copy))


def step_kinds(params, B, T, seed):
    from wavenet import WaveNetModel, optimizer_factory
    rng = np.random.default_rng(seed)
    audio = torch.from_numpy(rng.uniform(-0.9, 0.9, (B, T)).astype(
        np.float32)).cuda()
    kinds = []
    for name, kw in (('softmax', {}), ('mixture', dict(output_mixture=K))):
        net = WaveNetModel(
            batch_size=B, dilations=params['dilations'],
            filter_width=params['filter_width'],
            residual_channels=params['residual_channels'],
            dilation_channels=params['dilation_channels'],
            skip_channels=params['skip_channels'],
            quantization_channels=params['quantization_channels'],
            use_biases=params['use_biases'], scalar_input=True,
            initial_filter_width=params['initial_filter_width'], **kw)
        opt = optimizer_factory['adam'](learning_rate=1e-4, momentum=0.9)

        def step(net=net, opt=opt):
            opt.minimize(net.loss(audio))
        kinds.append((name, step))
    return tuple(kinds)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--samples', type=int, default=16000)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    params = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    B, T = a.batch, a.samples
    loss = report(alternate(loss_kinds(B, T, a.seed), a.warmup, a.rounds,
                            a.steps), unit=1e3, digits=1)
    step = report(alternate(step_kinds(params, B, T, a.seed), a.warmup,
                            a.rounds, a.steps))
    out = dict(batch=B, samples=T, components=K, steps=a.steps,
               rounds=a.rounds, loss_launch_us=loss, step_ms=step,
               note='loss_launch_us: xent / mixture include the copy that '
                    'restores the logits, timed alone as *_copy',
               config='wavenet_params.json with scalar_input',
               device=torch.cuda.get_device_name(0))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
