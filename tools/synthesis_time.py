"""What sorting by length buys the bulk synthesis path (one process, one
library):  python tools/synthesis_time.py [--out FILE] [--items 64]
                                          [--repeats 3] [--limit 120]
                                          [--queue_out FILE]
The default stack with Lc = 80 (rows at audio rate) and `items` utterances
with seeded lengths uniform in [2000, 16000].  Four arms, interleaved
a b c d a b c d ... after one warm-up pass of each, each call timed on the
wall clock between two device synchronisations:
  (a) synthesis.synthesize at batch 32: length-sorted rounds;
  (b) generate_batch over the items in the given order, 32 at a time, every
      batch padded to its longest item -- what there was before;
  (c) single-stream generate on four of the items, one after the other;
  (d) synthesis.synthesize(schedule='queue') at batch 32: a finished
      stream's slot takes the next item at once (default quantum).
Prints each arm's wall time (median and runs), samples/s (real samples),
lock-step steps and occupancy, then us per lock-step step of (a) and (b) and
time(a) / time(b) beside steps(a) / steps(b); writes the same lines to --out
(default profiles/synthesis_time.txt).  Arm (d) goes to --queue_out (default
profiles/synthesis_queue_time.txt): wall time, steps and segments, us per
lock-step step of (a) and (d) with (a)'s spread as the margin, and the cost
of an admission, (time_d - steps_d * step_time_a) / segments; and, to tell
the step itself from what a segment costs around it, one
continue_generation_batch call of --probe_steps steps timed on a generator
without restarted streams (the plain entry points) and on one with a
restarted stream (the _q entry points), alternating.  Every timed
call runs under its own
time limit (--limit seconds: the process is ended with a traceback when one
call takes longer)."""
import argparse
import faulthandler
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import json  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import WaveNetModel, synthesis  # noqa: E402
from util import model_kwargs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles',
                                              'synthesis_time.txt'))
ap.add_argument('--queue_out', default=os.path.join(
    ROOT, 'profiles', 'synthesis_queue_time.txt'))
ap.add_argument('--probe_steps', type=int, default=4000)
ap.add_argument('--items', type=int, default=64)
ap.add_argument('--repeats', type=int, default=3)
ap.add_argument('--limit', type=int, default=120)
args = ap.parse_args()

B, LC = 32, 80
p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
cfg = {k: p[k] for k in p if k != 'sample_rate'}
cfg['batch_size'] = 1
net = WaveNetModel(seed=0, local_condition_channels=LC, **model_kwargs(cfg))
rng = np.random.default_rng(0)
lengths = [int(v) for v in rng.integers(2000, 16001, args.items)]
seeds = list(range(1, args.items + 1))
gen = torch.Generator().manual_seed(1)
rows = [torch.randn((n, LC), generator=gen).to(net.device) for n in lengths]
singles = [0, args.items // 3, 2 * args.items // 3, args.items - 1]


def arm_a():
    return synthesis.synthesize(net, lengths, seeds=seeds, batch=B,
                                local_condition=rows).codes


def arm_b():
    codes = [None] * len(lengths)
    for i in range(0, len(lengths), B):
        items = list(range(i, min(i + B, len(lengths))))
        T = max(lengths[u] for u in items)
        lc = torch.zeros((len(items), T, LC), device=net.device)
        for j, u in enumerate(items):
            lc[j, 1:lengths[u]] = rows[u][:lengths[u] - 1]
        out = net.generate_batch(T, [seeds[u] for u in items],
                                 local_condition=lc)
        for j, u in enumerate(items):
            codes[u] = out[j, 1:1 + lengths[u]]
    return codes


def arm_c():
    codes = []
    for u in singles:
        n = lengths[u]
        lc = torch.cat([torch.zeros((1, LC), device=net.device),
                        rows[u][:n - 1]])
        codes.append(net.generate(n, seed_samples=[net.Q // 2], seed=seeds[u],
                                  local_condition=lc)[1:])
    return codes


def arm_d():
    return synthesis.synthesize(net, lengths, seeds=seeds, batch=B,
                                local_condition=rows, schedule='queue').codes


captures = [0]                 # hipGraph captures so far (torch.cuda.graph)
_enter = torch.cuda.graph.__enter__


def _counted_enter(self):
    captures[0] += 1
    return _enter(self)


torch.cuda.graph.__enter__ = _counted_enter


def timed(fn):
    faulthandler.dump_traceback_later(args.limit, exit=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    faulthandler.cancel_dump_traceback_later()
    return t, out


plan = synthesis.plan_rounds(lengths, B)
steps_b = sum(max(lengths[i:i + B]) for i in range(0, len(lengths), B))
quantum = max(1, int(net.fastgen_graph_steps) // 10)
qplan = synthesis.plan_queue(lengths, B, quantum)
arms = {
    'a': dict(fn=arm_a, what='synthesize, sorted rounds', steps=plan.steps,
              samples=sum(lengths), slots=B * plan.steps),
    'b': dict(fn=arm_b, what='generate_batch, given order', steps=steps_b,
              samples=sum(lengths), slots=B * steps_b),
    'c': dict(fn=arm_c, what='generate, %d items' % len(singles),
              steps=sum(lengths[u] for u in singles),
              samples=sum(lengths[u] for u in singles),
              slots=sum(lengths[u] for u in singles)),
    'd': dict(fn=arm_d, what='synthesize, restart queue', steps=qplan.steps,
              samples=sum(lengths), slots=B * qplan.steps),
}
out = {}
for k in 'abcd':                      # warm-up: buffers, graph capture
    c0 = captures[0]
    _, out[k] = timed(arms[k]['fn'])
    arms[k]['runs'], arms[k]['warm_captures'] = [], captures[0] - c0
    arms[k]['captures'] = 0
for _ in range(args.repeats):
    for k in 'abcd':
        c0 = captures[0]
        t, out[k] = timed(arms[k]['fn'])
        arms[k]['runs'].append(t)
        arms[k]['captures'] += captures[0] - c0
# the arms draw the same codes (the contract of wavenet/synthesis.py)
same_ab = all(torch.equal(x, y) for x, y in zip(out['a'], out['b']))
same_ac = all(torch.equal(out['a'][u], c) for u, c in zip(singles, out['c']))
same_ad = all(torch.equal(x, y) for x, y in zip(out['a'], out['d']))

lines = ['%d items, lengths uniform in [2000, 16000] (seed 0): %d samples; '
         'default stack, Lc = %d, batch %d; %d timed runs per arm, '
         'interleaved, after one warm-up pass each'
         % (args.items, sum(lengths), LC, B, args.repeats)]


def arm_line(k):
    a = arms[k]
    a['t'] = float(np.median(a['runs']))
    return ('(%s) %-28s %7.3f s  %9.0f samples/s  %6d steps  occupancy '
            '%.3f  us/step %.2f  runs %s'
            % (k, a['what'], a['t'], a['samples'] / a['t'], a['steps'],
               a['samples'] / float(a['slots']), a['t'] / a['steps'] * 1e6,
               [round(t, 3) for t in a['runs']]))


for k in 'abc':
    lines.append(arm_line(k))
ra = [t / arms['a']['steps'] * 1e6 for t in arms['a']['runs']]
rb = [t / arms['b']['steps'] * 1e6 for t in arms['b']['runs']]
lines.append('us per lock-step step: (a) %.2f .. %.2f, (b) %.2f .. %.2f'
             % (min(ra), max(ra), min(rb), max(rb)))
lines.append('time(a) / time(b) = %.4f, steps(a) / steps(b) = %.4f'
             % (arms['a']['t'] / arms['b']['t'],
                arms['a']['steps'] / float(arms['b']['steps'])))
lines.append('codes: (a) == (b) %s, (a) == (c) on its items %s'
             % (same_ab, same_ac))
text = '\n'.join(lines)
print(text)
with open(args.out, 'w') as f:
    f.write(text + '\n')

# the restart queue against the rounds of the same process
rd = [t / arms['d']['steps'] * 1e6 for t in arms['d']['runs']]
step_a = arms['a']['t'] / arms['a']['steps']
nseg = len(qplan.segments)
q1 = synthesis.plan_queue(lengths, B, 1).steps
qlines = [lines[0], arm_line('a'), arm_line('d')]
qlines.append('(d): quantum %d, %d segments (one generate_batch, %d '
              'continue_generation_batch with restart), longest %d steps; '
              'quantum 1 would take %d steps'
              % (quantum, nseg, nseg - 1, max(m for _, m in qplan.segments),
                 q1))
qlines.append('us per lock-step step: (a) %.2f .. %.2f (median %.2f, spread '
              '%.2f), (d) %.2f .. %.2f (median %.2f)'
              % (min(ra), max(ra), step_a * 1e6, max(ra) - min(ra), min(rd),
                 max(rd), arms['d']['t'] / arms['d']['steps'] * 1e6))
qlines.append('cost of an admission: (time(d) - steps(d) * step time(a)) / '
              'segments = %.1f us'
              % ((arms['d']['t'] - arms['d']['steps'] * step_a) / nseg * 1e6))
qlines.append('time(d) / time(a) = %.4f, steps(d) / steps(a) = %.4f'
              % (arms['d']['t'] / arms['a']['t'],
                 arms['d']['steps'] / float(arms['a']['steps'])))
qlines.append('hipGraph captures: warm-up pass (a) %d, (d) %d; timed runs '
              '(a) %d, (d) %d'
              % (arms['a']['warm_captures'], arms['d']['warm_captures'],
                 arms['a']['captures'], arms['d']['captures']))
qlines.append('codes: (a) == (d) %s' % same_ad)

# the step alone: the same call on the plain and on the _q entry points
N = args.probe_steps
plc = torch.randn((B, N, LC), generator=gen).to(net.device)
slc = plc[:, :200].contiguous()
probe = {'plain': [], '_q': []}
for rep in range(args.repeats + 1):      # (the first pass: graph capture)
    for kind in ('plain', '_q'):
        if kind == 'plain':
            last = net.generate_batch(200, seeds[:B], local_condition=slc,
                                      reserve_steps=N)[:, -1]
        else:
            last = net.continue_generation_batch(
                200, last, seeds[:B], local_condition=slc, restart=[0],
                reserve_steps=N)[:, -1]
        t, res = timed(lambda: net.continue_generation_batch(
            N, last, seeds[:B], local_condition=plc, reserve_steps=N))
        last = res[:, -1]
        if rep:
            probe[kind].append(t / N * 1e6)
qlines.append('one call of %d steps, us per step: plain entries %s, _q '
              'entries %s' % (N, [round(v, 2) for v in probe['plain']],
                              [round(v, 2) for v in probe['_q']]))
qtext = '\n'.join(qlines)
print(qtext)
with open(args.queue_out, 'w') as f:
    f.write(qtext + '\n')
