"""Cost of local conditioning in fast generation: the default stack
(wavenet_params.json) with Lc = 80 against the same weights without LC, runs
interleaved in one process (median of 5 of each):
  - us per sample of generate() on the persistent and the step-kernel paths
    (8000 samples);
  - us per step of generate_batch at B = 1, 32 and 256 (400 steps);
  - us per sample of the naive LC path (predict_proba over the window, as
    generate.py --fast_generation false) over 200 samples, for the speed-up.
    python tools/fastgen_lc_time.py [out.txt]
Writes profiles/fastgen_lc_time.txt by default."""
import json
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import WaveNetModel  # noqa: E402
from util import model_kwargs  # noqa: E402

LC = 80
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
    ROOT, 'profiles', 'fastgen_lc_time.txt')
p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
cfg = {k: p[k] for k in p if k != 'sample_rate'}
cfg['batch_size'] = 1
plain = WaveNetModel(seed=0, **model_kwargs(cfg))
cond = WaveNetModel(seed=0, local_condition_channels=LC, **model_kwargs(cfg))
src = dict(plain.named_variables())
with torch.no_grad():
    for n, v in cond.named_variables():
        if n in src:
            v.copy_(src[n])
        else:
            v.copy_(0.05 * torch.randn(v.shape, generator=torch.Generator()
                                       .manual_seed(1)))
rng = np.random.default_rng(0)


def timed(fn, per, reps=5):
    fn()                                  # warm (graphs, buffers)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / per * 1e6)
    return ts


def pair(name, fn_plain, fn_lc, per, unit):
    # interleaved: plain, LC, plain, LC, ...
    a, b = [], []
    for _ in range(5):
        a += timed(fn_plain, per, 1)
        b += timed(fn_lc, per, 1)
    ma, mb = float(np.median(a)), float(np.median(b))
    return '%-28s %9.2f %9.2f %+8.2f (%+.1f %%)  %s' % (
        name, ma, mb, mb - ma, 100.0 * (mb - ma) / ma, unit)


lines = ['# default stack (L = %d, S = %d, Q = %d), Lc = %d; median of 5 '
         'interleaved runs each' % (len(cfg['dilations']),
                                    cfg['skip_channels'],
                                    cfg['quantization_channels'], LC),
         '%-28s %9s %9s %8s' % ('', 'no LC', 'LC', 'delta')]
N = 8000
rows = rng.standard_normal((N, LC)).astype(np.float32)
for path, persistent in (('persistent', True), ('step kernels', False)):
    for net in (plain, cond):
        net.fastgen_multi_cu, net.fastgen_persistent = True, persistent
    lines.append(pair(
        'generate, %s' % path,
        lambda: plain.generate(N, seed_samples=[128], seed=2),
        lambda: cond.generate(N, seed_samples=[128], seed=2,
                              local_condition=rows),
        N, 'us / sample'))
S = 400
for B in (1, 32, 256):
    brows = rng.standard_normal((B, S, LC)).astype(np.float32)
    seeds = list(range(B))
    lines.append(pair(
        'generate_batch, B = %d' % B,
        lambda: plain.generate_batch(S, seeds),
        lambda: cond.generate_batch(S, seeds, local_condition=brows),
        S, 'us / step'))
# naive LC path: one predict_proba over the growing window per sample
W = 8000
cond.reserve(1, W)
hist = rng.integers(0, 256, W).astype(np.int32)
hrows = rng.standard_normal((W, LC)).astype(np.float32)


def naive(n=200):
    for i in range(n):
        cond.predict_proba(hist, local_condition=hrows[None])


ts = timed(naive, 200, 3)
cond.fastgen_persistent = True
tf = timed(lambda: cond.generate(N, seed_samples=[128], seed=2,
                                 local_condition=rows), N, 3)
lines.append('%-28s %9s %9.2f %8s  us / sample (window %d); fast persistent '
             '%.2f: %.0fx' % ('naive predict_proba, LC', '', np.median(ts),
                              '', W, np.median(tf),
                              np.median(ts) / np.median(tf)))
text = '\n'.join(lines) + '\n'
print(text, end='')
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    f.write(text)
