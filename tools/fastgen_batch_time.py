"""Batched fast-generation rate of the default stack (one process, one
library):  python tools/fastgen_batch_time.py [steps] [B ...]
For each B (default 1 8 32 64 128 256): generate_batch(steps, B seeds) after a
warm-up call of the same shape, timed with device events over the whole call
(median of 3 runs); prints us per step, samples/s over all streams and a
checksum of the drawn codes.  Single-stream generate() of the same model and
length is reported beside them.  Ends with one JSON line of the figures."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import WaveNetModel  # noqa: E402
from util import model_kwargs  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
Bs = [int(v) for v in sys.argv[2:]] or [1, 8, 32, 64, 128, 256]
p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
cfg = {k: p[k] for k in p if k != 'sample_rate'}
cfg['batch_size'] = 1
net = WaveNetModel(seed=0, **model_kwargs(cfg))


def timed(fn):
    fn()                                   # warm-up: graph capture, buffers
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(3):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)     # us
    return float(np.median(ts)), ts, out.cpu().numpy().astype(np.int64)


res = {'steps': n, 'single': None, 'batch': {}}
us, ts, out = timed(lambda: net.generate(n, seed_samples=[128], seed=2))
res['single'] = dict(us_per_step=us / n, samples_per_s=n / us * 1e6,
                     checksum=int(out.sum()))
print('single-stream generate: %.2f us/sample  %.0f samples/s  checksum %d'
      % (us / n, n / us * 1e6, int(out.sum())))
for B in Bs:
    seeds = [2 + b for b in range(B)]
    us, ts, out = timed(lambda: net.generate_batch(n, seeds))
    r = dict(us_per_step=us / n, samples_per_s=B * n / us * 1e6,
             checksum=int(out.sum()),
             runs_us_per_step=[round(t / n, 3) for t in ts])
    res['batch'][B] = r
    print('B = %3d: %7.2f us/step  %10.0f samples/s  (%.1f x single)  '
          'checksum %d  runs %s' % (B, r['us_per_step'], r['samples_per_s'],
                                    r['samples_per_s'] / res['single']['samples_per_s'],
                                    r['checksum'], r['runs_us_per_step']))
print(json.dumps(res))
