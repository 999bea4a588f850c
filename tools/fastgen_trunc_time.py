"""Cost of the truncated draw (top_k / top_p) on the default stack:
    python tools/fastgen_trunc_time.py [samples] [out]
us per sample (median of 3 runs; a batch: per step of all streams) and a
checksum of the drawn samples on the persistent path, the one-workgroup path
and generate_batch at B = 64, for: off, top_k=40, top_p=0.95, both.  Writes
the lines to `out` (default profiles/fastgen_trunc_time.txt) as well."""
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

n = int(sys.argv[1]) if len(sys.argv) > 1 else 8000
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(
    ROOT, 'profiles', 'fastgen_trunc_time.txt')
B = 64
SETTINGS = [('off', {}), ('top_k=40', dict(top_k=40)),
            ('top_p=0.95', dict(top_p=0.95)),
            ('top_k=40 top_p=0.95', dict(top_k=40, top_p=0.95))]
p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
cfg = {k: p[k] for k in p if k != 'sample_rate'}
cfg['batch_size'] = 1
gen = WaveNetModel(seed=0, **model_kwargs(cfg))


def one(kw):
    return gen.generate(n, seed_samples=[128], temperature=1.0, seed=2, **kw)


def batch(kw):
    return gen.generate_batch(n, list(range(2, 2 + B)), seed_samples=[128],
                              temperature=1.0, **kw)


lines = ['fastgen_trunc_time: default stack, %d samples, median of 3 runs' % n]
for path, multi, fn in (('persistent', True, one), ('one workgroup', False, one),
                        ('generate_batch B=%d' % B, True, batch)):
    gen.fastgen_multi_cu = multi
    base = None
    for name, kw in SETTINGS:
        fn(kw)                              # (warm: graphs, module load)
        torch.cuda.synchronize()
        ts = []
        for r in range(3):
            t0 = time.perf_counter()
            out = fn(kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) / n * 1e6)
        med = float(np.median(ts))
        base = med if base is None else base
        lines.append('%-20s %-20s %8.2f us/sample (runs %s)  %+6.2f us  checksum %d' % (
            path, name, med, ' '.join('%.2f' % t for t in ts), med - base,
            int(out.cpu().numpy().astype(np.int64).sum())))
        print(lines[-1], flush=True)
with open(out_path, 'w') as f:
    f.write('\n'.join(lines) + '\n')
