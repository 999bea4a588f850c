"""Where a batched generation step's time goes, per launch (default stack):
    python tools/fastgen_batch_stages.py [steps] [B ...]
Runs `steps` lock-step steps of generate_batch's state (B streams from
Q // 2) one launch at a time through wn_fastgen_batch_stages, with a device
event before every launch, and reports the mean time between consecutive
events for each of the five stages (draw, chain, skip + next pre-activations,
post1, logits) over the steps after the first 50.  Each figure is the
kernel plus the gap to the next launch; their sum is compared with the same
steps replayed from a hipGraph (generate_batch), which is what users get.
Ends with one JSON line."""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tensorflow-wavenet_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from wavenet import WaveNetModel, _lib, fastgen  # noqa: E402
from util import model_kwargs  # noqa: E402

STAGES = ('draw', 'chain', 'skip_pre', 'post1', 'logits')
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
Bs = [int(v) for v in sys.argv[2:]] or [32, 256]
p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
cfg = {k: p[k] for k in p if k != 'sample_rate'}
cfg['batch_size'] = 1
net = WaveNetModel(seed=0, **model_kwargs(cfg))
res = {'steps': n, 'batch': {}}
for B in Bs:
    seeds = np.asarray([2 + b for b in range(B)], np.uint64).view(np.int64)
    # graph-replayed reference (after a warm-up call of the same shape)
    net.generate_batch(n, list(range(2, 2 + B)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    ref = net.generate_batch(n, list(range(2, 2 + B)))
    e1.record()
    e1.synchronize()
    graph_us = e0.elapsed_time(e1) * 1e3 / n
    # the same steps, one launch at a time between events
    g = fastgen.batch_generator(net, B)
    fastgen.batch_reset(net, g)
    io = torch.full((B, n + 1), net.Q // 2, dtype=torch.int32, device=net.device)
    prep = fastgen.batch_prepare(net, g, io, 1, n, 1.0, seeds, None, 1, None)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(n)]
    st = _lib.stream()
    for i in range(n):
        for k in range(5):
            ev[i][k].record()
            _lib.call('wn_fastgen_batch_stages', k, k + 1, *prep['args'], st)
        ev[i][5].record()
    torch.cuda.synchronize()
    fastgen.batch_complete(net, g, prep, io, None, n)
    same = bool(torch.equal(io, ref))
    t = np.array([[ev[i][k].elapsed_time(ev[i][k + 1]) * 1e3 for k in range(5)]
                  for i in range(50, n)])
    mean = t.mean(axis=0)
    r = dict(graph_us_per_step=graph_us, staged_us_per_step=float(mean.sum()),
             stages_us={s: float(v) for s, v in zip(STAGES, mean)},
             stages_us_p90={s: float(v) for s, v in zip(STAGES, np.percentile(t, 90, axis=0))},
             same_codes_as_graph=same)
    res['batch'][B] = r
    print('B = %3d: graph %.2f us/step; staged %.2f = %s  (same codes: %s)' % (
        B, graph_us, mean.sum(),
        ' + '.join('%s %.2f' % (s, v) for s, v in zip(STAGES, mean)), same))
print(json.dumps(res))
