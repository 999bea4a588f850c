"""Fast generation's draw on every draw site against the host restatement
(tests/draw_ref.py) and a known distribution.  postprocess2 = 0 makes the
logits exactly postprocess2_bias at every step, whatever the history, so the
probabilities must be the float64 softmax of that vector and every drawn code
must be pick(weights(p, T), uniform(seed, counter)) -- the reference's
log(p) / T rule and inverse CDF (generate.py:228-240) with the device's
counter-based uniform.  The tests read back which entry point ran rather than
assuming it."""
import numpy as np
import pytest
import torch

import draw_ref as D
from util import MID, cfg_with, build_pair

pytestmark = [pytest.mark.gpu,
              # a launch that falls back to another path warns: an error here
              pytest.mark.filterwarnings('error')]

N_DRAW = 2000
TAUS = (1.0, 0.7, 0.05, 3.0, 100.0)
KINDS = ('random', 'cliff', 'near_ties')
SEED_CODES = 2          # seed_samples=[Q // 2, 3]: code k + 1 drawn with counter k
ENTRIES = ('wn_fastgen_run', 'wn_fastgen_step', 'wn_fastgen_persist',
           'wn_fastgen_run_wide', 'wn_fastgen_batch_step')
BATCH = 4               # streams of the batched site, each with its own seed

# (id, quantization channels, residual = dilation channels, device flags,
#  the entry point that must run, cooperative wide launch)
SITES = [('one_wg', Q, 32, dict(fastgen_multi_cu=False), 'wn_fastgen_run', None)
         for Q in (100, 256, 320, 512)] + \
        [('multi_cu_graph', Q, 32, dict(fastgen_multi_cu=True, fastgen_persistent=False),
          'wn_fastgen_step', None) for Q in (100, 256, 320, 512)] + \
        [('persistent', Q, 32, dict(fastgen_multi_cu=True, fastgen_persistent=True),
          'wn_fastgen_persist', None) for Q in (100, 256, 320, 512)] + \
        [('wide', 1024, 32, dict(), 'wn_fastgen_run_wide', False),
         ('wide_coop', 256, 64, dict(fastgen_wide_coop=True), 'wn_fastgen_run_wide', True),
         ('wide_single', 256, 64, dict(fastgen_wide_coop=False), 'wn_fastgen_run_wide', False),
         ('batch', 256, 32, dict(), 'wn_fastgen_batch_step', None)]


def _softmax32(logits):
    l = np.asarray(logits, np.float64)
    e = np.exp(l - l.max())
    return (e / e.sum()).astype(np.float32)


def _logits(kind, Q):
    """float32 logit vectors: N(0, 4^2); a cliff (one code at +120, three at
    +110, the rest at 0: probability exactly 0 at codes 0, Q // 2 and Q - 1);
    near-ties (three levels 2^-20 apart, many codes exactly equal)."""
    rng = np.random.default_rng(Q)
    if kind == 'random':
        return rng.normal(0, 4, Q).astype(np.float32)
    if kind == 'cliff':
        l = np.zeros(Q, np.float32)
        l[Q // 3] = 120.0
        l[[Q // 5, Q // 2 + 1, Q - 7]] = 110.0
        return l
    return (rng.integers(0, 3, Q) * 2.0 ** -20).astype(np.float32)


def _seed_with_extremes(counters, start):
    """The first seed from `start` whose uniforms over `counters` include one
    below 1e-3 and one above 1 - 1e-3 (chosen with the restatement)."""
    for s in range(start, start + 10000):
        u = D.uniform(s, counters)
        if u.min() < 1e-3 and u.max() > 1 - 1e-3:
            return s
    raise AssertionError('no seed found')


@pytest.mark.parametrize('site,Q,R,flags,entry,coop', SITES,
                         ids=['%s-Q%d-R%d' % (s[0], s[1], s[2]) for s in SITES])
def test_draw_matches_restatement(hip_lib, monkeypatch, site, Q, R, flags, entry, coop):
    """(a) the returned probabilities are the float64 softmax of the logit
    vector rounded to float32 (1 ulp; exactly 0 where that rounds to 0);
    (b) every drawn code is the restated one (a summation-order tie at most
    twice per run, and then only a code beside the boundary); (c) no code of
    probability 0 is drawn -- for temperatures 1, 0.7, 0.05, 3 and 100 (the
    near-ties vector: 1, 0.05 and 100), with graph replays crossed and seeds
    whose runs hold uniforms within 1e-3 of 0 and of 1.  The batched site
    (generate_batch) checks all of this for each of BATCH streams."""
    from wavenet import _lib
    cfg = cfg_with(MID, batch_size=1, quantization_channels=Q,
                   residual_channels=R, dilation_channels=R)
    net, var = build_pair(cfg)
    var['postprocessing']['postprocess2'][:] = 0.0
    net.load_nested(var)
    for k, v in flags.items():
        setattr(net, k, v)
    net.fastgen_graph_steps = 64           # 2001 steps: 31 replays of 64, 2 of 6
    lib = _lib.load()
    calls = {e: [] for e in ENTRIES}

    def counting(name, real):
        def f(*args):
            code = real(*args)
            calls[name].append((code, args[-2]))
            return code
        return f
    for e in ENTRIES:
        monkeypatch.setattr(lib, e, counting(e, getattr(lib, e)))
    bias = net.variables['postprocessing']['postprocess2_bias']
    counters = np.arange(1, N_DRAW + 1)
    for ki, kind in enumerate(KINDS):
        logits = _logits(kind, Q)
        with torch.no_grad():
            bias.copy_(torch.from_numpy(logits))
        p_ref = _softmax32(logits)
        for ti, T in enumerate(TAUS):
            if kind == 'near_ties' and T in (0.7, 3.0):
                continue                   # (GPU time: ties need no more temperatures)
            what = '%s Q=%d R=%d %s T=%g' % (site, Q, R, kind, T)
            seeds = [_seed_with_extremes(counters, 1000 * (ki * len(TAUS) + ti) + Q)]
            for e in ENTRIES:
                calls[e].clear()
            if net._gen is not None and net._gen.get('coop') is not None:
                net._gen['coop'].zero_()
            if site == 'batch':
                while len(seeds) < BATCH:
                    seeds.append(_seed_with_extremes(counters, seeds[-1] + 1))
                codes, proba = net.generate_batch(N_DRAW, seeds, seed_samples=[Q // 2, 3],
                                                  temperature=T, return_proba_every=1)
            else:
                codes, proba = net.generate(N_DRAW, seed_samples=[Q // 2, 3],
                                            temperature=T, seed=seeds[0],
                                            return_proba_every=1)
                codes, proba = codes[None], proba[None]
            codes, proba = codes.cpu().numpy(), proba.cpu().numpy()
            # the intended draw site ran, and nothing else
            assert calls[entry], (what, 'not called', entry)
            assert all(not calls[e] for e in ENTRIES if e != entry), \
                (what, {e: len(c) for e, c in calls.items()})
            assert not net._gen_launch_failed, (what, net._gen_launch_failed)
            if entry == 'wn_fastgen_persist':
                assert [c for c, _ in calls[entry]] == [0], (what, calls[entry])
            if coop is not None:
                assert all((a is not None) == coop for _, a in calls[entry]), what
            if coop:
                assert int(net._gen['coop'].count_nonzero()) > 0, \
                    (what, 'the cooperative launch did not run')
            # (a) probabilities
            B = len(seeds)
            assert proba.shape == (B, N_DRAW + 1, Q) and codes.shape == (B, N_DRAW + 2)
            assert np.array_equal(proba == 0, np.broadcast_to(p_ref == 0, proba.shape)), what
            ulp = np.abs(proba - p_ref) / np.spacing(p_ref)
            assert ulp.max() <= 1.0, (what, float(ulp.max()), np.unravel_index(ulp.argmax(), ulp.shape))
            # (b), (c) drawn codes: code k + 1 drawn with counter k from row k
            for b, seed in enumerate(seeds):
                u = D.uniform(seed, counters)
                assert u.min() < 1e-3 and u.max() > 1 - 1e-3
                assert codes[b, 0] == Q // 2 and codes[b, 1] == 3
                D.check_draws(codes[b, SEED_CODES:], proba[b, 1:], float(np.float32(T)), seed,
                              counters, what='%s stream %d' % (what, b))
                if kind == 'cliff' and T == 100.0:
                    # the three +110 codes carry weight exp(-0.1) each: the draw
                    # must not collapse onto the top code
                    assert len(np.unique(codes[b, SEED_CODES:])) == 4, what
