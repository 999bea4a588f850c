"""Top-k / nucleus truncation of the draw on every draw site against the
float64 restatement (tests/trunc_ref.py).  As tests/test_gpu_draw.py:
postprocess2 = 0 pins the logits to postprocess2_bias, and the tests read back
which entry point ran.

The near-ties vector with top_k = 1 keeps the whole top tie group (36, 83,
112, 181 codes at Q = 100, 256, 320, 512).  600 draws cannot visit all of a
181-code group (about 6 are missed on average), so the test asks for what the
rule implies: every draw inside the group, and the device visiting exactly the
codes the restatement visits."""
import numpy as np
import pytest
import torch

import draw_ref as D
import trunc_ref as T
from test_gpu_draw import SITES, BATCH, _logits, _softmax32, _seed_with_extremes
from util import MID, cfg_with, build_pair

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings('error')]

N_DRAW = 600
KINDS = ('random', 'cliff', 'near_ties')
# (tau, top_k, top_p)
SETTINGS = [(1.0, 10, None), (0.7, None, 0.9), (3.0, 40, 0.8), (1.0, 1, None),
            (100.0, None, 0.5), (1.0, 3, 0.999)]
PLAIN = ('wn_fastgen_run', 'wn_fastgen_step', 'wn_fastgen_persist',
         'wn_fastgen_run_wide', 'wn_fastgen_batch_step')
ENTRIES = PLAIN + tuple(e + '_lc' for e in PLAIN if e != 'wn_fastgen_run_wide') + \
    ('wn_fastgen_run_trunc', 'wn_fastgen_run_wide_trunc', 'wn_fastgen_run_lc_trunc')
# the entry a truncated call must take where the plain one has a scalar temperature
TRUNC_ENTRY = {'wn_fastgen_run': 'wn_fastgen_run_trunc',
               'wn_fastgen_run_wide': 'wn_fastgen_run_wide_trunc',
               'wn_fastgen_run_lc': 'wn_fastgen_run_lc_trunc'}
LC = 8
LC_SITES = [('one_wg_lc', 256, 32, dict(fastgen_multi_cu=False), 'wn_fastgen_run_lc', None),
            ('persistent_lc', 256, 32, dict(fastgen_multi_cu=True, fastgen_persistent=True),
             'wn_fastgen_persist_lc', None),
            ('batch_lc', 256, 32, dict(), 'wn_fastgen_batch_step_lc', None)]


def _count_calls(monkeypatch):
    from wavenet import _lib
    lib = _lib.load()
    calls = {e: [] for e in ENTRIES}

    def counting(name, real):
        def f(*args):
            code = real(*args)
            calls[name].append((code, args))
            return code
        return f
    for e in ENTRIES:
        monkeypatch.setattr(lib, e, counting(e, getattr(lib, e)))
    return calls


def _pinned_model(Q, R, flags, lc=False):
    if lc:
        from wavenet import WaveNetModel
        net = WaveNetModel(1, MID['dilations'], 2, R, R, MID['skip_channels'],
                           quantization_channels=Q, use_biases=True, seed=3,
                           local_condition_channels=LC)
        with torch.no_grad():
            net.variables['postprocessing']['postprocess2'].zero_()
    else:
        net, var = build_pair(cfg_with(MID, batch_size=1, quantization_channels=Q,
                                       residual_channels=R, dilation_channels=R))
        var['postprocessing']['postprocess2'][:] = 0.0
        net.load_nested(var)
    for k, v in flags.items():
        setattr(net, k, v)
    net.fastgen_graph_steps = 64            # 601 steps: 9 replays of 64, 4 of 6
    return net


def _only(calls, entry, what):
    assert calls[entry], (what, 'not called', entry)
    assert all(not calls[e] for e in ENTRIES if e != entry), \
        (what, {e: len(c) for e, c in calls.items() if c})


ALL_SITES = SITES + LC_SITES


@pytest.mark.parametrize('site,Q,R,flags,entry,coop', ALL_SITES,
                         ids=['%s-Q%d-R%d' % (s[0], s[1], s[2]) for s in ALL_SITES])
def test_truncated_draw_matches_restatement(hip_lib, monkeypatch, site, Q, R, flags, entry, coop):
    """Every drawn code is pick(truncated weights, uniform(seed, counter)) (a
    summation-order tie at most twice per run, a code beside the boundary);
    no code outside the kept set, without tolerance; the probabilities stay
    the untruncated softmax (1 ulp); the intended entry point ran alone."""
    lc = site.endswith('_lc')
    net = _pinned_model(Q, R, flags, lc)
    calls = _count_calls(monkeypatch)
    want = TRUNC_ENTRY.get(entry, entry)
    bias = net.variables['postprocessing']['postprocess2_bias']
    counters = np.arange(1, N_DRAW + 1)
    batch = site.startswith('batch')
    rows = np.random.default_rng(7).standard_normal((N_DRAW + 1, LC)).astype(np.float32) \
        if lc else None
    for ki, kind in enumerate(KINDS):
        logits = _logits(kind, Q)
        with torch.no_grad():
            bias.copy_(torch.from_numpy(logits))
        p_ref = _softmax32(logits)
        for si, (tau, K, P) in enumerate(SETTINGS):
            what = '%s Q=%d R=%d %s T=%g K=%r P=%r' % (site, Q, R, kind, tau, K, P)
            tau32 = float(np.float32(tau))
            w, keep, margin = T.truncate(p_ref, tau32, K, P)
            print(what, 'kept', int(keep.sum()), 'margin', margin)
            assert margin >= 1e-9, what
            seeds = [_seed_with_extremes(counters, 1000 * (ki * len(SETTINGS) + si) + Q)]
            for e in ENTRIES:
                calls[e].clear()
            if net._gen is not None and net._gen.get('coop') is not None:
                net._gen['coop'].zero_()
            kw = dict(temperature=tau, return_proba_every=1, top_k=K, top_p=P)
            if lc:
                kw['local_condition'] = rows
            if batch:
                while len(seeds) < BATCH:
                    seeds.append(_seed_with_extremes(counters, seeds[-1] + 1))
                codes, proba = net.generate_batch(N_DRAW, seeds, seed_samples=[Q // 2, 3], **kw)
            else:
                codes, proba = net.generate(N_DRAW, seed_samples=[Q // 2, 3], seed=seeds[0], **kw)
                codes, proba = codes[None], proba[None]
            codes, proba = codes.cpu().numpy(), proba.cpu().numpy()
            _only(calls, want, what)
            assert not net._gen_launch_failed, (what, net._gen_launch_failed)
            if 'persist' in want:
                assert [c for c, _ in calls[want]] == [0], what
            if coop is not None:
                # (..., coop, top_k, top_p, stream)
                assert all((a[-4] is not None) == coop for _, a in calls[want]), what
            if coop:
                assert int(net._gen['coop'].count_nonzero()) > 0, what
            # the probabilities: untruncated
            assert proba.shape == (len(seeds), N_DRAW + 1, Q)
            assert np.array_equal(proba == 0, np.broadcast_to(p_ref == 0, proba.shape)), what
            ulp = np.abs(proba - p_ref) / np.spacing(p_ref)
            assert ulp.max() <= 1.0, (what, float(ulp.max()))
            for b, seed in enumerate(seeds):
                assert codes[b, 0] == Q // 2 and codes[b, 1] == 3
                got = codes[b, 2:]
                ties, _, kept = T.check_draws(got, proba[b, 1:], tau32, K, P, seed, counters,
                                              what='%s stream %d' % (what, b))
                # (the device's rows give the set of the reference row)
                assert np.array_equal(kept, np.broadcast_to(keep, kept.shape)), what
                assert keep[got].all(), what
                if kind == 'near_ties' and K == 1 and P is None:
                    # the whole top tie group is drawn from, as the restatement does
                    assert np.array_equal(keep, p_ref == p_ref.max()) and keep.sum() > 30
                    ref = D.pick(w, D.uniform(seed, counters))
                    assert len(set(got) ^ set(ref)) <= 2 * ties, what
                    assert len(set(got)) > 30, what


OFF_SITES = [s for s in SITES if (s[0], s[1]) in (
    ('one_wg', 256), ('multi_cu_graph', 256), ('persistent', 256), ('wide_single', 256),
    ('batch', 256))]


@pytest.mark.parametrize('site,Q,R,flags,entry,coop', OFF_SITES, ids=[s[0] for s in OFF_SITES])
def test_off_is_the_old_path(hip_lib, monkeypatch, site, Q, R, flags, entry, coop):
    """No keywords, None and (top_k = Q, top_p = 1) call the same plain entry
    point and return equal codes."""
    net, _ = build_pair(cfg_with(MID, batch_size=1, quantization_channels=Q,
                                 residual_channels=R, dilation_channels=R))
    for k, v in flags.items():
        setattr(net, k, v)
    net.fastgen_graph_steps = 64
    calls = _count_calls(monkeypatch)
    outs = []
    for kw in (dict(), dict(top_k=None, top_p=None), dict(top_k=Q, top_p=1.0)):
        for e in ENTRIES:
            calls[e].clear()
        if site == 'batch':
            c = net.generate_batch(200, [5, 6, 7], seed_samples=[Q // 2], temperature=0.9, **kw)
        else:
            c = net.generate(200, seed_samples=[Q // 2], temperature=0.9, seed=5, **kw)
        _only(calls, entry, (site, kw))
        outs.append(c.cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])
    # and the truncation does change the draws of this model
    if site == 'batch':
        c = net.generate_batch(200, [5, 6, 7], seed_samples=[Q // 2], temperature=0.9, top_k=2)
    else:
        c = net.generate(200, seed_samples=[Q // 2], temperature=0.9, seed=5, top_k=2)
    assert not np.array_equal(outs[0], c.cpu().numpy())


@pytest.mark.parametrize('gc', [False, True], ids=['plain', 'gc'])
@pytest.mark.parametrize('path', ['persistent', 'batch'])
def test_changing_distribution(hip_lib, monkeypatch, path, gc):
    """An untouched model, 300 steps: every code against the restatement
    applied to that step's returned row (a row whose nucleus margin is below
    1e-9 may be left out: at most 2)."""
    cfg = cfg_with(MID, batch_size=1)
    if gc:
        cfg.update(global_condition_channels=4, global_condition_cardinality=5)
    net, _ = build_pair(cfg)
    net.fastgen_multi_cu, net.fastgen_persistent, net.fastgen_graph_steps = True, True, 64
    calls = _count_calls(monkeypatch)
    n, K, P, tau = 300, 20, 0.9, 0.8
    tau32 = float(np.float32(tau))
    kw = dict(temperature=tau, return_proba_every=1, top_k=K, top_p=P)
    if path == 'batch':
        seeds = [21, 22, 23]
        codes, proba = net.generate_batch(n, seeds, seed_samples=[128], **kw,
                                          global_condition=[1, 2, 3] if gc else None)
        _only(calls, 'wn_fastgen_batch_step', path)
    else:
        seeds = [21]
        codes, proba = net.generate(n, seed_samples=[128], seed=21, **kw,
                                    global_condition=[2] if gc else None)
        codes, proba = codes[None], proba[None]
        _only(calls, 'wn_fastgen_persist', path)
    codes, proba = codes.cpu().numpy(), proba.cpu().numpy()
    for b, seed in enumerate(seeds):
        _, skipped, kept = T.check_draws(codes[b, 1:], proba[b], tau32, K, P, seed,
                                         np.arange(n), max_skipped=2,
                                         what='%s gc=%r stream %d' % (path, gc, b))
        print(path, gc, b, 'rows left out', skipped, 'kept per row',
              int(kept.sum(1).min()), int(kept.sum(1).max()))
        assert kept.sum(1).min() >= 1
    # the distribution does change from step to step
    assert np.abs(proba[0, 1:] - proba[0, :-1]).max() > 1e-3


def test_per_call_and_consistent_across_paths(hip_lib):
    """continue_generation after a truncated generate draws untruncated
    unless asked; stream b of a truncated generate_batch equals a truncated
    generate with seeds[b]."""
    net, _ = build_pair(cfg_with(MID, batch_size=1))
    net.fastgen_multi_cu, net.fastgen_persistent, net.fastgen_graph_steps = True, True, 64
    trunc = dict(top_k=8, top_p=0.85)
    kw = dict(temperature=0.9, **trunc)
    a = net.generate(120, seed_samples=[128], seed=9, **kw).cpu().numpy()
    more_plain = net.continue_generation(100, int(a[-1]), 0.9, None, 9).cpu().numpy()
    b = net.generate(120, seed_samples=[128], seed=9, **kw).cpu().numpy()
    assert np.array_equal(a, b)
    more_trunc = net.continue_generation(100, int(b[-1]), 0.9, None, 9, **trunc).cpu().numpy()
    # the untruncated continuation is that of an untruncated run from the same state
    whole_trunc = net.generate(220, seed_samples=[128], seed=9, **kw).cpu().numpy()
    assert np.array_equal(whole_trunc, np.concatenate([b, more_trunc]))
    assert not np.array_equal(more_plain, more_trunc)
    c = net.generate(120, seed_samples=[128], seed=9, **kw).cpu().numpy()
    ref_plain = net.continue_generation(100, int(c[-1]), 0.9, None, 9,
                                        top_k=None, top_p=None).cpu().numpy()
    assert np.array_equal(more_plain, ref_plain)
    # batch stream b == single stream with seeds[b], on every single-stream path
    seeds = [9, 10, 11, 12]
    bat = net.generate_batch(120, seeds, seed_samples=[128], **kw).cpu().numpy()
    for multi, persist in ((False, False), (True, False), (True, True)):
        net.fastgen_multi_cu, net.fastgen_persistent = multi, persist
        for i, s in enumerate(seeds[:2]):
            one = net.generate(120, seed_samples=[128], seed=s, **kw).cpu().numpy()
            assert np.array_equal(bat[i], one), (multi, persist, i)
