"""BASELINE.json configs[4] (fast generation on the DEFAULT stack: L=50,
S=512, Q=256, dilations up to 512) checked for correctness, not only speed:
the device paths of WaveNetModel.generate / predict_proba_incremental against
the float64 restatement of the reference's generator
(oracle.IncrementalGenerator = model.py:332-387, 444-516, 592-626;
teacher-forced like test/test_generation.py:50-72, but over > 2 wraps of the
dilation-512 ring buffers and past the receptive field 5117)."""
import json
import os

import numpy as np
import pytest
import torch

import draw_ref as D
from util import O, ROOT, cfg_with, build_pair

pytestmark = pytest.mark.gpu
TOL = 1e-5            # probabilities, float32 device path vs float64 oracle
N_TRACE = 1200        # > 2 * 512 (two wraps of the longest ring) + graph replay
N_SEED = 6000         # > receptive field 5117
N_GEN = 16000         # BASELINE.json configs[4]: free-running draws
SHARP = 5.0           # postprocess2 scale of the gc case: max probability ~0.2 - 0.8
PATHS = (('one_wg', False, False), ('multi_cu_graph', True, False),
         ('multi_cu_persistent', True, True))


def default_cfg(**kw):
    p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    c = {k: p[k] for k in p if k != 'sample_rate'}
    c['batch_size'] = 1
    c.update(kw)
    return c


def _wave(n, seed):
    """Teacher-forcing codes that exercise all bins: a mu-law-coded sine plus
    uniformly random codes."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.6 * np.sin(2 * np.pi * 220.0 * t / 16000.0)
    w = O.mu_law_encode(x.astype(np.float32), 256)
    r = rng.integers(0, 256, n)
    return np.where(rng.uniform(size=n) < 0.5, w, r).astype(np.int32)


@pytest.fixture(scope='module', params=['plain', 'gc'])
def traced(request, hip_lib):
    """(net, cfg, var, wave, gc id, oracle probabilities of the first N_TRACE
    steps, oracle generator advanced over the whole N_SEED-sample seed)."""
    gc = request.param == 'gc'
    cfg = default_cfg(**(dict(global_condition_channels=32,
                              global_condition_cardinality=377) if gc else {}))
    net, var = build_pair(cfg)                 # biases ~ N(0, 0.1)
    gid = 123 if gc else None
    wave = _wave(N_SEED, 11)
    gen = O.IncrementalGenerator(cfg, var, dtype=np.float64)
    ids = None if gid is None else np.array([gid])
    probs = np.empty((N_SEED, 256), np.float32)
    for i, s in enumerate(wave):
        probs[i] = gen.step(int(s), ids)
    return net, cfg, var, wave, gid, probs, gen


@pytest.mark.parametrize('multi,persist', [(False, False), (True, False), (True, True)],
                         ids=['one_wg', 'multi_cu_graph', 'multi_cu_persistent'])
def test_default_stack_teacher_forced_trace(traced, multi, persist):
    """Every one of N_TRACE next-sample distributions of the three device paths
    (single-workgroup kernel; multi-CU step kernels replayed from a hipGraph;
    ONE persistent multi-CU launch for the whole run) equals the oracle's."""
    net, cfg, var, wave, gid, probs, _ = traced
    net.fastgen_multi_cu = multi
    net.fastgen_persistent = persist
    net.fastgen_graph_steps = 200              # 1199 steps -> 4 graph replays
    seed = wave[:N_TRACE]
    out, pr = net.generate(0, seed_samples=seed, return_proba_every=1,
                           global_condition=gid)
    pr = pr.cpu().numpy()
    assert np.array_equal(out.cpu().numpy(), seed)
    assert pr.shape == (N_TRACE - 1, 256)
    err = np.abs(pr - probs[:N_TRACE - 1]).max(axis=1)
    assert err.max() < TOL, (int(err.argmax()), float(err.max()))
    # the ring buffers wrapped: steps past 2 * 512 are covered
    assert err[1024:].max() < TOL


def test_default_stack_incremental_api_and_naive(traced):
    """predict_proba_incremental one sample at a time (the reference's calling
    pattern, generate.py:213-226) over 1100 steps, then the naive forward
    (model.py:564-590) on the same history: all equal to the oracle."""
    net, cfg, var, wave, gid, probs, _ = traced
    net.reset_generator()
    n = 1100
    worst = 0.0
    for i in range(n):
        p = net.predict_proba_incremental(int(wave[i]), global_condition=gid)
        if i % 50 == 0 or i >= n - 40:
            worst = max(worst, float(np.abs(p.cpu().numpy() - probs[i]).max()))
    assert worst < TOL
    # naive path over the full seed (longer than the receptive field, so it
    # sees exactly what the queues hold)
    naive = net.predict_proba(wave, None if gid is None else [gid])
    assert np.abs(naive.cpu().numpy() - probs[N_SEED - 1]).max() < TOL


def test_default_stack_prime_from_6000_sample_seed(traced):
    """prime_generator (ONE forward pass over a seed longer than the receptive
    field; the reference's TODO generate.py:199-201) then one incremental
    step: equals the oracle generator that consumed the seed sample by
    sample; and the sampling path continues from it."""
    net, cfg, var, wave, gid, probs, gen = traced
    net.prime_generator(wave[:N_SEED - 1], global_condition=gid)
    p = net.predict_proba_incremental(int(wave[N_SEED - 1]),
                                      global_condition=gid, push=False)
    assert np.abs(p.cpu().numpy() - probs[N_SEED - 1]).max() < TOL
    # generate() from the long seed: the first drawn sample's distribution is
    # probs[N_SEED-1]; teacher-force the drawn continuation through the oracle
    # and require it to be likely under the oracle's distributions
    for multi, persist in ((False, False), (True, False), (True, True)):
        net.fastgen_multi_cu = multi
        net.fastgen_persistent = persist
        net.fastgen_graph_steps = 50
        out = net.generate(120, seed_samples=wave, seed=5,
                           global_condition=gid).cpu().numpy()
        assert out.shape == (N_SEED + 120,)
        assert np.array_equal(out[:N_SEED], wave)
        g2 = _clone_generator(gen)
        ids = None if gid is None else np.array([gid])
        ll = np.log(probs[N_SEED - 1][out[N_SEED]] + 1e-30)
        for i in range(119):
            pi = g2.step(int(out[N_SEED + i]), ids)
            ll += np.log(pi[out[N_SEED + i + 1]] + 1e-30)
        # random-init network: near-uniform predictions; a drawn sequence
        # cannot be much less likely than uniform under the true distribution
        assert ll / 120 > np.log(1.0 / 256) - 1.0


def _clone_generator(gen):
    import copy
    g = copy.copy(gen)
    g.q0 = [a.copy() for a in gen.q0]
    g.queues = [[a.copy() for a in q] for q in gen.queues]
    return g


def test_persistent_launch_failure_restores_state_and_falls_back(hip_lib, monkeypatch):
    """A persistent generation launch whose workgroups cannot all be resident
    (CUs held by another process: invisible to the launch-time occupancy check)
    ends with an expired hand-over wait after it has rewritten part of the
    generator's state.  The host must restore its snapshot, warn, and finish
    the run on the step kernels: same samples as a model that took the step
    kernels from the start, also on the following call."""
    from wavenet import _lib
    cfg = default_cfg()
    a, _ = build_pair(cfg)
    b, _ = build_pair(cfg)
    a.fastgen_graph_steps = b.fastgen_graph_steps = 40
    b.fastgen_persistent = False
    lib = _lib.load()
    real = lib.wn_fastgen_persist
    calls = []

    def failing(*args):
        # the real launch runs (state, cursors, codes are rewritten), then
        # reports what an expired wait reports
        code = real(*args)
        torch.cuda.synchronize()
        a._gen['fgp_sync'][12] = 1
        calls.append(code)
        return code
    monkeypatch.setattr(lib, 'wn_fastgen_persist', failing)
    seed = _wave(700, 3)
    with pytest.warns(UserWarning, match='state restored'):
        out_a = a.generate(150, seed_samples=seed, seed=9).cpu().numpy()
    out_b = b.generate(150, seed_samples=seed, seed=9).cpu().numpy()
    assert calls == [0] and a._gen_launch_failed['persist']
    assert np.array_equal(out_a, out_b)
    assert a._gen['steps'] == b._gen['steps']
    more_a = a.continue_generation(90, int(out_a[-1]), seed=4).cpu().numpy()
    more_b = b.continue_generation(90, int(out_b[-1]), seed=4).cpu().numpy()
    assert calls == [0]                     # not tried again on this generator
    assert np.array_equal(more_a, more_b)
    assert torch.equal(a._gen['state'], b._gen['state'])


@pytest.fixture(scope='module', params=['plain', 'gc_sharp'])
def free_run(request, hip_lib):
    """configs[4] at its stated length: generate(16000, seed_samples=[128],
    seed=2) on each device path, plain and with GC 32 x 377 (id 123); in the
    gc case postprocess2 is scaled by SHARP so that the distributions are far
    from uniform and the drawn sequence follows them.  Returns (net, gid,
    {path: (codes [16001], probabilities [16000, 256], end-state peek
    [256])}, float64 oracle probabilities of all 16001 positions of the
    persistent run's codes, as float32)."""
    gc = request.param == 'gc_sharp'
    cfg = default_cfg(**(dict(global_condition_channels=32,
                              global_condition_cardinality=377) if gc else {}))
    net, var = build_pair(cfg)
    if gc:
        var['postprocessing']['postprocess2'] = var['postprocessing']['postprocess2'] * SHARP
        net.load_nested(var)
    gid = 123 if gc else None
    net.fastgen_graph_steps = 200
    runs = {}
    for name, multi, persist in PATHS:
        net.fastgen_multi_cu = multi
        net.fastgen_persistent = persist
        out, pr = net.generate(N_GEN, seed_samples=[128], seed=2, return_proba_every=1,
                               global_condition=gid)
        out = out.cpu().numpy()
        # the queues now hold codes 0 .. 15999; the last code is not pushed
        peek = net.predict_proba_incremental(int(out[-1]), global_condition=gid,
                                             push=False).cpu().numpy()
        runs[name] = (out, pr.cpu().numpy(), peek)
    codes = runs['multi_cu_persistent'][0]
    emb = O.embed_gc(cfg, var, None if gid is None else np.array([gid]), 1)
    logits = O.network_forward(cfg, var, O.one_hot(codes[None], 256, np.float64), emb)
    ref = O._softmax64(logits[0])
    return net, gid, runs, ref


def _agree(c, codes):
    """Number of leading codes two runs share (N_GEN + 1: all): probability
    rows 0 .. _agree - 1 were computed from the same history."""
    d = np.nonzero(c != codes)[0]
    return int(d[0]) if d.size else N_GEN + 1


def test_16000_samples_same_on_every_path(free_run):
    """The single workgroup, the step kernels (80 graph replays) and ONE
    persistent launch draw the same 16001 codes, their probabilities 1e-6
    apart.  Far from uniform (gc_sharp: logits 5x larger, so 5x the rounding)
    two paths may part at a rounding tie: the step's u * total lies between
    the two paths' CDF boundaries, no farther from either than the two
    probability rows are apart, and the codes are the two beside it."""
    _, gid, runs, ref = free_run
    codes, pr = runs['multi_cu_persistent'][:2]
    assert codes.shape == (N_GEN + 1,) and codes[0] == 128
    assert pr.shape == (N_GEN, 256)
    path_tol = 1e-6 if gid is None else 1e-6 * SHARP
    for name, (c, p, _) in runs.items():
        k = _agree(c, codes)
        if gid is None:
            assert k == N_GEN + 1, (name, 'first differing code', k)
        err = np.abs(p[:k] - pr[:k]).max(axis=1)
        assert err.max() <= path_tol, (name, int(err.argmax()), float(err.max()))
        if k <= N_GEN:
            r = k - 1                      # the step that drew code k
            u = D.uniform(2, r)
            wa, wb = D.weights(p[r], 1.0), D.weights(pr[r], 1.0)
            l1 = float(np.abs(wa - wb).sum())
            assert max(float(D.margin(wa, u)), float(D.margin(wb, u))) <= l1, (name, k)
            assert {int(c[k]), int(codes[k])} == set(D.boundary_codes(wb, u)), (name, k)
    if gid is not None:
        # (SHARP) the drawn sequence is not noise: the max probability is
        # large along it
        assert 0.2 < np.median(ref.max(axis=1)) < 0.95


def test_16000_samples_match_restatement(free_run):
    """Every one of the 16000 drawn codes of every path is
    pick(weights(p, 1), uniform(2, k)) for its step k and the probabilities
    the device returned for that step (tests/draw_ref.py)."""
    _, _, runs, _ = free_run
    for name, (c, p, _) in runs.items():
        D.check_draws(c[1:], p, 1.0, 2, np.arange(N_GEN), what=name)


def test_16000_samples_vs_float64_oracle(free_run):
    """The device's probabilities at ALL 16000 steps (~31 wraps of the d = 512
    rings, the sample and probability buffers at full length, the persistent
    launch held for the whole run) equal the float64 oracle teacher-forced on
    the drawn codes; so does the end state (a push=False peek at position
    16000).  A path that parted from the persistent run at a rounding tie
    (gc_sharp) is compared up to that step."""
    _, gid, runs, ref = free_run
    codes = runs['multi_cu_persistent'][0]
    for name, (c, p, peek) in runs.items():
        k = _agree(c, codes)
        assert k == N_GEN + 1 or (gid is not None and name != 'multi_cu_persistent')
        n = min(k, N_GEN)                 # rows computed from the persistent run's history
        err = np.abs(p[:n] - ref[:n]).max(axis=1)
        assert err.max() < TOL, (name, int(err.argmax()), float(err.max()))
        if k == N_GEN + 1:
            assert np.abs(peek - ref[N_GEN]).max() < TOL, name


def test_16000_samples_continued_in_two_halves(free_run):
    """generate(8000) then continue_generation(8000) on the persistent path
    draws the codes of the single 16000-sample call: the counter goes on
    from step 8000."""
    net, gid, runs, _ = free_run
    net.fastgen_multi_cu = net.fastgen_persistent = True
    a = net.generate(N_GEN // 2, seed_samples=[128], seed=2,
                     global_condition=gid).cpu().numpy()
    b = net.continue_generation(N_GEN // 2, int(a[-1]), 1.0, gid, 2).cpu().numpy()
    k = _agree(np.concatenate([a, b]), runs['multi_cu_persistent'][0])
    assert k == N_GEN + 1, ('first differing code', k)
