"""The generators at dilations that are not powers of two.  Ring cursors
(`tpos % d`, `pos == d ? 0`), re-entry (`steps_done % d`), priming from a
forward pass and restarts inside a running batch had only been run where
every ring wraps in phase with every other and every chunk boundary is a
multiple of most dilations.  Model: the MID widths on DIL_GEN =
[3, 5, 33, 7, 48, 17] (receptive field 114; on it the incremental and the
naive float64 oracle agree exactly).  Each statement is one the suite already
makes for power-of-two stacks, under the same bar."""
import numpy as np
import pytest
import torch

from util import DIL_GEN, MID, O, build_pair, cfg_with

pytestmark = pytest.mark.gpu
TOL = 1e-5            # probabilities, float32 device path vs float64 oracle

CFG = cfg_with(MID, batch_size=1, dilations=DIL_GEN)
Q = CFG['quantization_channels']
PATHS = [(False, False), (True, False), (True, True)]
PATH_IDS = ['one_wg', 'multi_cu_graph', 'multi_cu_persistent']


@pytest.fixture(scope='module')
def pair(hip_lib):
    return build_pair(CFG)


@pytest.fixture(scope='module')
def trace(pair):
    """260 codes (every ring wraps at least 5 times) and the float64 oracle's
    distribution after each of them; computed once"""
    _, var = pair
    wave = np.random.default_rng(9).integers(0, Q, 260).astype(np.int32)
    gen = O.IncrementalGenerator(CFG, var, dtype=np.float64)
    probs = np.stack([np.asarray(gen.step(int(c))).reshape(-1) for c in wave])
    assert len(wave) >= 5 * max(DIL_GEN)
    return wave, probs


def _select(net, multi, persist):
    net.fastgen_multi_cu = multi
    net.fastgen_persistent = persist
    net.fastgen_graph_steps = 50          # graph capture + replay, with a remainder


@pytest.mark.parametrize('multi,persist', PATHS, ids=PATH_IDS)
def test_teacher_forced_trace_vs_float64_oracle(pair, trace, multi, persist):
    net, _ = pair
    wave, probs = trace
    _select(net, multi, persist)
    out, pr = net.generate(0, seed_samples=wave, return_proba_every=1)
    assert np.array_equal(out.cpu().numpy(), wave)
    pr = pr.cpu().numpy()
    assert pr.shape == (len(wave) - 1, Q)
    err = np.abs(pr - probs[:len(wave) - 1]).max(axis=1)
    assert err.max() < TOL, (int(err.argmax()), float(err.max()))


def test_chunked_run_equals_one_call_on_every_path(pair):
    """generate 101, continue 83, continue 76: re-entry at cursors that are
    multiples of no dilation; sampled codes bit equal to the one-call run, and
    the same on the three device paths."""
    net, _ = pair
    runs = []
    for multi, persist in PATHS:
        _select(net, multi, persist)
        whole = net.generate(260, seed_samples=[128], seed=11).cpu().numpy()
        a = net.generate(101, seed_samples=[128], seed=11).cpu().numpy()
        b = net.continue_generation(83, int(a[-1]), seed=11).cpu().numpy()
        c = net.continue_generation(76, int(b[-1]), seed=11).cpu().numpy()
        assert a.shape == (102,) and b.shape == (83,) and c.shape == (76,)
        assert np.array_equal(whole, np.concatenate([a, b, c])), (multi, persist)
        assert whole.min() >= 0 and whole.max() < Q
        assert len(np.unique(whole)) > 8           # not stuck on one code
        runs.append(whole)
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


@pytest.mark.parametrize('n0', [2, 40, 150])
def test_prime_generator_from_forward_pass(pair, n0):
    """n0 below every dilation, between them, above the receptive field: the
    statements of tests/test_gpu_model.py::
    test_prime_generator_from_forward_pass."""
    net, var = pair
    rng = np.random.default_rng(n0)
    codes = rng.integers(0, Q, n0).astype(np.int32)
    nxt = int(rng.integers(0, Q))
    net.reset_generator()
    for c in codes:
        net.predict_proba_incremental(int(c))
    st_ref = net._gen['state'].clone()
    cur_ref = net._gen['cursors'].clone()
    p_ref = net.predict_proba_incremental(nxt, push=False).cpu().numpy()
    net.prime_generator(codes)
    assert torch.equal(net._gen['cursors'], cur_ref)
    assert (net._gen['state'] - st_ref).abs().max().item() < TOL
    p = net.predict_proba_incremental(nxt, push=False).cpu().numpy()
    assert np.abs(p - p_ref).max() < TOL
    gen = O.IncrementalGenerator(CFG, var, dtype=np.float64)
    for c in codes:
        gen.step(int(c))
    assert np.abs(p - np.asarray(gen.step(nxt)).reshape(-1)).max() < TOL


@pytest.mark.parametrize('B', [3, 33])
def test_batched_teacher_forced_streams_vs_float64_oracle(pair, B):
    """tests/test_gpu_fastgen_batch.py::test_teacher_forced_streams_vs_
    float64_oracle: more than two wraps of the longest ring, every step of
    every stream; 33 streams sit in two chain workgroups."""
    net, var = pair
    net.fastgen_graph_steps = 40
    n = 2 * max(DIL_GEN) + 40
    codes = np.random.default_rng(7).integers(0, Q, (B, n)).astype(np.int32)
    out, pr = net.generate_batch(0, list(range(11, 11 + B)), seed_samples=codes,
                                 return_proba_every=1)
    assert np.array_equal(out.cpu().numpy(), codes)
    pr = pr.cpu().numpy()
    assert pr.shape == (B, n - 1, Q)
    for b in range(B):
        gen = O.IncrementalGenerator(CFG, var, dtype=np.float64)
        ref = np.stack([np.asarray(gen.step(int(c))).reshape(-1)
                        for c in codes[b, :-1]])
        err = np.abs(pr[b] - ref).max(axis=1)
        assert err.max() < TOL, (b, int(err.argmax()), float(err.max()))


def test_streams_restarted_at_unaligned_steps(pair):
    """Three streams in calls of 37, 64 and 60 steps; stream 1 restarts with
    the second call (shared cursor 37), stream 2 with the third (101): every
    ring's cursor is then inside its ring.  The restarted streams are bit for
    bit their stand-alone generate_batch calls, stream 0 the one-call run."""
    net, _ = pair
    net.fastgen_graph_steps = 20
    seeds, seeds2, seeds3 = [11, 12, 13], [11, 52, 13], [11, 52, 93]
    first = [[7], [8], [9]]
    codes = lambda t: t.cpu().numpy()
    a = codes(net.generate_batch(37, seeds, seed_samples=first, temperature=0.9))
    last = a[:, -1].copy()
    last[1] = 40
    b = codes(net.continue_generation_batch(64, last, seeds2, temperature=0.9,
                                            restart=[1]))
    last = b[:, -1].copy()
    last[2] = 41
    c = codes(net.continue_generation_batch(60, last, seeds3, temperature=0.9,
                                            restart=[2]))
    alone = lambda n, seed, code: codes(net.generate_batch(
        n, [seed], seed_samples=[[code]], temperature=0.9))[0]
    s0 = alone(161, 11, 7)
    assert np.array_equal(s0, np.concatenate([a[0], b[0], c[0]]))
    s1 = alone(124, 52, 40)[1:]
    assert np.array_equal(b[1], s1[:64]) and np.array_equal(c[1], s1[64:])
    s2 = alone(60, 93, 41)[1:]
    assert np.array_equal(c[2], s2)
    # the stream that was not restarted in the third call went on
    assert np.array_equal(np.concatenate([a[2], b[2]]), alone(101, 13, 9))


def test_wide_cooperative_generator_equals_single_workgroup(hip_lib):
    """tests/test_gpu_model.py::test_wide_cooperative_generator_equals_single_
    workgroup on a 64-channel model with dilations [3, 5, 9]."""
    cfg = cfg_with(MID, batch_size=1, residual_channels=64, dilation_channels=56,
                   skip_channels=128, dilations=[3, 5, 9])
    net, var = build_pair(cfg)
    assert hip_lib.wn_fastgen_wide_coop_bytes(3, 64, 128, 256) > 0
    res = []
    for coop in (True, False):
        net.fastgen_wide_coop = coop
        net.reset_generator()
        o, p = net.generate(200, seed_samples=[128, 7, 250], seed=5, temperature=0.9,
                            return_proba_every=3)
        assert ('coop' in net._gen and net._gen['coop'] is not None) or not coop
        res.append((o.cpu().numpy(), p.cpu().numpy(), net._gen['state'].clone(),
                    net._gen['cursors'].clone()))
    assert np.array_equal(res[0][0], res[1][0])
    assert np.abs(res[0][1] - res[1][1]).max() < 1e-6
    assert torch.equal(res[0][3][:2], res[1][3][:2])
    scale = max(1.0, res[1][2].abs().max().item())
    assert (res[0][2] - res[1][2]).abs().max().item() < 1e-5 * scale
    # the cooperative launch against the float64 oracle, teacher-forced
    wave = np.random.default_rng(3).integers(0, 256, 60).astype(np.int32)
    gen = O.IncrementalGenerator(cfg, var, dtype=np.float64)
    ref = np.stack([np.asarray(gen.step(int(c))).reshape(-1) for c in wave[:-1]])
    net.fastgen_wide_coop = True
    out, pr = net.generate(0, seed_samples=wave, return_proba_every=1)
    assert np.array_equal(out.cpu().numpy(), wave)
    assert np.abs(pr.cpu().numpy() - ref).max() < TOL
    # a run continued on the other path
    net.fastgen_wide_coop = True
    more = net.continue_generation(50, int(res[1][0][-1]), 1.0, None, 6).cpu().numpy()
    assert more.shape == (50,) and more.min() >= 0 and more.max() < 256

