"""Batched fast generation (WaveNetModel.generate_batch /
continue_generation_batch, csrc/wn_fastgen_batch.hip) on the GPU: per-stream
probabilities against the float64 oracle (oracle.IncrementalGenerator),
every draw against the host restatement (tests/draw_ref.py), the default
stack against the single-stream path, bitwise batch invariance, priming,
chunking, isolation from the single-stream generator, and generate.py
--clips end to end."""
import glob
import json
import os
import sys

import numpy as np
import pytest
import torch

import draw_ref as D
from util import O, ROOT, cfg_with, build_pair

sys.path.insert(0, ROOT)
import generate  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5            # probabilities, float32 device path vs float64 oracle

# biases on, GC on, Q != 256, S != 512 (and neither a multiple of 16)
SMALL_GC = dict(batch_size=1, dilations=[1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
                filter_width=2, residual_channels=32, dilation_channels=32,
                skip_channels=100, quantization_channels=132, use_biases=True,
                global_condition_channels=8, global_condition_cardinality=10)
# biases off, no GC
SMALL_PLAIN = dict(batch_size=1, dilations=[1, 2, 4, 8, 16, 1, 2, 4, 8, 16],
                   filter_width=2, residual_channels=32, dilation_channels=32,
                   skip_channels=64, quantization_channels=256, use_biases=False)


def default_cfg(**kw):
    p = json.load(open(os.path.join(ROOT, 'wavenet_params.json')))
    c = {k: p[k] for k in p if k != 'sample_rate'}
    c['batch_size'] = 1
    c.update(kw)
    return c


def _codes(B, n, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, n)).astype(np.int32)


@pytest.fixture(scope='module')
def small_gc(hip_lib):
    net, var = build_pair(SMALL_GC)
    return net, var


@pytest.mark.parametrize('cfg', [SMALL_GC, SMALL_PLAIN], ids=['gc_biases', 'plain'])
def test_teacher_forced_streams_vs_float64_oracle(hip_lib, cfg):
    """B = 5 streams with different codes, GC ids and seeds, teacher-forced
    over more than two wraps of the longest ring: every step's probabilities
    of every stream equal one oracle generator per stream."""
    net, var = build_pair(cfg)
    net.fastgen_graph_steps = 40
    B, Q = 5, cfg['quantization_channels']
    n = 2 * max(cfg['dilations']) + 40
    codes = _codes(B, n, Q, 7)
    gc = 'global_condition_cardinality' in cfg
    ids = [2, 9, 0, 5, 2] if gc else None
    out, pr = net.generate_batch(0, [11, 12, 13, 14, 15], seed_samples=codes,
                                 global_condition=ids, return_proba_every=1)
    assert np.array_equal(out.cpu().numpy(), codes)
    pr = pr.cpu().numpy()
    assert pr.shape == (B, n - 1, Q)
    for b in range(B):
        gen = O.IncrementalGenerator(cfg, var, dtype=np.float64)
        gid = None if ids is None else np.array([ids[b]])
        ref = np.stack([gen.step(int(c), gid) for c in codes[b, :-1]])
        err = np.abs(pr[b] - ref).max(axis=1)
        assert err.max() < TOL, (b, int(err.argmax()), float(err.max()))


@pytest.fixture(scope='module', params=['plain', 'gc'])
def default_run(request, hip_lib):
    """Default stack (L = 50, S = 512, Q = 256), +- GC 32 x 377: B = 32
    streams free-running 2000 steps from Q // 2 with per-step
    probabilities."""
    gc = request.param == 'gc'
    cfg = default_cfg(**(dict(global_condition_channels=32,
                              global_condition_cardinality=377) if gc else {}))
    net, var = build_pair(cfg)
    B, N = 32, 2000
    seeds = [1000 + 7 * b for b in range(B)]
    ids = [(11 * b) % 377 for b in range(B)] if gc else None
    out, pr = net.generate_batch(N, seeds, global_condition=ids,
                                 return_proba_every=1)
    return net, seeds, ids, out.cpu().numpy(), pr.cpu().numpy()


def test_default_stack_draws_match_restatement(default_run):
    _, seeds, _, codes, pr = default_run
    assert codes.shape == (32, 2001) and pr.shape == (32, 2000, 256)
    assert (codes[:, 0] == 128).all()
    for b, s in enumerate(seeds):
        D.check_draws(codes[b, 1:], pr[b], 1.0, s, np.arange(2000),
                      what='stream %d' % b)
    # the streams are different random processes
    assert len({codes[b].tobytes() for b in range(32)}) == 32


def test_default_stack_equals_single_stream_path(default_run):
    """Teacher-forcing the (oracle-pinned) single-stream generate with a
    stream's own codes reproduces its probabilities."""
    net, _, ids, codes, pr = default_run
    for b in (0, 17, 31):
        _, p1 = net.generate(0, seed_samples=codes[b], return_proba_every=1,
                             global_condition=None if ids is None else ids[b])
        err = np.abs(p1.cpu().numpy() - pr[b]).max(axis=1)
        assert err.max() < TOL, (b, int(err.argmax()), float(err.max()))


def test_batch_invariance_bitwise(small_gc):
    """Stream k of a B = 37 batch (a partial second tile) equals the same
    stream run alone, bit for bit, and permuting the streams permutes the
    outputs."""
    net, _ = small_gc
    B, Q = 37, SMALL_GC['quantization_channels']
    rng = np.random.default_rng(5)
    seeds = [int(v) for v in rng.integers(0, 2**62, B)]
    seeds[3] = 2**64 - 5                          # a seed above 2**63
    codes = _codes(B, 20, Q, 9)
    ids = [int(v) for v in rng.integers(0, 10, B)]
    out, pr = net.generate_batch(150, seeds, seed_samples=codes,
                                 global_condition=ids, return_proba_every=1,
                                 temperature=0.9)
    out, pr = out.cpu().numpy(), pr.cpu().numpy()
    for k in (0, 3, 31, 32, 36):
        o1, p1 = net.generate_batch(150, [seeds[k]], seed_samples=codes[k:k + 1],
                                    global_condition=ids[k], return_proba_every=1,
                                    temperature=0.9)
        assert np.array_equal(o1.cpu().numpy()[0], out[k]), k
        assert np.array_equal(p1.cpu().numpy()[0], pr[k]), k
    perm = rng.permutation(B)
    o2, p2 = net.generate_batch(150, [seeds[i] for i in perm],
                                seed_samples=codes[perm],
                                global_condition=[ids[i] for i in perm],
                                return_proba_every=1, temperature=0.9)
    assert np.array_equal(o2.cpu().numpy(), out[perm])
    assert np.array_equal(p2.cpu().numpy(), pr[perm])
    # the draws follow the restatement at this temperature too
    tau = float(np.float32(0.9))
    for b in (0, 3, 36):
        D.check_draws(out[b, 20:], pr[b, 19:], tau, seeds[b], np.arange(19, 169),
                      what='stream %d' % b)


def test_forward_priming_equals_teacher_forced(small_gc):
    """A seed longer than fastgen_prime_forward_min, primed by the forward
    pass, leaves the queues where the teacher-forced steps do."""
    net, _ = small_gc
    B, Q = 5, SMALL_GC['quantization_channels']
    n_seed = 150
    assert n_seed - 1 >= net.fastgen_prime_forward_min
    codes = _codes(B, n_seed, Q, 21)
    seeds, ids = [3, 1, 4, 1, 5], [0, 3, 6, 9, 2]
    runs = []
    default_min = net.fastgen_prime_forward_min
    for prime_min in (default_min, 10 ** 9):     # forward pass; teacher-forced
        net.fastgen_prime_forward_min = prime_min
        try:
            a = net.generate_batch(1, seeds, seed_samples=codes,
                                   global_condition=ids).cpu().numpy()
            more, p = net.continue_generation_batch(60, a[:, -1], seeds,
                                                    global_condition=ids,
                                                    return_proba_every=1)
        finally:
            net.fastgen_prime_forward_min = default_min
        runs.append((a, more.cpu().numpy(), p.cpu().numpy()))
    (a0, m0, p0), (a1, m1, p1) = runs
    assert np.array_equal(a0[:, :n_seed], codes)
    assert np.array_equal(a0, a1) and np.array_equal(m0, m1)
    assert np.abs(p0 - p1).max() < TOL


def test_forward_primed_streams_batch_invariant_bitwise(small_gc):
    """The forward-pass priming route (long seeds, return_proba_every = 0):
    stream k of a B = 37 batch with distinct seeds and GC ids is bit for bit
    the same stream run alone, in codes and in the probabilities of the steps
    after it; a seed shared by every stream primes every stream alike."""
    net, _ = small_gc
    B, Q, n_seed = 37, SMALL_GC['quantization_channels'], 100
    assert n_seed - 1 >= net.fastgen_prime_forward_min
    rng = np.random.default_rng(31)
    seeds = [int(v) for v in rng.integers(0, 2**62, B)]
    codes = _codes(B, n_seed, Q, 33)
    ids = [int(v) for v in rng.integers(0, 10, B)]

    def run(sel, rows):
        a = net.generate_batch(20, [seeds[i] for i in sel], seed_samples=rows,
                               global_condition=[ids[i] for i in sel])
        a = a.cpu().numpy()
        m, p = net.continue_generation_batch(
            25, a[:, -1], [seeds[i] for i in sel],
            global_condition=[ids[i] for i in sel], return_proba_every=1)
        return np.concatenate([a, m.cpu().numpy()], axis=1), p.cpu().numpy()
    out, pr = run(range(B), codes)
    for k in (0, 31, 32, 36):
        o1, p1 = run([k], codes[k:k + 1])
        assert np.array_equal(o1[0], out[k]), k
        assert np.array_equal(p1[0], pr[k]), k
    # one seed shared by all streams (generate.py --clips): stream k as alone
    shared, _ = run(range(B), codes[5])
    o1, _ = run([36], codes[5])
    assert np.array_equal(shared[36], o1[0])


def test_chunked_equals_single_call(small_gc):
    net, _ = small_gc
    net.fastgen_graph_steps = 40
    seeds, ids = [7, 8, 9], 4
    a = net.generate_batch(200, seeds, seed_samples=[7, 9],
                           global_condition=ids).cpu().numpy()
    b1 = net.generate_batch(80, seeds, seed_samples=[7, 9],
                            global_condition=ids).cpu().numpy()
    b2 = net.continue_generation_batch(70, b1[:, -1], seeds,
                                       global_condition=ids).cpu().numpy()
    b3 = net.continue_generation_batch(50, b2[:, -1], seeds,
                                       global_condition=ids).cpu().numpy()
    assert np.array_equal(a, np.concatenate([b1, b2, b3], axis=1))


def test_batched_and_single_stream_generators_are_isolated(small_gc):
    net, _ = small_gc
    # single-stream: generate + continue, with and without a batched call
    # in between
    s = net.generate(60, seed_samples=[5, 6], seed=3, global_condition=1)
    ref = net.continue_generation(40, int(s[-1]), 1.0, 1, 3).cpu().numpy()
    s = net.generate(60, seed_samples=[5, 6], seed=3, global_condition=1)
    net.generate_batch(30, [1, 2, 3], global_condition=[4, 5, 6])
    got = net.continue_generation(40, int(s[-1]), 1.0, 1, 3).cpu().numpy()
    assert np.array_equal(ref, got)
    # batched: the same with a single-stream call in between
    b = net.generate_batch(60, [1, 2], global_condition=[7, 8]).cpu().numpy()
    ref = net.continue_generation_batch(40, b[:, -1], [1, 2],
                                        global_condition=[7, 8]).cpu().numpy()
    b = net.generate_batch(60, [1, 2], global_condition=[7, 8]).cpu().numpy()
    net.generate(30, seed_samples=[9], seed=5, global_condition=2)
    got = net.continue_generation_batch(40, b[:, -1], [1, 2],
                                        global_condition=[7, 8]).cpu().numpy()
    assert np.array_equal(ref, got)


def test_generate_cli_clips_with_gc_ids(hip_lib, tmp_path):
    from scipy.io import wavfile
    from wavenet import WaveNetModel
    params = {k: SMALL_GC[k] for k in ('dilations', 'filter_width',
                                       'residual_channels', 'dilation_channels',
                                       'quantization_channels', 'skip_channels',
                                       'use_biases')}
    params.update(sample_rate=16000, scalar_input=False, initial_filter_width=32)
    pj = str(tmp_path / 'params.json')
    json.dump(params, open(pj, 'w'))
    net = WaveNetModel(batch_size=1, global_condition_channels=8,
                       global_condition_cardinality=10, seed=2,
                       **{k: params[k] for k in params if k != 'sample_rate'})
    ck = str(tmp_path / 'model.ckpt-1')
    torch.save({'variables': net.state_dict()}, ck)
    wav = str(tmp_path / 'clip.wav')
    logdir = str(tmp_path / 'gen')
    assert generate.main([ck, '--samples', '90', '--wavenet_params', pj,
                          '--wav_out_path', wav, '--save_every', '40',
                          '--gc_channels', '8', '--gc_cardinality', '10',
                          '--gc_ids', '1,4,7', '--seed', '5',
                          '--logdir', logdir]) == 0
    for i in range(3):
        rate, data = wavfile.read(str(tmp_path / ('clip_%d.wav' % i)))
        assert rate == 16000 and data.shape == (91,) and np.abs(data).max() <= 1
    assert not os.path.exists(wav)
    saved = glob.glob(os.path.join(logdir, 'generate', '*', 'generated_codes.npy'))
    assert len(saved) == 1
    codes = np.load(saved[0])
    assert codes.shape == (3, 91) and codes.dtype == np.int32
    # clip i is stream i of generate_batch with seed 5 + i and gc id i
    ref = net.generate_batch(90, [5, 6, 7], seed_samples=codes[0, :1],
                             global_condition=[1, 4, 7]).cpu().numpy()
    assert np.array_equal(codes, ref)
