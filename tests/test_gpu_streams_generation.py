"""Fast generation under a stalled stream that is not the default stream
(tests/stall.py): every launch of a call -- the ones before and after a
hipGraph capture included -- takes the current stream, graphs captured under
one stream replay under another, and the codes and probabilities equal those
of the same calls on the default stream bit for bit (tests/test_gpu_draw.py
ties those to float64).

A generation call ends on the host (it stages its control words from a host
array and reads the expired-wait word back), so it waits for its stream by
design: the precondition -- the stall is pending -- is taken when the call
starts, and every call of a scenario gets a stall of its own.  A call that
warns about an expired hand-over wait fails its case: under a stall on its
own stream nothing competes for residency.

THROUGH_HOST names, for every entry of the fast-generation family, the
scenario that runs it; the scenario asserts (stall.spy) that the entry ran,
with the stalled stream's handle and never with the default stream's."""
import contextlib
import warnings

import numpy as np
import pytest
import torch

import stall
from util import MID, cfg_with, build_pair

pytestmark = pytest.mark.gpu

N = 65                # samples: with graphs of 20 one call replays graphs of
GRAPH = 20            # 20, graphs of 2 and runs single steps (_replay_steps)
TRUNC = dict(top_k=5, top_p=0.9)


class _On(object):
    """Where a scenario's calls run: the default stream (the reference), or
    stream i of `streams`, stalled when the call starts."""

    def __init__(self, streams=None, ms=None):
        self.streams, self.ms, self.held = streams, ms, []

    @contextlib.contextmanager
    def __call__(self, i=0):
        if self.streams is None:
            yield
            return
        s = self.streams[i]
        with torch.cuda.stream(s):
            st = stall.Stall(s, self.ms)
            self.held.append(st.pending())
            yield


def _mid(**sw):
    net, _ = build_pair(cfg_with(MID, batch_size=1))
    net.fastgen_graph_steps = GRAPH
    for k, v in sw.items():
        assert hasattr(net, k), k
        setattr(net, k, v)
    return net


def _wide(coop):
    net, _ = build_pair(cfg_with(MID, batch_size=1, residual_channels=64,
                                 dilation_channels=56, skip_channels=128))
    net.fastgen_wide_coop = coop
    return net


def _lc_net(path):
    from test_gpu_synthesis import DIL10, _model
    net = _model(5, DIL10, gc=7)
    net.fastgen_graph_steps = GRAPH
    net.fastgen_multi_cu = path != 'single'
    net.fastgen_persistent = path == 'persist'
    return net


def _rows(*shape):
    return np.random.default_rng(sum(shape)).standard_normal(shape) \
        .astype(np.float32)


# ---- scenarios: fn(on) -> tensors to compare ------------------------------
def s_persistent(on):
    net = _mid(fastgen_multi_cu=True, fastgen_persistent=True)
    with on():
        a, p = net.generate(N, seed_samples=[128], seed=11,
                            return_proba_every=4)
    assert not net._gen_launch_failed
    return [a, p]


def s_steps(on):
    """the step kernels: a capture under a stream that is not the default
    stream, then a second call on another stream that replays its graphs"""
    net = _mid(fastgen_multi_cu=True, fastgen_persistent=False)
    with on(0):
        a, p = net.generate(N, seed_samples=[128], seed=11,
                            return_proba_every=4)
    graphs = dict(net._gen['graphs'])
    assert sorted(k[1] for k in graphs) == [GRAPH // 10, GRAPH]
    with on(1):
        b, q = net.generate(N, seed_samples=[128], seed=12, temperature=0.8,
                            return_proba_every=4)
    assert dict(net._gen['graphs']) == graphs          # replayed, not captured
    return [a, p, b, q]


def s_one_workgroup(on):
    net = _mid(fastgen_multi_cu=False)
    with on():
        a, p = net.generate(N, seed_samples=[128], seed=11,
                            return_proba_every=4)
    with on():
        b = net.generate(N, seed_samples=[3, 200], seed=4, temperature=0.7,
                         **TRUNC)
    return [a, p, b]


def _s_wide(on, coop):
    net = _wide(coop)
    with on():
        a, p = net.generate(N, seed_samples=[128, 7, 250], seed=5,
                            temperature=0.9, return_proba_every=3)
    assert (net._gen.get('coop') is not None) == coop
    with on():
        b = net.generate(N, seed_samples=[128], seed=6, **TRUNC)
    assert not net._gen_launch_failed
    return [a, p, b]


def s_wide_single(on):
    return _s_wide(on, False)


def s_wide_cooperative(on):
    return _s_wide(on, True)


def s_prime_continue(on):
    net = _mid()
    codes = np.random.default_rng(40).integers(0, 256, 40).astype(np.int32)
    with on():
        net.prime_generator(codes)
        state = net._gen['state'].clone()
    with on():
        more = net.continue_generation(30, 7, 1.0, None, 6)
    out = [state, more]
    for c in (5, 250, 17):
        with on():
            out.append(net.predict_proba_incremental(c))
    with on():
        out.append(net.predict_proba_incremental(9, push=False))
    return out


def s_batch(on):
    """generate_batch with B = 3, then a continuation that restarts stream 1
    (tests/test_gpu_synthesis_queue.py's smallest case, without LC)"""
    from test_gpu_synthesis import DIL10, _model
    net = _model(None, DIL10)
    net.fastgen_graph_steps = GRAPH
    with on():
        a, p = net.generate_batch(45, [5, 6, 7], seed_samples=[[7], [8], [9]],
                                  temperature=0.9, return_proba_every=4)
        last = a[:, -1].cpu().numpy().copy()      # (read on a's stream)
    last[1] = 40
    with on():
        b = net.continue_generation_batch(23, last, [5, 56, 7],
                                          temperature=0.9, restart=[1])
    return [a, p, b]


def s_batch_stages(on):
    """a batched step one launch at a time (wn_fastgen_batch_stages, what
    tools/fastgen_batch_stages.py times): the codes of generate_batch"""
    from wavenet import _lib, fastgen
    from test_gpu_synthesis import DIL10, _model
    net = _model(None, DIL10)
    B, n = 3, 12
    seeds = np.asarray([2, 3, 4], np.int64)
    io = torch.full((B, n + 1), net.Q // 2, dtype=torch.int32,
                    device=net.device)
    with on():
        g = fastgen.batch_generator(net, B)
        fastgen.batch_reset(net, g)
        prep = fastgen.batch_prepare(net, g, io, 1, n, 1.0, seeds, None, 1,
                                     None)
        for _ in range(n):
            for k in range(5):
                _lib.call('wn_fastgen_batch_stages', k, k + 1, *prep['args'],
                          _lib.stream())
        fastgen.batch_complete(net, g, prep, io, None, n)
        io = io.clone()
    with on():
        ref = net.generate_batch(n, [2, 3, 4])
        same = torch.equal(io, ref)
    assert same
    return [io]


def _s_lc(on, path):
    net = _lc_net(path)
    lc = _rows(N + 1, 5)
    with on():
        a, p = net.generate(N, seed_samples=[3, 5], seed=11, temperature=0.9,
                            global_condition=3, return_proba_every=4,
                            local_condition=lc)
    out = [a, p]
    if path == 'single':
        with on():
            out.append(net.generate(N, seed_samples=[3, 5], seed=12,
                                    global_condition=2, local_condition=lc,
                                    **TRUNC))
    assert not net._gen_launch_failed
    return out


def s_lc_single(on):
    return _s_lc(on, 'single')


def s_lc_steps(on):
    return _s_lc(on, 'steps')


def s_lc_persistent(on):
    return _s_lc(on, 'persist')


def s_lc_batch(on):
    net = _lc_net('steps')
    B, n0, n1 = 3, 25, 23
    lc0 = _rows(B, n0, 5)
    rows = [torch.from_numpy(_rows(60 + b, 5)).cuda() for b in range(B)]
    torch.cuda.synchronize()
    with on():
        a = net.generate_batch(n0, [5, 6, 7], seed_samples=[[7], [8], [9]],
                               global_condition=[0, 1, 2], temperature=0.9,
                               local_condition=lc0)
        last = a[:, -1].cpu().numpy().copy()      # (read on a's stream)
    last[1] = 40
    with on():
        lc1 = net.batch_local_condition(
            [(rows[0], 0), (rows[1], n0), None], n0, n1)
    with on():
        b = net.continue_generation_batch(
            n1, last, [5, 56, 7], global_condition=[0, 6, 2], temperature=0.9,
            local_condition=lc1, restart=[1])
    return [a, lc1, b]


def _fg(names):
    return set('wn_fastgen_' + n for n in names.split())


# scenario -> the entries it must run
SCENARIOS = {
    'persistent': (s_persistent, _fg('init pack pre persist')),
    'steps_two_streams': (s_steps, _fg('init pack pre step finish')),
    'one_workgroup': (s_one_workgroup, _fg('init run run_trunc')),
    'wide_single': (s_wide_single, _fg('run_wide run_wide_trunc')),
    'wide_cooperative': (s_wide_cooperative, _fg('run_wide run_wide_trunc')),
    'prime_continue': (s_prime_continue, _fg('init')),
    'batch': (s_batch, _fg('batch_init batch_pre batch_step batch_finish '
                           'batch_restart batch_step_q batch_finish_q')),
    'batch_stages': (s_batch_stages, _fg('batch_stages')),
    'lc_single': (s_lc_single, _fg('lc_bias run_lc run_lc_trunc')),
    'lc_steps': (s_lc_steps, _fg('lc_bias pre_lc step_lc')),
    'lc_persistent': (s_lc_persistent, _fg('lc_bias persist_lc')),
    'lc_batch': (s_lc_batch, _fg('batch_pre_lc batch_step_lc '
                                 'batch_step_lc_q batch_lc_rows')),
}
# the persistent launches really ran: not one step kernel beside them
WITHOUT = {'persistent': _fg('step'), 'lc_persistent': _fg('step_lc')}
THROUGH_HOST = {e: 'test_generation_on_a_stalled_stream[%s]' % name
                for name, (_, entries) in sorted(SCENARIOS.items())
                for e in sorted(entries) if e.startswith('wn_fastgen_')}


def _run(fn, on):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        out = fn(on)
        torch.cuda.synchronize()
    expired = [str(w.message) for w in caught if 'expired' in str(w.message)]
    assert not expired, expired
    return [stall.bits(t) for t in out]


@pytest.mark.parametrize('name', sorted(SCENARIOS))
def test_generation_on_a_stalled_stream(hip_lib, name):
    fn, entries = SCENARIOS[name]
    ref = _run(fn, _On())
    again = _run(fn, _On())
    for a, b in zip(ref, again):
        assert torch.equal(a, b), name + ': two default-stream runs differ'
    default = torch.cuda.default_stream()
    s1 = stall.concurrent_stream(default)
    s2 = stall.concurrent_stream(default, s1)
    ours = {s1.cuda_stream, s2.cuda_stream}

    def attempt(ms):
        on = _On((s1, s2), ms)
        with stall.spy(hip_lib) as seen:
            got = _run(fn, on)
        print('%s ran: %s' % (name, ' '.join(sorted(seen))))
        assert entries <= set(seen), sorted(entries - set(seen))
        assert not WITHOUT.get(name, set()) & set(seen), sorted(seen)
        for e, handles in seen.items():
            assert default.cuda_stream not in handles, (e, handles)
            # (a capture runs on a stream of its own)
            assert handles & ours, (e, handles, ours)
        assert len(got) == len(ref)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert g.shape == r.shape and torch.equal(g, r), \
                '%s: result %d differs from the default-stream run' % (name, i)
        return bool(on.held) and all(on.held)
    stall.first_rung(attempt)
