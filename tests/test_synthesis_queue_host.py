"""The restart queue of bulk synthesis without a GPU: plan_queue against the
heap restatement of tests/queue_ref.py and pinned plans, synthesize(schedule=
'queue') on the fake model of queue_ref (every item's codes equal its
stand-alone process), argument errors before the library is touched, the
new entry points' argument checks and declarations, and the command lines'
--synthesis_schedule checks."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import queue_ref as QR
from util import ROOT

LENGTHS = [1, 2, 37, 150, 64, 150, 9]
LENGTHS_UP = [45, 1, 131, 8, 70, 23]
NEW = ('wn_fastgen_batch_step_q', 'wn_fastgen_batch_step_lc_q',
       'wn_fastgen_batch_finish_q', 'wn_fastgen_batch_restart',
       'wn_fastgen_batch_lc_rows')


# ---------------------------------------------------------------- plan_queue
@pytest.mark.parametrize('seed', range(40))
def test_plan_queue_matches_restatement_and_invariants(seed):
    from wavenet import synthesis
    rng = np.random.default_rng(seed)
    U, batch = int(rng.integers(1, 41)), int(rng.integers(1, 13))
    q = 1 if seed % 2 else int(rng.integers(1, 31))
    n = rng.integers(1, 201, size=U)
    plan = synthesis.plan_queue(n, batch, q)
    slot, start, segments, steps, occ = QR.plan_queue(n, batch, q)
    assert (list(plan.slot), list(plan.start)) == (slot, start)
    assert list(plan.segments) == segments and plan.steps == steps
    assert plan.occupancy == occ == n.sum() / float(batch * steps)
    # every item once, in a slot of the batch, at a multiple of the quantum
    assert len(plan.slot) == len(plan.start) == U
    assert all(0 <= s < batch for s in plan.slot)
    assert all(t >= 0 and t % q == 0 for t in plan.start)
    assert steps == max(t + int(m) for t, m in zip(plan.start, n))
    # no two items of a slot overlap
    for s in range(batch):
        spans = sorted((plan.start[u], plan.start[u] + int(n[u]))
                       for u in range(U) if plan.slot[u] == s)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    # the segments tile [0, steps) and cut at every start time
    assert segments[0][0] == 0 and sum(m for _, m in segments) == steps
    assert all(m >= 1 for _, m in segments)
    assert [a for a, _ in segments] == sorted(set(plan.start))
    # (larger quanta can lose against the rounds: not asserted there)
    if q == 1:
        assert steps <= synthesis.plan_rounds(n, batch).steps


def test_plan_queue_pinned_plans():
    from wavenet import synthesis
    p = synthesis.plan_queue(LENGTHS, 3)
    assert [a for a, _ in p.segments] == [0, 64, 101, 110, 112]
    assert p.segments[-1] == (112, 38)
    assert p.steps == 150 and p.occupancy == 413 / 450.0
    assert synthesis.plan_rounds(LENGTHS, 3).steps == 188
    # items 2, 6, 1, 0 follow item 4 in slot 2
    assert list(p.slot) == [2, 2, 2, 0, 2, 1, 2]
    assert list(p.start) == [112, 110, 64, 0, 0, 0, 101]
    assert synthesis.plan_queue(LENGTHS, 3, 20).steps == 161
    assert synthesis.plan_queue(LENGTHS, 3, quantum=20).start == \
        [160, 140, 80, 0, 0, 0, 120]
    assert synthesis.plan_queue(LENGTHS_UP, 4).steps == 131
    assert synthesis.plan_rounds(LENGTHS_UP, 4).steps == 139
    # one slot: the items back to back; batch >= items: one segment
    assert synthesis.plan_queue([3, 7, 1], 1).start == [7, 0, 10]
    assert synthesis.plan_queue([3, 7, 1], 8).segments == [(0, 7)]
    assert synthesis.plan_queue([3, 7, 1], 8).occupancy == 11 / 56.0


def test_plan_queue_the_committed_measurement_list():
    """The list of profiles/synthesis_time.txt: 25572 steps in rounds, 19903
    in the queue."""
    from wavenet import synthesis
    n = np.random.default_rng(0).integers(2000, 16001, 64)
    assert synthesis.plan_rounds(n, 32).steps == 25572
    assert synthesis.plan_queue(n, 32).steps == 19903


@pytest.mark.parametrize('lengths, batch, quantum', [
    ([], 4, 1), ([3, 0], 4, 1), ([3.5], 4, 1), ([3], 0, 1), ([3], 257, 1),
    ([3], 2, 0), ([3], 2, -1), ([3], 2, 1.5), ([3], 2, True)])
def test_plan_queue_refuses(lengths, batch, quantum):
    from wavenet import synthesis
    with pytest.raises(ValueError):
        synthesis.plan_queue(lengths, batch, quantum)


# ------------------------------------------------- synthesize on a fake model
@pytest.fixture
def no_library(monkeypatch):
    """The queue's host logic runs on the fake model: the library and the
    device checks are stubbed."""
    from wavenet import _lib
    monkeypatch.setattr(_lib, 'load', lambda: None)
    monkeypatch.setattr(_lib, 'require_gpu', lambda: None)


def _int_rows(rng, n, Lc, extra=3):
    """Small-integer rows, longer than the item and NaN from row n - 1 on."""
    r = rng.integers(-4, 5, (n + extra, Lc)).astype(np.float32)
    r[n - 1:] = np.nan
    return r


@pytest.mark.parametrize('quantum', [1, 20, None, 7])
@pytest.mark.parametrize('batch', [1, 3, 7, 12])
def test_queue_on_fake_rows_model(no_library, batch, quantum):
    from wavenet import synthesis
    net = QR.FakeNet(Q=64, Lc=5)
    rng = np.random.default_rng(3)
    U = len(LENGTHS)
    rows = [_int_rows(rng, n, 5) for n in LENGTHS]
    seeds = [100 + 3 * u for u in range(U)]
    first = [int(v) for v in rng.integers(0, 64, U)]
    gc = [6, 0, 3, 1, 5, 2, 4]
    syn = synthesis.synthesize(net, LENGTHS, seeds=seeds, batch=batch,
                               first_samples=first, global_condition=gc,
                               local_condition=rows, schedule='queue',
                               quantum=quantum)
    q = 2 if quantum is None else quantum      # fastgen_graph_steps // 10
    plan = QR.plan_queue(LENGTHS, batch, q)
    assert syn.rounds == synthesis.plan_rounds(LENGTHS, batch).rounds
    assert (syn.steps, syn.occupancy) == (plan[3], plan[4])
    for u, n in enumerate(LENGTHS):
        want = QR.alone(64, n, seeds[u], first[u], gc[u], rows[u])
        got = syn.codes[u].numpy()
        assert got.dtype == np.int32 and got.shape == (n,)
        assert (got == want).all(), u
    # one start, then one continuation per further segment, each restarting
    # exactly the slots admitted at its first step
    assert [c[0] for c in net.log] == ['generate_batch'] + \
        ['continue_generation_batch'] * (len(plan[2]) - 1)
    assert [(c[1], c[2]) for c in net.log] == plan[2]
    for name, a, _, restart in net.log[1:]:
        assert restart == sorted(plan[0][u] for u in range(U)
                                 if plan[1][u] == a)
    assert net.reserve == max(m for _, m in plan[2])


def test_queue_on_fake_upsampler_and_plain_models(no_library):
    from wavenet import synthesis
    rng = np.random.default_rng(8)
    net = QR.FakeNet(Q=32, Lc=6, hop=8)
    frames = [rng.integers(-3, 4, (-(-n // 8) + (2 if n == 70 else 0), 6)
                           ).astype(np.float32) for n in LENGTHS_UP]
    seeds = [7 * u + 1 for u in range(len(LENGTHS_UP))]
    syn = synthesis.synthesize(net, LENGTHS_UP, seeds=seeds, batch=4,
                               frames=frames, schedule='queue', quantum=1)
    assert syn.steps == 131 and syn.rounds == [[2, 4, 0, 5], [3, 1]]
    for u, n in enumerate(LENGTHS_UP):
        want = QR.alone(32, n, seeds[u], 16, None,
                        QR.upsample(frames[u], n, 8))
        assert (syn.codes[u].numpy() == want).all(), u
    # no LC; batch >= items: one call, no admission
    plain = QR.FakeNet(Q=32)
    syn = synthesis.synthesize(plain, [30, 1, 77, 12, 77], batch=8,
                               seeds=[5, 6, 7, 8, 9], schedule='queue')
    assert plain.log == [('generate_batch', 0, 77, None)]
    for u, n in enumerate([30, 1, 77, 12, 77]):
        assert (syn.codes[u].numpy() ==
                QR.alone(32, n, 5 + u, 16, None, None)).all()


def test_queue_memory_cap_is_per_segment(no_library):
    from wavenet import synthesis
    net = QR.FakeNet(Q=32, Lc=5)
    lengths = [1000, 3, 400]
    rows = [np.zeros((n, 5), np.float32) for n in lengths]
    # 2 streams; segments (0, 400), (400, 600): 2 x 600 x 5 x 4 = 24000 bytes
    kw = dict(seeds=[1, 2, 3], batch=2, local_condition=rows,
              schedule='queue', quantum=1)
    with pytest.raises(ValueError, match='24000 bytes.*23999'):
        synthesis.synthesize(net, lengths, max_round_bytes=23999, **kw)
    assert net.log == []
    synthesis.synthesize(net, lengths, max_round_bytes=24000, **kw)


# ------------------------------------------------------------ argument errors
@pytest.fixture
def untouchable(monkeypatch):
    from wavenet import WaveNetModel, _lib
    net = WaveNetModel(batch_size=1, dilations=[1, 2, 4, 8], filter_width=2,
                       residual_channels=32, dilation_channels=32,
                       skip_channels=64, quantization_channels=256,
                       use_biases=True, device='cpu')
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'call',
                        lambda *a: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    return net


@pytest.mark.parametrize('kw, what', [
    (dict(schedule='greedy'), 'schedule'),
    (dict(schedule=None), 'schedule'),
    (dict(schedule='queue', quantum=0), 'quantum'),
    (dict(schedule='queue', quantum=-3), 'quantum'),
    (dict(schedule='queue', quantum=2.0), 'quantum'),
    (dict(quantum=0), 'quantum'),
])
def test_synthesize_refuses_schedule_and_quantum(untouchable, kw, what):
    from wavenet import synthesis
    with pytest.raises(ValueError, match=what):
        synthesis.synthesize(untouchable, [4, 3], seeds=[1, 2], **kw)


@pytest.mark.parametrize('restart', [[3], [-1], [0, 0], [0.5], [True], 'ab',
                                     [[0]], 1])
def test_continue_refuses_bad_restart(untouchable, restart):
    with pytest.raises(ValueError, match='restart'):
        untouchable.continue_generation_batch(4, [1, 2, 3], [7, 8, 9],
                                              restart=restart)


def test_new_arguments_are_keyword_only():
    from wavenet import WaveNetModel, synthesis
    p = inspect.signature(WaveNetModel.continue_generation_batch).parameters
    assert p['restart'].kind is inspect.Parameter.KEYWORD_ONLY
    assert p['restart'].default is None
    p = inspect.signature(synthesis.synthesize).parameters
    for name, default in (('schedule', 'rounds'), ('quantum', None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY
        assert p[name].default == default
    assert synthesis.Synthesis._fields == ('codes', 'rounds', 'steps',
                                           'occupancy')
    assert synthesis.QueuePlan._fields == ('slot', 'start', 'segments',
                                           'steps', 'occupancy')


# ------------------------------------------------------------------------ ABI
def test_new_entries_are_declared_and_bound(hip_lib):
    from wavenet import _lib
    src = open(os.path.join(ROOT, 'include', 'wavenet_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    for name in NEW:
        assert re.search(r'\bint %s\s*\(' % name, src), name
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name)
    # the _q entries: the plain entry's arguments, origins, the stream
    for name in NEW[:3]:
        res, args = _lib.SIGNATURES[name]
        pres, pargs = _lib.SIGNATURES[name[:-2]]
        assert res is pres and args == pargs[:-1] + [_lib.P, _lib.P]


def test_new_entries_check_arguments_without_a_device(hip_lib):
    """All of these return before any launch."""
    lib = hip_lib
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def step(name, origins, L=4, S=64, Q=64, B=2, lc=()):
        return getattr(lib, name)(a, a, 0, a, None, a, None, a, None, None, 0,
                                  a, L, S, Q, B, a, a, a, a, a, a, None, 1, a,
                                  a, a, a, a, *lc, origins, None)
    for name, lc in (('wn_fastgen_batch_step_q', ()),
                     ('wn_fastgen_batch_step_lc_q', (a, 5, 64))):
        assert step(name, None, lc=lc) == -5            # no origins
        assert step(name, a, L=0, lc=lc) == -1
        assert step(name, a, B=0, lc=lc) == -1
        assert step(name, a, B=257, lc=lc) == -2
        assert step(name, a, S=600, lc=lc) == -2
    assert step('wn_fastgen_batch_step_lc_q', a, lc=(None, 5, 64)) == -5
    assert step('wn_fastgen_batch_step_lc_q', a, lc=(a, 0, 64)) == -1
    fin = lib.wn_fastgen_batch_finish_q
    assert fin(64, 2, a, a, a, a, None, a, None, None) == -5
    assert fin(64, 2, None, a, a, a, None, a, a, None) == -5
    assert fin(0, 2, a, a, a, a, None, a, a, None) == -1
    assert fin(600, 2, a, a, a, a, None, a, a, None) == -2
    assert fin(64, 0, a, a, a, a, None, a, a, None) == -1
    assert fin(64, 257, a, a, a, a, None, a, a, None) == -2
    rs = lib.wn_fastgen_batch_restart
    for i in (0, 1, 4, 5, 6, 7):
        args = [a, a, 4, 2, a, a, a, a, None]
        args[i] = None
        assert rs(*args) == -5, i
    assert rs(a, a, 0, 2, a, a, a, a, None) == -1
    assert rs(a, a, 65, 2, a, a, a, a, None) == -2
    assert rs(a, a, 4, 0, a, a, a, a, None) == -1
    assert rs(a, a, 4, 257, a, a, a, a, None) == -2
    rows = lib.wn_fastgen_batch_lc_rows
    assert rows(None, 2, 3, 5, 0, a, None) == -5
    assert rows(a, 2, 3, 5, 0, None, None) == -5
    assert rows(a, 0, 3, 5, 0, a, None) == -1
    assert rows(a, 257, 3, 5, 0, a, None) == -2
    assert rows(a, 2, 0, 5, 0, a, None) == -1
    assert rows(a, 2, 3, 0, 0, a, None) == -1
    assert rows(a, 2, 3, 5, -1, a, None) == -1


# --------------------------------------------------------------- command line
def _error_of(script, argv):
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stderr.decode()


@pytest.mark.parametrize('script, argv, what', [
    ('evaluate.py', ['ckpt', '--data_dir', 'in', '--synthesis_schedule',
                     'queue'], '--synthesis_schedule needs --synthesis true'),
    ('evaluate.py', ['ckpt', '--data_dir', 'in', '--synthesis', 'true',
                     '--synthesis_schedule', 'greedy'], 'invalid choice'),
    ('generate.py', ['ckpt', '--synthesis_schedule', 'queue'],
     '--synthesis_schedule needs --lc_wav_dir'),
    ('generate.py', ['ckpt', '--lc_wav_dir', 'in', '--wav_out_dir', 'out',
                     '--synthesis_schedule', 'greedy'], 'invalid choice'),
])
def test_command_lines_check_the_schedule(script, argv, what):
    code, err = _error_of(script, argv)
    assert code == 2 and what in err
