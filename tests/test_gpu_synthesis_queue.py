"""The restart queue on the GPU: synthesize(schedule='queue') keeps the
contract of wavenet/synthesis.py (item u's codes are bit for bit those of a
stand-alone generate_batch call of one stream) at admission times that fall
on an item's end, for items of 1 and 2 samples, graph and single-step
segments; continue_generation_batch(restart=...) directly;
wn_fastgen_batch_restart and wn_fastgen_batch_lc_rows bitwise against numpy;
the calls without restart take the launches they took before; and
evaluate.py / generate.py --synthesis_schedule queue end to end."""
import numpy as np
import pytest
import torch

from test_gpu_synthesis import DIL10, LENGTHS, NAN, _alone, _model

pytestmark = pytest.mark.gpu

KW = {'plain': {}, 'trunc': dict(top_k=5, top_p=0.9)}


def _codes(t):
    return t.cpu().numpy()


def _check(lengths, syn, want):
    assert len(syn.codes) == len(lengths)
    for u, n in enumerate(lengths):
        c = syn.codes[u]
        assert c.is_cuda and c.dtype == torch.int32 and tuple(c.shape) == (n,)
        assert (_codes(c) == want[u]).all(), u


# ------------------------------------------------------------- the contract
@pytest.fixture(scope='module')
def rows_case():
    """Case (i) of tests/test_gpu_synthesis.py; the rows passed are longer
    than the items, NaN from row n_u - 1 on.  References computed once."""
    net = _model(5, DIL10, gc=7)
    net.fastgen_graph_steps = 20
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal((n, 5)).astype(np.float32) for n in LENGTHS]
    seeds = [100 + 3 * u for u in range(len(LENGTHS))]
    first = [int(v) for v in rng.integers(0, 64, len(LENGTHS))]
    gc = [6, 0, 3, 1, 5, 2, 4]
    want = {name: [_alone(net, n, seeds[u], first[u], gc[u], rows[u],
                          temperature=0.9, **kw)
                   for u, n in enumerate(LENGTHS)]
            for name, kw in KW.items()}
    padded = []
    for r in rows:
        p = np.full((r.shape[0] + 4, 5), NAN, np.float32)
        p[:r.shape[0] - 1] = r[:-1]
        padded.append(p)
    return dict(net=net, rows=padded, seeds=seeds, first=first, gc=gc,
                want=want)


@pytest.mark.parametrize('quantum', [1, 20])
@pytest.mark.parametrize('name', ['plain', 'trunc'])
def test_queue_contract_rows_model(hip_lib, rows_case, name, quantum):
    from wavenet import synthesis
    c = rows_case
    syn = synthesis.synthesize(
        c['net'], LENGTHS, seeds=c['seeds'], batch=3,
        first_samples=c['first'], global_condition=c['gc'],
        local_condition=c['rows'], temperature=0.9, schedule='queue',
        quantum=quantum, **KW[name])
    assert syn.rounds == [[3, 5, 4], [2, 6, 1], [0]]
    assert syn.steps == {1: 150, 20: 161}[quantum]
    assert syn.occupancy == 413 / (3.0 * syn.steps)
    _check(LENGTHS, syn, c['want'][name])


def test_queue_isolation_from_nan_rows(hip_lib, rows_case):
    """Two items' rows are all NaN (one admitted at 0, one later, into the
    slot every later item shares): the others' codes are unchanged."""
    from wavenet import synthesis
    c = rows_case
    rows = [r.copy() for r in c['rows']]
    for u in (5, 6):
        rows[u][:] = NAN
    syn = synthesis.synthesize(
        c['net'], LENGTHS, seeds=c['seeds'], batch=3,
        first_samples=c['first'], global_condition=c['gc'],
        local_condition=[torch.tensor(r).cuda() for r in rows],
        temperature=0.9, schedule='queue', quantum=1)
    for u in range(len(LENGTHS)):
        if u not in (5, 6):
            assert (_codes(syn.codes[u]) == c['want']['plain'][u]).all(), u


def test_queue_contract_upsampler_model_with_context(hip_lib):
    from wavenet import synthesis
    net = _model(6, DIL10, local_condition_upsample_scales=(2, 4),
                 local_condition_context=1)
    net.fastgen_graph_steps = 20
    lengths = [45, 1, 131, 8, 70, 23]
    rng = np.random.default_rng(8)
    frames = [rng.standard_normal((-(-n // 8) + (2 if n == 70 else 0), 6)
                                  ).astype(np.float32) for n in lengths]
    seeds = [7 * u + 1 for u in range(len(lengths))]
    want = [_alone(net, n, seeds[u], 32,
                   None, net.upsample_local_condition(frames[u], n))
            for u, n in enumerate(lengths)]
    for quantum in (1, None):
        syn = synthesis.synthesize(net, lengths, seeds=seeds, batch=4,
                                   frames=frames, schedule='queue',
                                   quantum=quantum)
        assert syn.rounds == [[2, 4, 0, 5], [3, 1]]
        assert syn.steps == 131      # (the quantum 2 costs nothing here)
        _check(lengths, syn, want)


@pytest.mark.parametrize('batch', [1, 8])
def test_queue_model_without_lc(hip_lib, batch):
    """Batch 1 (every item restarts the one slot) and batch >= the items
    (one call, no admission): the stand-alone codes, which are those of
    schedule='rounds'."""
    from wavenet import synthesis
    net = _model(None, DIL10)
    net.fastgen_graph_steps = 20
    lengths = [30, 1, 77, 12, 77]
    seeds = [5, 6, 7, 8, 9]
    want = [_alone(net, n, seeds[u], 32, None, None)
            for u, n in enumerate(lengths)]
    rounds = synthesis.synthesize(net, lengths, seeds=seeds, batch=batch)
    queue = synthesis.synthesize(net, lengths, seeds=seeds, batch=batch,
                                 schedule='queue', quantum=1)
    assert queue.rounds == rounds.rounds
    assert queue.steps == (197 if batch == 1 else 77)
    _check(lengths, queue, want)
    _check(lengths, rounds, want)


def test_queue_restarts_in_the_second_chain_workgroup(hip_lib, rows_case):
    """Batch 33 (Bp = 64): stream 32 sits in the second chain workgroup and
    is restarted; 70 items of 1 .. 40 samples against schedule='rounds'
    (itself held to the contract by tests/test_gpu_synthesis.py) and, for
    the items of slot 32, against the stand-alone call."""
    from wavenet import synthesis
    net = rows_case['net']
    rng = np.random.default_rng(33)
    lengths = [int(v) for v in rng.integers(1, 41, 70)]
    plan = synthesis.plan_queue(lengths, 33, 1)
    last = [u for u in range(70) if plan.slot[u] == 32]
    assert len(last) > 1
    rows = [rng.standard_normal((n, 5)).astype(np.float32) for n in lengths]
    seeds = [1000 + u for u in range(70)]
    first = [int(v) for v in rng.integers(0, 64, 70)]
    gc = [int(v) for v in rng.integers(0, 7, 70)]
    kw = dict(seeds=seeds, batch=33, first_samples=first,
              global_condition=gc, local_condition=rows, temperature=0.9)
    rounds = synthesis.synthesize(net, lengths, **kw)
    queue = synthesis.synthesize(net, lengths, schedule='queue', quantum=1,
                                 **kw)
    assert queue.steps == plan.steps <= rounds.steps
    _check(lengths, queue, [_codes(c) for c in rounds.codes])
    for u in last:
        assert (_codes(queue.codes[u]) ==
                _alone(net, lengths[u], seeds[u], first[u], gc[u], rows[u],
                       temperature=0.9)).all(), u


# ------------------------------------------- continue_generation_batch(restart)
def test_continue_with_restart(hip_lib, rows_case):
    """B = 4, calls of 10, 12 and 9 steps; the second restarts streams 1 and
    3 (new seeds, GC ids and first codes).  Restarted streams: the
    stand-alone call of 12 steps, and with the third call one of 21; the
    others: the same calls without any restart."""
    net = rows_case['net']
    rng = np.random.default_rng(21)
    lc = [torch.tensor(rng.standard_normal((4, n, 5)).astype(np.float32))
          for n in (10, 12, 9)]
    seeds, seeds2 = [11, 12, 13, 14], [11, 52, 13, 54]
    gc, gc2 = [0, 1, 2, 3], [0, 6, 2, 5]

    def run(restart):
        a = net.generate_batch(10, seeds, seed_samples=[[7], [8], [9], [10]],
                               global_condition=gc, local_condition=lc[0],
                               temperature=0.9)
        last = _codes(a[:, -1]).copy()
        s, g = (seeds2, gc2) if restart else (seeds, gc)
        if restart:
            last[1], last[3] = 40, 41
        b = net.continue_generation_batch(
            12, last, s, global_condition=g, local_condition=lc[1],
            temperature=0.9, restart=restart)
        c = net.continue_generation_batch(
            9, b[:, -1], s, global_condition=g, local_condition=lc[2],
            temperature=0.9)
        return _codes(b), _codes(c)
    b0, c0 = run(None)
    b1, c1 = run([3, 1])
    for s in (0, 2):
        assert (b1[s] == b0[s]).all() and (c1[s] == c0[s]).all()
    for s, code in ((1, 40), (3, 41)):
        rows = torch.cat([lc[1][s], lc[2][s]])
        alone = _codes(net.generate_batch(
            21, [seeds2[s]], seed_samples=[[code]],
            global_condition=[gc2[s]], local_condition=rows[None],
            temperature=0.9)[0, 1:])
        assert (b1[s] == alone[:12]).all(), s
        assert (c1[s] == alone[12:]).all(), s
        short = _codes(net.generate_batch(
            12, [seeds2[s]], seed_samples=[[code]],
            global_condition=[gc2[s]], local_condition=lc[1][s][None],
            temperature=0.9)[0, 1:])
        assert (b1[s] == short).all(), s
        assert (b1[s] != b0[s]).any()


# --------------------------------------------------- wn_fastgen_batch_restart
@pytest.mark.parametrize('B, on', [(3, [0]), (3, [2]), (3, [0, 1, 2]),
                                   (33, [0]), (33, [32]), (33, [1, 31, 32]),
                                   (33, [])])
def test_restart_kernel_touches_flagged_streams_only(hip_lib, B, on):
    from wavenet import _lib
    dil = np.asarray(DIL10, np.int32)
    Bp = hip_lib.wn_fastgen_batch_rows(B)
    nfl = hip_lib.wn_fastgen_batch_state_floats(dil.ctypes.data, len(dil), B)
    assert nfl == 62 * Bp * 32
    rng = np.random.default_rng(B)
    state0 = rng.standard_normal(nfl).astype(np.float32)
    prev0 = rng.integers(0, 64, Bp).astype(np.int32)
    orig0 = rng.integers(0, 17, Bp).astype(np.int32)
    flags = np.zeros(Bp, np.int32)
    flags[on] = rng.integers(1, 5, len(on))
    flags[B:] = 1                      # padding rows: never touched
    dev = [torch.tensor(a).cuda() for a in
           (state0, dil, np.asarray([17, 0, 0, 0], np.int32), prev0, orig0,
            flags)]
    state, dild, cursors, prev, orig, fl = dev
    _lib.call('wn_fastgen_batch_restart', _lib.ptr(state), _lib.ptr(dild),
              len(dil), B, _lib.ptr(cursors), _lib.ptr(prev), _lib.ptr(orig),
              _lib.ptr(fl), _lib.stream())
    want = state0.reshape(62, Bp, 32).copy()
    want[:, on, :] = 0.0
    pw, ow = prev0.copy(), orig0.copy()
    pw[on], ow[on] = -1, 17
    assert (_codes(state).view(np.uint32) ==
            want.reshape(-1).view(np.uint32)).all()
    assert (_codes(prev) == pw).all() and (_codes(orig) == ow).all()
    assert (_codes(cursors) == [17, 0, 0, 0]).all()


# --------------------------------------------------- wn_fastgen_batch_lc_rows
@pytest.mark.parametrize('Lc', [1, 5, 80])
def test_lc_rows_bitwise_against_numpy(hip_lib, Lc):
    """Origins before and inside the segment, an item that ended before it,
    m = 0, an empty slot; the sources are longer than m and NaN from row m
    on."""
    net = _model(Lc, [1, 2])
    rng = np.random.default_rng(Lc)
    pos0, n = 50, 23
    # (origin, m): running since 0; starts inside; starts at the first
    # step; ends inside; ended before; no rows; no item
    spec = [(0, 90), (60, 30), (50, 5), (40, 20), (10, 30), (50, 0), None]
    items, want = [], np.zeros((len(spec), n, Lc), np.float32)
    for b, it in enumerate(spec):
        if it is None:
            items.append(None)
            continue
        origin, m = it
        src = rng.standard_normal((m + 3, Lc)).astype(np.float32)
        src[m:] = NAN
        for j in range(n):
            t = pos0 + j - origin
            if 1 <= t <= m:
                want[b, j] = src[t - 1]
        dev = torch.tensor(src).cuda()
        items.append((dev[:m], origin))
    got = net.batch_local_condition(items, pos0, n)
    assert got.is_cuda and got.dtype == torch.float32
    assert tuple(got.shape) == want.shape
    assert (_codes(got).view(np.uint32) == want.view(np.uint32)).all()
    assert want[0].any() and want[1, :10].any() == 0 and want[4].any() == 0


# ------------------------------------------------------------------ regression
def test_calls_without_restart_take_the_launches_of_before(hip_lib,
                                                           monkeypatch):
    """generate_batch + continue_generation_batch without restart call the
    batched entry points they called before this schedule existed -- also on
    a generator that has been through a restart -- and give the same
    codes."""
    from wavenet import _lib
    net = _model(None, DIL10)
    net.fastgen_graph_steps = 20
    names = []
    call = _lib.call
    monkeypatch.setattr(_lib, 'call',
                        lambda name, *a: (names.append(name), call(name, *a)))

    def run():
        del names[:]
        a = net.generate_batch(45, [1, 2, 3])
        b = net.continue_generation_batch(30, a[:, -1], [1, 2, 3])
        return _codes(a), _codes(b), {x for x in names if 'batch' in x}
    old = {'wn_fastgen_batch_init', 'wn_fastgen_batch_pre',
           'wn_fastgen_batch_step', 'wn_fastgen_batch_finish'}
    a0, b0, n0 = run()
    assert n0 == old
    del names[:]
    net.continue_generation_batch(5, b0[:, -1], [1, 2, 3], restart=[1])
    assert {x for x in names if 'batch' in x} == {
        'wn_fastgen_batch_restart', 'wn_fastgen_batch_pre',
        'wn_fastgen_batch_step_q', 'wn_fastgen_batch_finish_q'}
    a1, b1, n1 = run()
    assert n1 == old
    assert (a1 == a0).all() and (b1 == b0).all()
    # and a stream's codes are those of one longer call
    long = _codes(net.generate_batch(75, [1, 2, 3]))
    assert (long[:, :46] == a0).all() and (long[:, 46:] == b0).all()


# ------------------------------------------------------------- command line
def test_evaluate_and_generate_with_the_queue(hip_lib, tmp_path):
    """evaluate.py --synthesis_schedule queue: the six keys, steps and
    occupancy of plan_queue, and the distances of the rounds (the same
    audio); generate.py --lc_wav_dir writes the same files either way."""
    import json
    import os
    from scipy.io import wavfile
    import queue_ref as QR
    import test_gpu_synthesis as S
    from wavenet import evaluate as ev
    data = str(tmp_path / 'wavs')
    S._wavs(data)
    params = str(tmp_path / 'params.json')
    json.dump(S.PARAMS, open(params, 'w'))
    log = str(tmp_path / 'run')
    S._run('train.py', ['--data_dir', data, '--wavenet_params', params,
                        '--mask_padding', 'true', '--num_steps', '2',
                        '--checkpoint_every', '10', '--silence_threshold',
                        '0.3', '--logdir', log, '--lc_features', 'mel',
                        '--lc_n_fft', '64'] + S.MODEL)
    import train
    ck = train.latest_checkpoint(log)
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces
    lengths = [p[0].shape[0] for p in utts]
    argv = [ck, '--data_dir', data, '--wavenet_params', params,
            '--batch_size', '2', '--synthesis', 'true', '--synthesis_batch',
            '3', '--seed', '4'] + S.MODEL
    res = {}
    for schedule in ('rounds', 'queue'):
        line = S._run('evaluate.py', argv + ['--synthesis_schedule', schedule]
                      ).strip().splitlines()[-1]
        res[schedule] = json.loads(line)['synthesis']
        assert set(res[schedule]) == {'clips', 'samples', 'steps',
                                      'occupancy', 'log_mel_mae_db',
                                      'log_mel_lsd_db'}
    # quantum: a tenth of the default fastgen_graph_steps
    plan = QR.plan_queue(lengths, 3, 20)
    assert (res['queue']['steps'], res['queue']['occupancy']) == plan[3:]
    assert res['queue']['steps'] < res['rounds']['steps']
    for k in ('clips', 'samples', 'log_mel_mae_db', 'log_mel_lsd_db'):
        assert res['queue'][k] == res['rounds'][k], k
    out = {}
    for schedule in ('rounds', 'queue'):
        d = str(tmp_path / ('gen_' + schedule))
        S._run('generate.py', [ck, '--wavenet_params', params, '--lc_wav_dir',
                               data, '--wav_out_dir', d, '--clips', '3',
                               '--lc_upsample_scales', '4,4',
                               '--synthesis_schedule', schedule])
        out[schedule] = {f: wavfile.read(os.path.join(d, f))[1]
                         for f in sorted(os.listdir(d))}
    assert list(out['queue']) == list(out['rounds']) and len(out['queue']) == 4
    for f, w in out['rounds'].items():
        assert (out['queue'][f] == w).all(), f
