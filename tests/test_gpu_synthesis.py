"""Bulk synthesis on the device: wn_feature_distance against the float64
restatement of tests/synth_ref.py, wavenet/synthesis.py's contract -- item u's
codes are bit for bit those of a stand-alone generate_batch call of one
stream -- for a repetition-row model, an upsampler model with frame context
and a model without local conditioning, and evaluate.py --synthesis /
generate.py --lc_wav_dir end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import synth_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')
# (B, F, C): one element; the scalar path, one partial chunk of 64 frames;
# 16-byte loads with 20 of 64 lanes live and five chunks, the last of one
# frame; 32 lanes live; the channel cap: two trips of a lane's channel loop
SHAPES = [(1, 1, 1), (3, 33, 3), (2, 257, 80), (3, 40, 128), (1, 5, 512)]


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view(np.uint64)


_DATA = {}


def _data(shape):
    """Two float32 [B, F, C] tensors shaped like log-mel frames, computed
    once, shared, never written to."""
    if shape not in _DATA:
        rng = np.random.default_rng(sum(shape))
        pair = []
        for _ in range(2):
            x = (rng.standard_normal(shape) * 11 - 10).astype(np.float32)
            x.setflags(write=False)
            pair.append(x)
        _DATA[shape] = tuple(pair)
    return _DATA[shape]


def _ragged(B, F):
    """nframes mixing 0, 1 and F."""
    return {1: [F], 2: [1, F], 3: [0, F, 1]}[B]


def _poisoned(x, nframes):
    x = x.copy()
    x[~R.real_mask(x.shape[0], x.shape[1], nframes)] = NAN
    return x


# ------------------------------------------------------------ the distance
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_distance_matches_float64_numpy(hip_lib, shape):
    from wavenet import features
    B, F, C = shape
    a, b = _data(shape)
    for nf in (None, _ragged(B, F)):
        ref = R.distance(a, b, nf)
        pa, pb = (a, b) if nf is None else (_poisoned(a, nf), _poisoned(b, nf))
        d = features.frame_distance(pa, pb, nf)
        got = [t.cpu().numpy() for t in d]
        for g in got:
            assert g.dtype == np.float64 and g.shape == (B,)
            assert np.isfinite(g).all()          # (no NaN was read)
        # abs_sum, sq_sum: two summation orders of n = nframes * C float64
        # terms, 2 n 2^-53 sum|term|; rms_sum: the same over its F terms plus
        # F 2^-52 max_f rms_f for the square roots and the inner means
        bounds = (R.sum_bound(ref['terms'], ref['abs_sum']),
                  R.sum_bound(ref['terms'], ref['sq_sum']),
                  R.rms_bound(ref))
        for name, g, bound in zip(('abs_sum', 'sq_sum', 'rms_sum'), got,
                                  bounds):
            err = np.abs(g - ref[name])
            print('%s nframes %s %s: max err %.3g, bound %.3g'
                  % (shape, nf, name, err.max(), bound.max()))
            assert (err <= bound).all(), (name, err, bound)
        # two calls: the same bits
        again = features.frame_distance(pa, pb, nf)
        for x, y in zip(d, again):
            assert (_bits(x) == _bits(y)).all()
        # equal inputs: exact zeros
        for t in features.frame_distance(pa, pa.copy(), nf):
            assert not t.cpu().numpy().any()


def test_distance_of_equal_inputs_is_exactly_zero(hip_lib):
    from wavenet import features
    a, _ = _data((2, 257, 80))
    for t in features.frame_distance(a, a.copy()):
        z = t.cpu().numpy()
        assert (z == 0).all() and not np.signbit(z).any()


@pytest.mark.parametrize('shape', [(3, 33, 3), (3, 40, 128)], ids=str)
def test_distance_of_a_clip_does_not_depend_on_the_batch(hip_lib, shape):
    """Clip 2 of a batch of 3 alone (as [F, C] and as a batch of one): the
    same bits, whatever its neighbours hold."""
    from wavenet import features
    a, b = _data(shape)
    F = shape[1]
    for nf in (None, [F, 0, F - 1]):
        three = features.frame_distance(a, b, nf)
        n2 = None if nf is None else nf[2:]
        for alone in (features.frame_distance(a[2], b[2], n2),
                      features.frame_distance(a[2:], b[2:], n2)):
            for x, y in zip(three, alone):
                assert y.shape == (1,)
                assert _bits(x)[2] == _bits(y)[0]
    # device tensors in, device tensors out
    ta, tb = torch.tensor(a).cuda(), torch.tensor(b).cuda()
    d = features.frame_distance(ta, tb)
    assert d.abs_sum.is_cuda and (_bits(d.abs_sum) ==
                                  _bits(features.frame_distance(a, b).abs_sum)
                                  ).all()


def test_distance_summary_in_db(hip_lib):
    from wavenet import features
    a, b = _data((3, 40, 128))
    nf = [40, 7, 0]
    ref = R.distance(a, b, nf)
    mae, lsd = features.frame_distance(a, b, nf).summary(nf, 128)
    k = 10.0 / np.log(10.0)
    assert np.isclose(mae, k * ref['abs_sum'].sum() / (47 * 128), rtol=1e-12)
    assert np.isclose(lsd, k * ref['rms_sum'].sum() / 47, rtol=1e-12)


# ------------------------------------------------------------- the contract
def _model(lc, dilations, Q=64, gc=None, seed=0, **kw):
    from wavenet import WaveNetModel
    if gc:
        kw.update(global_condition_channels=gc,
                  global_condition_cardinality=gc)
    net = WaveNetModel(1, dilations, 2, 32, 32, 64, quantization_channels=Q,
                       use_biases=True, seed=seed,
                       local_condition_channels=lc, **kw)
    g = torch.Generator().manual_seed(seed + 11)
    with torch.no_grad():
        for n, v in net.named_variables():
            leaf = n.split('/')[-1]
            r = torch.randn(v.shape, generator=g, dtype=torch.float64).float()
            if 'bias' in leaf:
                v.copy_(0.1 * r)
            elif '/lc_upsample/' in n or '/lc_context/' in n:
                v.add_((0.3 * r).to(v.device))   # (not the identity)
            elif leaf.startswith('lc_'):
                v.copy_(0.3 * r)                 # (rows that matter)
    return net


def _alone(net, n, seed, first, gc, rows, **kw):
    """The contract's right-hand side for one item."""
    lc = None
    if rows is not None:
        rows = torch.as_tensor(rows, dtype=torch.float32)
        lc = torch.cat([torch.zeros(1, net.Lc), rows.cpu()[:n - 1]])[None]
    out = net.generate_batch(n, [seed], seed_samples=[[first]],
                             global_condition=None if gc is None else [gc],
                             local_condition=lc, **kw)
    return out[0, 1:].cpu().numpy()


def _check(net, lengths, syn, want):
    assert len(syn.codes) == len(lengths)
    for u, n in enumerate(lengths):
        c = syn.codes[u]
        assert c.is_cuda and c.dtype == torch.int32 and tuple(c.shape) == (n,)
        assert (c.cpu().numpy() == want[u]).all(), u


LENGTHS = [1, 2, 37, 150, 64, 150, 9]
DIL10 = [1, 2, 4, 8, 16, 1, 2, 4, 8, 16]


@pytest.fixture(scope='module')
def rows_case():
    """Case (i): the model, its inputs and the stand-alone references of the
    plain and the truncated draw, computed once."""
    net = _model(5, DIL10, gc=7)
    net.fastgen_graph_steps = 20     # a round: graphs of 20 and 2, then steps
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal((n, 5)).astype(np.float32) for n in LENGTHS]
    seeds = [100 + 3 * u for u in range(len(LENGTHS))]
    first = [int(v) for v in rng.integers(0, 64, len(LENGTHS))]
    gc = [6, 0, 3, 1, 5, 2, 4]
    want = {}
    for name, kw in (('plain', {}), ('trunc', dict(top_k=5, top_p=0.9))):
        want[name] = [_alone(net, n, seeds[u], first[u], gc[u], rows[u],
                             temperature=0.9, **kw)
                      for u, n in enumerate(LENGTHS)]
    return dict(net=net, rows=rows, seeds=seeds, first=first, gc=gc,
                want=want)


@pytest.mark.parametrize('name, kw', [('plain', {}),
                                      ('trunc', dict(top_k=5, top_p=0.9))])
def test_contract_rows_model(hip_lib, rows_case, name, kw):
    from wavenet import synthesis
    c = rows_case
    syn = synthesis.synthesize(
        c['net'], LENGTHS, seeds=c['seeds'], batch=3,
        first_samples=c['first'], global_condition=c['gc'],
        local_condition=c['rows'], temperature=0.9, **kw)
    plan = R.plan_rounds(LENGTHS, 3)
    assert syn.rounds == plan[0] == [[3, 5, 4], [2, 6, 1], [0]]
    assert syn.steps == plan[1] == 188 and syn.occupancy == plan[2]
    _check(c['net'], LENGTHS, syn, c['want'][name])
    # (the draws differ: the truncation is not a no-op here)
    assert any((a != b).any() for a, b in zip(c['want']['plain'],
                                              c['want']['trunc']))


def test_contract_isolation_from_nan_rows(hip_lib, rows_case):
    """Case (iv): two items' rows are NaN; every other item's codes are the
    stand-alone ones."""
    from wavenet import synthesis
    c = rows_case
    rows = [r.copy() for r in c['rows']]
    for u in (5, 6):                 # one in the first round, one in the second
        rows[u][:] = NAN
    syn = synthesis.synthesize(
        c['net'], LENGTHS, seeds=c['seeds'], batch=3,
        first_samples=c['first'], global_condition=c['gc'],
        local_condition=[torch.tensor(r).cuda() for r in rows],
        temperature=0.9)
    for u, n in enumerate(LENGTHS):
        if u not in (5, 6):
            assert (syn.codes[u].cpu().numpy() == c['want']['plain'][u]
                    ).all(), u


def test_contract_upsampler_model_with_context(hip_lib):
    """Case (ii): scales (2, 4), context 1, frames; lengths that are no
    multiples of the hop 8, one of them 1, one item with more frames than it
    needs."""
    from wavenet import synthesis
    net = _model(6, DIL10, local_condition_upsample_scales=(2, 4),
                 local_condition_context=1)
    lengths = [45, 1, 131, 8, 70, 23]
    rng = np.random.default_rng(8)
    frames = [rng.standard_normal((-(-n // 8) + (2 if n == 70 else 0), 6)
                                  ).astype(np.float32) for n in lengths]
    seeds = [7 * u + 1 for u in range(len(lengths))]
    want = [_alone(net, n, seeds[u], 32,
                   None, net.upsample_local_condition(frames[u], n))
            for u, n in enumerate(lengths)]
    syn = synthesis.synthesize(net, lengths, seeds=seeds, batch=4,
                               frames=frames)
    assert syn.rounds == [[2, 4, 0, 5], [3, 1]]
    _check(net, lengths, syn, want)


@pytest.mark.parametrize('batch', [1, 8])
def test_contract_model_without_lc(hip_lib, batch):
    """Case (iii): ragged lengths at batch 1 and at batch >= the items."""
    from wavenet import synthesis
    net = _model(None, DIL10)
    lengths = [30, 1, 77, 12, 77]
    seeds = [5, 6, 7, 8, 9]
    want = [_alone(net, n, seeds[u], 32, None, None)
            for u, n in enumerate(lengths)]
    syn = synthesis.synthesize(net, lengths, seeds=seeds, batch=batch)
    assert len(syn.rounds) == (5 if batch == 1 else 1)
    _check(net, lengths, syn, want)
    # another seed is another draw
    other = synthesis.synthesize(net, [77], seeds=[1234], batch=batch)
    assert (other.codes[0].cpu().numpy() != want[2]).any()


# ------------------------------------------------------------- command line
PARAMS = {"filter_width": 2, "sample_rate": 16000, "dilations": DIL10,
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 256, "skip_channels": 64,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
MODEL = ['--lc_channels', '8', '--lc_upsample_scales', '4,4']
OLD_KEYS = {'nll_per_sample', 'bits_per_sample', 'accuracy', 'samples',
            'clips'}


def _run(script, argv, seconds=300):
    """One child under its own time limit; a failure ends the test."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    out = p.stdout.decode()
    assert p.returncode == 0, '%s %s\n%s' % (script, ' '.join(argv), out)
    return out


def _wavs(directory):
    """Four short clips of different lengths, two behind near silence."""
    os.makedirs(directory)
    rng = np.random.default_rng(5)
    for i, (lead, n) in enumerate(((2048, 3000), (0, 2600), (2048, 3500),
                                   (0, 4000))):
        t = np.arange(n)
        tone = 0.8 * np.sin(2 * np.pi * (220.0 * (i + 1)) * t / 16000.0) + \
            0.05 * rng.standard_normal(n)
        x = np.concatenate([0.001 * rng.standard_normal(lead), tone])
        wavfile.write(os.path.join(directory, 'clip%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))


def test_evaluate_synthesis_and_generate_directory(hip_lib, tmp_path):
    from wavenet import audio_reader as ar
    from wavenet import evaluate as ev
    data = str(tmp_path / 'wavs')
    _wavs(data)
    params = str(tmp_path / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    log = str(tmp_path / 'run')
    _run('train.py', ['--data_dir', data, '--wavenet_params', params,
                      '--mask_padding', 'true', '--num_steps', '2',
                      '--checkpoint_every', '10', '--silence_threshold',
                      '0.3', '--logdir', log, '--lc_features', 'mel',
                      '--lc_n_fft', '64'] + MODEL)
    import train
    ck = train.latest_checkpoint(log)
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces
    want = {os.path.splitext(os.path.basename(p[1]))[0]: p[0].shape[0]
            for p in utts}
    assert len(want) == 4 and len(set(want.values())) > 1
    out_dir = str(tmp_path / 'copies')
    argv = [ck, '--data_dir', data, '--wavenet_params', params,
            '--batch_size', '2', '--synthesis', 'true', '--synthesis_batch',
            '3', '--synthesis_out', out_dir, '--seed', '4'] + MODEL
    line = _run('evaluate.py', argv).strip().splitlines()[-1]
    res = json.loads(line)
    assert set(res) == OLD_KEYS | {'synthesis'}
    syn = res['synthesis']
    assert set(syn) == {'clips', 'samples', 'steps', 'occupancy',
                        'log_mel_mae_db', 'log_mel_lsd_db'}
    assert all(np.isfinite(v) for v in syn.values())
    assert syn['clips'] == 4 == res['clips']
    assert syn['samples'] == sum(want.values())
    plan = R.plan_rounds([p[0].shape[0] for p in utts], 3)
    assert syn['steps'] == plan[1] and syn['occupancy'] == plan[2]
    assert syn['log_mel_mae_db'] > 0 and syn['log_mel_lsd_db'] > 0
    assert sorted(os.listdir(out_dir)) == sorted(k + '.wav' for k in want)
    for k, n in want.items():
        rate, got = wavfile.read(os.path.join(out_dir, k + '.wav'))
        assert rate == 16000 and got.shape == (n,) and np.isfinite(got).all()
    # again: the identical line
    assert _run('evaluate.py', argv).strip().splitlines()[-1] == line
    # generate.py --lc_wav_dir: the files as they are (no trimming)
    gen_dir = str(tmp_path / 'generated')
    _run('generate.py', [ck, '--wavenet_params', params, '--lc_wav_dir', data,
                         '--wav_out_dir', gen_dir, '--clips', '3',
                         '--lc_upsample_scales', '4,4'])
    assert sorted(os.listdir(gen_dir)) == \
        sorted(os.path.basename(f) for f in ar.find_files(data))
    for f in ar.find_files(data):
        rate, got = wavfile.read(os.path.join(gen_dir, os.path.basename(f)))
        assert rate == 16000 and got.shape == (ar.load_wav(f, 16000).shape[0],)
