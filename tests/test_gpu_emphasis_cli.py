"""Pre-emphasis from the command line, on a tiny model (two layers, 32
channels, Q = 64, 8 mels): train.py --preemphasis writes the checkpoint
entry; generate.py (fast and naive, in one go and with --save_every) and
evaluate.py --synthesis true apply the inverse filter that --preemphasis 0
leaves out; a run without the flag is the run with --preemphasis 0."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import emph_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = {"filter_width": 2, "sample_rate": 16000, "dilations": [1, 2],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 64, "skip_channels": 32,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
MODEL = ['--lc_upsample_scales', '4,4']
INT16 = 0.5 / 32767.0                  # int16 rounding of a [-1, 1] signal


def _run(script, argv, seconds=300):
    """One child under its own time limit; a failure ends the test."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    out = p.stdout.decode()
    assert p.returncode == 0, '%s %s\n%s' % (script, ' '.join(argv), out)
    return out


def _losses(out):
    return re.findall(r'step (\d+) - loss = ([0-9.]+)', out)


def _same_by_the_filter(with_filter, without, what):
    """The float32 wav `with_filter` against the float64 de-emphasis of the
    wav `without`, within int16 rounding."""
    ra, a = wavfile.read(with_filter)
    rb, b = wavfile.read(without)
    assert ra == rb == 16000 and a.dtype == b.dtype == np.float32
    assert a.shape == b.shape and a.shape[0] > 1
    y, bound = R.de64(b, 0.97)
    err = np.abs(a.astype(np.float64) - y)
    print('%s: %d samples, worst error %.3g (int16 rounding %.3g, float32 '
          'bound %.3g), peak %.3g' % (what, a.shape[0], err.max(), INT16,
                                      bound.max(), np.abs(a).max()))
    assert np.abs(a - b).max() > 100 * INT16        # (the filter ran)
    assert (err <= INT16).all()


@pytest.fixture(scope='module')
def run(hip_lib, tmp_path_factory):
    """train.py --synthetic --preemphasis 0.97, three steps."""
    tmp = tmp_path_factory.mktemp('emphasis_cli')
    params = str(tmp / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    common = ['--synthetic', '--wavenet_params', params, '--sample_size',
              '2000', '--batch_size', '2', '--num_steps', '3',
              '--checkpoint_every', '10', '--lc_channels', '8',
              '--lc_features', 'mel', '--lc_n_fft', '64'] + MODEL
    logdir = str(tmp / 'run')
    out = _run('train.py', common + ['--logdir', logdir, '--preemphasis',
                                     '0.97'])
    import train
    rng = np.random.default_rng(9)
    data = str(tmp / 'wavs')
    os.makedirs(data)
    # (the silence trimming works in hops of 512 samples: 1024 and 1536 stay)
    for i, n in enumerate((1300, 1700)):
        x = 0.7 * np.sin(2 * np.pi * 200.0 * (i + 1) * np.arange(n) / 16000.0) \
            + 0.05 * rng.standard_normal(n)
        wavfile.write(os.path.join(data, 'u%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))
    return dict(tmp=tmp, params=params, common=common, logdir=logdir, out=out,
                ck=train.latest_checkpoint(logdir), data=data)


def test_train_writes_the_entry(run):
    assert [k for k, _ in _losses(run['out'])] == ['0', '1', '2'], run['out']
    assert all(np.isfinite(float(v)) for _, v in _losses(run['out']))
    assert 'alpha = 0.97' in run['out']
    ck = torch.load(run['ck'], map_location='cpu')
    assert ck['emphasis'] == {'alpha': 0.97}
    assert ck['lc_features']['kind'] == 'mel'


def test_a_continued_run_refuses_another_alpha(run):
    p = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'train.py')] + run['common'] +
        ['--logdir', run['logdir'], '--preemphasis', '0.9'], cwd=ROOT,
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 1, out
    assert '0.9' in out and '0.97' in out and 'step ' not in out


@pytest.mark.parametrize('path', ['fast', 'naive'])
def test_generate_applies_the_inverse_filter(run, path):
    tmp = run['tmp'] / ('gen_' + path)
    os.makedirs(str(tmp))
    how = ['--lc_fast_generation', 'true'] if path == 'fast' else \
        ['--fast_generation', 'false']
    common = [run['ck'], '--wavenet_params', run['params'], '--lc_wav',
              os.path.join(run['data'], 'u1.wav'), '--samples', '40',
              '--seed', '3', '--logdir', str(tmp / 'log')] + MODEL + how
    wavs = {}
    for name, more in (('default', []), ('off', ['--preemphasis', '0']),
                       ('pieces', ['--save_every', '15'])):
        wavs[name] = str(tmp / (name + '.wav'))
        _run('generate.py', common + ['--wav_out_path', wavs[name]] + more)
    _same_by_the_filter(wavs['default'], wavs['off'], 'generate.py ' + path)
    assert open(wavs['pieces'], 'rb').read() == \
        open(wavs['default'], 'rb').read()


def test_evaluate_synthesis_de_emphasises(run):
    ev = [run['ck'], '--data_dir', run['data'], '--wavenet_params',
          run['params'], '--batch_size', '2', '--silence_threshold', '0.3',
          '--synthesis', 'true', '--synthesis_batch', '2', '--seed',
          '5'] + MODEL
    out_a, out_b = str(run['tmp'] / 'syn_a'), str(run['tmp'] / 'syn_b')
    res_a = json.loads(_run('evaluate.py', ev + ['--synthesis_out', out_a])
                       .strip().splitlines()[-1])
    res_b = json.loads(_run('evaluate.py', ev + ['--synthesis_out', out_b,
                                                 '--preemphasis', '0'])
                       .strip().splitlines()[-1])
    for res in (res_a, res_b):
        assert res['clips'] == 2 and np.isfinite(res['nll_per_sample'])
        syn = res['synthesis']
        assert syn['clips'] == 2 and 2 < syn['samples'] <= 1300 + 1700
        assert np.isfinite(syn['log_mel_mae_db']) and \
            np.isfinite(syn['log_mel_lsd_db'])
    # the scoring went through the pre-emphasis step, the distance through
    # the de-emphasised audio
    assert res_a['nll_per_sample'] != res_b['nll_per_sample']
    assert res_a['synthesis']['log_mel_lsd_db'] != \
        res_b['synthesis']['log_mel_lsd_db']
    for name in ('u0.wav', 'u1.wav'):
        _same_by_the_filter(os.path.join(out_a, name),
                            os.path.join(out_b, name), 'evaluate.py ' + name)


def test_without_the_flag_nothing_changes(run):
    import train
    logs, outs = [], []
    for name, more in (('plain', []), ('zero', ['--preemphasis', '0'])):
        logs.append(str(run['tmp'] / name))
        outs.append(_run('train.py', run['common'] + ['--logdir', logs[-1]]
                         + more))
    assert _losses(outs[0]) == _losses(outs[1])
    assert [k for k, _ in _losses(outs[0])] == ['0', '1', '2']
    assert _losses(outs[0]) != _losses(run['out'])     # (the flag does train
    #                                                     on another signal)
    a, b = (torch.load(train.latest_checkpoint(d), map_location='cpu')
            for d in logs)
    assert 'emphasis' not in a and 'emphasis' not in b
    assert sorted(a['variables']) == sorted(b['variables'])
    for k in a['variables']:
        assert torch.equal(a['variables'][k], b['variables'][k]), k
