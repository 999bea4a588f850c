"""The mixture-of-logistics head from the command line, on a tiny model (two
layers, 32 channels, scalar input): train.py --output_mixture writes the
checkpoint entry and refuses to continue with another; evaluate.py scores
through it ("accuracy": null); generate.py's naive path writes a 16-bit wav
that is the same run to run and equals a Python loop of predict_mixture and
mol.sample_reference; the flag combinations that stay refused say why."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = {"filter_width": 2, "sample_rate": 16000, "dilations": [1, 2],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 64, "skip_channels": 32,
          "use_biases": True, "scalar_input": True,
          "initial_filter_width": 4, "residual_postproc": False}


def _child(script, argv, seconds=300):
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    return p.returncode, p.stdout.decode()


def _run(script, argv):
    code, out = _child(script, argv)
    assert code == 0, '%s %s\n%s' % (script, ' '.join(argv), out)
    return out


def _losses(out):
    return re.findall(r'step (\d+) - loss = ([-0-9.]+)', out)


@pytest.fixture(scope='module')
def run(hip_lib, tmp_path_factory):
    """train.py --synthetic --output_mixture 4, three steps."""
    tmp = tmp_path_factory.mktemp('mol_cli')
    params = str(tmp / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    common = ['--synthetic', '--wavenet_params', params, '--sample_size',
              '2000', '--batch_size', '2', '--num_steps', '3',
              '--checkpoint_every', '10']
    logdir = str(tmp / 'run')
    out = _run('train.py', common + ['--logdir', logdir, '--output_mixture',
                                     '4'])
    import train
    rng = np.random.default_rng(9)
    data = str(tmp / 'wavs')
    os.makedirs(data)
    for i, n in enumerate((1300, 1700)):
        x = 0.7 * np.sin(2 * np.pi * 200.0 * (i + 1) * np.arange(n) / 16000.0) \
            + 0.05 * rng.standard_normal(n)
        wavfile.write(os.path.join(data, 'u%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))
    return dict(tmp=tmp, params=params, common=common, logdir=logdir, out=out,
                ck=train.latest_checkpoint(logdir), data=data)


def test_train_runs_and_writes_the_entry(run):
    assert [k for k, _ in _losses(run['out'])] == ['0', '1', '2'], run['out']
    assert all(np.isfinite(float(v)) for _, v in _losses(run['out']))
    assert 'mixture of 4 logistics' in run['out']
    ck = torch.load(run['ck'], map_location='cpu')
    assert ck['output'] == {'kind': 'mol', 'components': 4,
                            'log_scale_min': -14.0, 'levels': 65536}
    assert tuple(ck['variables']['wavenet/postprocessing/postprocess2'].shape) \
        == (1, 32, 12)


def test_a_continued_run_refuses_other_values(run):
    for more in (['--output_mixture', '8'],
                 ['--output_mixture', '4', '--mixture_log_scale_min', '-10'],
                 []):
        code, out = _child('train.py', run['common'] +
                           ['--logdir', run['logdir']] + more)
        assert code == 1, out
        assert 'checkpoint was trained with' in out and 'this run asks' in out
        assert "'components': 4" in out and 'step ' not in out


def test_flag_errors_name_both(run):
    onehot = str(run['tmp'] / 'onehot.json')
    json.dump(dict(PARAMS, scalar_input=False), open(onehot, 'w'))
    code, out = _child('train.py', ['--synthetic', '--wavenet_params', onehot,
                                    '--output_mixture', '4'])
    assert code == 2 and '--output_mixture' in out and 'scalar_input' in out
    code, out = _child('train.py', ['--synthetic', '--wavenet_params',
                                    run['params'], '--mixture_log_scale_min',
                                    '-9'])
    assert code == 2 and '--mixture_log_scale_min needs --output_mixture' in out
    code, out = _child('train.py', ['--synthetic', '--wavenet_params',
                                    run['params'], '--output_mixture', '40'])
    assert code == 2 and 'from 1 to 32' in out


def test_a_run_without_the_flag_writes_no_entry(run):
    import train
    logdir = str(run['tmp'] / 'plain')
    out = _run('train.py', run['common'] + ['--logdir', logdir])
    assert [k for k, _ in _losses(out)] == ['0', '1', '2']
    ck = torch.load(train.latest_checkpoint(logdir), map_location='cpu')
    assert 'output' not in ck
    assert tuple(ck['variables']['wavenet/postprocessing/postprocess2'].shape) \
        == (1, 32, 64)


def test_evaluate_reports_bits_and_no_accuracy(run):
    ev = [run['ck'], '--data_dir', run['data'], '--wavenet_params',
          run['params'], '--batch_size', '2', '--silence_threshold', '0.3']
    res = json.loads(_run('evaluate.py', ev).strip().splitlines()[-1])
    assert res['accuracy'] is None and res['clips'] == 2
    assert np.isfinite(res['nll_per_sample'])
    assert abs(res['bits_per_sample'] - res['nll_per_sample'] / np.log(2)) \
        < 1e-9
    # an untrained mixture is far from the 16 bits of a uniform guess on
    # either side, but finite
    assert 0 < res['samples'] <= 3000
    for more, what in ((['--synthesis', 'true'], 'follow-up'),
                       (['--input_noise', '0.1,2'], 'not codes')):
        code, out = _child('evaluate.py', ev + more)
        assert code == 1 and 'mixture-of-logistics' in out and what in out, out


def test_generate_writes_a_reproducible_16_bit_wav(run):
    from wavenet import mol
    from wavenet.cli import model_from_params
    n, seed, tau = 30, 3, 0.8
    common = [run['ck'], '--wavenet_params', run['params'], '--samples',
              str(n), '--seed', str(seed), '--temperature', str(tau),
              '--fast_generation', 'false']
    wavs = []
    for name in ('a', 'b'):
        wavs.append(str(run['tmp'] / (name + '.wav')))
        _run('generate.py', common + ['--wav_out_path', wavs[-1], '--logdir',
                                      str(run['tmp'] / ('log_' + name))])
    assert open(wavs[0], 'rb').read() == open(wavs[1], 'rb').read()
    rate, pcm = wavfile.read(wavs[0])
    assert rate == 16000 and pcm.dtype == np.int16 and pcm.shape == (n + 1,)
    # the same process as a Python loop on the checkpoint's weights
    ck = torch.load(run['ck'], map_location='cpu')
    net = model_from_params(PARAMS, 1, **mol.model_keywords(
        mol.check_entry(ck['output'])))
    net.load_state_dict(ck['variables'])
    lv = np.random.default_rng(seed).integers(65536, size=(1,))
    levels, wave = [int(lv[0])], mol.centres(lv).tolist()
    for step in range(n):
        p = net.predict_mixture(np.asarray(wave, np.float32)).cpu().numpy()
        j, c = mol.sample_reference(p[None], [seed], [step], tau)
        levels.append(int(j[0]))
        wave.append(float(c[0]))
    assert pcm.astype(np.int32).tolist() == [j - 32768 for j in levels]
    assert len(set(levels)) > 3


def test_refused_generation_flags_say_why(run):
    common = [run['ck'], '--wavenet_params', run['params'], '--samples', '4']
    code, out = _child('generate.py', common)       # (--fast_generation true)
    assert code == 1 and 'follow-up' in out and '--fast_generation' in out
    for flag in (['--top_k', '5'], ['--top_p', '0.9']):
        code, out = _child('generate.py', common + ['--fast_generation',
                                                    'false'] + flag)
        assert code == 1 and '--top_k / --top_p' in out, out
