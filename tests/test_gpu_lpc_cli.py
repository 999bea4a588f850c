"""Linear prediction from the command line, on a tiny model (two layers, 32
channels, Q = 64, 8 mels, hop 16) and three generated wavs: train.py
--lc_features mel --lpc_order 8 writes the checkpoint entry; evaluate.py
--synthesis true and generate.py (--lc_wav and --lc_path) run what the model
generates through the all-pole filter -- every written wav is recomputed from
the decoded codes (the same run with --lpc_order 0) through
reference_synthesis; a run without the flag writes no entry."""
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
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
MODEL = ['--lc_channels', '8', '--lc_upsample_scales', '4,4']
MEL = ['--lc_n_fft', '64', '--lc_normalize', 'range', '--lc_range=-23,7']
SILENCE = ['--silence_threshold', '0.3']
ENTRY = {'order': 8, 'noise': 1e-4, 'lag_window': 40.0, 'gain': 2.0}


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


def _front_end(ck):
    """(lp, spec): the checkpoint's linear prediction over its front end."""
    from wavenet import features, lpc
    e = dict(ck['lc_features'])
    assert e.pop('kind') == 'mel'
    norm = features.Normalizer.from_entry(e.pop('normalizer'))
    spec = features.MelSpec(**e, normalizer=norm)
    return lpc.LinearPrediction.from_entry(spec, ck['lpc']), spec


@pytest.fixture(scope='module')
def run(hip_lib, tmp_path_factory):
    tmp = tmp_path_factory.mktemp('lpc_cli')
    params = str(tmp / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    data = str(tmp / 'wavs')
    os.makedirs(data)
    rng = np.random.default_rng(9)
    # (the silence trimming works in hops of 512 samples)
    for i, n in enumerate((1300, 1700, 2100)):
        x = 0.6 * np.sin(2 * np.pi * 200.0 * (i + 1) * np.arange(n) / 16000.0) \
            + 0.05 * rng.standard_normal(n)
        wavfile.write(os.path.join(data, 'u%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))
    common = ['--data_dir', data, '--wavenet_params', params, '--batch_size',
              '2', '--mask_padding', 'true', '--num_steps', '3',
              '--checkpoint_every', '10', '--lc_features', 'mel'] + MEL + \
        MODEL + SILENCE
    logdir = str(tmp / 'run')
    out = _run('train.py', common + ['--logdir', logdir, '--lpc_order', '8',
                                     '--lpc_gain', '2', '--validation_dir',
                                     data, '--validation_batches', '1'])
    import train
    return dict(tmp=tmp, params=params, common=common, logdir=logdir, out=out,
                ck=train.latest_checkpoint(logdir), data=data)


def test_train_writes_the_entry(run):
    assert [k for k, _ in _losses(run['out'])] == ['0', '1', '2'], run['out']
    assert all(np.isfinite(float(v)) for _, v in _losses(run['out']))
    assert 'linear-prediction excitation' in run['out']
    assert 'validation loss' in run['out']
    ck = torch.load(run['ck'], map_location='cpu')
    assert ck['lpc'] == ENTRY
    assert ck['lc_features']['kind'] == 'mel' and 'emphasis' not in ck


def test_a_continued_run_refuses_other_settings(run):
    p = subprocess.run(
        [sys.executable, os.path.join(ROOT, 'train.py')] + run['common'] +
        ['--logdir', run['logdir'], '--lpc_order', '6'], cwd=ROOT,
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 1, out
    assert "'order': 6" in out and "'order': 8" in out and 'step ' not in out


def test_evaluate_synthesis_runs_the_all_pole_filter(run):
    from wavenet import evaluate as wev
    ev = [run['ck'], '--data_dir', run['data'], '--wavenet_params',
          run['params'], '--batch_size', '2', '--synthesis', 'true',
          '--synthesis_batch', '2', '--seed', '5',
          '--lc_upsample_scales', '4,4'] + SILENCE
    out_a, out_b = str(run['tmp'] / 'syn_a'), str(run['tmp'] / 'syn_b')
    res_a = json.loads(_run('evaluate.py', ev + ['--synthesis_out', out_a])
                       .strip().splitlines()[-1])
    res_b = json.loads(_run('evaluate.py', ev + ['--synthesis_out', out_b,
                                                 '--lpc_order', '0'])
                       .strip().splitlines()[-1])
    for res in (res_a, res_b):
        assert res['clips'] == 3 and np.isfinite(res['nll_per_sample'])
        assert res['synthesis']['clips'] == 3
        assert np.isfinite(res['synthesis']['log_mel_lsd_db'])
    # the scoring scored the excitation, the distance the filtered audio
    assert res_a['nll_per_sample'] != res_b['nll_per_sample']
    assert res_a['synthesis']['log_mel_lsd_db'] != \
        res_b['synthesis']['log_mel_lsd_db']
    lp, _ = _front_end(torch.load(run['ck'], map_location='cpu'))
    pieces = wev.ValidationSet(run['data'], 16000,
                               silence_threshold=0.3).pieces
    assert len(pieces) == 3
    for audio, path in ((p[0], p[1]) for p in pieces):
        name = os.path.splitext(os.path.basename(path))[0] + '.wav'
        ra, a = wavfile.read(os.path.join(out_a, name))
        rb, b = wavfile.read(os.path.join(out_b, name))
        assert ra == rb == 16000 and a.dtype == b.dtype == np.float32
        assert a.shape == b.shape == audio.shape
        # b: the decoded codes as they are; a: b through the filter of the
        # natural original's frames
        cf = lp.coefficients_of(np.asarray(audio, np.float32)).cpu().numpy()
        want = lp.reference_synthesis(b, cf)
        assert np.array_equal(a.view(np.int32), want.view(np.int32)), name
        assert np.abs(a - b).max() > 1e-3            # (the filter ran)


def _generate(run, name, source, more=()):
    tmp = run['tmp'] / name
    os.makedirs(str(tmp), exist_ok=True)
    wav = str(tmp / 'out.wav')
    _run('generate.py', [run['ck'], '--wavenet_params', run['params'],
                         '--lc_upsample_scales', '4,4', '--seed', '3',
                         '--lc_fast_generation', 'true', '--wav_out_path',
                         wav, '--logdir', str(tmp / 'log')] + list(source) +
         list(more))
    rate, got = wavfile.read(wav)
    assert rate == 16000 and got.dtype == np.float32
    return got


def test_generate_from_a_wav(run):
    from wavenet.audio_reader import load_wav
    src = os.path.join(run['data'], 'u1.wav')
    source = ['--lc_wav', src, '--samples', '150']
    on = _generate(run, 'wav_on', source)
    off = _generate(run, 'wav_off', source, ['--lpc_order', '0'])
    pieces = _generate(run, 'wav_pieces', source, ['--save_every', '64'])
    assert on.shape == off.shape == (151,)
    lp, _ = _front_end(torch.load(run['ck'], map_location='cpu'))
    wav = load_wav(src, 16000).reshape(-1)[:150]
    cf = lp.coefficients_of(np.asarray(wav, np.float32)).cpu().numpy()
    want = np.concatenate([off[:1], lp.reference_synthesis(off[1:], cf)])
    assert np.array_equal(on.view(np.int32), want.view(np.int32))
    assert np.array_equal(pieces.view(np.int32), on.view(np.int32))
    assert np.abs(on - off).max() > 1e-3


def test_generate_from_a_feature_file(run):
    from wavenet.audio_reader import load_wav
    ck = torch.load(run['ck'], map_location='cpu')
    lp, spec = _front_end(ck)
    wav = load_wav(os.path.join(run['data'], 'u2.wav'), 16000).reshape(-1)[:160]
    feats = spec(np.asarray(wav, np.float32)).cpu().numpy()
    assert feats.shape == (10, 8)
    path = str(run['tmp'] / 'mel.npy')
    np.save(path, feats)
    source = ['--lc_path', path, '--lc_hop', '16']
    on = _generate(run, 'npy_on', source)
    off = _generate(run, 'npy_off', source, ['--lpc_order', '0'])
    assert on.shape == off.shape == (161,)
    cf = lp.coefficients(spec.normalizer.invert(feats)).cpu().numpy()
    want = np.concatenate([off[:1], lp.reference_synthesis(off[1:], cf)])
    assert np.array_equal(on.view(np.int32), want.view(np.int32))
    assert np.abs(on - off).max() > 1e-3


def test_without_the_flag_nothing_is_written(run):
    import train
    logdir = str(run['tmp'] / 'plain')
    out = _run('train.py', run['common'] + ['--logdir', logdir])
    assert [k for k, _ in _losses(out)] == ['0', '1', '2']
    assert 'linear-prediction' not in out
    assert _losses(out) != _losses(run['out'])
    ck = torch.load(train.latest_checkpoint(logdir), map_location='cpu')
    assert 'lpc' not in ck
