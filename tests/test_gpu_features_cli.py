"""The log-mel front end from the command line: train.py --lc_features mel on
a directory of wavs alone against the same run on the .npy files
tools/make_lc_features.py writes (the same losses), evaluate.py picking the
front end up from the checkpoint, generate.py --lc_wav (copy synthesis)."""
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

PARAMS = {"filter_width": 2, "sample_rate": 16000,
          "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 256, "skip_channels": 64,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
MODEL = ['--lc_channels', '8', '--lc_upsample_scales', '4,4']
MEL = ['--lc_n_fft', '64']
SILENCE = ['--silence_threshold', '0.3']


def _run(script, argv, seconds=300):
    """One child under its own time limit; a failure ends the test."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    out = p.stdout.decode()
    assert p.returncode == 0, '%s %s\n%s' % (script, ' '.join(argv), out)
    return out


def _wavs(directory):
    """Three clips of different lengths: tones louder than the silence
    threshold, two of them behind 2048 samples of near silence (the trimming
    then starts at sample 2048, not 0, and ends before the file does)."""
    os.makedirs(directory)
    rng = np.random.default_rng(5)
    for i, (lead, n) in enumerate(((2048, 3000), (0, 5000), (2048, 4100))):
        t = np.arange(n)
        tone = 0.8 * np.sin(2 * np.pi * (220.0 * (i + 1)) * t / 16000.0) + \
            0.05 * rng.standard_normal(n)
        x = np.concatenate([0.001 * rng.standard_normal(lead), tone])
        wavfile.write(os.path.join(directory, 'clip%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _lines(out):
    losses = re.findall(r'step (\d+) - loss = ([0-9.]+), .*?(\d+) real', out)
    val = re.findall(r'validation loss = ([0-9.]+), bits/sample = ([0-9.]+)',
                     out)
    return losses, val


def test_train_from_audio_matches_train_from_written_features(tmp_path):
    from wavenet import audio_reader as ar
    data = str(tmp_path / 'wavs')
    _wavs(data)
    params = str(tmp_path / 'params.json')
    json.dump(PARAMS, open(params, 'w'))
    # (one clip per step, train.py's default: the file-based run takes a
    # batch's frames at offset + the LONGEST clip's length, which the frames
    # of a shorter trimmed file need not cover)
    common = ['--data_dir', data, '--wavenet_params', params,
              '--mask_padding', 'true', '--num_steps', '3',
              '--checkpoint_every', '10'] + MODEL + SILENCE
    validation = ['--validation_dir', data, '--validation_batches', '1',
                  '--batch_size', '1']
    # 1. features from the dequeued audio: no .npy anywhere
    log_a = str(tmp_path / 'run_a')
    out_a = _run('train.py', common + validation +
                 ['--logdir', log_a, '--lc_features', 'mel'] + MEL)
    assert not ar.find_files(data, '*.npy')
    losses_a, val_a = _lines(out_a)
    assert [k for k, _, _ in losses_a] == ['0', '1', '2'], out_a
    assert len(val_a) == 2, out_a        # (after step 0 and after the last)
    import train
    ck = train.latest_checkpoint(log_a)
    entry = torch.load(ck, map_location='cpu')['lc_features']
    assert entry['kind'] == 'mel' and entry['n_fft'] == 64 and \
        entry['hop'] == 16 and entry['n_mels'] == 8 and \
        entry['sample_rate'] == 16000
    # 2. evaluate.py: the front end comes from the checkpoint (there are no
    # feature files to read)
    ev = ['--data_dir', data, '--wavenet_params', params, '--batch_size',
          '2'] + MODEL + SILENCE
    res = json.loads(_run('evaluate.py', [ck] + ev).strip().splitlines()[-1])
    assert res['clips'] == 3 and np.isfinite(res['nll_per_sample'])
    # 3. generate.py --lc_wav: copy synthesis of the requested length
    wav = str(tmp_path / 'copy.wav')
    _run('generate.py', [ck, '--wavenet_params', params, '--lc_wav',
                         os.path.join(data, 'clip1.wav'),
                         '--lc_upsample_scales', '4,4', '--samples', '150',
                         '--lc_fast_generation', 'true', '--wav_out_path',
                         wav, '--logdir', str(tmp_path / 'gen')])
    rate, got = wavfile.read(wav)
    assert rate == 16000 and got.shape == (1 + 150,)
    assert np.isfinite(got).all()
    # 4. the same training run on the files the tool writes
    out = _run('tools/make_lc_features.py',
               [data, '--sample_rate', '16000', '--lc_channels', '8',
                '--lc_hop', '16'] + MEL + SILENCE)
    assert len(ar.find_files(data, '*.npy')) == 3, out
    for f in ar.find_files(data):
        feats = np.load(ar.lc_path_of(f))
        n = ar.load_wav(f, 16000).shape[0]
        assert feats.shape == (-(-n // 16), 8) and feats.dtype == np.float32
    log_b = str(tmp_path / 'run_b')
    out_b = _run('train.py', common + ['--logdir', log_b])
    assert 'lc_features' not in torch.load(train.latest_checkpoint(log_b),
                                           map_location='cpu')
    losses_b, _ = _lines(out_b)
    assert losses_b == losses_a, (out_a, out_b)
