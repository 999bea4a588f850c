"""--lc_features mel+f0 end to end, one chain on a directory of three 0.3 s
synthetic wavs and a tiny model (10 local-conditioning channels = 8 mels + F0
+ voicing, hop 64): train.py writes a checkpoint whose 'lc_features' entry
names the composite front end; evaluate.py and generate.py --lc_wav take the
front end from it without a front-end flag; and the same training runs from
the device corpus with whole-utterance frames."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import test_gpu_pitch_cli as base

pytestmark = pytest.mark.gpu

MODEL = ['--lc_channels', '10', '--lc_upsample_scales', '4,4,4']
FRONT = ['--lc_features', 'mel+f0', '--lc_f0_interpolate', 'true',
         '--lc_n_fft', '256']


def _wavs(directory):
    """Three harmonic clips of 0.3 s, the middle of each silent."""
    os.makedirs(directory)
    rng = np.random.default_rng(11)
    for i, (f, n) in enumerate(((140.0, 4800), (220.0, 4700), (310.0, 4600))):
        ph = 2 * np.pi * f * np.arange(n) / 16000.0
        x = 0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 1.0) + \
            0.02 * rng.standard_normal(n)
        x[1800:3300] = 0.002 * rng.standard_normal(1500)
        wavfile.write(os.path.join(directory, 'clip%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))


def test_train_evaluate_generate(hip_lib, tmp_path):
    data = str(tmp_path / 'wavs')
    _wavs(data)
    params = str(tmp_path / 'params.json')
    json.dump(base.PARAMS, open(params, 'w'))
    log = str(tmp_path / 'run')
    common = ['--data_dir', data, '--wavenet_params', params,
              '--mask_padding', 'true', '--num_steps', '2',
              '--checkpoint_every', '10', '--silence_threshold', '0.3']
    # 1. training
    base._run('train.py', common + ['--logdir', log] + FRONT + MODEL)
    import train
    ck = train.latest_checkpoint(log)
    # 2. the checkpoint's entry
    entry = torch.load(ck, map_location='cpu', weights_only=False)[
        'lc_features']
    assert entry['kind'] == 'mel+f0'
    assert (entry['n_mels'], entry['hop'], entry['n_fft'],
            entry['sample_rate']) == (8, 64, 256, 16000)
    assert 'normalizer' not in entry
    pitch = entry['pitch']
    assert (pitch['fmin'], pitch['fmax'], pitch['hop'], pitch['sample_rate'],
            pitch['path'], pitch['interpolate']) == \
        (60.0, 500.0, 64, 16000, None, True)
    from wavenet import features, frontend
    spec = frontend.MelPitchSpec.from_settings(entry)
    assert features.checkpoint_entry(spec) == entry
    # 3. evaluate.py, no front-end flag: one JSON line
    out = base._run('evaluate.py', [ck, '--data_dir', data,
                                    '--wavenet_params', params,
                                    '--batch_size', '2',
                                    '--silence_threshold', '0.3',
                                    '--lc_upsample_scales', '4,4,4'])
    res = json.loads(out.strip().splitlines()[-1])
    assert set(res) == base.OLD_KEYS
    assert res['clips'] == 3 and np.isfinite(res['nll_per_sample'])
    # 4. generate.py --lc_wav: a wav of the input's length (behind the seed
    # sample every generated file starts with)
    wav_in = os.path.join(data, 'clip2.wav')
    wav_out = str(tmp_path / 'copy.wav')
    base._run('generate.py', [ck, '--wavenet_params', params, '--lc_wav',
                              wav_in, '--lc_upsample_scales', '4,4,4',
                              '--lc_fast_generation', 'true', '--wav_out_path',
                              wav_out, '--logdir', str(tmp_path / 'gen')])
    rate, wav = wavfile.read(wav_out)
    assert rate == 16000 and wav.shape == (1 + 4600,)
    assert np.isfinite(wav).all()
    # 5. the same training from the device corpus, whole-utterance frames
    out = base._run('train.py', common + [
        '--logdir', str(tmp_path / 'run2'), '--device_corpus', 'true',
        '--lc_feature_context', 'utterance', '--sample_size', '2000',
        '--lc_normalize', 'corpus'] + FRONT + MODEL)
    ck2 = train.latest_checkpoint(str(tmp_path / 'run2'))
    entry2 = torch.load(ck2, map_location='cpu', weights_only=False)[
        'lc_features']
    assert entry2['kind'] == 'mel+f0' and entry2['pitch'] == pitch
    assert len(entry2['normalizer']['shift']) == 8
    stats = features.FeatureStats.load(os.path.join(str(tmp_path / 'run2'),
                                                    'lc_stats.npz'))
    assert stats.n_channels == 8
