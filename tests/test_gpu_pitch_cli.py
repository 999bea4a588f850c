"""evaluate.py --synthesis true --synthesis_pitch true end to end: a tiny
local-conditioning model trained a few steps, two utterances copy-synthesised,
and the "synthesis_pitch" entry against pitch.f0_error computed here from the
wavs that were written and the originals.  Without the flag the JSON line is
what it was."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"filter_width": 2, "sample_rate": 16000,
          "dilations": [1, 2, 4, 8, 16, 1, 2, 4, 8, 16],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 256, "skip_channels": 64,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
MODEL = ['--lc_channels', '8', '--lc_upsample_scales', '4,4']
OLD_KEYS = {'nll_per_sample', 'bits_per_sample', 'accuracy', 'samples',
            'clips'}
SYNTHESIS_KEYS = {'clips', 'samples', 'steps', 'occupancy', 'log_mel_mae_db',
                  'log_mel_lsd_db'}


def _run(script, argv, seconds=300):
    """One child under its own time limit; a failure ends the test."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    out = p.stdout.decode()
    assert p.returncode == 0, '%s %s\n%s' % (script, ' '.join(argv), out)
    return out


def _wavs(directory):
    """Three short harmonic clips of different lengths and pitches."""
    os.makedirs(directory)
    rng = np.random.default_rng(9)
    for i, (f, n) in enumerate(((140.0, 2600), (220.0, 3000), (310.0, 2200))):
        ph = 2 * np.pi * f * np.arange(n) / 16000.0
        x = 0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 1.0) + \
            0.02 * rng.standard_normal(n)
        wavfile.write(os.path.join(directory, 'clip%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))


def test_evaluate_synthesis_pitch(hip_lib, tmp_path):
    from wavenet import evaluate as ev
    from wavenet import pitch
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
    out_dir = str(tmp_path / 'copies')
    argv = [ck, '--data_dir', data, '--wavenet_params', params,
            '--batch_size', '2', '--synthesis', 'true', '--synthesis_out',
            out_dir, '--max_clips', '2', '--seed', '3'] + MODEL
    res = json.loads(_run('evaluate.py', argv + ['--synthesis_pitch', 'true'])
                     .strip().splitlines()[-1])
    assert set(res) == OLD_KEYS | {'synthesis', 'synthesis_pitch'}
    assert set(res['synthesis']) == SYNTHESIS_KEYS
    got = res['synthesis_pitch']
    assert set(got) == {'f0_rmse_cents', 'gross_pitch_error', 'vuv_error',
                        'voiced_frames', 'frames', 'fmin', 'fmax'}
    assert got['fmin'] == 60.0 and got['fmax'] == 500.0

    # the same numbers from the wavs that were written, utterance by utterance
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces[:2]
    tracker = pitch.PitchTracker(16000, hop=16)
    parts = []
    for audio, path, _, _ in utts:
        stem = os.path.splitext(os.path.basename(path))[0]
        rate, wav = wavfile.read(os.path.join(out_dir, stem + '.wav'))
        assert rate == 16000 and wav.dtype == np.float32 and \
            wav.shape == audio.shape
        parts.append(pitch.f0_error(tracker(wav), tracker(audio)))
    assert sorted(os.listdir(out_dir)) == sorted(
        os.path.splitext(os.path.basename(p[1]))[0] + '.wav' for p in utts)
    want = pitch.F0Error(*(torch.cat(t) for t in zip(*parts))).summary()
    assert want['frames'] == sum(-(-p[0].shape[0] // 16) for p in utts)
    assert want['voiced_frames'] > 0.5 * want['frames']     # harmonic clips
    for k, v in want.items():
        if v is None:
            assert got[k] is None, k
        else:
            assert got[k] == pytest.approx(v, rel=1e-9), k

    # without the flag: no such key, the line of before
    plain = json.loads(_run('evaluate.py', argv).strip().splitlines()[-1])
    assert set(plain) == OLD_KEYS | {'synthesis'}
    assert plain == {k: res[k] for k in plain}
