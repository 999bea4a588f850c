"""evaluate.py --synthesis true --synthesis_pitch true --pitch_path true end
to end, on the tiny checkpoint recipe of tests/test_gpu_pitch_cli.py: the
"synthesis_pitch" entry names the path and its weights and holds
pitch.f0_error of the two PitchPath tracks, computed here from the wavs that
were written; without the flag the line has exactly the keys it had; and the
flag without --synthesis_pitch true is an argparse error."""
import json
import os
import subprocess
import sys

import pytest
import torch
from scipy.io import wavfile

import test_gpu_pitch_cli as base

pytestmark = pytest.mark.gpu

ROOT = base.ROOT
PITCH_KEYS = {'f0_rmse_cents', 'gross_pitch_error', 'vuv_error',
              'voiced_frames', 'frames', 'fmin', 'fmax'}


def test_evaluate_pitch_path(hip_lib, tmp_path):
    from wavenet import evaluate as ev
    from wavenet import pitch
    data = str(tmp_path / 'wavs')
    base._wavs(data)
    params = str(tmp_path / 'params.json')
    json.dump(base.PARAMS, open(params, 'w'))
    log = str(tmp_path / 'run')
    base._run('train.py', ['--data_dir', data, '--wavenet_params', params,
                           '--mask_padding', 'true', '--num_steps', '2',
                           '--checkpoint_every', '10', '--silence_threshold',
                           '0.3', '--logdir', log, '--lc_features', 'mel',
                           '--lc_n_fft', '64'] + base.MODEL)
    import train
    ck = train.latest_checkpoint(log)
    out_dir = str(tmp_path / 'copies')
    argv = [ck, '--data_dir', data, '--wavenet_params', params,
            '--batch_size', '2', '--synthesis', 'true', '--synthesis_out',
            out_dir, '--max_clips', '2', '--seed', '3', '--synthesis_pitch',
            'true'] + base.MODEL
    res = json.loads(base._run('evaluate.py', argv + [
        '--pitch_path', 'true', '--pitch_jump', '0.4']).strip()
        .splitlines()[-1])
    assert set(res) == base.OLD_KEYS | {'synthesis', 'synthesis_pitch'}
    got = res['synthesis_pitch']
    assert set(got) == PITCH_KEYS | {'tracker', 'jump', 'octave_bias',
                                     'switch'}
    assert (got['tracker'], got['jump'], got['octave_bias'], got['switch'],
            got['fmin'], got['fmax']) == ('path', 0.4, 0.05, 0.2, 60.0, 500.0)

    # the same numbers from the wavs that were written, through PitchPath
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces[:2]
    path = pitch.PitchPath(pitch.PitchTracker(16000, hop=16), jump=0.4)
    parts = []
    for audio, name, _, _ in utts:
        stem = os.path.splitext(os.path.basename(name))[0]
        rate, wav = wavfile.read(os.path.join(out_dir, stem + '.wav'))
        assert rate == 16000 and wav.shape == audio.shape
        parts.append(pitch.f0_error(path(wav), path(audio)))
    want = pitch.F0Error(*(torch.cat(t) for t in zip(*parts))).summary()
    assert want['voiced_frames'] > 0.5 * want['frames']     # harmonic clips
    for k, v in want.items():
        if v is None:
            assert got[k] is None, k
        else:
            assert got[k] == pytest.approx(v, rel=1e-9), k

    # without the flag: today's keys, and the rest of the line unchanged
    plain = json.loads(base._run('evaluate.py', argv).strip()
                       .splitlines()[-1])
    assert set(plain) == set(res)
    assert set(plain['synthesis_pitch']) == PITCH_KEYS
    assert {k: v for k, v in plain.items() if k != 'synthesis_pitch'} == \
        {k: v for k, v in res.items() if k != 'synthesis_pitch'}


def test_pitch_path_needs_synthesis_pitch():
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py'),
                        'ckpt', '--data_dir', 'in', '--synthesis', 'true',
                        '--pitch_path', 'true'], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert p.returncode == 2
    assert '--pitch_path needs --synthesis_pitch true' in p.stderr.decode()
