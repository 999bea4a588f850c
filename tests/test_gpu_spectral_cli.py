"""evaluate.py --synthesis true --synthesis_stft true --synthesis_mcd true end
to end: the tiny local-conditioning model of tests/test_gpu_pitch_cli.py
trained a few steps, two utterances copy-synthesised, and the "synthesis_stft"
and "synthesis_mcd" entries against spectral.StftDistance and
synthesis.mel_cepstral_distortion applied here to the wavs that were written
and the originals.  Without the flags the JSON line is what it was."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from test_gpu_pitch_cli import (MODEL, OLD_KEYS, PARAMS, SYNTHESIS_KEYS,
                                _run, _wavs)

pytestmark = pytest.mark.gpu

RES = '64:16:64,128:32:96'


def test_evaluate_synthesis_stft_and_mcd(hip_lib, tmp_path):
    from wavenet import evaluate as ev
    from wavenet import features, spectral, synthesis
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
    res = json.loads(_run('evaluate.py', argv + [
        '--synthesis_stft', 'true', '--stft_resolutions', RES,
        '--synthesis_mcd', 'true', '--mcd_order', '5'])
        .strip().splitlines()[-1])
    assert set(res) == OLD_KEYS | {'synthesis', 'synthesis_stft',
                                   'synthesis_mcd'}
    assert set(res['synthesis']) == SYNTHESIS_KEYS
    for k in OLD_KEYS | SYNTHESIS_KEYS:
        v = res.get(k, res['synthesis'].get(k))
        assert isinstance(v, (int, float)), k
    got = res['synthesis_stft']
    assert set(got) == {'spectral_convergence', 'log_stft_magnitude',
                        'per_resolution'}
    assert [set(p) for p in got['per_resolution']] == \
        [{'n_fft', 'hop', 'win_length', 'spectral_convergence',
          'log_stft_magnitude'}] * 2
    assert [(p['n_fft'], p['hop'], p['win_length'])
            for p in got['per_resolution']] == [(64, 16, 64), (128, 32, 96)]
    mcd = res['synthesis_mcd']
    assert set(mcd) == {'mcd_db', 'order', 'n_mels', 'frames'}
    assert (mcd['order'], mcd['n_mels']) == (5, 8)

    # the same numbers from the wavs that were written, utterance by
    # utterance: a clip's sums do not depend on how evaluate.py grouped it
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces[:2]
    dist = spectral.StftDistance(((64, 16, 64), (128, 32, 96)))
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    wavs, origs, parts, cep = [], [], [], []
    for audio, path, _, _ in utts:
        stem = os.path.splitext(os.path.basename(path))[0]
        rate, wav = wavfile.read(os.path.join(out_dir, stem + '.wav'))
        assert rate == 16000 and wav.dtype == np.float32 and \
            wav.shape == audio.shape
        wavs.append(torch.from_numpy(wav).cuda())
        origs.append(audio)
        parts.append(dist(wav, audio))
        cep.append(spectral.cepstral_distance(spec(wav), spec(audio),
                                              None, 5))
    lengths = [int(w.shape[0]) for w in wavs]
    alone = spectral.StftSums.cat(parts)
    # ... and grouped as evaluate.py groups them: one padded batch
    (g, o, n), = synthesis._padded_groups(wavs, origs, [[0, 1]])
    batch = dist(g, o, n)
    for x, y in zip(alone, batch):
        assert torch.equal(x.cpu().view(torch.int64),
                           y.cpu().view(torch.int64))
    nf = -(-n // 16)
    both = spectral.cepstral_distance(spec(g, n), spec(o, n), nf, 5)
    assert torch.equal(torch.cat(cep).cpu().view(torch.int64),
                       both.cpu().view(torch.int64))
    want = alone.summary(lengths)
    assert want['spectral_convergence'] > 0
    for k in ('spectral_convergence', 'log_stft_magnitude'):
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
        for p, q in zip(got['per_resolution'], want['per_resolution']):
            assert p[k] == pytest.approx(q[k], rel=1e-12), k
    w = synthesis.mel_cepstral_distortion(spec, wavs, origs, [[1], [0]], 5)
    assert w['frames'] == mcd['frames'] == \
        sum(-(-p[0].shape[0] // 16) for p in utts)
    assert mcd['mcd_db'] == pytest.approx(w['mcd_db'], rel=1e-12)
    assert mcd['mcd_db'] == pytest.approx(
        spectral.mcd_db(torch.cat(cep), [int(v) for v in nf]), rel=1e-12)
    assert mcd['mcd_db'] > 0
    s = synthesis.stft_distance(dist, wavs, origs, [[0, 1]])
    assert s == want

    # without the flags: no such key, the line of before
    plain = json.loads(_run('evaluate.py', argv).strip().splitlines()[-1])
    assert set(plain) == OLD_KEYS | {'synthesis'}
    assert plain == {k: res[k] for k in plain}
