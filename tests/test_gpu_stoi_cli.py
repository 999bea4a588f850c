"""evaluate.py --synthesis true --synthesis_stoi true end to end: the tiny
local-conditioning model of tests/test_gpu_pitch_cli.py trained a few steps,
two utterances of half a second copy-synthesised and reconstructed by
Griffin-Lim; the "synthesis_stoi" entry and the baseline's "stoi" sub-entry
against the float64 restatement (tests/stoi_ref.py) applied here to the wavs
that were written, within the bound of tests/test_gpu_stoi.py; without the
switch the JSON line is what it was."""
import json
import os

import numpy as np
import pytest
from scipy.io import wavfile

import stoi_ref as S
from test_gpu_pitch_cli import MODEL, OLD_KEYS, PARAMS, SYNTHESIS_KEYS, _run

pytestmark = pytest.mark.gpu

STOI_KEYS = {'stoi', 'estoi', 'clips', 'skipped_clips', 'segments',
             'kept_frames', 'frames', 'sample_rate'}


def _wavs(directory):
    """Three harmonic clips of about half a second (30 frames at 10 kHz are
    6554 samples at 16 kHz)."""
    os.makedirs(directory)
    rng = np.random.default_rng(9)
    for i, (f, n) in enumerate(((140.0, 7400), (220.0, 8000), (310.0, 7000))):
        ph = 2 * np.pi * f * np.arange(n) / 16000.0
        x = 0.5 * np.sin(ph) + 0.25 * np.sin(2 * ph + 1.0) + \
            0.02 * rng.standard_normal(n)
        wavfile.write(os.path.join(directory, 'clip%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _recomputed(meter, pairs):
    """(the restatement's corpus entry, the bound per score) of (generated,
    original) pairs."""
    results, tol = [], {'stoi': 0.0, 'estoi': 0.0}
    for wav, audio in pairs:
        want = S.stoi64(wav, audio, meter.resampler)
        assert S.decisive(want['margin']) and want['segments'] > 0
        ref = meter.reference(wav, audio)
        assert ref['kept'] == want['kept']
        alt = S.alt32(wav, audio, meter.resampler, want['keep'])
        for k, other in (('stoi', alt[0]), ('estoi', alt[1])):
            tol[k] = max(tol[k], S.bound(want[k], [
                ref[k + '_sum'] / ref['segments'], other]))
        results.append(want)
    return S.corpus(results), tol


def test_evaluate_synthesis_stoi(hip_lib, tmp_path):
    from wavenet import evaluate as ev
    from wavenet import stoi
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
            out_dir, '--max_clips', '2', '--seed', '3',
            '--synthesis_baseline', 'griffin_lim', '--gl_iterations', '8'] + \
        MODEL
    res = json.loads(_run('evaluate.py', argv + ['--synthesis_stoi', 'true'])
                     .strip().splitlines()[-1])
    top = OLD_KEYS | {'synthesis', 'synthesis_baseline'}
    assert set(res) == top | {'synthesis_stoi'}
    assert set(res['synthesis']) == SYNTHESIS_KEYS       # keeps its keys
    got, base = res['synthesis_stoi'], res['synthesis_baseline']['stoi']
    assert set(got) == set(base) == STOI_KEYS

    # the same numbers from the wavs that were written
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces[:2]
    meter = stoi.Stoi(16000)
    for entry, suffix in ((got, ''), (base, '_gl')):
        pairs = []
        for audio, path, _, _ in utts:
            stem = os.path.splitext(os.path.basename(path))[0]
            rate, wav = wavfile.read(os.path.join(out_dir,
                                                  stem + suffix + '.wav'))
            assert rate == 16000 and wav.dtype == np.float32 and \
                wav.shape == audio.shape
            pairs.append((wav, audio))
        want, tol = _recomputed(meter, pairs)
        for k in STOI_KEYS - {'stoi', 'estoi'}:
            assert entry[k] == want[k], (suffix, k)
        assert entry['clips'] == 2 and entry['sample_rate'] == 10000
        for k in ('stoi', 'estoi'):
            err = abs(entry[k] - want[k])
            print('%s%s: evaluate.py %.9f, float64 %.9f, error %.3e, bound '
                  '%.3e' % (k, suffix, entry[k], want[k], err, tol[k]))
            assert err <= tol[k], (suffix, k)
    # Griffin-Lim keeps the envelopes; two training steps do not
    assert base['stoi'] > got['stoi']

    # without the switch: no such key, the line of before
    plain_dir = str(tmp_path / 'plain')
    plain = json.loads(_run('evaluate.py', [
        plain_dir if v == out_dir else v for v in argv])
        .strip().splitlines()[-1])
    assert set(plain) == top
    assert 'stoi' not in plain['synthesis_baseline']
    res['synthesis_baseline'].pop('stoi')
    assert plain == {k: res[k] for k in plain}
