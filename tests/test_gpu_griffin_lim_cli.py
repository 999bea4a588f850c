"""evaluate.py --synthesis true --synthesis_baseline griffin_lim end to end:
the tiny local-conditioning model of tests/test_gpu_pitch_cli.py trained a few
steps, two utterances copy-synthesised AND reconstructed by Griffin-Lim from
their natural log-mel features; the "synthesis_baseline" entry against the
helpers applied here to the <stem>_gl.wav files that were written, which are
bit for bit what griffin_lim.GriffinLim gives here under another grouping;
without the switch the JSON line is what it was.  And tools/griffin_lim.py from
an .npy of frames with --checkpoint and from a wav with flags."""
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from test_gpu_pitch_cli import (MODEL, OLD_KEYS, PARAMS, SYNTHESIS_KEYS,
                                _run, _wavs)

pytestmark = pytest.mark.gpu

BASE_KEYS = {'kind', 'iterations', 'momentum', 'clips', 'samples',
             'log_mel_mae_db', 'log_mel_lsd_db'}


def test_evaluate_baseline_and_the_tool(hip_lib, tmp_path):
    from wavenet import evaluate as ev
    from wavenet import features, griffin_lim, pitch, spectral, synthesis
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
            '--synthesis_stft', 'true', '--stft_resolutions', '64:16:64',
            '--synthesis_mcd', 'true', '--mcd_order', '5',
            '--synthesis_pitch', 'true'] + MODEL
    res = json.loads(_run('evaluate.py', argv + [
        '--synthesis_baseline', 'griffin_lim', '--gl_iterations', '8',
        '--gl_momentum', '0.5']).strip().splitlines()[-1])
    top = OLD_KEYS | {'synthesis', 'synthesis_stft', 'synthesis_mcd',
                      'synthesis_pitch'}
    assert set(res) == top | {'synthesis_baseline'}
    assert set(res['synthesis']) == SYNTHESIS_KEYS
    got = res['synthesis_baseline']
    assert set(got) == BASE_KEYS | {'stft', 'mcd', 'pitch'}
    assert (got['kind'], got['iterations'], got['momentum']) == \
        ('griffin_lim', 8, 0.5)
    assert got['clips'] == res['synthesis']['clips'] == 2
    assert got['samples'] == res['synthesis']['samples']
    assert set(got['stft']) == set(res['synthesis_stft'])
    assert set(got['mcd']) == set(res['synthesis_mcd'])
    assert set(got['pitch']) == set(res['synthesis_pitch'])

    # the same numbers from the wavs that were written
    utts = ev.ValidationSet(data, 16000, silence_threshold=0.3).pieces[:2]
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    wavs, origs = [], []
    for audio, path, _, _ in utts:
        stem = os.path.splitext(os.path.basename(path))[0]
        assert os.path.exists(os.path.join(out_dir, stem + '.wav'))
        rate, wav = wavfile.read(os.path.join(out_dir, stem + '_gl.wav'))
        assert rate == 16000 and wav.dtype == np.float32 and \
            wav.shape == audio.shape
        wavs.append(torch.from_numpy(wav).cuda())
        origs.append(audio)
    groups = [[0, 1]]
    mae, lsd = synthesis.log_mel_distance(spec, wavs, origs, groups)
    assert got['log_mel_mae_db'] == pytest.approx(mae, rel=1e-9)
    assert got['log_mel_lsd_db'] == pytest.approx(lsd, rel=1e-9)
    assert mae > 0                     # pinv-and-clip is not an exact inverse
    dist = spectral.StftDistance(((64, 16, 64),))
    want = synthesis.stft_distance(dist, wavs, origs, groups)
    for k in ('spectral_convergence', 'log_stft_magnitude'):
        assert got['stft'][k] == pytest.approx(want[k], rel=1e-9), k
    w = synthesis.mel_cepstral_distortion(spec, wavs, origs, groups, 5)
    assert got['mcd']['mcd_db'] == pytest.approx(w['mcd_db'], rel=1e-9)
    assert got['mcd']['frames'] == w['frames']
    p = synthesis.pitch_distance(pitch.PitchTracker(16000, hop=16), wavs,
                                 origs, groups)
    for k, v in p.items():
        if isinstance(v, float):
            assert got['pitch'][k] == pytest.approx(v, rel=1e-9), k
        else:
            assert got['pitch'][k] == v, k
    # ... which are the bits of a run here, one utterance per group
    gl = griffin_lim.GriffinLim(spec, iterations=8, momentum=0.5, seed=3)
    mine = synthesis.griffin_lim_baseline(gl, spec, origs, [[1], [0]])
    for a, b in zip(mine, wavs):
        assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))
    with pytest.raises(ValueError, match='another front end'):
        synthesis.griffin_lim_baseline(
            griffin_lim.GriffinLim(features.MelSpec(16000, n_fft=64, hop=16,
                                                    n_mels=9)),
            spec, origs, groups)

    # without the switch: no such key, no _gl.wav, the line of before
    plain_dir = str(tmp_path / 'plain')
    plain = json.loads(_run('evaluate.py', [
        plain_dir if v == out_dir else v for v in argv])
        .strip().splitlines()[-1])
    assert set(plain) == top
    assert plain == {k: res[k] for k in plain}
    assert sorted(os.listdir(plain_dir)) == sorted(
        f for f in os.listdir(out_dir) if not f.endswith('_gl.wav'))

    # tools/griffin_lim.py: from a wav with flags ...
    audio, path = utts[0][0], utts[0][1]
    out = str(tmp_path / 'tool' / 'from_wav.wav')
    said = _run('tools/griffin_lim.py', [
        path, '--out', out, '--sample_rate', '16000', '--lc_channels', '8',
        '--lc_hop', '16', '--lc_n_fft', '64', '--gl_iterations', '4'])
    rate, wav = wavfile.read(out)
    from wavenet import audio_reader as ar
    whole = ar.load_wav(path, 16000)
    assert rate == 16000 and wav.dtype == np.float32 and \
        wav.shape == whole.shape and str(whole.shape[0]) in said
    gl4 = griffin_lim.GriffinLim(spec, iterations=4)
    mine = gl4(spec(whole), lengths=[whole.shape[0]])
    assert np.array_equal(mine.cpu().numpy().view(np.int32), wav.view(np.int32))
    assert np.isfinite(wav).all() and np.abs(wav).max() > 0.01
    # ... and from an .npy of frames with the checkpoint's front end
    frames = spec(audio).cpu().numpy()
    npy = str(tmp_path / 'tool' / 'frames.npy')
    np.save(npy, frames)
    out = str(tmp_path / 'tool' / 'from_npy.wav')
    _run('tools/griffin_lim.py', [npy, '--out', out, '--checkpoint', ck,
                                  '--gl_iterations', '4'])
    rate, wav = wavfile.read(out)
    assert rate == 16000 and wav.shape == (frames.shape[0] * 16,)
    mine = gl4(frames)
    assert np.array_equal(mine.cpu().numpy().view(np.int32), wav.view(np.int32))


@pytest.mark.parametrize('kind,channels', [('mel', 8), ('mel+f0', 10)])
def test_the_tool_inverts_a_normalised_npy(hip_lib, tmp_path, kind, channels):
    """An .npy of NORMALISED frames, as tools/make_lc_features.py writes them
    for a front end with a normaliser, mel and mel+f0 (run in this process:
    the command line itself is the test above): the wav is, bit for bit,
    Griffin-Lim of the inverted mel channels, and those are the raw log-mel
    frames within the clamp (four float32 operations on values within 40 of
    each other: 4 * 40 * 2^-24)."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), 'tools')
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import griffin_lim as tool
    from wavenet import griffin_lim
    ph = 2 * np.pi * 180.0 * np.arange(1500) / 16000.0
    audio = (0.5 * np.sin(ph) + 0.2 * np.sin(3 * ph + 1.0)).astype(np.float32)
    npy, out = str(tmp_path / 'f.npy'), str(tmp_path / 'o.wav')
    lo, hi = -14.0, 2.0
    argv = [npy, '--out', out, '--sample_rate', '16000', '--lc_channels',
            str(channels), '--lc_hop', '16', '--lc_n_fft', '64',
            '--lc_features', kind, '--lc_normalize', 'range', '--lc_range',
            '%g,%g' % (lo, hi), '--gl_iterations', '4', '--seed', '5']
    spec = tool.front_end(tool.get_arguments(argv))
    normed = spec(audio).cpu().numpy()
    assert normed.shape == (94, channels)
    assert normed[:, :8].min() >= 0 and normed[:, :8].max() <= 1
    np.save(npy, normed)
    assert tool.main(argv) == 0
    rate, wav = wavfile.read(out)
    assert rate == 16000 and wav.shape == (94 * 16,) and np.isfinite(wav).all()
    mel = spec if kind == 'mel' else spec.mel
    raw = mel.with_normalizer(None)(audio).cpu().numpy()
    back = spec.normalizer.invert(np.ascontiguousarray(normed[:, :8])).numpy()
    assert np.abs(back - np.clip(raw, lo, hi)).max() <= 4 * 40 * 2.0 ** -24
    gl = griffin_lim.GriffinLim(mel.with_normalizer(None), iterations=4, seed=5)
    assert np.array_equal(gl(back).cpu().numpy().view(np.int32),
                          wav.view(np.int32))
    # (not what the normalised values themselves would give)
    assert not np.array_equal(
        gl(np.ascontiguousarray(normed[:, :8])).cpu().numpy().view(np.int32),
        wav.view(np.int32))
