"""Feature normalisation from the command line: train.py --lc_normalize
corpus on a device corpus writes the statistics and a checkpoint that carries
the normaliser; evaluate.py and generate.py --lc_wav pick it up from the
checkpoint alone; the tools reproduce the statistics and the normalised
frames; --lc_normalize range needs no statistics."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import featnorm_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAMS = {"filter_width": 2, "sample_rate": 16000,
          "dilations": [1, 2, 4, 8, 16, 32],
          "residual_channels": 32, "dilation_channels": 32,
          "quantization_channels": 256, "skip_channels": 64,
          "use_biases": True, "scalar_input": False,
          "initial_filter_width": 32, "residual_postproc": False}
MODEL = ['--lc_channels', '8', '--lc_upsample_scales', '4,4']
MEL = ['--lc_n_fft', '64']
PIECES = ['--sample_size', '2000', '--batch_size', '3',
          '--silence_threshold', '0.3']
TOOL = ['--sample_rate', '16000', '--lc_channels', '8', '--lc_hop', '16',
        '--silence_threshold', '0.3'] + MEL


def _run(script, argv, seconds=300):
    """One child under its own time limit; a failure ends the test."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=seconds)
    out = p.stdout.decode()
    assert p.returncode == 0, '%s %s\n%s' % (script, ' '.join(argv), out)
    return out


def _wavs(directory):
    """Five short clips of different lengths and levels, all louder than the
    silence threshold; some begin with near silence that the trimming
    removes."""
    os.makedirs(directory)
    rng = np.random.default_rng(5)
    for i in range(5):
        n, lead = 2600 + 517 * i, 2048 * (i % 2)
        tone = (0.5 + 0.1 * i) * np.sin(
            2 * np.pi * 110.0 * (i + 2) * np.arange(n) / 16000.0) + \
            0.05 * rng.standard_normal(n)
        x = np.concatenate([0.001 * rng.standard_normal(lead), tone])
        wavfile.write(os.path.join(directory, 'clip%d.wav' % i), 16000,
                      (np.clip(x, -1, 1) * 32767).astype(np.int16))


def _validation(logdir):
    lines = [json.loads(l) for l in open(os.path.join(logdir,
                                                      'events.jsonl'))]
    return [e for e in lines if 'validation_loss' in e]


@pytest.fixture(scope='module')
def run(hip_lib, tmp_path_factory):
    """train.py on a device corpus with utterance-context features normalised
    by the corpus's own statistics, three steps, validated on the same
    directory."""
    tmp = tmp_path_factory.mktemp('featnorm_cli')
    data, params, logdir = str(tmp / 'wavs'), str(tmp / 'params.json'), \
        str(tmp / 'run')
    _wavs(data)
    json.dump(PARAMS, open(params, 'w'))
    common = ['--data_dir', data, '--wavenet_params', params,
              '--mask_padding', 'true', '--checkpoint_every', '10',
              '--lc_features', 'mel'] + MODEL + MEL + PIECES
    out = _run('train.py', common + [
        '--logdir', logdir, '--num_steps', '3', '--device_corpus', 'true',
        '--lc_feature_context', 'utterance', '--lc_normalize', 'corpus',
        '--lc_norm_clip', '4', '--validation_dir', data])
    return dict(tmp=tmp, data=data, params=params, logdir=logdir, out=out,
                common=common)


@pytest.fixture(scope='module')
def raw_frames(run):
    """The corpus's raw frames, computed here: (corpus, host [NF, 8])."""
    from wavenet import features
    from wavenet.corpus import DeviceCorpus
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    corpus = DeviceCorpus(run['data'], 16000, False, silence_threshold=0.3,
                          spec=spec)
    return corpus, corpus.frames_flat.cpu().numpy().reshape(-1, 8)


def test_train_writes_the_statistics_and_the_normaliser(run, raw_frames):
    import train
    from wavenet import features
    steps = re.findall(r'step (\d+) - loss = ([0-9.]+)', run['out'])
    assert [k for k, _ in steps] == ['0', '1', '2'], run['out']
    assert all(np.isfinite(float(v)) for _, v in steps)
    stats = features.FeatureStats.load(os.path.join(run['logdir'],
                                                    'lc_stats.npz'))
    _, raw = raw_frames
    n, s1, s2, a1, a2 = R.sums(raw[None])
    cnt, g1, g2 = stats.sums()
    assert cnt == n
    assert (np.abs(g1 - s1) <= R.sum_bound(n, a1)).all()
    assert (np.abs(g2 - s2) <= R.sum_bound(n, a2)).all()
    ck = torch.load(train.latest_checkpoint(run['logdir']),
                    map_location='cpu')
    entry = ck['lc_features']
    assert entry['kind'] == 'mel' and entry['n_fft'] == 64
    want = features.Normalizer.from_stats(stats, clip=4.0)
    assert entry['normalizer'] == want.entry()
    assert entry['normalizer']['lo'] == -4.0 and \
        entry['normalizer']['count'] == n
    assert ck['device_corpus']['lc_feature_context'] == 'utterance'


def test_evaluate_takes_the_normaliser_from_the_checkpoint(run):
    import train
    ck = train.latest_checkpoint(run['logdir'])
    val = _validation(run['logdir'])
    assert [e['step'] for e in val] == [0, 2]
    ev = [ck, '--data_dir', run['data'], '--wavenet_params', run['params']] \
        + MODEL + PIECES
    got = json.loads(_run('evaluate.py', ev).strip().splitlines()[-1])
    assert got['clips'] > 0 and np.isfinite(got['nll_per_sample'])
    # the weights after the last step: train.py's last validation line
    assert abs(val[-1]['validation_loss'] - got['nll_per_sample']) <= \
        1e-9 * got['nll_per_sample']
    assert 'validation loss = %.3f' % got['nll_per_sample'] in run['out']
    off = json.loads(_run('evaluate.py', ev + ['--lc_normalize', 'none'])
                     .strip().splitlines()[-1])
    assert np.isfinite(off['nll_per_sample']) and \
        off['nll_per_sample'] != got['nll_per_sample']
    assert off['samples'] == got['samples']


def test_generate_lc_wav_runs_from_the_checkpoint(run):
    import train
    ck = train.latest_checkpoint(run['logdir'])
    wav = str(run['tmp'] / 'copy.wav')
    _run('generate.py', [ck, '--wavenet_params', run['params'], '--lc_wav',
                         os.path.join(run['data'], 'clip1.wav'),
                         '--lc_upsample_scales', '4,4', '--samples', '150',
                         '--lc_fast_generation', 'true', '--wav_out_path',
                         wav, '--logdir', str(run['tmp'] / 'gen')])
    rate, got = wavfile.read(wav)
    assert rate == 16000 and got.shape == (1 + 150,)
    assert np.isfinite(got).all()


def test_a_continued_run_keeps_its_normaliser(run):
    import train
    log = str(run['tmp'] / 'continued')
    shutil.copytree(run['logdir'], log)
    before = torch.load(train.latest_checkpoint(log),
                        map_location='cpu')['lc_features']
    out = _run('train.py', run['common'] + [
        '--logdir', log, '--num_steps', '4', '--device_corpus', 'true',
        '--lc_feature_context', 'utterance'])
    assert 'feature normaliser continues' in out
    assert re.findall(r'step (\d+) - loss', out) == ['3']
    ck = train.latest_checkpoint(log)
    assert ck.endswith('model.ckpt-3')
    assert torch.load(ck, map_location='cpu')['lc_features'] == before


def test_the_tools_reproduce_statistics_and_frames(run, raw_frames):
    from wavenet import audio_reader as ar, features
    corpus, raw = raw_frames
    data = str(run['tmp'] / 'wavs_copy')
    shutil.copytree(run['data'], data)
    path = str(run['tmp'] / 'tool_stats.npz')
    out = _run('tools/make_lc_stats.py', [data, '--out', path] + TOOL)
    assert 'frames' in out
    tool = features.FeatureStats.load(path)
    n, s1, s2, a1, a2 = R.sums(raw[None])
    cnt, g1, g2 = tool.sums()
    assert cnt == n
    assert (np.abs(g1 - s1) <= R.sum_bound(n, a1)).all()
    assert (np.abs(g2 - s2) <= R.sum_bound(n, a2)).all()
    # the normalised .npy files: a whole utterance's frames are the corpus's
    # (the trimming starts at a multiple of 512, which the hop divides)
    stats = os.path.join(run['logdir'], 'lc_stats.npz')
    _run('tools/make_lc_features.py',
         [data, '--lc_normalize', 'corpus', '--lc_stats', stats,
          '--lc_norm_clip', '4'] + TOOL)
    norm = features.Normalizer.from_stats(features.FeatureStats.load(stats),
                                          clip=4.0)
    want = norm.reference(raw)
    files = ar.find_files(data)
    assert len(files) == 5 and len(ar.find_files(data, '*.npy')) == 5
    assert [os.path.basename(f) for f in corpus.files] == \
        [os.path.basename(f) for f in files]
    o = 0
    for f, F in zip(files, corpus.frame_counts.tolist()):
        audio = ar.load_wav(f, 16000)
        lo, hi = (int(v) for v in ar.trim_bounds(audio, 0.3))
        assert lo % 16 == 0 and -(-(hi - lo) // 16) == F
        feats = np.load(ar.lc_path_of(f))
        assert feats.dtype == np.float32 and \
            feats.shape == (-(-audio.shape[0] // 16), 8)
        f0 = lo // 16
        assert feats[f0:f0 + F].tobytes() == want[o:o + F].tobytes()
        assert not feats[:f0].any() and not feats[f0 + F:].any()
        o += F
    assert o == raw.shape[0]


def test_range_normalisation_needs_no_statistics(run):
    import train
    from wavenet import features
    log = str(run['tmp'] / 'range')
    out = _run('train.py', run['common'] + [
        '--logdir', log, '--num_steps', '2', '--lc_normalize', 'range',
        '--lc_range', '-23,7'])
    assert re.findall(r'step (\d+) - loss', out) == ['0', '1']
    assert not os.path.exists(os.path.join(log, 'lc_stats.npz'))
    entry = torch.load(train.latest_checkpoint(log),
                       map_location='cpu')['lc_features']
    assert entry['normalizer'] == \
        features.Normalizer.from_range(-23.0, 7.0, 8).entry()
    assert 'device_corpus' not in torch.load(train.latest_checkpoint(log),
                                             map_location='cpu')
