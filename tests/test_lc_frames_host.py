"""The mel + F0 front end's host side (wavenet/frontend.py, include/
wavenet_lc_frames.h) without a device: MelPitchSpec.reference_channels against
the float64 restatement of tests/lc_frames_ref.py on hand-made tracks (H1),
mode 0 against the formula of PitchTracker.channels (H2), the constructor's
refusals before the library (H3), settings and checkpoint entries (H4), the
argparse errors of the new flags (H5), the binding table against the header
(H6) and the coverage of its writing entries by
tests/test_gpu_guard_lc_frames.py (H7)."""
import argparse
import math
import os
import re

import numpy as np
import pytest

import lc_frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'wavenet_lc_frames.h'
OTHERS = ('wavenet_hip.h', 'wavenet_pitch.h', 'wavenet_pitch_path.h')
# two correct float64 evaluations differ by ~1e-16, which can flip the single
# rounding to float32 by one float32 ulp: at most 2^-24 on [0, 1]; twice that
BOUND = 2.0 ** -23


def _no_library(monkeypatch):
    from wavenet import _lib

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libwavenet_hip.so')


def _spec(interpolate=False, path=False, hop=64, n_mels=8, **tracker_kw):
    from wavenet import features, frontend, pitch
    mel = features.MelSpec(16000, n_fft=256, hop=hop, n_mels=n_mels)
    t = pitch.PitchTracker(16000, hop=hop, **tracker_kw)
    return frontend.MelPitchSpec(mel, t, pitch.PitchPath(t) if path else None,
                                 interpolate)


# ------------------------------------------ H1: the rule on hand-made tracks
def _hand_tracks():
    F = 23
    z = np.zeros(F, np.float32)
    tracks = {'all unvoiced': z.copy()}
    for name, at in (('first', 0), ('middle', 11), ('last', F - 1)):
        t = z.copy()
        t[at] = 140.0
        tracks['one voiced frame, %s' % name] = t
    t = R.track(F, [(0, 3), (4, 6), (16, 19)], seed=1)
    tracks['gaps of 1 and of 10 frames'] = t
    t = R.track(F, [(2, 20)], seed=2)
    t[5], t[6], t[9] = np.nan, -100.0, -0.0
    t[12], t[13] = 30.0, 900.0                     # (clamped to 0 and to 1)
    tracks['NaN, negative and out-of-range f0'] = t
    t = R.track(F, [(0, F)], seed=3)
    t[7] = np.inf
    tracks['all voiced, one infinite'] = t
    return tracks


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('name', sorted(_hand_tracks()))
def test_reference_channels_against_the_restatement(monkeypatch, name, mode):
    _no_library(monkeypatch)
    spec = _spec()
    f0 = _hand_tracks()[name]
    F = f0.shape[0]
    for n in (F, F - 1, 12, 1, 0):
        got = spec.reference_channels(f0, [n], mode)
        ch0, flag = R.channels(f0, n, mode, 60.0, 500.0)
        assert got.dtype == np.float32 and got.shape == (F, 2)
        assert np.array_equal(got[:, 1], flag), (name, n)
        assert np.abs(got[:, 0].astype(np.float64) - ch0).max() <= BOUND
        assert (got[n:] == 0).all()
        assert ((got[:, 0] >= 0) & (got[:, 0] <= 1)).all()
    # a batch with ragged nframes is its clips
    batch = np.stack([f0, f0[::-1], f0])
    n = [F, 0, 9]
    got = spec.reference_channels(batch, n, mode)
    for b in range(3):
        assert np.array_equal(got[b], spec.reference_channels(batch[b],
                                                              [n[b]], mode))


def test_interpolation_has_no_step_at_a_voicing_edge(monkeypatch):
    _no_library(monkeypatch)
    spec = _spec(interpolate=True)
    f0 = np.zeros(12, np.float32)
    f0[2], f0[8] = 120.0, 240.0
    got = spec.reference_channels(f0)
    ra, rb = R.rel(120.0, 60.0, 500.0), R.rel(240.0, 60.0, 500.0)
    want = [ra, ra, ra] + [ra + (rb - ra) * k / 6 for k in range(1, 6)] + \
        [rb] * 4
    assert np.abs(got[:, 0] - np.array(want)).max() <= BOUND
    assert got[:, 1].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0]
    with pytest.raises(ValueError):
        spec.reference_channels(f0, mode=2)
    with pytest.raises(ValueError):
        spec.reference_channels(f0, [13])


# ---------------------------------------------------- H2: mode 0 is channels
def test_mode_zero_is_the_formula_of_tracker_channels(monkeypatch):
    _no_library(monkeypatch)
    spec = _spec(fmin=70.0, fmax=410.0)
    rng = np.random.default_rng(5)
    f0 = np.exp(rng.uniform(math.log(40.0), math.log(700.0), (3, 50))) \
        .astype(np.float32)
    f0[rng.uniform(size=f0.shape) < 0.4] = 0
    n = np.array([50, 17, 0])
    voiced = (f0 > 0) & (np.arange(50)[None, :] < n[:, None])
    safe = np.where(voiced, f0.astype(np.float64), 70.0)
    rel = np.log2(safe / 70.0) / math.log2(410.0 / 70.0)
    want = np.stack([np.where(voiced, np.clip(rel, 0.0, 1.0), 0.0)
                     .astype(np.float32), voiced.astype(np.float32)], -1)
    got = spec.reference_channels(f0, n, 0)
    assert np.array_equal(got[..., 1], want[..., 1])
    assert np.abs(got[..., 0] - want[..., 0]).max() <= BOUND
    # ... and of the torch ops themselves, on the CPU
    import torch
    ch = spec.tracker.channels(torch.from_numpy(f0), n).numpy()
    assert np.array_equal(got[..., 1], ch[..., 1])
    assert np.abs(got[..., 0] - ch[..., 0]).max() <= BOUND


# ------------------------------------------------- H3: refusals, attributes
def test_constructor_refuses_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features, frontend, pitch
    mel = features.MelSpec(16000, n_fft=256, hop=64, n_mels=8)
    t = pitch.PitchTracker(16000, hop=64)
    bad = [
        (dict(sample_rate=16000, hop=64), t, None, False),
        (mel, 16000, None, False),
        (mel, pitch.PitchPath(t), None, False),
        (mel, t, t, False),
        (mel, t, pitch.PitchPath(pitch.PitchTracker(16000, hop=64)), False),
        (mel, pitch.PitchTracker(16000, hop=32), None, False),
        (mel, pitch.PitchTracker(22050, hop=64), None, False),
        (mel, t, None, 1), (mel, t, None, 'true'), (mel, t, None, None),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            frontend.MelPitchSpec(*args)
    spec = frontend.MelPitchSpec(mel, t, pitch.PitchPath(t), True)
    assert (spec.hop, spec.sample_rate, spec.n_mels, spec.channels) == \
        (64, 16000, 8, 10)
    assert spec.num_frames(129) == 3 and spec.mode == 1
    assert spec.normalizer is None and spec.mel.normalizer is None
    assert features.is_spec(spec) and features.is_spec(mel)
    assert not features.is_spec(t) and not features.is_spec(None)
    assert mel.channels == 8
    # the normaliser is the mel channels'
    norm = features.Normalizer.from_range(-23.0, 7.0, 8)
    with pytest.raises(ValueError):
        spec.with_normalizer(features.Normalizer.from_range(-23.0, 7.0, 10))
    other = spec.with_normalizer(norm)
    assert other.normalizer is norm and spec.normalizer is None
    assert other.tracker is t and other.path is spec.path
    assert other.mel.normalizer is None and other.mel.melw is mel.melw
    assert other.with_normalizer(None).normalizer is None
    # bad audio: before the library too
    for audio, lengths in ((np.zeros((2, 100), np.int16), None),
                           (np.zeros((2, 3, 4), np.float32), None),
                           (np.zeros((0, 4), np.float32), None),
                           (np.zeros((2, 100), np.float32), [100]),
                           (np.zeros((2, 100), np.float32), [0, 100])):
        with pytest.raises(ValueError):
            spec(audio, lengths)


# ------------------------------------------- H4: settings and checkpoints
def test_settings_round_trip(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features, frontend, pitch
    norm = features.Normalizer(np.linspace(-9, -2, 8), np.linspace(0.3, 2, 8),
                               -4.0, 4.0, count=123)
    mel = features.MelSpec(22050, n_fft=512, hop=100, n_mels=8,
                           win_length=400, fmin=30.0, fmax=9000.0,
                           floor=1e-7, normalizer=norm)
    t = pitch.PitchTracker(22050, hop=100, fmin=70.3, fmax=412.7, window=576,
                           threshold=0.1 + 0.2, silence=3e-9)
    for path, interp in ((None, False), (pitch.PitchPath(t, jump=0.7), True)):
        spec = frontend.MelPitchSpec(mel, t, path, interp)
        d = spec.settings()
        assert set(d) == set(mel.settings()) | {'pitch'}
        assert {k: v for k, v in d.items() if k != 'pitch'} == mel.settings()
        assert set(d['pitch']) == set(t.settings()) | {'path', 'interpolate'}
        assert d['pitch']['interpolate'] is interp
        if path is None:
            assert d['pitch']['path'] is None
        else:
            assert d['pitch']['path'] == {k: v for k, v in
                                          path.settings().items()
                                          if k != 'tracker'}
        again = frontend.MelPitchSpec.from_settings(d)
        assert again.settings() == d
        assert np.array_equal(again.normalizer.shift, norm.shift)
        assert (again.path is None) == (path is None)
    with pytest.raises(ValueError):
        frontend.MelPitchSpec.from_settings(mel.settings())


def _parser():
    from wavenet import features
    p = argparse.ArgumentParser()
    p.add_argument('--lc_channels', type=int, default=None)
    features.add_cli_flags(p)
    return p


def test_checkpoint_entry_round_trip(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features, frontend
    p = _parser()
    # mel: what it was
    a = p.parse_args(['--lc_features', 'mel', '--lc_n_fft', '256'])
    mel = features.spec_from_cli(a, 16000, 8, 64)
    entry = features.checkpoint_entry(mel)
    assert isinstance(mel, features.MelSpec)
    assert entry == dict(kind='mel', **mel.settings())
    assert features.stored_channels(entry) == 8
    again = features.spec_from_cli(p.parse_args([]), 16000, None, None, entry)
    assert isinstance(again, features.MelSpec)
    assert again.settings() == mel.settings()
    # mel+f0: --lc_channels is the model's, the front end has two fewer mels
    a = p.parse_args(['--lc_features', 'mel+f0', '--lc_n_fft', '256',
                      '--lc_f0_fmin', '70', '--lc_f0_path', 'true',
                      '--lc_f0_interpolate', 'true', '--lc_normalize', 'range',
                      '--lc_range', '-23,7'])
    spec = features.spec_from_cli(a, 16000, 10, 64)
    assert isinstance(spec, frontend.MelPitchSpec)
    assert (spec.n_mels, spec.channels, spec.hop) == (8, 10, 64)
    assert spec.tracker.fmin == 70.0 and spec.tracker.fmax == 500.0
    assert spec.path is not None and spec.interpolate
    assert spec.normalizer.n_channels == 8
    entry = features.checkpoint_entry(spec)
    assert entry['kind'] == 'mel+f0' and entry['n_mels'] == 8
    assert entry == dict(kind='mel+f0', **spec.settings())
    assert entry['pitch']['interpolate'] is True
    assert entry['pitch']['path']['jump'] == 0.3
    assert features.stored_channels(entry) == 10
    # without flags the entry decides, flag by flag
    for channels, hop in ((None, None), (10, 64)):
        again = features.spec_from_cli(p.parse_args([]), 16000, channels, hop,
                                       entry)
        assert isinstance(again, frontend.MelPitchSpec)
        assert again.settings() == spec.settings()
    over = features.spec_from_cli(
        p.parse_args(['--lc_f0_path', 'false', '--lc_f0_fmax', '400']), 16000,
        None, None, entry)
    assert over.path is None and over.interpolate
    assert (over.tracker.fmin, over.tracker.fmax) == (70.0, 400.0)
    # a plain spec without the flags: the tracker's defaults
    plain = features.spec_from_cli(p.parse_args(['--lc_features', 'mel+f0']),
                                   16000, 10, 64)
    assert (plain.tracker.fmin, plain.tracker.fmax, plain.path,
            plain.interpolate) == (60.0, 500.0, None, False)
    # contradictions name both values
    for argv, channels, hop, both in (
            ([], 12, 64, ('10 channels', '--lc_channels 12')), ([], 10, 32, ('64', '32')),
            (['--lc_features', 'mel'], 10, 64, ('mel+f0', 'mel'))):
        with pytest.raises(ValueError) as e:
            features.spec_from_cli(p.parse_args(argv), 16000, channels, hop,
                                   entry)
        assert all(v in str(e.value) for v in both), str(e.value)
    with pytest.raises(ValueError) as e:
        features.spec_from_cli(p.parse_args(['--lc_features', 'mel+f0']),
                               16000, 8, 64, features.checkpoint_entry(mel))
    assert "'mel'" in str(e.value) and 'mel+f0' in str(e.value)
    # the flags alone are refused
    for argv, stored in ((['--lc_f0_fmin', '70'], None),
                         (['--lc_features', 'mel', '--lc_f0_path', 'true'],
                          None),
                         (['--lc_f0_interpolate', 'true'],
                          features.checkpoint_entry(mel))):
        with pytest.raises(ValueError) as e:
            features.spec_from_cli(p.parse_args(argv), 16000, 8, 64, stored)
        assert '%s needs --lc_features mel+f0' % argv[-2] in str(e.value)
    with pytest.raises(ValueError) as e:
        features.spec_from_cli(p.parse_args(['--lc_features', 'mel+f0']),
                               16000, 2, 64)
    assert '--lc_channels >= 3' in str(e.value)


# ------------------------------------------------------ H5: argparse errors
def _exits(get_arguments, argv, capsys):
    with pytest.raises(SystemExit) as e:
        get_arguments(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_argparse_errors(capsys):
    import evaluate
    import generate
    import train
    sys_path = os.path.join(ROOT, 'tools')
    import sys
    if sys_path not in sys.path:
        sys.path.insert(0, sys_path)
    import make_lc_features
    import make_lc_stats
    base = ['--data_dir', 'in', '--lc_hop', '64']
    f0 = [('--lc_f0_fmin', '70'), ('--lc_f0_fmax', '400'),
          ('--lc_f0_path', 'true'), ('--lc_f0_interpolate', 'true')]
    for flag, value in f0:
        for front in ([], ['--lc_features', 'mel'], ['--lc_features', 'none']):
            err = _exits(train.get_arguments, base + [
                '--lc_channels', '8', flag, value] + front, capsys)
            assert '%s needs --lc_features mel+f0' % flag in err
        # evaluate.py and generate.py: a checkpoint may name the front end,
        # an explicit other choice may not go with the flag
        err = _exits(evaluate.get_arguments, [
            'ckpt', '--data_dir', 'in', '--lc_features', 'mel', flag, value],
            capsys)
        assert '%s needs --lc_features mel+f0' % flag in err
        evaluate.get_arguments(['ckpt', '--data_dir', 'in', flag, value])
        err = _exits(generate.get_arguments, [
            'ckpt', '--lc_wav', 'a.wav', '--lc_features', 'mel', flag, value],
            capsys)
        assert '%s needs --lc_features mel+f0' % flag in err
        err = _exits(generate.get_arguments, ['ckpt', flag, value], capsys)
        assert '%s needs --lc_wav' % flag in err
        for tool in (make_lc_features, make_lc_stats):
            argv = ['DIR', '--sample_rate', '16000', '--lc_channels', '8',
                    '--lc_hop', '64', flag, value]
            if tool is make_lc_stats:
                argv += ['--out', 'x.npz']
            err = _exits(tool.get_arguments, argv, capsys)
            assert '%s needs --lc_features mel+f0' % flag in err
    for flag in ('--lc_f0_path', '--lc_f0_interpolate'):
        err = _exits(train.get_arguments, base + [
            '--lc_channels', '8', '--lc_features', 'mel+f0', flag, 'maybe'],
            capsys)
        assert 'true or false' in err
    for n in ('2', '1', '0'):
        err = _exits(train.get_arguments, base + [
            '--lc_channels', n, '--lc_features', 'mel+f0'], capsys)
        assert '--lc_channels >= 3' in err and 'voicing flag' in err
    err = _exits(train.get_arguments, ['--data_dir', 'in', '--lc_hop', '64',
                                       '--lc_features', 'mel+f0'], capsys)
    assert '--lc_features mel+f0 needs --lc_channels' in err
    err = _exits(train.get_arguments, ['--data_dir', 'in', '--lc_channels',
                                       '10', '--lc_features', 'mel+f0'],
                 capsys)
    assert '--lc_features mel+f0 needs --lc_hop' in err
    # and what parses
    a = train.get_arguments(base + [
        '--lc_channels', '10', '--lc_features', 'mel+f0', '--lc_f0_fmin',
        '70', '--lc_f0_path', 'true', '--lc_f0_interpolate', 'false',
        '--device_corpus', 'true', '--lc_feature_context', 'utterance'])
    assert (a.lc_features, a.lc_f0_fmin, a.lc_f0_path, a.lc_f0_interpolate) \
        == ('mel+f0', 70.0, True, False)
    a = make_lc_features.get_arguments([
        'DIR', '--sample_rate', '16000', '--lc_channels', '10', '--lc_hop',
        '64', '--lc_features', 'mel+f0', '--lc_f0_interpolate', 'true'])
    assert a.lc_features == 'mel+f0'
    a = make_lc_features.get_arguments([
        'DIR', '--sample_rate', '16000', '--lc_channels', '10', '--lc_hop',
        '64'])
    assert a.lc_features == 'mel'


# ------------------------------------------------------ H6, H7: the ABI
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(1): [' '.join(p.split()) for p in m.group(2).split(',')]
            for m in re.finditer(
                r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_binding_table_matches_its_header():
    """Every declaration of wavenet_lc_frames.h is bound with the types it
    declares (double among them) and nothing else is; none of them is
    declared in the other three headers or bound in the other three tables."""
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_lc_frames_chunk', 'wn_lc_frames'}
    assert set(_lib.LC_FRAMES_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, params in decl.items():
        want = [] if params == ['void'] else \
            [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        res, args = _lib.LC_FRAMES_SIGNATURES[name]
        assert args == want, name
        assert res is _lib.c_int, name
    assert _lib.LC_FRAMES_SIGNATURES['wn_lc_frames'][1].count(
        _lib.c_double) == 2
    for other in OTHERS:
        src = open(os.path.join(ROOT, 'include', other)).read()
        assert not any(re.search(r'\b%s\b' % k, src) for k in decl), other
    assert not set(decl) & (set(_lib.SIGNATURES) | set(_lib.PITCH_SIGNATURES)
                            | set(_lib.PITCH_PATH_SIGNATURES))


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_lc_frames as tgl
    w = {k: [p for p in v if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_lc_frames': ['float* out']}
    assert set(tgl.ENTRIES) == set(w)


def test_entry_checks_without_a_device(hip_lib):
    """wn_lc_frames refuses every bad argument before any launch (no device
    is needed to be refused); the chunk is a positive multiple of 64."""
    CH = hip_lib.wn_lc_frames_chunk()
    assert CH >= 64 and CH % 64 == 0
    good = dict(mel=4096, ld_mel=12, M=8, shift=8192, scale=12288, lo=-4.0,
                hi=4.0, f0=16384, mode=1, fmin=60.0, span=3.0, nframes=20480,
                B=2, F=5, out=24576, ld_out=12, c0=8, stream=0)
    order = list(good)
    pointers = ('mel', 'shift', 'scale', 'f0', 'nframes', 'out', 'stream')

    def code(**kw):
        a = dict(good, **kw)
        return hip_lib.wn_lc_frames(*[a[k] or None if k in pointers else a[k]
                                      for k in order])
    for kw in (dict(out=0), dict(mel=0, f0=0), dict(shift=0), dict(scale=0)):
        assert code(**kw) == -5, kw
    for kw in (dict(B=0), dict(B=65536), dict(F=0), dict(F=(1 << 30) + 1),
               dict(M=0), dict(M=-1), dict(M=513), dict(ld_mel=7),
               dict(ld_out=7), dict(ld_out=0), dict(c0=7), dict(c0=11),
               dict(c0=-1), dict(mode=2), dict(mode=-1), dict(fmin=0.0),
               dict(fmin=-60.0), dict(fmin=float('nan')),
               dict(fmin=float('inf')), dict(span=0.0),
               dict(span=float('nan')), dict(span=float('inf')),
               dict(lo=1.0, hi=-1.0), dict(lo=float('nan')),
               dict(ld_out=(1 << 20) + 1), dict(ld_mel=(1 << 20) + 1)):
        assert code(**kw) == -1, kw
    for name in pointers[:-1]:
        assert code(**{name: 4098}) == -3, name
