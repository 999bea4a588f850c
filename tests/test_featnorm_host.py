"""Feature normalisation without a device: the argument checks (before the
library or a GPU is touched), the dict / checkpoint-entry round trips, the
command-line errors, FeatureStats' arithmetic against tests/featnorm_ref.py,
the statistics' sum over two gloo ranks, and the numbers that motivate it."""
import argparse
import os
import socket

import numpy as np
import pytest

import featnorm_ref as R


def _no_library(monkeypatch):
    from wavenet import _lib

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)


def _argparse_error(capsys, fn, argv):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def _stats(frames):
    from wavenet import features
    n, s1, s2 = R.sums(np.asarray(frames, np.float32)[None])[:3]
    return features.FeatureStats.from_sums(n, s1, s2)


def _frames(F=50, C=8, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((F, C)) * 11 - 10).astype(np.float32)


# ------------------------------------------------------------ argument checks
def test_normalizer_argument_checks(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    N = features.Normalizer
    one = np.ones(4, np.float32)
    for shift, scale in ((np.ones((2, 2)), np.ones((2, 2))),     # not [C]
                         (np.ones(4), np.ones(3)),               # C differs
                         (np.zeros(0), np.zeros(0)),             # no channel
                         (np.ones(513), np.ones(513)),           # C > 512
                         (np.array([0, np.nan, 0, 0]), one),     # non-finite
                         (np.array([0, np.inf, 0, 0]), one),
                         (one, np.array([1, 0, 1, 1])),          # zero scale
                         (one, np.array([1, np.inf, 1, 1])),
                         (one, np.array([1e300, 1, 1, 1]))):     # inf as f32
        with pytest.raises(ValueError):
            N(shift, scale)
    with pytest.raises(ValueError, match='lo'):
        N(one, one, lo=2.0, hi=1.0)
    with pytest.raises(ValueError):
        N(one, one, lo=float('nan'))
    norm = N(one, one, -1.0, 1.0)
    for bad in (np.ones((3, 5), np.float32),            # channels
                np.ones((3, 4), np.float64),            # dtype
                np.ones((2, 3, 4, 4), np.float32),      # rank
                np.ones(4, np.float32)):
        with pytest.raises(ValueError):
            norm(bad)
        with pytest.raises(ValueError):
            norm.reference(bad)
    ok = np.ones((2, 3, 4), np.float32)
    for bad_n in ([1], [1, 4], [-1, 0], [1.0, 2.0], [[1, 2]]):
        with pytest.raises(ValueError, match='nframes'):
            norm(ok, nframes=bad_n)
    with pytest.raises(ValueError, match='out'):
        norm(ok, out=np.empty_like(ok))


def test_from_stats_and_from_range_checks(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    st = _stats(_frames())
    for clip in (0, -1.0, float('nan'), float('inf'), True):
        with pytest.raises(ValueError, match='clip'):
            features.Normalizer.from_stats(st, clip=clip)
    with pytest.raises(ValueError, match='min_std'):
        features.Normalizer.from_stats(st, min_std=0.0)
    with pytest.raises(ValueError):
        features.Normalizer.from_stats('stats')
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0)):
        with pytest.raises(ValueError):
            features.Normalizer.from_range(lo, hi, 8)
    with pytest.raises(ValueError):
        features.Normalizer.from_range(-23.0, 7.0, 0)
    empty = features.FeatureStats(8)
    for fn in (empty.mean, empty.std,
               lambda: features.Normalizer.from_stats(empty)):
        with pytest.raises(ValueError, match='no frames'):
            fn()
    for bad in (0, 513, 8.0, True):
        with pytest.raises(ValueError):
            features.FeatureStats(bad)
    for bad in (np.ones((3, 7), np.float32), np.ones((3, 8), np.float64),
                np.ones(8, np.float32)):
        with pytest.raises(ValueError):
            empty.update(bad)
    with pytest.raises(ValueError, match='nframes'):
        empty.update(np.ones((2, 3, 8), np.float32), nframes=[4, 0])
    with pytest.raises(ValueError):
        features.FeatureStats.from_sums(-1, np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        features.FeatureStats.from_sums(1, np.zeros(3), np.zeros(4))
    with pytest.raises(ValueError):
        empty.merge(features.FeatureStats(9))


def test_melspec_and_corpus_checks(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    from wavenet.corpus import DeviceCorpus
    norm8 = features.Normalizer(np.zeros(8), np.ones(8))
    norm9 = features.Normalizer(np.zeros(9), np.ones(9))
    with pytest.raises(ValueError, match='channels'):
        features.MelSpec(16000, n_fft=64, hop=16, n_mels=8, normalizer=norm9)
    with pytest.raises(ValueError):
        features.MelSpec(16000, n_fft=64, hop=16, n_mels=8, normalizer='yes')
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    with pytest.raises(ValueError, match='channels'):
        spec.with_normalizer(norm9)
    with pytest.raises(TypeError):           # keyword-only
        features.MelSpec(16000, 64, 16, 8, None, 0.0, None, 1e-10, norm8)
    clips = [np.zeros(100, np.float32), np.zeros(60, np.float32)]
    # normalize without frames to normalise
    with pytest.raises(ValueError, match='spec'):
        DeviceCorpus.from_arrays(clips, normalize='corpus')
    with pytest.raises(ValueError, match='spec'):
        DeviceCorpus('/nowhere', 16000, False, normalize='corpus')
    # per-shard statistics would differ between ranks
    with pytest.raises(ValueError, match='stats_allreduce'):
        DeviceCorpus('/nowhere', 16000, False, rank=0, world=2, spec=spec,
                     normalize='corpus')
    with pytest.raises(ValueError, match='stats_allreduce'):
        DeviceCorpus.from_arrays(clips, spec=spec, normalize='corpus',
                                 world=2)
    for kw in (dict(normalize='utterance'), dict(normalize=norm9),
               dict(normalize=norm8, normalize_clip=3.0),
               dict(normalize='corpus', normalize_clip=0.0),
               dict(normalize='corpus', stats_allreduce=3)):
        with pytest.raises(ValueError):
            DeviceCorpus.from_arrays(clips, spec=spec, **kw)
    with pytest.raises(TypeError):           # keyword-only
        DeviceCorpus('/nowhere', 16000, False, None, None, 'pieces', 0, 0, 1,
                     spec, None, 1 << 30, 'corpus')


# ------------------------------------------------------- dicts and round trips
def test_settings_without_a_normalizer_are_unchanged(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8, fmax=7000.0)
    today = dict(sample_rate=16000, n_fft=64, hop=16, n_mels=8,
                 win_length=64, fmin=0.0, fmax=7000.0, floor=1e-10)
    assert spec.settings() == today
    assert list(spec.settings()) == list(today)
    assert features.checkpoint_entry(spec) == dict(kind='mel', **today)
    norm = features.Normalizer.from_stats(_stats(_frames()), clip=4.0)
    with_n = spec.with_normalizer(norm)
    assert spec.normalizer is None and with_n.normalizer is norm
    assert with_n.melw is spec.melw and with_n._dev is spec._dev
    assert with_n.settings() == dict(today, normalizer=norm.entry())
    assert features.checkpoint_entry(with_n) == \
        dict(kind='mel', normalizer=norm.entry(), **today)
    assert with_n.with_normalizer(None).settings() == today


def test_entry_round_trip_is_bit_exact(monkeypatch, tmp_path):
    _no_library(monkeypatch)
    import torch
    from wavenet import features
    st = _stats(_frames(seed=3))
    for norm in (features.Normalizer.from_stats(st),
                 features.Normalizer.from_stats(st, clip=4.0),
                 features.Normalizer.from_range(-23.0, 7.0, 8)):
        e = norm.entry()
        assert all(type(v) is float for v in e['shift'] + e['scale'])
        assert e['lo'] is None or type(e['lo']) is float
        # through a checkpoint file, as train.py writes it
        path = str(tmp_path / 'ck')
        torch.save({'lc_features': {'normalizer': e}}, path)
        e2 = torch.load(path, map_location='cpu')['lc_features']['normalizer']
        back = features.Normalizer.from_entry(e2)
        assert back.shift.dtype == np.float32
        assert back.shift.tobytes() == norm.shift.tobytes()
        assert back.scale.tobytes() == norm.scale.tobytes()
        assert (back.lo, back.hi, back.count) == (norm.lo, norm.hi,
                                                  norm.count)
        assert back.entry() == e
    assert features.Normalizer.from_stats(st).count == st.count
    r = features.Normalizer.from_range(-23.0, 7.0, 8)
    assert (r.lo, r.hi) == (0.0, 1.0) and (r.shift == -23.0).all() and \
        (r.scale == np.float32(1.0 / 30.0)).all()
    with pytest.raises(ValueError):
        features.Normalizer.from_entry({'shift': [0.0]})


def _cli(argv):
    from wavenet import features
    p = argparse.ArgumentParser()
    features.add_cli_flags(p)
    return p.parse_args(argv)


def test_spec_from_cli_rebuilds_the_normalizer(monkeypatch, tmp_path):
    _no_library(monkeypatch)
    from wavenet import features
    st = _stats(_frames(seed=4))
    norm = features.Normalizer.from_stats(st, clip=4.0)
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8,
                            normalizer=norm)
    entry = features.checkpoint_entry(spec)
    again = features.spec_from_cli(_cli([]), 16000, None, None, entry)
    assert again.settings() == spec.settings()
    assert again.normalizer.shift.tobytes() == norm.shift.tobytes()
    assert again.normalizer.scale.tobytes() == norm.scale.tobytes()
    # --lc_normalize none drops it, the other settings stay
    off = features.spec_from_cli(_cli(['--lc_normalize', 'none']), 16000, 8,
                                 16, entry)
    assert off.normalizer is None and off.n_fft == 64
    assert 'normalizer' not in off.settings()
    # flag by flag: a clip alone replaces the stored clamp
    c = features.spec_from_cli(_cli(['--lc_norm_clip', '2']), 16000, 8, 16,
                               entry).normalizer
    assert (c.lo, c.hi) == (-2.0, 2.0) and \
        c.scale.tobytes() == norm.scale.tobytes()
    # range and a statistics file need no checkpoint
    r = features.spec_from_cli(
        _cli(['--lc_features', 'mel', '--lc_normalize', 'range',
              '--lc_range', '-23,7']), 16000, 8, 16).normalizer
    assert r.entry() == features.Normalizer.from_range(-23, 7, 8).entry()
    path = str(tmp_path / 'stats.npz')
    st.save(path)
    assert os.path.exists(path)
    got = features.FeatureStats.load(path).sums()
    assert got[0] == st.count and all(
        a.tobytes() == b.tobytes() for a, b in zip(got[1:], st.sums()[1:]))
    f = features.spec_from_cli(
        _cli(['--lc_features', 'mel', '--lc_normalize', 'corpus',
              '--lc_stats', path, '--lc_norm_clip', '4']), 16000, 8,
        16).normalizer
    assert f.entry() == norm.entry()
    # a device corpus supplies the statistics later
    assert features.spec_from_cli(
        _cli(['--lc_features', 'mel', '--lc_normalize', 'corpus']), 16000, 8,
        16, corpus=True).normalizer is None
    # a file of another width
    with pytest.raises(ValueError, match='--lc_stats'):
        features.spec_from_cli(
            _cli(['--lc_features', 'mel', '--lc_normalize', 'corpus',
                  '--lc_stats', path]), 16000, 10, 16)
    with pytest.raises(ValueError, match='--lc_stats'):
        features.spec_from_cli(
            _cli(['--lc_features', 'mel', '--lc_normalize', 'corpus',
                  '--lc_stats', str(tmp_path / 'missing.npz')]), 16000, 8, 16)


# ------------------------------------------------------------ argparse errors
MEL = ['--lc_features', 'mel', '--lc_channels', '8', '--lc_hop', '16']


def test_train_flags_name_what_is_missing(capsys):
    import train
    a = train.get_arguments([])
    assert a.lc_normalize is None and a.lc_norm_clip is None and \
        a.lc_range is None and a.lc_stats is None
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_normalize', 'corpus'])
    assert '--device_corpus' in err and '--lc_stats' in err
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_normalize', 'range'])
    assert '--lc_range' in err
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_normalize', 'range', '--lc_range',
                                 '7,-23'])
    assert '--lc_range' in err
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_range', '-23,7'])
    assert '--lc_range' in err and '--lc_normalize' in err
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_stats', 's.npz'])
    assert '--lc_stats' in err and '--lc_normalize' in err
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_normalize', 'corpus', '--lc_stats',
                                 's.npz', '--lc_norm_clip', '-1'])
    assert '--lc_norm_clip' in err
    err = _argparse_error(capsys, train.get_arguments,
                          MEL + ['--lc_normalize', 'whiten'])
    assert 'lc_normalize' in err
    # each needs the front end
    for flag, v in (('--lc_normalize', 'range'), ('--lc_norm_clip', '4'),
                    ('--lc_range', '-23,7'), ('--lc_stats', 's.npz')):
        err = _argparse_error(capsys, train.get_arguments,
                              ['--lc_channels', '8', '--lc_hop', '16', flag,
                               v])
        assert flag in err and '--lc_features mel' in err
    a = train.get_arguments(MEL + ['--lc_normalize', 'corpus', '--lc_stats',
                                   's.npz', '--lc_norm_clip', '4'])
    assert (a.lc_normalize, a.lc_stats, a.lc_norm_clip) == \
        ('corpus', 's.npz', 4.0)
    a = train.get_arguments(MEL + ['--lc_normalize', 'corpus', '--data_dir',
                                   'd', '--device_corpus', 'true'])
    assert a.lc_normalize == 'corpus' and a.device_corpus


def test_generate_flags_need_lc_wav(capsys):
    import generate
    err = _argparse_error(capsys, generate.get_arguments,
                          ['ckpt', '--lc_normalize', 'none'])
    assert '--lc_normalize' in err and '--lc_wav' in err


# ------------------------------------------------------ FeatureStats arithmetic
def test_feature_stats_arithmetic(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    fr = _frames(F=301, C=6, seed=7)
    n, s1, s2, a1, a2 = R.sums(fr[None])
    st = features.FeatureStats.from_sums(n, s1, s2)
    mean, std = R.mean_std(n, s1, s2)
    assert st.count == 301 and st.n_channels == 6
    assert np.array_equal(st.mean(), mean) and np.array_equal(st.std(), std)
    # against the textbook values, loosely (the formula cancels)
    assert np.allclose(mean, fr.astype(np.float64).mean(0), rtol=1e-12)
    assert np.allclose(std, fr.astype(np.float64).std(0), rtol=1e-9)
    shift, scale = R.shift_scale(n, s1, s2)
    norm = features.Normalizer.from_stats(st)
    assert norm.shift.tobytes() == shift.tobytes() and \
        norm.scale.tobytes() == scale.tobytes()
    assert norm.lo is None and norm.hi is None
    # two shards merged: the whole, within the bound of two summation orders
    a, b = _stats(fr[:120]), _stats(fr[120:])
    m = features.FeatureStats(6).merge(a).merge(b)
    cnt, m1, m2 = m.sums()
    assert cnt == n
    assert (np.abs(m1 - s1) <= R.sum_bound(n, a1)).all()
    assert (np.abs(m2 - s2) <= R.sum_bound(n, a2)).all()
    assert np.array_equal(m1, a.sums()[1] + b.sums()[1])
    v = m.vector()
    assert v.dtype == np.float64 and v.shape == (13,) and v[0] == n
    back = features.FeatureStats.from_vector(v)
    assert back.count == n and np.array_equal(back.sums()[1], m1)


def test_a_constant_channel_never_gives_inf(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    fr = _frames(F=40, C=4, seed=1)
    fr[:, 2] = np.float32(-23.02585)
    st = _stats(fr)
    norm = features.Normalizer.from_stats(st, min_std=1e-3)
    assert np.isfinite(norm.scale).all()
    assert norm.scale[2] == np.float32(1.0 / 1e-3)
    assert features.Normalizer.from_stats(st).scale[2] == np.float32(1e5)
    out = norm.reference(fr)
    assert np.isfinite(out).all() and np.abs(out[:, 2]).max() < 1e-2
    assert np.array_equal(out, R.normalize(fr[None], norm.shift,
                                           norm.scale)[0])


def test_reference_is_the_restated_rule(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    fr = _frames(F=12, C=5, seed=2).reshape(2, 6, 5).copy()
    fr[0, 1, 3] = np.nan
    st = _stats(_frames(F=12, C=5, seed=2))
    for norm in (features.Normalizer.from_stats(st, clip=1.0),
                 features.Normalizer.from_stats(st),
                 features.Normalizer.from_range(-23.0, 7.0, 5)):
        for nf in (None, [6, 0], [2, 5]):
            got = norm.reference(fr, nf)
            want = R.normalize(fr, norm.shift, norm.scale,
                               -np.inf if norm.lo is None else norm.lo,
                               np.inf if norm.hi is None else norm.hi, nf)
            assert got.dtype == np.float32
            assert got.tobytes() == want.tobytes()
    assert np.isnan(got[0, 1, 3]) and not got[1, 5].any()


# ---------------------------------------------------------------- gloo world 2
def test_stats_allreduce_gives_every_rank_the_host_merge(tmp_path):
    import torch.multiprocessing as mp
    import featnorm_gloo_worker as W
    from wavenet import features
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    world = 2
    mp.spawn(W.worker, args=(world, port, str(tmp_path)), nprocs=world,
             join=True)
    host = features.FeatureStats(5)
    for r in range(world):
        host.merge(_stats(W.shard_frames(r, world)))
    want = host.sums()
    for r in range(world):
        got = features.FeatureStats.load(
            str(tmp_path / ('rank%d.npz' % r))).sums()
        assert got[0] == want[0]
        assert got[1].tobytes() == want[1].tobytes()
        assert got[2].tobytes() == want[2].tobytes()


# -------------------------------------------------------- the motivation, pinned
def test_raw_frames_saturate_a_xavier_projection_normalised_ones_do_not():
    """16000 samples at 16 kHz, 80 mels, hop 256: log-mel frames times a
    Xavier [80, 32] matrix (the LC weights' initialisation) have a standard
    deviation far beyond tanh's range raw, and of order one normalised."""
    from wavenet import features
    spec = features.MelSpec(16000)
    x = R.motivation_clip()
    raw = features.logmel_reference(x, spec)
    assert raw.shape == (63, 80)
    assert raw.min() == pytest.approx(np.log(1e-10)) and raw.max() > 5.0
    W = R.xavier(80, 32)
    assert (raw @ W).std() > 10.0
    norm = features.Normalizer.from_stats(_stats(raw.astype(np.float32)))
    normed = features.logmel_reference(x, spec.with_normalizer(norm))
    assert np.array_equal(
        normed.astype(np.float32),
        R.normalize(raw.astype(np.float32)[None], norm.shift, norm.scale)[0])
    assert (normed @ W).std() < 2.0
    print('std of frames @ W: raw %.2f, normalised %.2f'
          % ((raw @ W).std(), (normed @ W).std()))
