"""The log-mel front end without a GPU: argument checks before any library
or device is touched, the C entry's validation, the host tables against
formulas written out here, the numpy reference against the independent
float64 oracle tests/mel_ref.py, and the float32 yardstick of the GPU test's
tolerance."""
import ctypes
import math

import numpy as np
import pytest

import mel_ref


def _no_library(monkeypatch):
    from wavenet import _lib

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)


BAD = [
    dict(n_fft=1000), dict(n_fft=32), dict(n_fft=4096), dict(n_fft=1024.0),
    dict(hop=0), dict(hop=300, win_length=256), dict(win_length=2048),
    dict(hop=2048), dict(n_mels=0), dict(n_mels=129), dict(n_mels=True),
    dict(fmax=8000.5), dict(fmin=-1.0), dict(fmin=4000.0, fmax=4000.0),
    dict(floor=0.0), dict(floor=-1e-3), dict(floor=float('nan')),
]


@pytest.mark.parametrize('kw', BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_bad_arguments_raise_before_the_library(monkeypatch, kw):
    _no_library(monkeypatch)
    from wavenet import features
    with pytest.raises(ValueError):
        features.MelSpec(16000, **kw)


def test_good_arguments_and_bad_lengths(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import features
    spec = features.MelSpec(16000)
    assert (spec.n_fft, spec.hop, spec.n_mels, spec.win_length) == \
        (1024, 256, 80, 1024)
    assert spec.fmax == 8000.0 and spec.floor == 1e-10
    audio = np.zeros((2, 100), np.float32)
    for lengths in ([0, 100], [100, 101], [100], [1.0, 2.0], [True, True]):
        with pytest.raises(ValueError):
            spec(audio, lengths)
    with pytest.raises(ValueError):
        spec(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        spec(np.zeros((2, 100), np.int32))
    # good arguments reach the library (which the patch refuses)
    with pytest.raises(AssertionError):
        spec(audio, [5, 100])


def test_entry_validates_without_gpu(hip_lib):
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def call(audio=a, ld=100, B=1, T=100, lengths=None, window=a, basis=a,
             melw=a, n_fft=64, hop=16, n_bins=33, n_mels=10, floor=1e-10,
             out=a):
        return hip_lib.wn_melspec(audio, ld, B, T, lengths, window, basis,
                                  melw, n_fft, hop, n_bins, n_mels, floor,
                                  out, None)
    for name in ('audio', 'window', 'basis', 'melw', 'out'):
        assert call(**{name: None}) == -5, name
    for kw in (dict(n_fft=96, n_bins=49), dict(n_fft=32, n_bins=17),
               dict(n_fft=4096, n_bins=2049), dict(n_bins=32), dict(hop=0),
               dict(hop=65), dict(n_mels=0), dict(n_mels=129),
               dict(floor=0.0), dict(floor=-1.0), dict(B=0), dict(B=65536),
               dict(T=0), dict(ld=99)):
        assert call(**kw) == -1, kw
    for name in ('basis', 'melw', 'out'):
        assert call(**{name: a + 4}) == -3, name
    for name in ('audio', 'window', 'lengths'):
        assert call(**{name: a + 2}) == -3, name


@pytest.mark.parametrize('name', ['a', 'b', 'c'])
def test_tables_follow_the_formulas(name):
    from wavenet import features
    kw = dict(mel_ref.SHAPES[name])
    sr = kw.pop('sample_rate')
    spec = features.MelSpec(sr, fmin=100.0, fmax=0.45 * sr, **kw)
    N, W, nb = spec.n_fft, spec.win_length, spec.n_fft // 2 + 1
    # periodic Hann of win_length, centred
    lo = (N - W) // 2
    for j in range(N):
        want = 0.5 - 0.5 * math.cos(2 * math.pi * (j - lo) / W) \
            if lo <= j < lo + W else 0.0
        assert abs(float(spec.window[j]) - want) <= 1e-7
    assert spec.window.dtype == np.float32 and spec.window[lo] == 0.0
    # the filterbank
    w = spec.melw
    assert w.shape == (spec.n_mels, nb) and w.dtype == np.float32
    assert (w >= 0).all() and w.max() <= 1.0
    fk = np.arange(nb) * sr / N
    assert not w[:, (fk <= 100.0) | (fk >= 0.45 * sr)].any()
    assert (w.sum(axis=1) > 0).all()
    edges = [700.0 * (10 ** (m / 2595.0) - 1) for m in np.linspace(
        2595.0 * math.log10(1 + 100.0 / 700.0),
        2595.0 * math.log10(1 + 0.45 * sr / 700.0), spec.n_mels + 2)]
    for m in range(spec.n_mels):
        for k in range(nb):
            up = (fk[k] - edges[m]) / (edges[m + 1] - edges[m])
            down = (edges[m + 2] - fk[k]) / (edges[m + 2] - edges[m + 1])
            assert abs(float(w[m, k]) - max(0.0, min(up, down))) <= 1e-6
    assert np.abs(w - mel_ref.filterbank(sr, N, spec.n_mels, 100.0,
                                         0.45 * sr)).max() <= 1e-6
    # the basis
    cos, sin = spec.basis64()
    for j, k in ((0, 0), (1, 1), (N - 1, nb - 1), (N // 3, nb // 2)):
        assert abs(cos[j, k] - math.cos(2 * math.pi * j * k / N)) <= 1e-12
        assert abs(sin[j, k] - math.sin(2 * math.pi * j * k / N)) <= 1e-12


@pytest.mark.parametrize('n,hop,want', [(1, 16, 1), (16, 16, 1), (17, 16, 2),
                                        (100, 16, 7), (799, 24, 34),
                                        (16000, 256, 63)])
def test_frame_count(n, hop, want):
    from wavenet import features
    spec = features.MelSpec(8000, n_fft=256, hop=hop, n_mels=8)
    assert spec.num_frames(n) == want == -(-n // hop)
    x = np.random.default_rng(0).uniform(-1, 1, n)
    assert features.logmel_reference(x, spec).shape == (want, 8)
    assert mel_ref.logmel(x, 8000, 256, hop, 256, 8).shape == (want, 8)


def _clips(name):
    x, lengths = mel_ref.make_audio(name)
    for b in range(x.shape[0]):
        yield x[b, :x.shape[1] if lengths is None else lengths[b]]


@pytest.mark.parametrize('name', sorted(mel_ref.SHAPES))
def test_reference_agrees_with_the_oracle(name):
    from wavenet import features
    kw = dict(mel_ref.SHAPES[name])
    spec = features.MelSpec(kw.pop('sample_rate'), **kw)
    for x in _clips(name):
        ref = mel_ref.logmel(x, **mel_ref.SHAPES[name])
        assert mel_ref.mel_energy(x, **mel_ref.SHAPES[name]).min() > 1e-6
        got = features.logmel_reference(x, spec)
        assert got.dtype == np.float64
        assert np.abs(got - ref).max() <= 1e-9


def test_float32_restatement_is_within_the_gpu_tolerance():
    """The kernel is held to 4 x the largest error of the float32 numpy
    restatement over the shapes (a) - (c) (mel_ref.MEL_F32_ERR, measured once
    and written down; BLAS summation orders differ between hosts): whatever
    this host's order, the restatement itself stays within that bound."""
    worst = 0.0
    for name in 'abc':
        for x in _clips(name):
            err = np.abs(mel_ref.logmel_f32_matmul(x, **mel_ref.SHAPES[name]) -
                         mel_ref.logmel(x, **mel_ref.SHAPES[name])).max()
            worst = max(worst, float(err))
    print('float32 restatement: max abs error %.3g' % worst)
    assert mel_ref.MEL_TOL == 4.0 * mel_ref.MEL_F32_ERR
    assert worst <= mel_ref.MEL_TOL


@pytest.mark.parametrize('name', sorted(mel_ref.MEL_YARDSTICK_BY_SHAPE))
def test_both_float32_restatements_are_within_the_shape_bound(name):
    """The sibling for the shapes (d) - (i) and the pairs at the staging
    limit: each is held to 4 x its OWN yardstick (mel_ref.MEL_F32_MEASURED:
    the matmul order, the sequential order and one float32 ulp of the largest
    output, measured once and written down), and on any host both summation
    orders stay within that bound themselves."""
    matmul, seq, ulp = mel_ref.yardstick_terms(name)
    tol = mel_ref.shape_tol(name)
    print('shape (%s): matmul order %.3g, sequential order %.3g, ulp %.3g '
          '(recorded %s; bound %.3g)'
          % (name, matmul, seq, ulp, mel_ref.MEL_F32_MEASURED[name], tol))
    assert tol == 4.0 * max(mel_ref.MEL_F32_MEASURED[name])
    assert ulp <= max(mel_ref.MEL_F32_MEASURED[name]) * 1.05  # (the record's digits)
    assert matmul <= tol and seq <= tol


def test_the_new_shapes_leave_the_old_tolerance_alone():
    assert mel_ref.MEL_F32_ERR == 9.2e-6 and mel_ref.MEL_TOL == 4.0 * 9.2e-6
    assert sorted(mel_ref.MEL_F32_ERR_BY_SHAPE) == ['a', 'b', 'c']
    assert set(mel_ref.NEW_SHAPES) <= set(mel_ref.MEL_YARDSTICK_BY_SHAPE)
    # (a) - (c) keep their signal: the first samples, as they always were
    x, lengths = mel_ref.make_audio('a')
    assert x.shape == (3, 100) and lengths == (5, 100, 33)
    rng = np.random.default_rng(11)
    want = rng.uniform(-0.1, 0.1, (3, 100))
    t = np.arange(100) / 8000
    want += 0.3 * np.sin(2 * np.pi * 0.055 * 8000 * t)[None, :]
    want += 0.2 * np.sin(2 * np.pi * 0.21 * 8000 * t + 1.0)[None, :]
    assert np.array_equal(x, want.astype(np.float32))


# ------------------------------------------------------------ command line
def _argparse_error(capsys, fn, argv):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_train_lc_features_names_what_is_missing(capsys):
    import train
    err = _argparse_error(capsys, train.get_arguments,
                          ['--lc_features', 'mel', '--lc_hop', '16'])
    assert '--lc_channels' in err
    for extra in ([], ['--lc_context', '1']):
        err = _argparse_error(capsys, train.get_arguments,
                              ['--lc_features', 'mel', '--lc_channels', '8']
                              + extra)
        assert '--lc_hop' in err and '--lc_upsample_scales' in err
    err = _argparse_error(capsys, train.get_arguments,
                          ['--lc_channels', '8', '--lc_hop', '16',
                           '--lc_n_fft', '64'])
    assert '--lc_features' in err
    err = _argparse_error(capsys, train.get_arguments,
                          ['--lc_features', 'stft', '--lc_channels', '8',
                           '--lc_hop', '16'])
    assert 'lc_features' in err
    for hop in (['--lc_hop', '16'], ['--lc_upsample_scales', '4,4']):
        a = train.get_arguments(['--lc_features', 'mel', '--lc_channels',
                                 '8', '--lc_n_fft', '64'] + hop)
        assert a.lc_features == 'mel' and a.lc_n_fft == 64
    # without the flags nothing changes
    a = train.get_arguments([])
    assert a.lc_features is None and a.lc_n_fft is None


def test_generate_lc_wav_and_lc_path_exclude_each_other(capsys):
    import generate
    err = _argparse_error(capsys, generate.get_arguments,
                          ['ckpt', '--lc_wav', 'a.wav', '--lc_path', 'a.npy'])
    assert '--lc_wav' in err and '--lc_path' in err
    err = _argparse_error(capsys, generate.get_arguments,
                          ['ckpt', '--lc_features', 'mel'])
    assert '--lc_wav' in err
    a = generate.get_arguments(['ckpt', '--lc_wav', 'a.wav'])
    assert a.lc_wav == 'a.wav' and a.samples == generate.SAMPLES and \
        not a.samples_given
    assert generate.get_arguments(['ckpt']).samples == generate.SAMPLES


def test_spec_from_cli_and_the_checkpoint_entry(monkeypatch):
    _no_library(monkeypatch)
    import train
    from wavenet import features
    a = train.get_arguments(['--lc_features', 'mel', '--lc_channels', '8',
                             '--lc_hop', '16', '--lc_n_fft', '64',
                             '--lc_fmax', '7000'])
    spec = features.spec_from_cli(a, 16000, 8, 16)
    assert (spec.n_fft, spec.hop, spec.n_mels, spec.win_length, spec.fmax) \
        == (64, 16, 8, 64, 7000.0)
    entry = features.checkpoint_entry(spec)
    assert entry['kind'] == 'mel' and entry['n_fft'] == 64
    # the entry alone rebuilds the front end; flags override single settings
    none = train.get_arguments([])
    again = features.spec_from_cli(none, 16000, None, None, entry)
    assert again.settings() == spec.settings()
    assert features.spec_from_cli(none, 16000, 8, 16) is None
    none.lc_features = 'none'
    assert features.spec_from_cli(none, 16000, 8, 16, entry) is None
    none.lc_features, none.lc_fmax = None, 6000.0
    assert features.spec_from_cli(none, 16000, 8, 16, entry).fmax == 6000.0
    with pytest.raises(ValueError, match='hop'):
        features.spec_from_cli(none, 16000, 8, 32, entry)
    with pytest.raises(ValueError, match='n_mels'):
        features.spec_from_cli(none, 16000, 10, 16, entry)
    with pytest.raises(ValueError):          # MelSpec's own limits
        a.lc_n_fft = 100
        features.spec_from_cli(a, 16000, 8, 16)
