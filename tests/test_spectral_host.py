"""The synthesis metrics' host side (wavenet/spectral.py, include/
wavenet_spectral.h) without a device: the float64 restatement of
tests/stft_ref.py against torch.stft on its own padded signal (H1), closed
forms (H2), StftDistance.reference and cepstral_reference against the
restatement within the device's bounds, and the yardstick those bounds come
from (H3), refusals before the library, settings and the summary's arithmetic
(H4), the argparse errors of evaluate.py's new flags (H5), the binding table
against the header and the coverage of its writing entries by
tests/test_gpu_guard_spectral.py (H6), the entries' checks (H7)."""
import math
import os
import re

import numpy as np
import pytest

import stft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'wavenet_spectral.h'
OTHERS = ('wavenet_hip.h', 'wavenet_pitch.h', 'wavenet_pitch_path.h',
          'wavenet_lc_frames.h')
SMALL = ('tiles', 'idle', 'oddhop', 'r512')


def _no_library(monkeypatch):
    from wavenet import _lib

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libwavenet_hip.so')


def _clips(name):
    """(g, o) of each clip of a shape, cut to its length."""
    T, lengths = R.SHAPES[name][3:]
    g, o = R.make_pair(name)
    return [(g[b, :T if lengths is None else lengths[b]],
             o[b, :T if lengths is None else lengths[b]]) for b in range(4)]


# ------------------------------------------------- H1: against torch.stft
@pytest.mark.parametrize('name', ['tiles', 'oddhop', 'r512', 'r2048'])
def test_restatement_against_torch_stft(name):
    import torch
    n_fft, hop, win = R.SHAPES[name][:3]
    for g, o in _clips(name):
        x = o.astype(np.float64)
        p = R.padded(x, n_fft, hop)
        s = torch.stft(torch.from_numpy(p), n_fft, hop_length=hop,
                       window=torch.from_numpy(R.hann(n_fft, win)),
                       center=False, return_complex=True).numpy().T
        want = s.real ** 2 + s.imag ** 2
        got = R.power(x, n_fft, hop, win)
        assert got.shape == want.shape == (-(-x.shape[0] // hop),
                                           n_fft // 2 + 1)
        assert np.abs(got - want).max() <= 1e-10 * want.max()


# ------------------------------------------------------ H2: closed forms
@pytest.mark.parametrize('gain', [0.8, 1.25, 0.1])
def test_a_gain_has_closed_forms(monkeypatch, gain):
    _no_library(monkeypatch)
    from wavenet import spectral
    rng = np.random.default_rng(3)
    o = 1000.0 * R.original(rng, 3000)         # every bin far above the floor
    res = (512, 50, 240)
    assert R.power(gain * o, *res).min() > 100 * R.FLOOR
    sc, lm = R.metrics(gain * o, o, *res)
    assert sc == pytest.approx(abs(1 - gain), rel=1e-9)
    assert lm == pytest.approx(abs(math.log(gain)), rel=1e-9)
    # the package's float32 rule: the same forms within float32
    o32 = o.astype(np.float32)
    g32 = (np.float32(gain) * o32).astype(np.float32)
    num, den, lg = spectral.StftDistance((res,)).reference(g32, o32)[0]
    assert math.sqrt(num / den) == pytest.approx(
        abs(1 - float(np.float32(gain))), rel=1e-4)
    assert lg / (60 * 257) == pytest.approx(
        abs(math.log(float(np.float32(gain)))), rel=1e-4)


def test_a_gain_leaves_the_cepstral_distance_at_zero(monkeypatch):
    """log-mel of gain * x is log-mel of x plus 2 ln gain in every channel,
    and no DCT row but c0's sums to anything: mcd = 0.  With values that
    float32 adds exactly the difference is exactly the constant."""
    _no_library(monkeypatch)
    from wavenet import spectral
    rng = np.random.default_rng(4)
    a = (rng.integers(-23 * 64, 7 * 64, (2, 9, 80)) / 64.0).astype(np.float32)
    b = a + np.float32(0.5)
    assert np.array_equal((b - a).astype(np.float64), np.full(a.shape, 0.5))
    # |sum_m dct[n][m]| <= C 2^-53 sqrt(2 / C) per row, not exactly zero
    assert spectral.cepstral_reference(a, b, None, 13).max() <= 1e-12
    assert R.mcd_sums(a, b, None, 13)[0].max() <= 1e-12
    # ... while a tilt across the channels is seen
    c = a + np.linspace(0, 1, 80, dtype=np.float32)[None, None, :]
    assert spectral.cepstral_reference(a, c, None, 13).min() > 1.0


def test_equal_signals_give_exact_zeros(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import spectral
    _, o = R.make_pair('r512')
    got = spectral.StftDistance().reference(o[0], o[0].copy())
    assert got.shape == (3, 3)
    assert (got[:, 0] == 0).all() and (got[:, 2] == 0).all()
    assert (got[:, 1] > 0).all()
    assert R.stft_sums(o[0], o[0], 512, 50, 240)[0] == 0.0
    a, _ = R.logmel_pair(1, 2, 5, 80)
    assert (spectral.cepstral_reference(a, a.copy()) == 0).all()
    assert (R.mcd_sums(a, a, None, 13)[0] == 0).all()


# ------------------------------- H3: the rule against the restatement
@pytest.mark.parametrize('name', SMALL)
def test_reference_against_the_restatement(monkeypatch, name):
    _no_library(monkeypatch)
    from wavenet import spectral
    res = R.SHAPES[name][:3]
    dist = spectral.StftDistance((res,))
    for g, o in _clips(name):
        got = dist.reference(g, o)[0]
        ref, scale = R.stft_sums(g, o, *res), R.scales(g, o, *res)
        for k, out in enumerate(R.OUTPUTS):
            assert abs(got[k] - ref[k]) <= R.rel_tol(name, out) * scale[k], \
                (name, out)


@pytest.mark.parametrize('name', SMALL)
def test_yardstick_terms_reproduce_what_is_recorded(name):
    got = R.yardstick_terms(name)
    for out in R.OUTPUTS:
        rec = R.STFT_F32_MEASURED[name][out]
        assert rec[2] == pytest.approx(2.0 ** -23, rel=0.05)
        for k in range(2):
            # (two digits are recorded; a BLAS may order a matmul otherwise)
            assert rec[k] / 1.5 <= got[out][k] <= rec[k] * 1.5, (out, k)
        assert R.rel_tol(name, out) == R.TOL_FACTOR * max(rec)
    assert set(R.STFT_F32_MEASURED) == set(R.SHAPES)


@pytest.mark.parametrize('C,K', [(80, 13), (5, 4), (128, 64), (3, 1)])
def test_cepstral_reference_against_the_restatement(monkeypatch, C, K):
    _no_library(monkeypatch)
    from wavenet import spectral
    a, b = R.logmel_pair(C, 3, 20, C)
    nf = np.array([20, 7, 0])
    want, bound = R.mcd_sums(a, b, nf, K)
    got = spectral.cepstral_reference(a, b, nf, K)
    assert got.dtype == np.float64 and got.shape == (3,)
    assert (np.abs(got - want) <= bound).all() and got[2] == 0
    assert (bound[:2] < 1e-9 * want[:2]).all()        # (the bound is tight)
    assert np.abs(spectral.dct_table(C, K) - R.dct_table(C, K)).max() < 1e-15
    assert spectral.mcd_db(got, nf) == pytest.approx(
        R.mcd_db(a, b, nf, K), rel=1e-12)
    # the DCT rows are orthonormal: the full transform keeps the distance
    if K == C - 1:
        t = np.vstack([np.full((1, C), math.sqrt(1.0 / C)),
                       R.dct_table(C, K)])
        assert np.abs(t @ t.T - np.eye(C)).max() < 1e-12


# ------------------------------------- H4: refusals, settings, summary
def test_refusals_arrive_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import spectral
    S = spectral.StftDistance
    for bad in ((), [(1024, 120, 600)] * 9, ((1000, 100, 400),),
                ((32, 8, 32),), ((4096, 100, 400),), ((1024, 0, 600),),
                ((1024, 700, 600),), ((1024, 120, 1025),), ((1024, 120),),
                ((1024.0, 120, 600),), ((True, 1, 1),), 7, ((1024, 120, 600), 5)):
        with pytest.raises(ValueError):
            S(bad)
    for fl in (0.0, -1e-7, float('nan'), float('inf'), 1e-60, 'x', None):
        with pytest.raises(ValueError):
            S(floor=fl)
    d = S(((64, 16, 64),))
    x = np.zeros((2, 100), np.float32)
    for g, o, n in ((x, x[:, :99], None), (x, x[0], None),
                    (x.astype(np.int32), x, None), (x[:, :0], x[:, :0], None),
                    (np.zeros((2, 2, 5), np.float32),) * 2 + (None,),
                    (x, x, [100]), (x, x, [100, 101]), (x, x, [-1, 5]),
                    (x, x, [1.0, 2.0]), (x, x, [[1, 2]])):
        with pytest.raises(ValueError):
            d(g, o, n)
    a = np.zeros((2, 4, 8), np.float32)
    for args in ((a, a[:, :3]), (a, a, None, 0), (a, a, None, 8),
                 (a, a, None, 2.0), (a.astype(np.float64), a), (a, a, [4]),
                 (a, a, [4, 5]), (np.zeros((2, 4, 600), np.float32),) * 2,
                 (np.zeros((2, 4, 1), np.float32),) * 2):
        with pytest.raises(ValueError):
            spectral.cepstral_distance(*args)
        with pytest.raises(ValueError):
            spectral.cepstral_reference(*args)
    # C = 80 allows order 64 and not 65
    b = np.zeros((1, 1, 80), np.float32)
    assert spectral.cepstral_reference(b, b, None, 64)[0] == 0
    with pytest.raises(ValueError):
        spectral.cepstral_reference(b, b, None, 65)
    for s, n in (([1.0], [0]), ([1.0], [-1]), ([1.0, 2.0], [1]),
                 ([1.0], [1.5])):
        with pytest.raises(ValueError):
            spectral.mcd_db(np.array(s), n)
    assert spectral.mcd_db(np.array([1.0, 3.0]), [3, 5]) == pytest.approx(
        10 / math.log(10) * 4.0 / 8)
    assert spectral.mcd_db(np.array([1.0, 3.0]), 4) == pytest.approx(
        10 / math.log(10) * 4.0 / 8)


def test_settings_round_trip(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import spectral
    d = spectral.StftDistance()
    assert d.resolutions == ((1024, 120, 600), (2048, 240, 1200),
                             (512, 50, 240)) and d.floor == 1e-7
    e = spectral.StftDistance(((256, 64, 128),), floor=1e-5)
    s = e.settings()
    assert s == {'resolutions': [[256, 64, 128]], 'floor': 1e-5}
    f = spectral.StftDistance.from_settings(s)
    assert f.resolutions == e.resolutions and f.floor == e.floor
    assert f.settings() == s
    for bad in ({}, {'resolutions': [[256, 64, 128]]}, 3,
                dict(s, more=1)):
        with pytest.raises(ValueError):
            spectral.StftDistance.from_settings(bad)
    # the tables are the log-mel front end's own
    from wavenet import features
    m = features.MelSpec(16000, n_fft=256, hop=64, n_mels=8, win_length=128)
    assert np.array_equal(e._specs[0].window, m.window)
    assert np.array_equal(m.window.astype(np.float64),
                          R.hann(256, 128).astype(np.float32))


def test_summary_arithmetic(monkeypatch):
    _no_library(monkeypatch)
    import torch
    from wavenet import spectral
    res = ((64, 16, 64), (128, 32, 128))
    num = torch.tensor([[4.0, 1.0, 0.0], [9.0, 4.0, 0.0]], dtype=torch.float64)
    den = torch.tensor([[16.0, 4.0, 0.0], [36.0, 64.0, 0.0]],
                       dtype=torch.float64)
    lg = torch.tensor([[66.0, 33.0, 0.0], [130.0, 65.0, 0.0]],
                      dtype=torch.float64)
    sums = spectral.StftSums(num, den, lg, res)
    n = [32, 16, 0]                          # frames: (2, 1) and (1, 1)
    s = sums.summary(n)
    assert set(s) == {'spectral_convergence', 'log_stft_magnitude',
                      'per_resolution'}
    p0, p1 = s['per_resolution']
    assert set(p0) == {'n_fft', 'hop', 'win_length', 'spectral_convergence',
                       'log_stft_magnitude'}
    assert (p0['n_fft'], p0['hop'], p0['win_length']) == (64, 16, 64)
    assert p0['spectral_convergence'] == (0.5 + 0.5) / 2
    assert p0['log_stft_magnitude'] == (66.0 / (2 * 33) + 33.0 / 33) / 2
    assert p1['spectral_convergence'] == (0.5 + 0.25) / 2
    assert p1['log_stft_magnitude'] == (130.0 / 65 + 65.0 / 65) / 2
    assert s['spectral_convergence'] == (0.5 + 0.375) / 2
    assert s['log_stft_magnitude'] == pytest.approx((1.0 + 1.5) / 2)
    for bad in ([0, 0, 0], [32, 16], None, [1.0, 2.0, 3.0], [-1, 2, 3]):
        with pytest.raises(ValueError):
            sums.summary(bad)
    # one int for all clips; cat keeps the clips' order
    two = spectral.StftSums(num[:, :2], den[:, :2], lg[:, :2], res)
    assert two.summary(32)['per_resolution'][0]['log_stft_magnitude'] == \
        (66.0 / 66 + 33.0 / 66) / 2
    both = spectral.StftSums.cat([sums, sums])
    assert both.sc_num.shape == (2, 6)
    assert both.summary(n + n) == s
    with pytest.raises(ValueError):
        spectral.StftSums.cat([])
    with pytest.raises(ValueError):
        spectral.StftSums.cat([sums, spectral.StftSums(num, den, lg,
                                                       res[::-1])])


# ------------------------------------------------- H5: the command line
def _exits(fn, argv, capsys):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_evaluate_flags(capsys):
    import evaluate
    base = ['ckpt', '--data_dir', 'in']
    syn = base + ['--synthesis', 'true']
    for flag in ('--synthesis_stft', '--synthesis_mcd'):
        err = _exits(evaluate.get_arguments, base + [flag, 'true'], capsys)
        assert '%s needs --synthesis true' % flag in err
        err = _exits(evaluate.get_arguments, syn + [flag, 'maybe'], capsys)
        assert flag in err
    err = _exits(evaluate.get_arguments,
                 syn + ['--stft_resolutions', '512:50:240'], capsys)
    assert '--stft_resolutions needs --synthesis_stft true' in err
    err = _exits(evaluate.get_arguments, syn + ['--mcd_order', '5'], capsys)
    assert '--mcd_order needs --synthesis_mcd true' in err
    stft = syn + ['--synthesis_stft', 'true', '--stft_resolutions']
    for bad in ('512:50', '512:50:240:1', 'a:b:c', '512;50;240', '',
                '512:50:240,', '500:50:240', '512:0:240', '512:300:240',
                '512:50:600', ','.join(['512:50:240'] * 9)):
        err = _exits(evaluate.get_arguments, stft + [bad], capsys)
        assert '--stft_resolutions' in err, bad
    mcd = syn + ['--synthesis_mcd', 'true', '--mcd_order']
    for bad in ('0', '-3', '65', '2.5', 'x'):
        err = _exits(evaluate.get_arguments, mcd + [bad], capsys)
        assert '--mcd_order' in err, bad
    # and what parses
    a = evaluate.get_arguments(stft + ['512:50:240,256:64:128'])
    assert a.stft.resolutions == ((512, 50, 240), (256, 64, 128))
    a = evaluate.get_arguments(syn + ['--synthesis_stft', 'true',
                                      '--synthesis_mcd', 'true'])
    assert a.stft.resolutions == ((1024, 120, 600), (2048, 240, 1200),
                                  (512, 50, 240))
    assert a.synthesis_mcd is True and a.mcd_order is None
    a = evaluate.get_arguments(mcd + ['7'])
    assert a.mcd_order == 7 and a.stft is None
    a = evaluate.get_arguments(syn)
    assert a.stft is None and not a.synthesis_mcd
    assert {'synthesis_stft', 'synthesis_mcd'} <= set(evaluate.SYNTHESIS_FLAGS)
    # an order the front end's mels cannot give is named before any work
    import argparse
    from wavenet import features
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    ns = argparse.Namespace(lc_channels=8, synthesis_batch=None,
                            max_clips=None, synthesis_mcd=True, mcd_order=8)
    assert '--mcd_order 8' in evaluate._synthesis_refused(ns, spec)
    ns.mcd_order = 7
    assert evaluate._synthesis_refused(ns, spec) is None
    ns.mcd_order = None                     # (the default 13 > 8 - 1)
    assert '--mcd_order 13' in evaluate._synthesis_refused(ns, spec)


# ------------------------------------------------------ H6: the ABI
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(2): (m.group(1), [' '.join(p.split())
                                      for p in m.group(3).split(',')])
            for m in re.finditer(
                r'\b(int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_binding_table_matches_its_header():
    """Every declaration of wavenet_spectral.h is bound with the types it
    declares and nothing else is; none of them is declared in the other four
    headers or bound in the other four tables; load() binds the table."""
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_stft_distance_partials',
                         'wn_stft_distance_staged', 'wn_stft_distance',
                         'wn_cepstral_distance_partials',
                         'wn_cepstral_distance'}
    assert set(_lib.SPECTRAL_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, (res, params) in decl.items():
        want = [] if params == ['void'] else \
            [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.SPECTRAL_SIGNATURES[name] == (ctype[res], want), name
    for other in OTHERS:
        assert not set(decl) & set(_declarations(other)), other
    assert not set(decl) & (set(_lib.SIGNATURES) | set(_lib.PITCH_SIGNATURES)
                            | set(_lib.PITCH_PATH_SIGNATURES)
                            | set(_lib.LC_FRAMES_SIGNATURES))


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.SPECTRAL_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_spectral as tgs
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_stft_distance': ['double* sc_num', 'double* sc_den',
                                      'double* log_sum', 'double* partials'],
                 'wn_cepstral_distance': ['double* mcd_sum',
                                          'double* partials']}
    assert set(tgs.ENTRIES) == set(w)


# ------------------------------------------ H7: the entries' own checks
def test_entry_checks_without_a_device(hip_lib):
    """Both entries refuse every bad argument before any launch (no device is
    needed to be refused); the host queries."""
    q = hip_lib.wn_stft_distance_partials
    assert q(1, 1, 1) == 3 and q(8, 160000, 240) == 3 * 8 * 21
    assert q(4, 100, 1) == 3 * 4 * 4 and q(65535, 1 << 30, 1) > 0
    for bad in ((0, 10, 1), (65536, 10, 1), (1, 0, 1), (1, (1 << 30) + 1, 1),
                (1, 10, 0)):
        assert q(*bad) == -1, bad
    st = hip_lib.wn_stft_distance_staged
    for name, want in R.STAGED.items():
        assert st(*R.SHAPES[name][:2]) == want, name
    assert [st(*r[:2]) for r in ((1024, 120), (2048, 240), (512, 50))] == \
        [1, 1, 1]
    assert st(2048, 2048) == 0 and st(100, 10) == 0 and st(64, 65) == 0
    good = dict(gen=4096, ld_gen=100, org=8192, ld_org=100, B=2, T=100,
                lengths=12288, window=16384, basis=20480, n_fft=64, hop=16,
                n_bins=33, floor=1e-7, sc_num=24576, sc_den=28672,
                log_sum=32768, partials=36864, stream=0)
    order = list(good)
    pointers = ('gen', 'org', 'lengths', 'window', 'basis', 'sc_num',
                'sc_den', 'log_sum', 'partials', 'stream')

    def code(**kw):
        a = dict(good, **kw)
        return hip_lib.wn_stft_distance(*[a[k] or None if k in pointers
                                          else a[k] for k in order])
    for name in pointers:
        if name not in ('lengths', 'stream'):
            assert code(**{name: 0}) == -5, name
    for kw in (dict(B=0), dict(B=65536), dict(T=0), dict(T=(1 << 30) + 1),
               dict(ld_gen=99), dict(ld_org=99), dict(n_fft=32, n_bins=17),
               dict(n_fft=100, n_bins=51), dict(n_fft=2112, n_bins=1057),
               dict(hop=0), dict(hop=65), dict(n_bins=32), dict(n_bins=64),
               dict(floor=0.0), dict(floor=-1.0), dict(floor=float('nan')),
               dict(floor=float('inf'))):
        assert code(**kw) == -1, kw
    for name, off in (('gen', 2), ('org', 2), ('lengths', 2), ('window', 2),
                      ('basis', 4), ('basis', 8), ('sc_num', 4),
                      ('sc_den', 4), ('log_sum', 4), ('partials', 4)):
        assert code(**{name: good[name] + off}) == -3, (name, off)

    c = hip_lib.wn_cepstral_distance_partials
    assert c(1, 1) == 1 and c(8, 625) == 80 and c(3, 64) == 3 and \
        c(3, 65) == 6
    for bad in ((0, 1), (1, 0), (1 << 16, 1 << 16)):
        assert c(*bad) == -1, bad
    good = dict(a=4096, b=8192, B=2, F=5, C=80, nframes=12288, dct=16384,
                K=13, mcd_sum=20480, partials=24576, stream=0)
    order = list(good)
    pointers = ('a', 'b', 'nframes', 'dct', 'mcd_sum', 'partials', 'stream')

    def code2(**kw):
        a = dict(good, **kw)
        return hip_lib.wn_cepstral_distance(*[a[k] or None if k in pointers
                                              else a[k] for k in order])
    for name in ('a', 'b', 'dct', 'mcd_sum', 'partials'):
        assert code2(**{name: 0}) == -5, name
    for kw in (dict(B=0), dict(F=0), dict(C=0), dict(C=513), dict(K=0),
               dict(K=80), dict(K=65), dict(C=5, K=5), dict(C=1, K=1),
               dict(B=1 << 16, F=1 << 16)):
        assert code2(**kw) == -1, kw
    for name, off in (('a', 2), ('b', 2), ('nframes', 2), ('dct', 4),
                      ('mcd_sum', 4), ('partials', 4)):
        assert code2(**{name: good[name] + off}) == -3, (name, off)
