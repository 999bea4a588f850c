"""Linear prediction without a device: wavenet/lpc.py's numpy rules against
the independent float64 restatement of tests/lpc_ref.py, the fixtures'
margins (reflection coefficients, minimum phase), the stop rule, limits,
settings, checkpoint entries, the command lines' errors and the binding
table against include/wavenet_lpc.h."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import lpc_ref as R
from util import ROOT

HEADER = 'wavenet_lpc.h'
OTHERS = ('wavenet_hip.h', 'wavenet_pitch.h', 'wavenet_pitch_path.h',
          'wavenet_lc_frames.h', 'wavenet_spectral.h',
          'wavenet_griffin_lim.h')
EPS64 = 2.0 ** -52


def _all_fixture_frames():
    """(name, lp, frames) of every fixture the device tests compare on."""
    yield 'vowel', R.make_lp(), R.vowel_frames()
    yield 'white', R.make_lp(), R.white_frames()
    for c in R.CASES:
        yield c[0], R.case_lp(c[0]), R.case_frames(c[0])


# ------------------------------------------------------ rule vs restatement
@pytest.mark.parametrize('name', ['vowel', 'white'] + [c[0] for c in R.CASES])
def test_rule_agrees_with_the_restatement(name):
    """Both paths get the rule's float32 power spectrum and are float64 from
    there: table sums + Levinson-Durbin against irfft + a Toeplitz solve.
    What they may differ by is float64 rounding through the conditioning of
    the normal equations: a relative perturbation u of r moves the solution by
    at most cond(R) u |a| (to first order); u: the n_bins-term float64 sums
    and the solve, together below 4 n_bins 2^-52."""
    lp, fr = {n: (l, f) for n, l, f in _all_fixture_frames()}[name]
    P = lp.reference_power(fr)
    got = lp.reference_coefficients(fr).astype(np.float64)
    r = R.autocorrelation64(lp, P.astype(np.float64))
    want = R.coefficients_from_power(lp, P)
    # (the rule's own autocorrelation is the irfft's)
    r_rule = lp.reference_autocorrelation(P)
    assert np.abs(r_rule - r).max() <= 4 * lp.n_bins * EPS64 * np.abs(r).max()
    worst = 0.0
    for f in range(fr.shape[0]):
        bound = 4 * lp.n_bins * EPS64 * R.toeplitz_cond(r[f]) * \
            max(1.0, np.abs(want[f]).max()) + \
            np.spacing(np.float32(np.abs(want[f]).max()))   # (the float32 cast)
        err = np.abs(got[f] - want[f]).max()
        worst = max(worst, err / bound)
        assert err <= bound, (name, f, err, bound)
    print('%s: worst error / bound %.3g' % (name, worst))


def test_reflection_coefficients_keep_their_distance():
    """Every fixture frame: all |k| <= 1 - 1e-3 and Levinson runs to the full
    order, so no device comparison straddles the stop."""
    for name, lp, fr in _all_fixture_frames():
        r = lp.reference_autocorrelation(lp.reference_power(fr))
        from wavenet import lpc
        worst = 0.0
        for f in range(fr.shape[0]):
            assert r[f, 0] > 1e-30, (name, f)
            a, ks, err = lpc.levinson(r[f])
            assert ks.shape[0] == lp.order, (name, f, ks.shape)
            worst = max(worst, np.abs(ks).max())
            assert err > 0
        print('%s: largest |k| %.6f' % (name, worst))
        assert worst <= 1 - 1e-3, (name, worst)


def test_float32_predictors_are_minimum_phase():
    worst = 0.0
    for name, lp, fr in _all_fixture_frames():
        cf = lp.reference_coefficients(fr)
        for f in range(cf.shape[0]):
            poly = np.concatenate([[1.0], -cf[f].astype(np.float64)])
            rad = np.abs(np.roots(poly)).max() if lp.order else 0.0
            worst = max(worst, rad)
            assert rad < 1.0, (name, f, rad)
    print('largest pole radius %.4f' % worst)


def test_levinson_stop_rule():
    from wavenet import lpc
    # r[1] > r[0]: the first reflection coefficient is not below 1
    a, ks, err = lpc.levinson([1.0, 1.5, 0.2])
    assert np.array_equal(a, [1.0, 0.0, 0.0]) and ks.shape == (0,)
    a, ks, _ = lpc.levinson([1.0, -1.0, 1.0])            # |k| == 1 exactly
    assert np.array_equal(a, [1.0, 0.0, 0.0]) and ks.shape == (0,)
    # positive definite up to order 1, not beyond: order 1 stands
    a, ks, err = lpc.levinson([1.0, 0.5, -0.9, 0.3])
    assert ks.shape == (1,) and ks[0] == -0.5
    assert np.array_equal(a, [1.0, -0.5, 0.0, 0.0])
    assert err == 0.75
    # a NaN or an infinity further up stops there too
    a, ks, _ = lpc.levinson([1.0, 0.5, np.nan, 0.1])
    assert np.array_equal(a, [1.0, -0.5, 0.0, 0.0])
    a, ks, _ = lpc.levinson([np.inf, np.inf, 1.0])
    assert np.array_equal(a, [1.0, 0.0, 0.0])
    # a clean case against the Toeplitz solve
    r = np.array([1.0, 0.8, 0.5, 0.2])
    a, ks, _ = lpc.levinson(r)
    assert ks.shape == (3,) and np.abs(ks).max() < 1
    assert np.allclose(-a[1:], R.solve64(r), rtol=0, atol=1e-13)


def test_nan_and_inf_frames_give_the_identity():
    lp = R.make_lp()
    fr = R.broken_frames()
    cf = lp.reference_coefficients(fr)
    clean = lp.reference_coefficients(R.vowel_frames()[20:30])
    assert cf.shape == (10, 16) and np.isfinite(cf).all()
    assert not cf[R.NAN_FRAME].any() and not cf[R.INF_FRAME].any()
    keep = [f for f in range(10) if f not in (R.NAN_FRAME, R.INF_FRAME)]
    assert np.array_equal(cf[keep], clean[keep])
    assert clean[R.NAN_FRAME].any() and clean[R.INF_FRAME].any()
    # whatever bits a frame holds, the output is finite
    rng = np.random.default_rng(1)
    wild = rng.integers(-2 ** 31, 2 ** 31, (40, 80), dtype=np.int64) \
        .astype(np.int32).view(np.float32)
    assert np.isfinite(lp.reference_coefficients(wild)).all()
    # nframes: frames at or behind it are zeros
    both = lp.reference_coefficients(
        np.stack([R.vowel_frames()[:6], R.vowel_frames()[6:12]]), [6, 2])
    assert both[1, :2].any() and not both[1, 2:].any()
    assert np.array_equal(both[0], lp.reference_coefficients(
        R.vowel_frames()[:6]))


def test_prediction_gain_on_the_voiced_stretch():
    lp = R.make_lp()
    x = R.vowel()
    e = lp.reference_analysis(x, lp.reference_coefficients(R.vowel_frames()))
    lo, hi = R.VOICED[0] + 1024, R.VOICED[1] - 1024
    gain = 10 * np.log10(np.square(x[lo:hi].astype(np.float64)).sum() /
                         np.square(e[lo:hi].astype(np.float64)).sum())
    print('prediction gain on the voiced stretch: %.1f dB, max |e| %.3f '
          'beside max |x| %.3f' % (gain, np.abs(e).max(), np.abs(x).max()))
    assert gain > 0


# ---------------------------------------------------------------- filters
def test_filters_follow_the_direct_form_bit_for_bit():
    """reference_analysis (vectorised) and reference_synthesis (transposed
    form) against the header's direct form written sample by sample."""
    rng = np.random.default_rng(5)
    for order, hop, T, gain in ((16, 256, 700, 1.0), (32, 7, 300, 8.0),
                                (1, 1, 50, 0.25), (17, 16, 17, 1.0),
                                (5, 16, 3, 1.0)):
        lp = R.make_lp(order, 8, 64, hop if hop <= 64 else 16, gain=gain) \
            if hop != 256 else R.make_lp(order, gain=gain)
        hop = lp.hop
        F = -(-T // hop)
        cf = (rng.uniform(-1, 1, (F, order)) * 0.9 / order).astype(np.float32)
        x = rng.uniform(-1, 1, T).astype(np.float32)
        e = lp.reference_analysis(x, cf)
        assert np.array_equal(e.view(np.int32),
                              R.analysis32_direct(x, cf, hop, gain)
                              .view(np.int32)), (order, hop, T)
        y = lp.reference_synthesis(e, cf)
        assert np.array_equal(y.view(np.int32),
                              R.synthesis32_direct(e, cf, hop, gain)
                              .view(np.int32)), (order, hop, T)
        # float64 loops: the same numbers to float32 accuracy
        assert np.abs(e - R.analysis64(x, cf, hop, gain)).max() < 1e-5 * gain
        # ragged lengths: zeros behind them, nothing read there
        xb = np.stack([x, x])
        xb[1, T // 2:] = np.nan
        n = [T, max(T // 2, 1)]
        cb = np.stack([cf, cf])
        eb = lp.reference_analysis(xb, cb, n)
        assert np.array_equal(eb[0], e) and not eb[1, n[1]:].any()
        assert np.array_equal(eb[1, :n[1]], e[:n[1]])
        yb = lp.reference_synthesis(eb, cb, n)
        assert np.array_equal(yb[0], y) and not yb[1, n[1]:].any()
        assert np.array_equal(yb[1, :n[1]], y[:n[1]])


def test_zero_coefficients_are_the_identity_times_the_gain():
    lp = R.make_lp(16, gain=8.0)
    x = R.white()[:1000]
    cf = np.zeros((4, 16), np.float32)
    e = lp.reference_analysis(x, cf)
    assert np.array_equal(e, x * np.float32(8))
    assert np.array_equal(lp.reference_synthesis(e, cf), x)


def test_round_trip_within_the_measured_bound():
    lp = R.make_lp()
    lo = 8192
    x = np.array(R.vowel()[lo:lo + 12288])
    cf = lp.reference_coefficients(R.vowel_frames())[lo // 256:]
    y = lp.reference_synthesis(lp.reference_analysis(x, cf), cf)
    err = np.abs(y.astype(np.float64) - x).max()
    bound = R.round_trip_bound(x, cf, 256)
    print('round trip: error %.3g, bound %.3g' % (err, bound))
    assert err <= bound
    # the float64 loops invert each other far below that
    y64 = R.synthesis64(R.analysis64(x, cf, 256), cf, 256)
    assert np.abs(y64 - x).max() < 1e-12


# ---------------------------------------------- limits, settings, entries
def test_limits():
    from wavenet import features, lpc
    spec = features.MelSpec(R.SR)
    small = features.MelSpec(R.SR, n_fft=64, hop=16, n_mels=8)
    ok = lpc.LinearPrediction(spec, order=32, noise=0, lag_window=0,
                              gain=2.0 ** 10)
    assert ok.order == 32 and ok.lagwin[0] == 1.0 and (ok.lagwin == 1).all()
    lpc.LinearPrediction(small, order=32, gain=2.0 ** -10)
    for kw in (dict(order=0), dict(order=33), dict(order=16.0),
               dict(order=True), dict(noise=-1e-9), dict(noise=1.0),
               dict(noise=float('nan')), dict(lag_window=-1.0),
               dict(lag_window=float('inf')), dict(gain=2.0 ** -11),
               dict(gain=2.0 ** 10 + 1), dict(gain=0), dict(gain='1')):
        with pytest.raises(ValueError):
            lpc.LinearPrediction(spec, **kw)
    with pytest.raises(ValueError):
        lpc.LinearPrediction(small, order=33)
    with pytest.raises(ValueError):
        lpc.LinearPrediction('mel')
    # order <= n_fft / 2
    tiny = features.MelSpec(R.SR, n_fft=64, hop=16, n_mels=8)
    lpc.LinearPrediction(tiny, order=32)
    # the checks come before any library or device: bad arguments of the
    # device methods raise ValueError here, without a GPU
    lp = lpc.LinearPrediction(spec)
    with pytest.raises(ValueError):
        lp.coefficients(np.zeros((3, 79), np.float32))
    with pytest.raises(ValueError):
        lp.coefficients(np.zeros((3, 80), np.float64))
    with pytest.raises(ValueError):
        lp.coefficients(np.zeros((2, 3, 80), np.float32), [4, 1])
    with pytest.raises(ValueError):       # too few frames of coefficients
        lp.analysis(np.zeros(600, np.float32), np.zeros((2, 16), np.float32))
    with pytest.raises(ValueError):       # another order
        lp.synthesis(np.zeros(600, np.float32), np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError):
        lp.analysis(np.zeros((2, 600), np.float32),
                    np.zeros((2, 3, 16), np.float32), [600, 601])
    with pytest.raises(ValueError):
        lp.analysis(np.zeros((2, 600), np.float32),
                    np.zeros((3, 3, 16), np.float32))


def test_settings_and_entries_round_trip():
    from wavenet import features, lpc
    spec = features.MelSpec(R.SR, n_fft=512, hop=128, n_mels=40, fmin=50.0)
    lp = lpc.LinearPrediction(spec, order=12, noise=1e-3, lag_window=60.0,
                              gain=4.0)
    again = lpc.LinearPrediction.from_settings(lp.settings())
    assert again.settings() == lp.settings()
    assert np.array_equal(again.ctab, lp.ctab) and \
        np.array_equal(again.lagwin, lp.lagwin) and \
        np.array_equal(again.pinv, lp.pinv)
    assert lp.entry() == {'order': 12, 'noise': 1e-3, 'lag_window': 60.0,
                          'gain': 4.0}
    assert lpc.LinearPrediction.from_entry(spec, lp.entry()).entry() == \
        lp.entry()
    assert lpc.LinearPrediction.from_entry(spec, None) is None
    for bad in ({}, {'order': 12}, dict(lp.entry(), more=1),
                dict(lp.entry(), order=40), 'x'):
        with pytest.raises(ValueError):
            lpc.LinearPrediction.from_entry(spec, bad)
    with pytest.raises(ValueError):
        lpc.LinearPrediction.from_settings(dict(lp.settings(), extra=1))
    # the pseudo-inverse is the Griffin-Lim baseline's own
    from wavenet import griffin_lim
    assert np.array_equal(griffin_lim.GriffinLim(spec).pinv, lp.pinv)


def test_from_cli():
    import argparse
    from wavenet import features, lpc
    spec = features.MelSpec(R.SR, n_fft=64, hop=16, n_mels=8)

    def args(**kw):
        d = dict(lpc_order=None, lpc_gain=None, lpc_noise=None,
                 lpc_lag_window=None)
        d.update(kw)
        return argparse.Namespace(**d)
    assert lpc.from_cli(args(), spec) is None
    lp = lpc.from_cli(args(lpc_order=8, lpc_gain=2.0), spec)
    assert lp.entry() == {'order': 8, 'noise': 1e-4, 'lag_window': 40.0,
                          'gain': 2.0}
    stored = lp.entry()
    assert lpc.from_cli(args(), spec, stored).entry() == stored
    assert lpc.from_cli(args(lpc_order=0), spec, stored) is None
    assert lpc.from_cli(args(lpc_order=4), spec, stored).entry() == \
        dict(stored, order=4)
    # a continued run keeps its checkpoint's settings
    assert lpc.from_cli(args(), spec, stored, True).entry() == stored
    assert lpc.from_cli(args(lpc_order=8, lpc_gain=2.0), spec, stored,
                        True).entry() == stored
    for a, st in ((args(lpc_order=4), stored), (args(lpc_order=0), stored),
                  (args(lpc_order=8, lpc_gain=1.0), stored),
                  (args(lpc_order=8), None)):
        with pytest.raises(ValueError) as e:
            lpc.from_cli(a, spec, st, True)
        assert 'lpc_order' in str(e.value) and repr(st) in str(e.value)
    with pytest.raises(ValueError):
        lpc.from_cli(args(lpc_order=8), None)         # no front end
    with pytest.raises(ValueError):
        lpc.from_cli(args(), spec, {'order': 8})      # a broken entry


def _normalised_front_ends():
    """(mel, mel+f0): a MelSpec with a range normaliser that clamps, and the
    composite front end over it."""
    from wavenet import features, frontend, pitch
    norm = features.Normalizer.from_range(-12.0, 2.0, 8)
    mel = features.MelSpec(R.SR, n_fft=64, hop=16, n_mels=8, normalizer=norm)
    return mel, frontend.MelPitchSpec(mel, pitch.PitchTracker(R.SR, hop=16))


def test_a_feature_file_gets_the_front_ends_normaliser_inverted():
    """generate.py --lc_path: the coefficients of a normalised file are those
    of normalizer.invert(mel columns) -- for a mel file and for a mel+f0
    file, whose `.mel` part carries no normaliser of its own."""
    import argparse
    import generate
    from wavenet import lpc
    mel, both = _normalised_front_ends()
    raw = R.logmel(R.vowel()[:2000], R.make_lp(8, 8, 64, 16))
    feats = mel.normalizer.reference(raw)                # [125, 8], clamped
    assert (feats == 0).any() and (feats == 1).any()     # (the clamp bites)
    f0 = np.linspace(0, 1, 2 * raw.shape[0], dtype=np.float32).reshape(-1, 2)
    args = argparse.Namespace(lpc_order=8, lpc_gain=None, lpc_noise=None,
                              lpc_lag_window=None)

    class OnTheHost(lpc.LinearPrediction):
        def coefficients(self, frames, nframes=None):
            return self.reference_coefficients(np.asarray(frames), nframes)
    for spec, data in ((mel, feats), (both, np.concatenate([feats, f0], 1))):
        lp = lpc.from_cli(args, spec)
        assert lp.spec.normalizer is None or spec is mel
        lp.__class__ = OnTheHost
        back = np.asarray(spec.normalizer.invert(feats))
        got_raw = np.asarray(lpc.frames_of_file(data, spec))
        assert np.array_equal(got_raw, back)
        assert np.abs(back - raw).max() > 1.0            # (clamped stays so)
        assert np.abs(back - feats).max() > 1.0          # (and it was inverted)
        got = generate._lpc_from_file(lp, data, spec)
        want = lp.reference_coefficients(back)
        assert np.array_equal(got, want) and want.any()
        assert not np.array_equal(got, lp.reference_coefficients(feats))
        # a file without the mel columns
        assert generate._lpc_from_file(lp, data[:, :5], spec) is None
        assert lpc.frames_of_file(data[0], spec) is None
    # without a normaliser the columns are taken as they are
    plain = mel.with_normalizer(None)
    assert np.array_equal(lpc.frames_of_file(raw, plain), raw)


def test_with_lpc_refuses_another_front_end():
    from wavenet import evaluate as ev, features
    mel, both = _normalised_front_ends()
    lp = R.make_lp(8, 8, 64, 16)
    # (the same raw front end, with or without a normaliser, mel or mel+f0)
    for spec in (mel, both, mel.with_normalizer(None)):
        assert list(ev.with_lpc(lp, spec, iter(()))) == []
    other = features.MelSpec(R.SR, n_fft=128, hop=16, n_mels=8)
    with pytest.raises(ValueError) as e:
        ev.with_lpc(lp, other, iter(()))
    assert 'another front end' in str(e.value)


# ------------------------------------------------------ the command lines
def _refused(script, argv):
    """The message of the script's argparse error alone: what follows
    'error:' on the last line (the usage text in front of it lists every
    flag of the script and proves nothing)."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv,
                       cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 2, out          # (argparse's own exit status)
    last = out.strip().splitlines()[-1]
    assert ': error: ' in last, out
    return last.split(': error: ', 1)[1]


MEL = ['--lc_features', 'mel', '--lc_channels', '8', '--lc_hop', '16',
       '--lc_n_fft', '64']


@pytest.mark.parametrize('argv,words', [
    (['--lpc_order', '8'], ['--lpc_order needs --lc_features mel or mel+f0']),
    (MEL + ['--lpc_order', '8', '--preemphasis', '0.97'],
     ['--lpc_order and --preemphasis', 'choose one']),
    (MEL + ['--lpc_order', '8', '--device_corpus', 'true', '--data_dir', 'x',
            '--lc_feature_context', 'utterance'],
     ['--lpc_order does not go with --lc_feature_context utterance']),
    (MEL + ['--lpc_gain', '2'], ['--lpc_gain needs --lpc_order']),
    (MEL + ['--lpc_noise', '1e-3'], ['--lpc_noise needs --lpc_order']),
    (MEL + ['--lpc_lag_window', '50'],
     ['--lpc_lag_window needs --lpc_order']),
    (MEL + ['--lpc_order', '33'], ['--lpc_order', 'order must be', '33']),
    (MEL + ['--lpc_order', '-1'], ['--lpc_order', 'order must be', '-1']),
    (MEL + ['--lpc_order', 'x'],
     ['argument --lpc_order: invalid int value']),
    (MEL + ['--lpc_order', '8', '--lpc_gain', '0'],
     ['--lpc_gain', 'gain must lie']),
    (MEL + ['--lpc_order', '8', '--lpc_gain', 'big'],
     ['argument --lpc_gain: invalid float value']),
    (MEL + ['--lpc_order', '8', '--lpc_noise', '1'],
     ['--lpc_noise', 'noise must lie']),
    (MEL + ['--lpc_order', '8', '--lpc_lag_window', '-3'],
     ['--lpc_lag_window', 'lag_window must be']),
])
def test_train_refuses(argv, words):
    msg = _refused('train.py', ['--synthetic'] + argv)
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize('script,argv,words', [
    ('generate.py', ['ck', '--lpc_order', '8', '--wav_seed', 's.wav'],
     ['--lpc_order does not go with --wav_seed']),
    ('generate.py', ['ck', '--lpc_order', '8', '--preemphasis', '0.9'],
     ['--lpc_order and --preemphasis', 'choose one']),
    ('generate.py', ['ck', '--lpc_gain', '2'],
     ['--lpc_gain needs --lpc_order']),
    ('generate.py', ['ck', '--lpc_order', '40'],
     ['--lpc_order', 'order must be', '40']),
    ('evaluate.py', ['ck', '--data_dir', 'd', '--lpc_noise', '0.1'],
     ['--lpc_noise needs --lpc_order']),
    ('evaluate.py', ['ck', '--data_dir', 'd', '--lpc_order', '8',
                     '--preemphasis', '0.9'],
     ['--lpc_order and --preemphasis', 'choose one']),
    ('evaluate.py', ['ck', '--data_dir', 'd', '--lpc_order', '8',
                     '--lpc_gain', '1e9'], ['--lpc_gain', 'gain must lie']),
])
def test_generate_and_evaluate_refuse(script, argv, words):
    msg = _refused(script, argv)
    for w in words:
        assert w in msg, msg


def test_generate_needs_frames_for_an_lpc_checkpoint(tmp_path):
    """A checkpoint with an 'lpc' entry and no --lc_wav / --lc_wav_dir /
    --lc_path: refused, naming the flags, before any model is built."""
    import torch
    ck = str(tmp_path / 'model.ckpt-0')
    torch.save({'variables': {}, 'step': 0,
                'lpc': {'order': 8, 'noise': 1e-4, 'lag_window': 40.0,
                        'gain': 1.0}}, ck)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), ck,
                        '--samples', '4'], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 1, out
    for w in ('--lpc_order', '--lc_wav', '--lc_path'):
        assert w in out, out
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'generate.py'), ck,
                        '--samples', '4', '--wav_seed', 'seed.wav'], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=300)
    assert p.returncode == 1 and '--wav_seed' in p.stdout.decode()


# ------------------------------------------------------------ the bindings
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(2): (m.group(1), [' '.join(p.split())
                                      for p in m.group(3).split(',')])
            for m in re.finditer(
                r'\b(int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_binding_table_matches_its_header():
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_lpc_from_mel', 'wn_lpc_analysis_tile',
                         'wn_lpc_analysis', 'wn_lpc_synthesis'}
    assert set(_lib.LPC_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double}
    for name, (res, params) in decl.items():
        params = [p for p in params if p != 'void']
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.LPC_SIGNATURES[name] == (ctype[res], want), name
    for other in OTHERS:
        assert not set(decl) & set(_declarations(other)), other
    assert not set(decl) & (set(_lib.SIGNATURES) | set(_lib.PITCH_SIGNATURES)
                            | set(_lib.PITCH_PATH_SIGNATURES)
                            | set(_lib.LC_FRAMES_SIGNATURES)
                            | set(_lib.SPECTRAL_SIGNATURES)
                            | set(_lib.GRIFFIN_LIM_SIGNATURES))


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.LPC_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_lpc as tg
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_lpc_from_mel': ['float* out'],
                 'wn_lpc_analysis': ['float* out'],
                 'wn_lpc_synthesis': ['float* out']}
    assert set(tg.ENTRIES) == set(w)


OK, BAD_SHAPE, MISALIGNED, NULL = 0, -1, -3, -5


def test_the_entries_own_checks(hip_lib):
    """Every refusal comes back before any launch (no device here)."""
    import ctypes
    assert hip_lib.wn_lpc_analysis_tile() == 1024
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    fm = hip_lib.wn_lpc_from_mel
    good = [a, 2, 3, 80, None, a, 513, a, a, 16, a, None]

    def with_(i, v):
        g = list(good)
        g[i] = v
        return g
    for i in (0, 5, 7, 8, 10):
        assert fm(*with_(i, None)) == NULL
    for i, v in ((1, 0), (1, 65536), (2, 0), (3, 0), (3, 129), (6, 1),
                 (6, 1026), (9, 0), (9, 33)):
        assert fm(*with_(i, v)) == BAD_SHAPE, (i, v)
    assert fm(a, 2, 3, 8, None, a, 9, a, a, 9, a, None) == BAD_SHAPE
    assert fm(*with_(0, a + 2)) == MISALIGNED
    assert fm(*with_(7, a + 4)) == MISALIGNED
    assert fm(*with_(4, a + 1)) == MISALIGNED
    for fn, alias in ((hip_lib.wn_lpc_analysis, False),
                      (hip_lib.wn_lpc_synthesis, True)):
        # in, ld, coeffs, F, order, hop, lengths, B, T, g, out, ld, stream
        good = [a, 600, a + 8192, 3, 16, 256, None, 2, 600, 1.0, a + 16384,
                600, None]
        for i in (0, 2, 10):
            assert fn(*with_(i, None)) == NULL
        for i, v in ((1, 599), (3, 0), (3, 2), (4, 0), (4, 33), (5, 0),
                     (5, 4097), (7, 0), (7, 65536), (8, 0), (8, 2 ** 30 + 1),
                     (9, 0.0), (9, -1.0), (9, float('inf')),
                     (9, float('nan')), (11, 599)):
            assert fn(*with_(i, v)) == BAD_SHAPE, (i, v)
        # with lengths the frames are the caller's to check
        assert fn(*with_(6, a + 2)) == MISALIGNED
        assert fn(*with_(0, a + 1)) == MISALIGNED
        assert fn(*with_(10, a + 16386)) == MISALIGNED
        same = with_(10, a)
        if not alias:
            assert fn(*same) == BAD_SHAPE
        else:
            same[11] = 608                 # the same pointer, another ld
            assert fn(*same) == BAD_SHAPE
