"""The pitch tracker's host side (wavenet/pitch.py, include/wavenet_pitch.h)
without a device: argument checks before the library, the lag range of the C
queries, PitchTracker.reference against the float64 oracle of
tests/pitch_ref.py, the oracle against steady tones, the recorded float32
yardsticks, the share of decisive frames on the GPU test's inputs, f0_error and
channels on CPU tensors, evaluate.py's flag errors and the coverage of the
header's writing entries by tests/test_gpu_guard_pitch.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pitch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_library(monkeypatch):
    from wavenet import _lib

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libwavenet_hip.so')


BAD = [
    dict(sample_rate=0), dict(sample_rate=-16000), dict(sample_rate='16k'),
    dict(sample_rate=float('nan')), dict(sample_rate=True),
    dict(hop=0), dict(hop=4097), dict(hop=256.0), dict(hop=True),
    dict(window=32), dict(window=1000), dict(window=2112), dict(window=1024.0),
    dict(fmin=0.0), dict(fmin=500.0), dict(fmin=600.0), dict(fmax=float('inf')),
    dict(fmin=None),
    dict(threshold=0.0), dict(threshold=1.0), dict(threshold=-0.1),
    dict(threshold=1e-60), dict(threshold=float('nan')),
    dict(silence=-1e-9), dict(silence=float('nan')), dict(silence=None),
    dict(fmin=15.0),                          # tau_max 1067 > 1024
    dict(sample_rate=48000, fmin=46.8),       # tau_max 1026
    dict(fmin=7000.0, fmax=7900.0),           # lags 2 .. 3: no tau_min + 2
]


@pytest.mark.parametrize('kw', BAD, ids=lambda kw: ','.join(
    '%s=%r' % kv for kv in kw.items()))
def test_bad_settings_raise_before_the_library(monkeypatch, kw):
    _no_library(monkeypatch)
    from wavenet import pitch
    with pytest.raises(ValueError):
        pitch.PitchTracker(**dict(dict(sample_rate=16000), **kw))


def test_limits_that_pass(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import pitch
    t = pitch.PitchTracker(16000)
    assert (t.hop, t.window, t.fmin, t.fmax, t.threshold, t.silence) == \
        (256, 1024, 60.0, 500.0, 0.15, 1e-7)
    assert (t.tau_min, t.tau_max) == (32, 267)
    assert t.num_frames(1) == 1 and t.num_frames(256) == 1 and \
        t.num_frames(257) == 2
    for kw in (dict(hop=1), dict(hop=4096), dict(window=64),
               dict(window=2048), dict(silence=0.0), dict(fmin=15.625),
               dict(sample_rate=48000, fmin=46.875),
               dict(sample_rate=1000, fmin=300.0, fmax=400.0)):
        pitch.PitchTracker(**dict(dict(sample_rate=16000), **kw))
    assert pitch.PitchTracker(16000, fmin=15.625).tau_max == 1024
    assert pitch.PitchTracker(16000, fmax=8000.0).tau_min == 2
    assert pitch.PitchTracker(16000, fmax=16000.0).tau_min == 2


def test_bad_audio_and_lengths_raise_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import pitch
    t = pitch.PitchTracker(16000)
    x = np.zeros((2, 100), np.float32)
    for audio, lengths in ((np.zeros((2, 100), np.int16), None),
                           (np.zeros((2, 3, 4), np.float32), None),
                           (np.zeros((0, 4), np.float32), None),
                           (np.zeros(0, np.float32), None),
                           (torch.zeros(2, 100, dtype=torch.int32), None),
                           (x, [100]), (x, [0, 100]), (x, [100, 101]),
                           (x, [1.0, 2.0]), (x, [[1, 2]])):
        with pytest.raises(ValueError):
            t(audio, lengths)


def test_settings_round_trip(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import pitch
    for kw in (dict(sample_rate=16000),
               dict(sample_rate=22050.0, hop=300, fmin=70.3, fmax=412.7,
                    window=576, threshold=0.1 + 0.2, silence=3e-9)):
        t = pitch.PitchTracker(**kw)
        d = t.settings()
        assert set(d) == {'sample_rate', 'hop', 'fmin', 'fmax', 'window',
                          'threshold', 'silence'}
        assert all(type(v) in (int, float) for v in d.values())
        u = pitch.PitchTracker.from_settings(d)
        assert u.settings() == d
        assert (u.tau_min, u.tau_max) == (t.tau_min, t.tau_max)
        assert type(u.sample_rate) is type(kw['sample_rate'])
    with pytest.raises(ValueError):
        pitch.PitchTracker.from_settings({'hop': 256})


def test_c_queries_equal_python(hip_lib):
    from wavenet import _lib, pitch
    assert set(_lib.PITCH_SIGNATURES) == {
        'wn_pitch_tau_min', 'wn_pitch_tau_max', 'wn_pitch_lds_bytes',
        'wn_pitch_track'}
    assert not set(_lib.PITCH_SIGNATURES) & set(_lib.SIGNATURES)
    rates = (8000, 11025, 16000, 22050, 24000, 44100, 48000, 16000.5)
    lows = (46.875, 50.0, 60.0, 62.5, 70.3, 80.0, 100.0, 110.25, 125.0)
    highs = (250.0, 320.0, 400.0, 441.0, 500.0, 800.0, 1102.5, 4000.0,
             8000.0, 24000.0)
    for sr in rates:
        for fmin in lows:
            for fmax in highs:
                lo, hi = pitch.lag_range(sr, fmin, fmax)
                assert hip_lib.wn_pitch_tau_min(sr, fmax) == lo, (sr, fmax)
                assert hip_lib.wn_pitch_tau_max(sr, fmin) == hi, (sr, fmin)
                # (float32 numbers all but one: the oracle's formula in
                # plain doubles gives the same lags)
                if fmin != 70.3:
                    assert (lo, hi) == R.lag_range(sr, fmin, fmax)
    # exact divisions stay exact
    assert hip_lib.wn_pitch_tau_min(16000, 500.0) == 32
    assert hip_lib.wn_pitch_tau_max(16000, 62.5) == 256
    assert hip_lib.wn_pitch_tau_max(48000, 46.875) == 1024
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert hip_lib.wn_pitch_tau_min(16000, bad) == -1
        assert hip_lib.wn_pitch_tau_max(bad, 60.0) == -1


def test_lds_bytes_and_entry_checks_without_a_device(hip_lib):
    """wn_pitch_lds_bytes is the header's formula; wn_pitch_track refuses
    every bad argument before any launch (no device is needed to be
    refused)."""
    def want(W, tmax):
        NS = (W + tmax + 8 + 3) // 4 * 4
        G4 = (tmax + 3) // 4 * 4
        return 4 * (NS + W + 8 * G4) + 64
    for W, tmax, hop in ((1024, 267, 256), (64, 9, 1), (2048, 1024, 461),
                         (128, 65, 100), (64, 4, 4096)):
        assert hip_lib.wn_pitch_lds_bytes(W, tmax, hop) == want(W, tmax)
    assert hip_lib.wn_pitch_lds_bytes(2048, 1024, 256) == 53344
    for W, tmax, hop in ((0, 267, 256), (1000, 267, 256), (2112, 267, 256),
                         (1024, 3, 256), (1024, 1025, 256), (1024, 267, 0),
                         (1024, 267, 4097)):
        assert hip_lib.wn_pitch_lds_bytes(W, tmax, hop) == -1
    good = dict(audio=256, lengths=0, ld=100, B=1, T=100, hop=256,
                window=1024, tau_min=32, tau_max=267, threshold=0.15,
                silence=1e-7, sample_rate=16000.0, f0=512, aper=768,
                lag=1024, cmnd=0, stream=0)
    order = list(good)

    def code(**kw):
        a = dict(good, **kw)
        return hip_lib.wn_pitch_track(*[a[k] or None if k in (
            'audio', 'lengths', 'f0', 'aper', 'lag', 'cmnd', 'stream')
            else a[k] for k in order])
    for name in ('audio', 'f0', 'aper', 'lag'):
        assert code(**{name: 0}) == -5, name
    for kw in (dict(hop=0), dict(hop=4097), dict(window=32),
               dict(window=1000), dict(window=2112), dict(tau_min=1),
               dict(tau_min=266), dict(tau_max=1025), dict(threshold=0.0),
               dict(threshold=1.0), dict(threshold=float('nan')),
               dict(silence=-1.0), dict(silence=float('nan')),
               dict(sample_rate=0.0), dict(sample_rate=float('inf')),
               dict(B=0), dict(B=65536), dict(T=0), dict(T=(1 << 30) + 1),
               dict(ld=99)):
        assert code(**kw) == -1, kw
    for name in ('audio', 'lengths', 'f0', 'aper', 'lag', 'cmnd'):
        assert code(**{name: 4098}) == -3, name


# ------------------------------------------------------ rule and oracle
@pytest.fixture(scope='module')
def oracle():
    """name -> the `track` results of the clips of make_audio, computed once
    and shared."""
    return {name: [R.track(clip, **R.settings(name))
                   for clip in R.clips(name)] for name in R.SHAPES}


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_reference_is_the_oracle(oracle, name):
    from wavenet import pitch
    kw = R.settings(name)
    t = pitch.PitchTracker(**kw)
    assert (t.tau_min, t.tau_max) == R.LAGS[name] == \
        R.lag_range(kw['sample_rate'], kw['fmin'], kw['fmax'])
    for clip, ref in zip(R.clips(name), oracle[name]):
        p = t.reference(clip)
        assert p.f0.dtype == np.float64 and p.lag.dtype == np.int32
        assert p.f0.shape == (t.num_frames(clip.shape[0]),)
        assert p.cmnd.shape == (p.f0.shape[0], t.tau_max + 1)
        assert np.array_equal(p.lag, ref['lag'])
        assert np.array_equal(p.f0 > 0, ref['voiced'])
        assert np.abs(p.cmnd - ref['cmnd']).max() <= 1e-12
        assert np.abs(p.aper - ref['aper']).max() <= 1e-12
        assert np.allclose(p.f0, ref['f0'], rtol=1e-12, atol=0)
        # float32: the same picks on the decisive frames, c' within the
        # device's bound
        q = t.reference(clip, np.float32)
        assert q.f0.dtype == np.float32 and q.cmnd.dtype == np.float32
        m = R.shape_tol(name)
        assert np.abs(q.cmnd.astype(np.float64) - ref['cmnd']).max() <= m
        dec = R.decisive_frames(ref, m, **kw)
        assert np.array_equal(q.lag[dec], ref['lag'][dec])
        assert np.array_equal(q.f0[dec] > 0, ref['voiced'][dec])


def test_signal_reaches_every_kind_of_frame(oracle):
    """Shape (a): voiced, unvoiced and silent frames, and a frame whose first
    window + tau_min - 1 samples are the constant (S[tau] = 0 and c'[tau] = 1
    for tau < tau_min, not throughout)."""
    ref = oracle['a'][0]
    loud = ~ref['silent']
    assert ref['voiced'].sum() >= 5 and ref['silent'].sum() >= 1
    assert (loud & ~ref['voiced']).sum() >= 3
    c = ref['cmnd']
    flat = loud & (c[:, 1:32] == 1.0).all(1) & (c[:, 32:] != 1.0).any(1)
    assert flat.sum() >= 1
    x, lengths = R.make_audio('a')
    assert (x == 0.25).sum() >= x.shape[0] * (1024 + 31)
    assert (x == 0.0).sum() >= x.shape[0] * 1024


@pytest.mark.parametrize('f', R.TONES)
def test_steady_tones(f):
    """Every interior frame of a three-harmonic tone is voiced and within
    TONE_BOUND of the truth, for the oracle and for the package's rule."""
    from wavenet import pitch
    err = R.tone_error(f)
    print('tone %g Hz: |f0 / f - 1| <= %.3g (recorded %.3g)'
          % (f, err, R.TONE_ERR_MEASURED[f]))
    assert err <= R.TONE_BOUND <= 1e-3
    assert 0.9 * err <= R.TONE_ERR_MEASURED[f] <= R.TONE_BOUND
    t = pitch.PitchTracker(16000)
    x = R.tone(f)
    p = t.reference(x)
    idx = R.interior(p.f0.shape[0], x.shape[0], t.hop, t.window, t.tau_max)
    assert len(idx) >= 20
    assert (p.f0[idx] > 0).all()
    assert np.abs(p.f0[idx] / f - 1.0).max() <= R.TONE_BOUND


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_recorded_yardstick(name):
    """PITCH_F32_MEASURED is what this host measures (numpy's pairwise sum
    may differ a little between builds)."""
    got = R.yardstick_terms(name)
    rec = R.PITCH_F32_MEASURED[name]
    print('%s: measured %s, recorded %s' % (name, got, rec))
    assert rec[2] == got[2] == 2.0 ** -23
    for g, r in zip(got[:2], rec[:2]):
        assert g <= 1.25 * r and r <= 2.0 * g + 1e-30
    assert R.shape_tol(name) == 4.0 * max(rec)


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_at_most_one_frame_in_twenty_is_not_decisive(oracle, name):
    """The cap, on the oracle alone: the GPU test asserts lag, voicing, f0
    and aper on the decisive frames only, and they are (nearly) all."""
    kw = R.settings(name)
    m = R.shape_tol(name)
    total = bad = 0
    for ref in oracle[name]:
        dec = R.decisive_frames(ref, m, **kw)
        total += dec.size
        bad += int((~dec).sum())
    print('%s: %d of %d frames are not decisive at m = %.3g'
          % (name, bad, total, m))
    assert total >= 1 and bad <= 0.05 * total


def test_decisive_is_conservative():
    """Rows built by hand: each clause alone turns `decisive` off."""
    m, thr = 1e-3, 0.15
    base = np.full(41, 0.5)
    base[0] = 1.0

    def row(**at):
        c = base.copy()
        for k, v in at.items():
            c[int(k[1:])] = v
        return c
    args = (m, 10, 40, thr)
    good = row(t19=0.3, t20=0.05, t21=0.3)
    assert R.pick(good, 10, 40, thr)[:2] == (20, True)
    assert R.decisive(good, *args)
    # a value within m of the threshold in front of the pick
    assert not R.decisive(row(t15=thr + 0.5 * m, t19=0.3, t20=0.05, t21=0.3),
                          *args)
    # the walk down the slope compares two values within 2 m
    assert not R.decisive(row(t19=0.3, t20=0.05, t21=0.05 + m, t22=0.3),
                          *args)
    # a neighbour within 2 m of the minimum
    assert not R.decisive(row(t19=0.05 + m, t20=0.05, t21=0.3), *args)
    # a flat parabola: 3 m / den > 1 / 4
    flat = row(t19=0.055, t20=0.05, t21=0.055)
    assert R.parabola(flat, 20)[1] < 12 * m and not R.decisive(flat, *args)
    # unvoiced: a unique minimum is decisive, a second one within 2 m is not
    assert R.decisive(row(t30=0.4), *args)
    assert R.pick(row(t30=0.4), 10, 40, thr)[:2] == (30, False)
    assert not R.decisive(row(t30=0.4, t12=0.4 + m), *args)
    assert not R.decisive(base, *args)         # all equal: a tie


# -------------------------------------------------- f0_error and channels
def _tracks():
    rng = np.random.default_rng(7)
    fb = rng.uniform(60, 500, (3, 50))
    fb[rng.uniform(size=fb.shape) < 0.3] = 0.0
    fa = fb * rng.uniform(0.97, 1.03, fb.shape)
    flip = rng.uniform(size=fb.shape)
    fa[flip < 0.1] *= 2.0                               # octave errors
    fa[(flip > 0.1) & (flip < 0.2)] = 0.0               # lost voicing
    fa[(flip > 0.2) & (flip < 0.3) & (fb == 0)] = 111.0   # false voicing
    fa[0, 3], fb[0, 3] = 120.0, 100.0                   # exactly at 20 %
    return fa.astype(np.float32), fb.astype(np.float32)


@pytest.mark.parametrize('nframes', [None, [50, 17, 0]])
def test_f0_error_on_cpu_tensors(nframes):
    from wavenet import pitch
    fa, fb = _tracks()
    want = R.f0_error(fa, fb, nframes)
    got = pitch.f0_error(torch.from_numpy(fa), torch.from_numpy(fb), nframes)
    for k in ('frames', 'both', 'gross', 'fine', 'vuv', 'voiced_ref'):
        t = getattr(got, k)
        assert t.dtype == torch.int64 and t.shape == (3,)
        assert np.array_equal(t.numpy(), want[k]), k
    assert got.sq_cents.dtype == torch.float64
    assert np.allclose(got.sq_cents.numpy(), want['sq_cents'], rtol=1e-9,
                       atol=0)
    assert want['gross'].sum() > 0 and want['vuv'].sum() > 0
    s, ws = got.summary(), R.f0_summary(want)
    assert set(s) == {'f0_rmse_cents', 'gross_pitch_error', 'vuv_error',
                      'voiced_frames', 'frames'}
    for k in s:
        assert s[k] == pytest.approx(ws[k], rel=1e-9), k
    # Pitch in, [F] in
    p = pitch.Pitch(torch.from_numpy(fa), None, None, None)
    q = pitch.Pitch(torch.from_numpy(fb), None, None, None)
    again = pitch.f0_error(p, q, nframes)
    assert all(torch.equal(a, b) for a, b in zip(again, got))
    one = pitch.f0_error(torch.from_numpy(fa[1]), torch.from_numpy(fb[1]))
    assert one.frames.shape == (1,) and int(one.frames) == 50


def test_f0_error_empty_denominators_and_bad_arguments():
    from wavenet import pitch
    z = torch.zeros(2, 5)
    v = torch.full((2, 5), 100.0)
    s = pitch.f0_error(z, z).summary()             # nothing voiced
    assert s == {'f0_rmse_cents': None, 'gross_pitch_error': None,
                 'vuv_error': 0.0, 'voiced_frames': 0, 'frames': 10}
    s = pitch.f0_error(v * 2, v).summary()         # all gross: no fine frame
    assert s['f0_rmse_cents'] is None and s['gross_pitch_error'] == 1.0
    assert s['voiced_frames'] == 10
    s = pitch.f0_error(v, z).summary()
    assert s['vuv_error'] == 1.0 and s['gross_pitch_error'] is None
    s = pitch.f0_error(v * 2 ** (1 / 12), v).summary()     # a semitone
    assert s['f0_rmse_cents'] == pytest.approx(100.0, rel=1e-6)
    with pytest.raises(ValueError):
        pitch.f0_error(z, z, [0, 0]).summary()     # no frames at all
    with pytest.raises(ValueError):
        pitch.f0_error(z, torch.zeros(2, 6))
    with pytest.raises(ValueError):
        pitch.f0_error(z, z, [5])
    with pytest.raises(ValueError):
        pitch.f0_error(z.long(), z.long())


@pytest.mark.parametrize('nframes', [None, [50, 17, 0]])
def test_channels_on_cpu_tensors(nframes):
    from wavenet import pitch
    fa, _ = _tracks()
    fa[0, :4] = (30.0, 60.0, 500.0, 900.0)         # below, at, at, above
    t = pitch.PitchTracker(16000)
    want = R.channels(fa, 60.0, 500.0, nframes)
    got = t.channels(torch.from_numpy(fa), nframes)
    assert got.dtype == torch.float32 and got.shape == (3, 50, 2)
    assert np.allclose(got.numpy(), want, rtol=1e-9, atol=0)
    assert np.array_equal(got.numpy()[..., 1], want[..., 1])
    assert got.numpy()[0, :4, 0].tolist() == [0.0, 0.0, 1.0, 1.0]
    assert got.numpy()[..., 0].min() == 0.0 and got.numpy().max() == 1.0
    assert np.array_equal(got.numpy()[fa == 0], np.zeros(((fa == 0).sum(), 2)))
    p = pitch.Pitch(torch.from_numpy(fa), None, None, None)
    assert torch.equal(t.channels(p, nframes), got)
    assert t.channels(torch.from_numpy(fa[2])).shape == (50, 2)


# ------------------------------------------------------------ command line
def _error_of(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py')] +
                       argv, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stderr.decode()


def test_evaluate_pitch_flags_need_their_switch():
    code, err = _error_of(['ckpt', '--data_dir', 'in', '--synthesis_pitch',
                           'true'])
    assert code == 2 and '--synthesis_pitch needs --synthesis true' in err
    code, err = _error_of(['ckpt', '--data_dir', 'in', '--synthesis', 'true',
                           '--pitch_fmin', '70'])
    assert code == 2 and '--pitch_fmin needs --synthesis_pitch true' in err


def test_evaluate_builds_the_tracker_from_the_front_end(monkeypatch):
    _no_library(monkeypatch)
    import argparse
    import evaluate
    from wavenet import features
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    t = evaluate._pitch_tracker(
        argparse.Namespace(pitch_fmin=None, pitch_fmax=None), spec)
    assert t.settings() == dict(sample_rate=16000, hop=16, fmin=60.0,
                                fmax=500.0, window=1024, threshold=0.15,
                                silence=1e-7)
    t = evaluate._pitch_tracker(
        argparse.Namespace(pitch_fmin=100.0, pitch_fmax=400.0), spec)
    assert (t.fmin, t.fmax, t.tau_min, t.tau_max) == (100.0, 400.0, 40, 160)
    with pytest.raises(ValueError):
        evaluate._pitch_tracker(
            argparse.Namespace(pitch_fmin=10.0, pitch_fmax=None), spec)
    assert 'synthesis_pitch' in evaluate.SYNTHESIS_FLAGS


# ---------------------------------------------------- coverage of the ABI
def _entries_that_write(header):
    """tests/test_guard_host.py::_entries_that_write on another header: name
    -> the non-const pointer parameters of every int / long wn_*
    declaration (the stream handle is not an operand)."""
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src):
        params = [' '.join(p.split()) for p in m.group(2).split(',')]
        w = [p for p in params if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
        if w:
            out[m.group(1)] = w
    return out


def test_every_writing_entry_of_the_pitch_header_is_guarded():
    import test_gpu_guard_pitch as tgp
    w = _entries_that_write('wavenet_pitch.h')
    assert w == {'wn_pitch_track': ['float* f0', 'float* aper',
                                    'int32_t* lag', 'float* cmnd']}
    assert set(tgp.ENTRIES) == set(w)


def test_pitch_binding_table_matches_its_header():
    """Every declaration of wavenet_pitch.h is bound with as many arguments
    as it declares, and nothing else is."""
    from wavenet import _lib
    src = open(os.path.join(ROOT, 'include', 'wavenet_pitch.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    decl = {m.group(1): len(m.group(2).split(','))
            for m in re.finditer(r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;',
                                 src)}
    assert decl == {k: len(v[1]) for k, v in _lib.PITCH_SIGNATURES.items()}
    main = open(os.path.join(ROOT, 'include', 'wavenet_hip.h')).read()
    assert not any(re.search(r'\b%s\b' % k, main) for k in decl)
