"""The pitch path's host side (wavenet/pitch.py: PitchPath, include/
wavenet_pitch_path.h) without a device: the float64 oracle of
tests/pitch_path_ref.py against enumeration (H1), PitchPath.reference against
the oracle within the derived rounding bound (H2), the tie rules against a
sequential restatement (H3), the octave case (H4), a steady tone (H5),
argument checks, settings and tables (H6), the binding table against the
header (H7) and the coverage of the header's writing entries by
tests/test_gpu_guard_pitch_path.py (H8)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pitch_path_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'wavenet_pitch_path.h'


def _no_library(monkeypatch):
    from wavenet import _lib

    def boom(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libwavenet_hip.so')


def _path(tau_min=None, tau_max=None, **kw):
    """A PitchPath on the default tracker, or on one with the given lags
    (sample rate 16000: fmax just under 16000 / tau_min, fmin just over
    16000 / tau_max)."""
    from wavenet import pitch
    return pitch.PitchPath(R.tracker_with_lags(pitch, tau_min, tau_max), **kw)


def _weights(path):
    t = path.tracker
    return dict(tau_min=t.tau_min, tau_max=t.tau_max, jump=path.jump,
                octave_bias=path.octave_bias, switch=path.switch,
                unvoiced=path.unvoiced)


# ------------------------------------------------------------ H1: the oracle
@pytest.mark.parametrize('N,F', [(2, 1), (2, 2), (2, 4), (3, 1), (3, 3),
                                 (3, 4)])
def test_oracle_against_enumeration(N, F):
    for seed in range(4):
        c, lag = R.random_rows(seed, F, 2 + N, silent=0.3)
        kw = dict(tau_min=2, tau_max=2 + N, jump=0.3, octave_bias=0.05,
                  switch=0.2, unvoiced=0.15)
        states, J = R.solve(c, lag, **kw)
        assert J == pytest.approx(R.brute(c, lag, **kw), rel=1e-14, abs=1e-15)
        assert R.score(states, c, lag, **kw) == pytest.approx(J, rel=1e-14)
        assert ((states >= 0) & (states <= N)).all()


# --------------------------------------- H2: the reference against the oracle
def _check_against_oracle(path, c, lag):
    t = path.tracker
    p, cost, vmax = path.reference(c, lag, return_vmax=True)
    Fb = c.shape[0]
    # six float32 roundings per state per frame at most, of magnitudes up to
    # Vmax, on the reference's path and on the optimum: derived, not measured
    bound = 2 * Fb * 6 * 2.0 ** -24 * vmax
    kw = _weights(path)
    _, J = R.solve(c, lag, **kw)
    mine = R.score(R.states_of(p.lag, t.tau_min, t.tau_max), c, lag, **kw)
    print('F %d N %d: J* %.9g, path %.9g, cost %.9g, Vmax %.3g, bound %.3g'
          % (Fb, t.tau_max - t.tau_min, J, mine, cost, vmax, bound))
    assert cost.dtype == np.float64 and p.cmnd is None
    assert p.f0.dtype == np.float32 and p.aper.dtype == np.float32 and \
        p.lag.dtype == np.int32
    assert mine <= J + bound
    assert abs(float(cost) - J) <= bound
    # the outputs are the path's: lag 0 <-> f0 0 and aper 1, else c' at the lag
    un = p.lag == 0
    assert (p.f0[un] == 0).all() and (p.aper[un] == 1).all()
    assert ((p.lag[~un] >= t.tau_min) & (p.lag[~un] < t.tau_max)).all()
    assert np.array_equal(p.aper[~un], c[np.nonzero(~un)[0], p.lag[~un]])
    return p


@pytest.mark.parametrize('tau_min,tau_max,F', [(2, 4, 9), (2, 7, 30),
                                               (5, 70, 40), (32, 267, 25),
                                               (2, 1024, 6)])
def test_reference_is_the_oracle_on_random_rows(monkeypatch, tau_min, tau_max,
                                                F):
    _no_library(monkeypatch)
    path = _path(tau_min, tau_max)
    for seed in (1, 2):
        c, lag = R.random_rows(seed, F, tau_max, silent=0.25)
        assert (lag == 0).any() and (lag != 0).any()
        _check_against_oracle(path, c, lag)


@pytest.fixture(scope='module')
def tracked():
    """name -> the default tracker's float32 reference on each test signal,
    computed once and left unchanged."""
    from wavenet import pitch
    t = pitch.PitchTracker(16000)
    sig = {'tone': R.harmonic_tone(200.0), 'glide': R.glide(),
           'noise': R.noise(), 'octave': R.octave_signal()}
    return {k: t.reference(x, np.float32) for k, x in sig.items()}


@pytest.mark.parametrize('name', ['tone', 'glide', 'noise', 'octave'])
def test_reference_is_the_oracle_on_tracked_signals(tracked, name):
    raw = tracked[name]
    _check_against_oracle(_path(), raw.cmnd, raw.lag)


# ----------------------------------------------------------------- H3: ties
def _sequential(path, c, lag):
    """The tie rules one state after the other, in float32 scalars: the
    states [F] of the path (N: unvoiced)."""
    f32 = np.float32
    t = path.tracker
    tmin, N = t.tau_min, t.tau_max - t.tau_min
    pen, bias = path.tables()
    sw, unv = f32(path.switch), f32(path.unvoiced)
    V, U, pred = None, None, []
    for f in range(c.shape[0]):
        loc = [f32(c[f, tmin + s]) + bias[tmin + s] for s in range(N)]
        lu = f32(0) if lag[f] == 0 else unv
        row = [N] * (N + 1)
        if f == 0:
            nV, nU = loc, lu
        else:
            nV = []
            for s in range(N):
                ma, ia = None, 0
                for k in range(0, s + 1):           # the first minimum below
                    a = V[k] - pen[tmin + k]
                    if ma is None or a < ma:
                        ma, ia = a, k
                mb, ib = None, 0
                for k in range(s, N):               # the first minimum above
                    b = V[k] + pen[tmin + k]
                    if mb is None or b < mb:
                        mb, ib = b, k
                L, Rr = ma + pen[tmin + s], mb - pen[tmin + s]
                vv, pr = (L, ia) if L <= Rr else (Rr, ib)
                fu = U + sw
                pv, pr = (vv, pr) if vv <= fu else (fu, N)
                nV.append(pv + loc[s])
                row[s] = pr
            kb = 0
            for k in range(1, N):
                if V[k] < V[kb]:
                    kb = k
            fv = V[kb] + sw
            if U <= fv:
                nU, row[N] = U + lu, N
            else:
                nU, row[N] = fv + lu, kb
        m = nU
        for v in nV:
            if v < m:
                m = v
        V, U = [v - m for v in nV], nU - m
        pred.append(row)
    kb = 0
    for k in range(1, N):
        if V[k] < V[kb]:
            kb = k
    st = N if U <= V[kb] else kb
    states = []
    for f in range(c.shape[0] - 1, -1, -1):
        states.append(st)
        st = pred[f][st]
    return np.array(states[::-1])


TIE_WEIGHTS = [dict(jump=0.0),
               dict(jump=0.0, octave_bias=0.0, switch=0.25, unvoiced=0.25),
               dict(jump=0.0, octave_bias=0.0, switch=0.0, unvoiced=0.5)]


@pytest.mark.parametrize('kw', TIE_WEIGHTS, ids=('bias', 'quarters', 'free'))
@pytest.mark.parametrize('tau_min,tau_max,F', [(2, 5, 12), (2, 11, 14),
                                               (4, 40, 10)])
def test_ties_follow_the_rule(monkeypatch, tau_min, tau_max, F, kw):
    _no_library(monkeypatch)
    path = _path(tau_min, tau_max, **kw)
    assert not path.tables()[0].any()
    for seed in (3, 4, 5):
        c, lag = R.random_rows(seed, F, tau_max, silent=0.3, quantum=0.25)
        want = _sequential(path, c, lag)
        got = R.states_of(path.reference(c, lag)[0].lag, tau_min, tau_max)
        assert np.array_equal(got, want), seed
    if not path.octave_bias:
        # (the inputs do tie: some frame has two equal minima)
        loc = c[:, tau_min:tau_max]
        assert ((loc == loc.min(1, keepdims=True)).sum(1) > 1).any()


# ----------------------------------------------------- H4: the octave case
def test_octave_slips_leave_the_path(tracked):
    raw = tracked['octave']
    up = (raw.lag > 0) & (raw.lag < 120)
    print('raw track: %d frames an octave up, lags %s'
          % (up.sum(), sorted(set(raw.lag[up].tolist()))))
    assert up.sum() >= 10
    p, _ = _path().reference(raw.cmnd, raw.lag)
    assert not ((p.lag > 0) & (p.lag < 120)).any()
    voiced = p.f0 > 0
    assert voiced.sum() >= 40
    assert np.array_equal(voiced, p.lag > 0)
    assert (np.abs(p.lag[voiced] - 160) <= 1).all()


# ------------------------------------------------------- H5: a steady tone
def test_steady_tone_keeps_the_raw_lags(tracked):
    raw = tracked['tone']
    voiced = raw.f0 > 0
    assert voiced.sum() >= 50
    p, _ = _path().reference(raw.cmnd, raw.lag)
    assert np.array_equal(p.lag[voiced], raw.lag[voiced])
    assert np.array_equal(p.f0[voiced], raw.f0[voiced])
    assert np.array_equal(p.aper[voiced], raw.aper[voiced])


# ------------------------------------- H6: arguments, settings and tables
BAD = [dict(jump=-0.1), dict(jump=float('nan')), dict(jump=float('inf')),
       dict(jump='0.3'), dict(jump=True), dict(jump=1e60),
       dict(octave_bias=-1e-9), dict(octave_bias=None),
       dict(switch=-0.2), dict(switch=float('nan')),
       dict(unvoiced=0.0), dict(unvoiced=-0.15), dict(unvoiced=1e-60),
       dict(unvoiced=float('inf')), dict(unvoiced='x'),
       dict(max_bytes=0), dict(max_bytes=1.5), dict(max_bytes=True)]


@pytest.mark.parametrize('kw', BAD, ids=lambda kw: ','.join(
    '%s=%r' % kv for kv in kw.items()))
def test_bad_weights_raise_before_the_library(monkeypatch, kw):
    _no_library(monkeypatch)
    from wavenet import pitch
    with pytest.raises(ValueError):
        pitch.PitchPath(pitch.PitchTracker(16000), **kw)


def test_bad_tracker_and_inputs_raise_before_the_library(monkeypatch):
    _no_library(monkeypatch)
    import torch
    from wavenet import pitch
    for bad in (None, 16000, dict(sample_rate=16000)):
        with pytest.raises(ValueError):
            pitch.PitchPath(bad)
    path = _path()
    for audio, lengths in ((np.zeros((2, 100), np.int16), None),
                           (np.zeros((2, 3, 4), np.float32), None),
                           (np.zeros((0, 4), np.float32), None),
                           (np.zeros((2, 100), np.float32), [100]),
                           (np.zeros((2, 100), np.float32), [0, 100])):
        with pytest.raises(ValueError):
            path(audio, lengths)
    # one clip above max_bytes: both sizes are named
    small = _path(max_bytes=1000)
    with pytest.raises(ValueError) as e:
        small(np.zeros((2, 2560), np.float32))
    need = small.clip_bytes(10)
    assert need == 10 * (4 * 268 + 2 * 236)
    assert str(need) in str(e.value) and '1000' in str(e.value)
    # decode: shapes, dtypes and the device, before the library
    c = torch.zeros(2, 5, 268)
    lag = torch.zeros(2, 5, dtype=torch.int32)
    for args in ((c[..., :267], lag), (c.double(), lag), (c, lag.long()),
                 (c, lag[:, :4]), (c.numpy(), lag), (c, lag, [5]),
                 (c, lag, [5, 6]), (c, lag, [-1, 5]), (c, lag, [1.0, 2.0]),
                 (c, lag)):                     # (the last: not on a device)
        with pytest.raises(ValueError):
            path.decode(*args)
    with pytest.raises(ValueError):
        path.reference(np.zeros((5, 267), np.float32), np.zeros(5, np.int32))


def test_defaults_and_settings_round_trip(monkeypatch):
    _no_library(monkeypatch)
    from wavenet import pitch
    path = _path()
    assert (path.jump, path.octave_bias, path.switch, path.unvoiced,
            path.max_bytes) == (0.3, 0.05, 0.2, 0.15, 1 << 30)
    assert path.unvoiced == path.tracker.threshold and path.hop == 256
    assert 2 * path.switch + path.unvoiced >= path.jump
    assert path.last_cost is None
    t = pitch.PitchTracker(22050.0, hop=300, fmin=70.3, fmax=412.7,
                           window=576, threshold=0.1 + 0.2, silence=3e-9)
    for p in (path, pitch.PitchPath(t, jump=0.7, octave_bias=0.0, switch=1,
                                    unvoiced=0.25, max_bytes=12345678)):
        d = p.settings()
        assert set(d) == {'tracker', 'jump', 'octave_bias', 'switch',
                          'unvoiced', 'max_bytes'}
        assert d['tracker'] == p.tracker.settings()
        q = pitch.PitchPath.from_settings(d)
        assert q.settings() == d
        assert all(np.array_equal(a, b)
                   for a, b in zip(q.tables(), p.tables()))
    assert pitch.PitchPath(t).unvoiced == t.threshold
    with pytest.raises(ValueError):
        pitch.PitchPath.from_settings({'jump': 0.3})


@pytest.mark.parametrize('tau_min,tau_max', [(2, 4), (32, 267), (2, 1024),
                                             (7, 333)])
def test_tables(monkeypatch, tau_min, tau_max):
    """Made in float64, rounded once: within half a float32 ulp of the
    product computed here with math.log2."""
    _no_library(monkeypatch)
    path = _path(tau_min, tau_max, jump=0.37, octave_bias=0.061)
    pen, bias = path.tables()
    assert pen.dtype == bias.dtype == np.float32
    assert pen.shape == bias.shape == (tau_max + 1,)
    assert pen[0] == 0 and pen[1] == 0 and bias[tau_min] == 0
    assert (np.diff(pen[1:]) > 0).all() and (bias[tau_min + 1:] > 0).all()
    half = 2.0 ** -24 * (1 + 1e-9)
    for k in range(1, tau_max + 1):
        want = 0.37 * math.log2(k)
        assert abs(float(pen[k]) - want) <= half * want + 1e-45
        want = 0.061 * (math.log2(k) - math.log2(tau_min))
        assert abs(float(bias[k]) - want) <= half * abs(want) + 1e-16


# ------------------------------------------------------------ command line
def _error_of(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'evaluate.py')] +
                       argv, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stderr.decode()


def test_evaluate_path_flags_need_their_switches():
    code, err = _error_of(['ckpt', '--data_dir', 'in', '--synthesis', 'true',
                           '--pitch_path', 'true'])
    assert code == 2 and '--pitch_path needs --synthesis_pitch true' in err
    code, err = _error_of(['ckpt', '--data_dir', 'in', '--synthesis', 'true',
                           '--synthesis_pitch', 'true', '--pitch_jump', '0.5'])
    assert code == 2 and '--pitch_jump needs --pitch_path true' in err


def test_evaluate_builds_the_path(monkeypatch):
    _no_library(monkeypatch)
    import argparse
    import evaluate
    from wavenet import features, pitch
    spec = features.MelSpec(16000, n_fft=64, hop=16, n_mels=8)
    ns = dict(pitch_fmin=None, pitch_fmax=None, pitch_path=None,
              pitch_jump=None, pitch_octave_bias=None, pitch_switch=None)
    t = evaluate._pitch_tracker(argparse.Namespace(**ns), spec)
    assert isinstance(t, pitch.PitchTracker)
    p = evaluate._pitch_tracker(
        argparse.Namespace(**dict(ns, pitch_path=True)), spec)
    assert isinstance(p, pitch.PitchPath) and p.hop == 16
    assert (p.jump, p.octave_bias, p.switch) == (0.3, 0.05, 0.2)
    assert p.tracker.settings() == t.settings()
    p = evaluate._pitch_tracker(
        argparse.Namespace(**dict(ns, pitch_path=True, pitch_jump=0.5,
                                  pitch_octave_bias=0.0, pitch_switch=0.3,
                                  pitch_fmin=100.0)), spec)
    assert (p.jump, p.octave_bias, p.switch, p.tracker.fmin) == \
        (0.5, 0.0, 0.3, 100.0)
    with pytest.raises(ValueError):
        evaluate._pitch_tracker(
            argparse.Namespace(**dict(ns, pitch_path=True, pitch_jump=-1.0)),
            spec)


# ---------------------------------------------------- H7, H8: the ABI
def _declarations(header):
    src = open(os.path.join(ROOT, 'include', header)).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    return {m.group(1): [' '.join(p.split()) for p in m.group(2).split(',')]
            for m in re.finditer(
                r'\b(?:int|long)\s+(wn_\w+)\s*\(([^)]*)\)\s*;', src)}


def test_binding_table_matches_its_header():
    """Every declaration of wavenet_pitch_path.h is bound with as many
    arguments as it declares and nothing else is; none of them is declared in
    the other two headers or bound in the other two tables."""
    from wavenet import _lib
    decl = _declarations(HEADER)
    assert set(decl) == {'wn_pitch_path_workspace_bytes', 'wn_pitch_path'}
    assert {k: len(v) for k, v in decl.items()} == \
        {k: len(v[1]) for k, v in _lib.PITCH_PATH_SIGNATURES.items()}
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float}
    for name, params in decl.items():
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.PITCH_PATH_SIGNATURES[name][1] == want, name
    assert _lib.PITCH_PATH_SIGNATURES['wn_pitch_path'][0] is _lib.c_int
    assert _lib.PITCH_PATH_SIGNATURES['wn_pitch_path_workspace_bytes'][0] \
        is _lib.c_long
    for other in ('wavenet_hip.h', 'wavenet_pitch.h'):
        src = open(os.path.join(ROOT, 'include', other)).read()
        assert not any(re.search(r'\b%s\b' % k, src) for k in decl), other
    assert not set(decl) & (set(_lib.SIGNATURES) | set(_lib.PITCH_SIGNATURES))


def test_every_writing_entry_of_the_path_header_is_guarded():
    import test_gpu_guard_pitch_path as tgp
    w = {k: [p for p in v if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_pitch_path': ['void* workspace', 'float* f0',
                                   'float* aper', 'int32_t* lag',
                                   'double* cost']}
    assert set(tgp.ENTRIES) == set(w)


def test_workspace_bytes_and_entry_checks_without_a_device(hip_lib):
    """wn_pitch_path_workspace_bytes is the header's formula; wn_pitch_path
    refuses every bad argument before any launch (no device is needed to be
    refused)."""
    ws = hip_lib.wn_pitch_path_workspace_bytes
    assert ws(1, 1, 2, 4) == 2 * 3
    assert ws(8, 625, 32, 267) == 2 * 8 * 625 * 236
    assert ws(65535, 1 << 20, 2, 1024) == 2 * 65535 * (1 << 20) * 1023
    for args in ((0, 1, 2, 4), (65536, 1, 2, 4), (1, 0, 2, 4),
                 (1, (1 << 20) + 1, 2, 4), (1, 1, 1, 4), (1, 1, 2, 3),
                 (1, 1, 2, 1025), (1, 1, 1023, 1024)):
        assert ws(*args) == -1, args
    good = dict(cmnd=256, lag_in=512, nframes=0, B=1, F=4, tau_min=32,
                tau_max=267, pen=768, bias=1024, switch_cost=0.2,
                unvoiced_cost=0.15, sample_rate=16000.0, workspace=1280,
                f0=1536, aper=1792, lag=2048, cost=2304, stream=0)
    order = list(good)
    pointers = ('cmnd', 'lag_in', 'nframes', 'pen', 'bias', 'workspace', 'f0',
                'aper', 'lag', 'cost', 'stream')

    def code(**kw):
        a = dict(good, **kw)
        return hip_lib.wn_pitch_path(*[a[k] or None if k in pointers
                                       else a[k] for k in order])
    for name in pointers:
        if name not in ('nframes', 'stream'):
            assert code(**{name: 0}) == -5, name
    for kw in (dict(B=0), dict(B=65536), dict(F=0), dict(F=(1 << 20) + 1),
               dict(tau_min=1), dict(tau_min=266), dict(tau_max=1025),
               dict(tau_max=33)):
        assert code(**kw) == -1, kw
    for name in pointers[:-1]:
        off = 4098 if name != 'workspace' else 4097
        assert code(**{name: off}) == -3, name
    assert code(cost=2308) == -3
