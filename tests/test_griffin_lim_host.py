"""The Griffin-Lim baseline without a device (wavenet/griffin_lim.py, include/
wavenet_griffin_lim.h): the float64 restatement of tests/gl_ref.py against
torch.stft and its own inverse (H1), where the windows' squares vanish (H2),
the loop's convergence in float64 (H3), mel inversion (H4), the package's numpy
float32 rule against the restatement within the device's bounds and the phase
draw bit for bit (H5), settings, limits and refusals before the library (H6),
Normalizer.invert (H7), the binding table against the header and the coverage
of its writing entries by tests/test_gpu_guard_griffin_lim.py (H8), the
entries' own checks (H9)."""
import os
import re

import numpy as np
import pytest
import torch

import gl_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = 'wavenet_griffin_lim.h'
OTHERS = ('wavenet_hip.h', 'wavenet_pitch.h', 'wavenet_pitch_path.h',
          'wavenet_lc_frames.h', 'wavenet_spectral.h')
# (n_fft, hop, win_length, T)
GRIDS = [(64, 16, 64, 257), (128, 25, 100, 700), (64, 64, 64, 640),
         (1024, 256, 1024, 3000), (256, 64, 256, 2049), (64, 64, 64, 130),
         (128, 100, 100, 1001), (192, 1, 64, 70), (2048, 512, 1200, 3000)]
SMALL = ('ragged', 'oddhop', 'nooverlap', 'tile33')


def _gl(res, n_mels=20, **kw):
    from wavenet import features, griffin_lim
    spec = features.MelSpec(R.RUN_RATE, n_fft=res[0], hop=res[1],
                            n_mels=n_mels, win_length=res[2])
    return griffin_lim.GriffinLim(spec, **kw)


# ------------------------------------------------ H1: the restatement itself
@pytest.mark.parametrize('n_fft,hop,win,T', GRIDS)
def test_oracle_stft_is_torch_stft_on_padded_signals(n_fft, hop, win, T):
    x = R.signal(T, T)
    buf, s0 = R.padded(x, n_fft, hop)
    F = R.num_frames(T, hop)
    seg = torch.from_numpy(buf[s0:s0 + (F - 1) * hop + n_fft])
    want = torch.stft(seg, n_fft, hop_length=hop, win_length=n_fft,
                      window=torch.from_numpy(R.hann(n_fft, win)),
                      center=False, return_complex=True).numpy().T
    got = R.stft(x, n_fft, hop, win)
    assert got.shape == want.shape == (F, n_fft // 2 + 1)
    assert np.abs(got - want).max() <= 1e-10


@pytest.mark.parametrize('n_fft,hop,win,T', GRIDS)
def test_oracle_inverse_returns_the_signal(n_fft, hop, win, T):
    x = R.signal(T + 1, T)
    back = R.istft(R.stft(x, n_fft, hop, win), T, n_fft, hop, win)
    ok = R.window_square_sum(T, n_fft, hop, win) > R.DEN_FLOOR
    assert np.abs(back - x)[ok].max() <= 1e-12
    assert (back[~ok] == 0).all()


# ---------------------------------- H2: where the windows' squares vanish
@pytest.mark.parametrize('n_fft,hop,win,T', GRIDS)
def test_vanishing_denominators_are_the_multiples_of_hop(n_fft, hop, win, T):
    den = R.window_square_sum(T, n_fft, hop, win)
    bad = np.nonzero(den <= R.DEN_FLOOR)[0]
    if hop == win:
        # the periodic Hann's zero is every frame's first sample
        assert bad.tolist() == list(range(0, T, hop))
    else:
        assert bad.size == 0
    if hop == win == n_fft and T % hop == 0:
        # the share the device tests compare on: 33 of 64
        assert (den >= 0.25 * den.max()).mean() >= 0.5


# -------------------------------------------------- H3: the loop in float64
@pytest.mark.parametrize('res', [(256, 64, 256), (512, 128, 512),
                                 (128, 25, 100)])
def test_oracle_trace_falls_without_momentum(res):
    x = R.signal(7, 4000)
    A = np.abs(R.stft(x, *res))
    plain = R.ratio(R.griffin_lim(A, 4000, res, 32, 0.0)[1])
    fast = R.ratio(R.griffin_lim(A, 4000, res, 32, 0.99)[1])
    print(res, plain[0], plain[8], plain[-1], fast[-1])
    assert plain.shape == (33,)
    assert (np.diff(plain) <= 0).all()
    assert plain[0] > 0.5 and plain[-1] < 0.25 and plain[-1] < plain[8]
    assert fast[-1] < plain[-1]


# ------------------------------------------------------ H4: mel inversion
@pytest.mark.parametrize('n_mels', [1, 33, 80, 128])
def test_pinv_returns_a_power_spectrum_of_the_row_space(n_mels):
    melw = R.filterbank(R.RUN_RATE, 1024, n_mels)
    rng = np.random.default_rng(n_mels)
    P = melw.T @ rng.uniform(0.5, 2.0, (n_mels, 6))        # [n_bins, 6] >= 0
    frames = np.log(melw @ P).T
    A = R.magnitude(frames, melw)
    assert np.abs(A * A - P.T).max() <= 1e-9 * P.max()


def test_pinv_and_clip_is_not_an_exact_inverse():
    """What the README says: mel(A^2) is not the mel spectrum that went in."""
    melw = R.filterbank(R.RUN_RATE, 256, 40)
    S = R.stft(R.signal(3, 2000), 256, 64, 256)
    M = (np.abs(S) ** 2) @ melw.T
    A = R.magnitude(np.log(M), melw)
    assert np.abs((A * A) @ melw.T - M).max() > 1e-6 * M.max()


# ------------------------------ H5: the package's numpy rule, the phase draw
def _clip(name, b=0):
    n = R.SHAPES[name][4][b]
    return R.make_audio(name)[b, :n].astype(np.float64), n


@pytest.mark.parametrize('name', SMALL)
def test_reference_primitives_against_the_restatement(name):
    res = R.SHAPES[name][:3]
    gl = _gl(res)
    for b in range(len(R.SHAPES[name][4])):
        x, n = _clip(name, b)
        S = R.stft(x, *res)
        re, im = gl.reference_stft(x)
        tol = R.TOL_FACTOR * R.yardstick(
            S, [R.stft_f32(x, *res, o) for o in ('matmul', 'sequential')])
        assert np.abs(re + 1j * im - S).max() <= tol
        assert (im[:, 0] == 0).all() and (im[:, -1] == 0).all()
        Sx = R.make_spectrum(name)[b, :R.num_frames(n, res[1])]
        want = R.istft(Sx, n, *res)
        den = R.window_square_sum(n, *res)
        keep = den >= 0.25 * den.max()
        tol = R.TOL_FACTOR * R.yardstick(
            want[keep], [R.istft_f32(Sx, n, *res, o)[keep]
                         for o in ('matmul', 'sequential')])
        got = gl.reference_istft(Sx.real, Sx.imag, n)
        assert np.abs(got - want)[keep].max() <= tol
        assert np.isfinite(got).all() and (got[den <= R.DEN_FLOOR] == 0).all()


@pytest.mark.parametrize('n_mels', [1, 33, 80, 128])
def test_reference_magnitude_against_the_restatement(n_mels):
    gl = _gl((256, 64, 256), n_mels)
    melw = R.filterbank(R.RUN_RATE, 256, n_mels)
    assert np.abs(gl.spec.melw64 - melw).max() <= 1e-12
    frames = R.logmel_frames(n_mels, 1, 9, n_mels)[0]
    want = R.magnitude(frames, melw)
    tol = R.TOL_FACTOR * R.yardstick(
        want, [R.magnitude_f32(frames, melw, o)
               for o in ('matmul', 'sequential')])
    assert np.abs(gl.reference_magnitude(frames) - want).max() <= tol


def test_reference_project_against_the_restatement():
    name = 'tile33'
    res = R.SHAPES[name][:3]
    gl = _gl(res, momentum=0.5)
    x, n = _clip(name, 1)
    rng = np.random.default_rng(5)
    S = R.stft(x, *res)
    A = rng.uniform(0.1, 2.0, S.shape).astype(np.float32)
    tp = R.make_spectrum(name)[1, :S.shape[0]]
    t, c, tr = R.project(S, A.astype(np.float64), tp.astype(np.complex128),
                         0.5)
    (tre, tim), (cre, cim), gtr = gl.reference_project(x, A, tp.real, tp.imag)
    keep = np.abs(S) >= 1e-3 * np.abs(S).max()
    assert keep.mean() >= 0.95
    rest = [R.project_f32(x, A, tp, 0.5, res, o)
            for o in ('matmul', 'sequential')]
    for got, want, k in ((tre + 1j * tim, t, 0), (cre + 1j * cim, c, 1)):
        tol = R.TOL_FACTOR * R.yardstick(want[keep], [r[k][keep] for r in rest])
        assert np.abs(got - want)[keep].max() <= tol
    assert gtr[0] == pytest.approx(tr[0], rel=1e-5)
    assert gtr[1] == pytest.approx(tr[1], rel=1e-6)


@pytest.mark.parametrize('seed,key', [(0, 0), (12345, 3), (2 ** 64 - 1, 2 ** 24 - 1)])
def test_phase_draw_is_the_python_integer_restatement(seed, key):
    from wavenet import griffin_lim
    F, nb = 5, 33
    p = griffin_lim.phase_indices(seed, key, F, nb)
    want = [[R.phase_index(seed, key, f, k, nb) for k in range(nb)]
            for f in range(F)]
    assert p.tolist() == want
    assert (p[:, 0] == 0).all() and (p[:, -1] == 0).all()
    assert len(set(p[:, 1:-1].reshape(-1).tolist())) > 50
    assert (griffin_lim.phase_indices(seed, key, F, nb, 'zero') == 0).all()
    # the table and the one float32 multiply per component
    gl = _gl((64, 16, 64), seed=seed)
    A = np.random.default_rng(1).uniform(0, 2, (F, nb)).astype(np.float32)
    re, im = gl.reference_initial(A, key)
    c = R.initial(A.astype(np.float64), seed, key)
    tab = griffin_lim.phase_table()
    assert tab.dtype == np.float32 and tab.shape == (1024, 2)
    assert np.abs(re - c.real).max() <= 2 * R.ULP32 * 2
    assert np.abs(im - c.imag).max() <= 2 * R.ULP32 * 2
    assert (im[:, 0] == 0).all() and np.array_equal(re[:, 0], A[:, 0])


def test_reference_loop_against_the_restatement():
    """One iteration (the trajectories part after a few) within 4 x the
    float32 loops' own error; iterations = 0 is istft(init)."""
    res, n = (64, 16, 64), 300
    melw = R.filterbank(R.RUN_RATE, 64, 12)
    S = R.stft(R.signal(2, n), *res)
    frames = np.log(np.maximum((np.abs(S) ** 2) @ melw.T, 1e-10)) \
        .astype(np.float32)
    gl = _gl(res, 12, iterations=1, momentum=0.5, seed=9)
    A32 = gl.reference_magnitude(frames).astype(np.float64)
    want, wtr = R.griffin_lim(A32, n, res, 1, 0.5, seed=9, key=4)
    rest = [R.griffin_lim_f32(A32, n, res, 1, 0.5, seed=9, key=4, order=o)[0]
            for o in ('matmul', 'sequential')]
    got, gtr = gl.reference(frames, n, key=4, return_trace=True)
    assert got.dtype == np.float32 and got.shape == (n,)
    assert np.abs(got - want).max() <= R.TOL_FACTOR * R.yardstick(want, rest)
    assert gtr.shape == (2, 2)
    assert np.allclose(gtr, wtr, rtol=1e-4)
    gl0 = _gl(res, 12, iterations=0, seed=9)
    re, im = gl0.reference_initial(gl0.reference_magnitude(frames), 4)
    assert np.array_equal(gl0.reference(frames, n, key=4),
                          gl0.reference_istft(re, im, n))
    with pytest.raises(ValueError, match='frames'):
        gl.reference(frames[:3], n)


# ------------------------------------- H6: settings, limits and refusals
def test_settings_round_trip():
    from wavenet import griffin_lim
    gl = _gl((128, 25, 100), 33, iterations=5, momentum=0.25, seed=77,
             init='zero', max_bytes=12345)
    d = gl.settings()
    assert d['spec']['n_fft'] == 128 and 'normalizer' not in d['spec']
    back = griffin_lim.GriffinLim.from_settings(d)
    assert back.settings() == d
    assert np.array_equal(back.pinv, gl.pinv)
    for bad in (None, {}, dict(d, extra=1), dict(d, spec=3)):
        with pytest.raises(ValueError, match='settings'):
            griffin_lim.GriffinLim.from_settings(bad)
    assert gl.pinv.shape == (65, 33) and gl.pinv.dtype == np.float32
    assert gl.bytes_per_clip(10) == 10 * (65 * 20 + 128 * 4)


@pytest.mark.parametrize('kw,match', [
    (dict(iterations=-1), 'iterations'), (dict(iterations=4097), 'iterations'),
    (dict(iterations=2.0), 'iterations'), (dict(iterations=True), 'iterations'),
    (dict(momentum=1.0), 'momentum'), (dict(momentum=-0.1), 'momentum'),
    (dict(momentum=float('nan')), 'momentum'), (dict(momentum='a'), 'momentum'),
    (dict(momentum=1 - 1e-9), 'momentum'),
    (dict(seed=-1), 'seed'), (dict(seed=2 ** 64), 'seed'), (dict(seed=0.5), 'seed'),
    (dict(init='phase_gradient'), 'init'), (dict(max_bytes=0), 'max_bytes'),
    (dict(max_bytes=1.5), 'max_bytes')])
def test_constructor_refusals(kw, match):
    with pytest.raises(ValueError, match=match):
        _gl((64, 16, 64), **kw)


def test_constructor_wants_a_melspec_and_takes_the_limits():
    from wavenet import frontend, griffin_lim
    with pytest.raises(ValueError, match='MelSpec'):
        griffin_lim.GriffinLim(dict(n_fft=64))
    _gl((64, 16, 64), iterations=0, momentum=0.0)
    _gl((2048, 1, 2048), 128, iterations=4096, seed=2 ** 64 - 1)
    with pytest.raises(ValueError, match=r'\.mel'):
        griffin_lim.GriffinLim(object.__new__(frontend.MelPitchSpec))


def test_calls_refuse_before_the_library(monkeypatch):
    from wavenet import _lib
    gl = _gl((64, 16, 64), 12)

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'load', boom)
    monkeypatch.setattr(_lib, 'require_gpu', boom)
    fr = np.zeros((2, 5, 12), np.float32)
    for call, match in [
            (lambda: gl(fr.astype(np.float64)), 'float32'),
            (lambda: gl(fr[:, :, :11]), 'float32'),
            (lambda: gl(fr, lengths=[81, 1]), 'lengths'),
            (lambda: gl(fr, lengths=[1.0, 2.0]), 'lengths'),
            (lambda: gl(fr, nframes=[6, 1]), 'nframes'),
            (lambda: gl(fr, lengths=[80, 17], nframes=[5, 1]), 'ceil'),
            (lambda: gl(fr, keys=[0]), 'keys'),
            (lambda: gl(fr, keys=[0, 2 ** 24]), 'keys'),
            (lambda: gl(fr, keys=[0, -1]), 'keys'),
            (lambda: gl.magnitude(fr, nframes=[1]), 'nframes'),
            (lambda: gl.magnitude(np.zeros((5, 13), np.float32)), 'float32'),
            (lambda: gl.stft(np.zeros((2, 0), np.float32)), 'shape'),
            (lambda: gl.stft(np.zeros((2, 9), np.int32)), 'float'),
            (lambda: gl.stft(np.zeros((2, 9), np.float32), [10, 1]), 'lengths'),
            (lambda: gl.istft(np.zeros((2, 5, 33), np.float32)), 'complex'),
            (lambda: gl.istft(np.zeros((2, 5, 32), np.complex64)), '33'),
            (lambda: gl.istft(np.zeros((5, 33), np.complex64), [81]), 'lengths'),
    ]:
        with pytest.raises(ValueError, match=match):
            call()
    small = _gl((64, 16, 64), 12, max_bytes=1000)
    with pytest.raises(ValueError) as e:
        small(fr)
    assert str(small.bytes_per_clip(5)) in str(e.value) and '1000' in str(e.value)


# ------------------------------------------------- H7: Normalizer.invert
def test_normalizer_invert_undoes_what_was_not_clamped():
    from wavenet import features
    rng = np.random.default_rng(0)
    shift = rng.normal(-5, 1, 7).astype(np.float32)
    scale = rng.uniform(0.2, 3, 7).astype(np.float32)
    norm = features.Normalizer(shift, scale, -1.0, 1.0)
    x = rng.normal(-5, 1, (2, 6, 7)).astype(np.float32)
    v = norm.reference(x, nframes=[6, 4])
    back = norm.invert(torch.from_numpy(v), nframes=[6, 4])
    assert isinstance(back, torch.Tensor) and back.dtype == torch.float32
    want = (v / scale + shift).astype(np.float32)
    want[1, 4:] = 0
    assert np.array_equal(back.numpy(), want)
    inside = (np.abs((x - shift) * scale) < 1.0)
    inside[1, 4:] = False
    assert inside.any() and not inside[0].all()
    assert np.abs(back.numpy() - x)[inside].max() <= 1e-5
    # clamped values do not come back
    assert np.abs(back.numpy() - x)[0][~inside[0]].max() > 1e-3
    one = norm.invert(v[0])
    assert tuple(one.shape) == (6, 7)
    with pytest.raises(ValueError, match='nframes'):
        norm.invert(v, nframes=[7, 1])
    with pytest.raises(ValueError, match='float32'):
        norm.invert(v.astype(np.float64))


# -------------------------------------------------- H7b: the command lines
def _exits(fn, argv, capsys):
    with pytest.raises(SystemExit) as e:
        fn(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_evaluate_flags(capsys):
    import evaluate
    base = ['ckpt', '--data_dir', 'in']
    syn = base + ['--synthesis', 'true']
    err = _exits(evaluate.get_arguments,
                 base + ['--synthesis_baseline', 'griffin_lim'], capsys)
    assert '--synthesis_baseline needs --synthesis true' in err
    err = _exits(evaluate.get_arguments,
                 syn + ['--synthesis_baseline', 'world'], capsys)
    assert '--synthesis_baseline' in err
    for flag, value in (('--gl_iterations', '8'), ('--gl_momentum', '0.5')):
        err = _exits(evaluate.get_arguments, syn + [flag, value], capsys)
        assert '%s needs --synthesis_baseline griffin_lim' % flag in err
    gl = syn + ['--synthesis_baseline', 'griffin_lim']
    for bad in ('-1', '4097', '2.5', 'x', ''):
        err = _exits(evaluate.get_arguments, gl + ['--gl_iterations', bad],
                     capsys)
        assert '--gl_iterations' in err, bad
    for bad in ('1', '1.5', '-0.1', 'nan', 'x'):
        err = _exits(evaluate.get_arguments, gl + ['--gl_momentum', bad],
                     capsys)
        assert '--gl_momentum' in err, bad
    a = evaluate.get_arguments(gl)
    assert a.synthesis_baseline == 'griffin_lim'
    assert a.gl_iterations is None and a.gl_momentum is None
    a = evaluate.get_arguments(gl + ['--gl_iterations', '0', '--gl_momentum',
                                     '0'])
    assert a.gl_iterations == 0 and a.gl_momentum == 0.0
    a = evaluate.get_arguments(syn)
    assert a.synthesis_baseline is None
    assert 'synthesis_baseline' in evaluate.SYNTHESIS_FLAGS
    assert (evaluate.GL_ITERATIONS, evaluate.GL_MOMENTUM) == (32, 0.99)


def test_tool_flags(capsys):
    sys_path = os.path.join(ROOT, 'tools')
    import sys
    if sys_path not in sys.path:
        sys.path.insert(0, sys_path)
    import griffin_lim as tool
    flags = ['--sample_rate', '16000', '--lc_channels', '8', '--lc_hop', '16']
    err = _exits(tool.get_arguments, ['in.npy'] + flags, capsys)
    assert '--out' in err
    err = _exits(tool.get_arguments, ['in.txt', '--out', 'o.wav'] + flags,
                 capsys)
    assert '.npy' in err
    for k in range(3):
        part = flags[:2 * k] + flags[2 * k + 2:]
        err = _exits(tool.get_arguments, ['in.npy', '--out', 'o.wav'] + part,
                     capsys)
        assert '%s is required without --checkpoint' % flags[2 * k] in err
    ok = ['in.wav', '--out', 'o.wav'] + flags
    for flag, bad in (('--gl_iterations', '4097'), ('--gl_iterations', '-1'),
                      ('--gl_momentum', '1'), ('--gl_momentum', 'nan'),
                      ('--seed', '-1'), ('--lc_features', 'none')):
        err = _exits(tool.get_arguments, ok + [flag, bad], capsys)
        assert flag in err, (flag, bad)
    a = tool.get_arguments(ok + ['--lc_n_fft', '64'])
    assert (a.gl_iterations, a.gl_momentum, a.seed) == (32, 0.99, 0)
    assert a.lc_features == 'mel'
    spec = tool.front_end(a)
    assert (spec.n_fft, spec.hop, spec.n_mels) == (64, 16, 8)
    a = tool.get_arguments(['in.npy', '--out', 'o.wav', '--checkpoint', 'ck'])
    assert a.sample_rate is None and a.lc_features is None
    with pytest.raises(ValueError, match='names no front end'):
        tool.front_end(a)
    # an .npy of the wrong width is named, no device needed
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'f.npy')
        np.save(path, np.zeros((4, 9), np.float32))
        with pytest.raises(ValueError, match=r'frames \[F, 8\]'):
            tool.frames_of(spec, path)


@pytest.mark.parametrize('kind,channels', [('mel', 8), ('mel+f0', 10)])
@pytest.mark.parametrize('rng_flag', ['-30,10', '-9,-1'])
def test_tool_inverts_the_normaliser_of_an_npy(tmp_path, kind, channels,
                                               rng_flag):
    """An .npy of NORMALISED frames comes back as raw log-mel, for a mel and
    for a mel+f0 front end (whose .mel never carries the normaliser), within
    the clamp: what the range cut off returns as the range's edge.  Four
    float32 operations on values within 40 of each other: 4 * 40 * 2^-24."""
    import sys
    if os.path.join(ROOT, 'tools') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import griffin_lim as tool
    path = str(tmp_path / 'f.npy')
    a = tool.get_arguments([
        path, '--out', 'o.wav', '--sample_rate', '16000', '--lc_channels',
        str(channels), '--lc_hop', '16', '--lc_n_fft', '64', '--lc_features',
        kind, '--lc_normalize', 'range', '--lc_range', rng_flag])
    spec = tool.front_end(a)
    assert spec.channels == channels and spec.normalizer is not None
    lo, hi = (float(v) for v in rng_flag.split(','))
    raw = R.logmel_frames(channels, 1, 11, 8)[0]            # in [-12, 3]
    normed = np.zeros((11, channels), np.float32)
    normed[:, :8] = spec.normalizer.reference(raw)
    normed[:, 8:] = 0.5                                     # (F0, voicing)
    np.save(path, normed)
    frames, n = tool.frames_of(spec, path)
    assert n is None and tuple(frames.shape) == (11, 8)
    got = np.asarray(frames)
    clamped = (raw < lo) | (raw > hi)
    assert clamped.any() == (rng_flag == '-9,-1')
    assert np.abs(got - np.clip(raw, lo, hi)).max() <= 4 * 40 * 2.0 ** -24
    assert np.abs(got - normed[:, :8]).max() > 1.0          # (it was inverted)


# ---------------------------------------------------------- H8: the ABI
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
    assert set(decl) == {'wn_stft', 'wn_istft_scratch_bytes', 'wn_istft',
                         'wn_mel_to_magnitude', 'wn_gl_init',
                         'wn_gl_project_partials', 'wn_gl_project'}
    assert set(_lib.GRIFFIN_LIM_SIGNATURES) == set(decl)
    ctype = {'int': _lib.c_int, 'long': _lib.c_long, 'float': _lib.c_float,
             'double': _lib.c_double, 'uint64_t': _lib.c_u64}
    for name, (res, params) in decl.items():
        want = [_lib.P if '*' in p else ctype[p.split()[0]] for p in params]
        assert _lib.GRIFFIN_LIM_SIGNATURES[name] == (ctype[res], want), name
    for other in OTHERS:
        assert not set(decl) & set(_declarations(other)), other
    assert not set(decl) & (set(_lib.SIGNATURES) | set(_lib.PITCH_SIGNATURES)
                            | set(_lib.PITCH_PATH_SIGNATURES)
                            | set(_lib.LC_FRAMES_SIGNATURES)
                            | set(_lib.SPECTRAL_SIGNATURES))


def test_load_binds_the_table(hip_lib):
    from wavenet import _lib
    for name, (res, args) in _lib.GRIFFIN_LIM_SIGNATURES.items():
        fn = getattr(hip_lib, name)
        assert fn.restype is res and fn.argtypes == args, name


def test_every_writing_entry_of_the_header_is_guarded():
    import test_gpu_guard_griffin_lim as tg
    w = {k: [p for p in v[1] if '*' in p and not p.startswith('const ')
             and not re.search(r'\bstream$', p)]
         for k, v in _declarations(HEADER).items()}
    w = {k: v for k, v in w.items() if v}
    assert w == {'wn_stft': ['float* out'],
                 'wn_istft': ['float* scratch', 'float* x'],
                 'wn_mel_to_magnitude': ['float* out'],
                 'wn_gl_init': ['float* c0'],
                 'wn_gl_project': ['float* t_out', 'float* c_out',
                                   'double* trace', 'double* partials']}
    assert set(tg.ENTRIES) == set(w)


# ------------------------------------------ H9: the entries' own checks
OK, BAD_SHAPE, UNSUPPORTED, MISALIGNED, NULL = 0, -1, -2, -3, -5


def test_host_queries(hip_lib):
    assert hip_lib.wn_istft_scratch_bytes(3, 257, 64, 16) == 4 * 3 * 17 * 64
    assert hip_lib.wn_istft_scratch_bytes(65535, 2 ** 30, 2048, 1) == \
        4 * 65535 * 2 ** 30 * 2048
    for bad in ((0, 9, 64, 16), (65536, 9, 64, 16), (1, 0, 64, 16),
                (1, 2 ** 30 + 1, 64, 16), (1, 9, 32, 16), (1, 9, 96, 16),
                (1, 9, 2112, 16), (1, 9, 64, 0), (1, 9, 64, 65)):
        assert hip_lib.wn_istft_scratch_bytes(*bad) == -1, bad
    assert hip_lib.wn_gl_project_partials(3, 2049, 64) == 2 * 3 * 2
    assert hip_lib.wn_gl_project_partials(1, 2048, 64) == 2
    for bad in ((0, 9, 1), (65536, 9, 1), (1, 0, 1), (1, 2 ** 30 + 1, 1),
                (1, 9, 0)):
        assert hip_lib.wn_gl_project_partials(*bad) == -1, bad


def test_entries_refuse_before_any_launch(hip_lib):
    """Host addresses stand for device ones: every call here must return
    before it launches anything."""
    buf = np.zeros(512, np.float64)
    p = buf.ctypes.data
    p += (-p) % 16
    stft = lambda **k: hip_lib.wn_stft(*_args(
        dict(x=p, ld=100, B=1, T=100, n=p, w=p, b=p, N=64, hop=16, nb=33,
             out=p, s=None), k))
    assert stft(x=None) == NULL and stft(w=None) == NULL
    assert stft(b=None) == NULL and stft(out=None) == NULL
    for k in (dict(N=32), dict(N=96), dict(N=2112), dict(hop=0), dict(hop=65),
              dict(nb=32), dict(B=0), dict(B=65536), dict(T=0),
              dict(T=2 ** 30 + 1, ld=2 ** 30 + 1), dict(ld=99)):
        assert stft(**k) == BAD_SHAPE, k
    for k in (dict(x=p + 2), dict(n=p + 2), dict(w=p + 1), dict(b=p + 4),
              dict(out=p + 4)):
        assert stft(**k) == MISALIGNED, k

    istft = lambda **k: hip_lib.wn_istft(*_args(
        dict(sp=p, B=1, T=100, n=p, w=p, b=p, N=64, hop=16, nb=33, sc=p, x=p,
             ld=100, s=None), k))
    for k in ('sp', 'w', 'b', 'sc', 'x'):
        assert istft(**{k: None}) == NULL, k
    for k in (dict(N=0), dict(hop=65), dict(nb=34), dict(B=0), dict(T=0),
              dict(ld=99)):
        assert istft(**k) == BAD_SHAPE, k
    for k in (dict(sp=p + 4), dict(b=p + 8), dict(sc=p + 2), dict(x=p + 1)):
        assert istft(**k) == MISALIGNED, k

    mag = lambda **k: hip_lib.wn_mel_to_magnitude(*_args(
        dict(fr=p, B=1, F=4, C=20, nf=p, pinv=p, nb=33, out=p, s=None), k))
    for k in ('fr', 'pinv', 'out'):
        assert mag(**{k: None}) == NULL, k
    for k in (dict(C=0), dict(C=129), dict(nb=0), dict(nb=1026), dict(B=0),
              dict(B=65536), dict(F=0), dict(B=3, F=2 ** 30)):
        assert mag(**k) == BAD_SHAPE, k
    for k in (dict(fr=p + 2), dict(nf=p + 1), dict(pinv=p + 2), dict(out=p + 2)):
        assert mag(**k) == MISALIGNED, k

    init = lambda **k: hip_lib.wn_gl_init(*_args(
        dict(A=p, B=1, F=4, nb=33, keys=p, seed=1, mode=0, tab=p, c=p,
             s=None), k))
    for k in ('A', 'keys', 'tab', 'c'):
        assert init(**{k: None}) == NULL, k
    for k in (dict(nb=1), dict(nb=34), dict(nb=1057), dict(B=0), dict(F=0),
              dict(F=2 ** 31 - 1, nb=1025)):      # (f * n_bins + k >= 2^40)
        assert init(**k) == BAD_SHAPE, k
    assert init(mode=2) == UNSUPPORTED and init(mode=-1) == UNSUPPORTED
    for k in (dict(A=p + 2), dict(keys=p + 4), dict(tab=p + 4), dict(c=p + 4)):
        assert init(**k) == MISALIGNED, k

    q = p + 256
    proj = lambda **k: hip_lib.wn_gl_project(*_args(
        dict(x=p, ld=100, B=1, T=100, n=p, w=p, b=p, N=64, hop=16, nb=33,
             A=p + 1024, tp=p, alpha=0.5, t=p, c=q, tr=p, parts=p, s=None), k))
    for k in ('x', 'w', 'b', 'A', 'tp', 't', 'c', 'tr', 'parts'):
        assert proj(**{k: None}) == NULL, k       # (a trace needs partials)
    for k in (dict(N=96), dict(hop=0), dict(nb=32), dict(ld=99),
              dict(alpha=1.0), dict(alpha=-0.5), dict(alpha=float('nan')),
              dict(c=p), dict(c=p, t=q), dict(A=p), dict(A=q),
              dict(A=p + 512, t=p + 512)):
        assert proj(**k) == BAD_SHAPE, k          # (aliasing but t_out == t_prev)
    for k in (dict(tp=p + 4), dict(t=p + 4), dict(c=q + 4), dict(tr=p + 4),
              dict(parts=p + 4), dict(A=p + 1026)):
        assert proj(**k) == MISALIGNED, k


def _args(base, change):
    base.update(change)
    return list(base.values())
