"""The Griffin-Lim kernels (include/wavenet_griffin_lim.h, wavenet/
griffin_lim.py) on the device against the float64 restatement of
tests/gl_ref.py, at every shape of gl_ref.SHAPES -- tiny ragged clips on idle
waves, an odd hop with win_length < n_fft, no overlap, exactly 32 frames and a
33rd on a partial tile, more bin chunks than waves -- every output within 4 x
its case's yardstick (the larger of two float32 restatements' errors and one
float32 ulp of the output's scale, measured on the CPU when the test runs;
no figure comes from the device); exact zeros where the rule says zero; and
whole runs: a clip alone against the clip in a batch and under two groupings,
run to run, iterations = 0, a NaN frame, the trace without momentum, and the
final inconsistency against the float64 loop's."""
import functools

import numpy as np
import pytest
import torch

import gl_ref as R

pytestmark = pytest.mark.gpu

KINDS = ('matmul', 'sequential')


@functools.lru_cache(maxsize=None)
def _gl(res, n_mels=20, **kw):
    from wavenet import features, griffin_lim
    spec = features.MelSpec(R.RUN_RATE, n_fft=res[0], hop=res[1],
                            n_mels=n_mels, win_length=res[2])
    return griffin_lim.GriffinLim(spec, **dict(kw))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _keep(n, res):
    den = R.window_square_sum(n, *res)
    return den, den >= 0.25 * den.max()


# ------------------------------------------------------------------ wn_stft
@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_stft_against_the_restatement(hip_lib, name):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    res = (n_fft, hop, win)
    audio = R.make_audio(name).copy()
    for b, n in enumerate(lengths):
        audio[b, n:] = np.nan                 # nothing behind n[b] is read
    got = _gl(res).stft(audio, lengths).cpu().numpy()
    assert got.shape == (len(lengths), R.num_frames(T, hop), n_fft // 2 + 1)
    assert got.dtype == np.complex64
    for b, n in enumerate(lengths):
        x = audio[b, :n].astype(np.float64)
        want = R.stft(x, *res)
        Fb = want.shape[0]
        tol = R.TOL_FACTOR * R.yardstick(
            want, [R.stft_f32(x, *res, k) for k in KINDS])
        err = np.abs(got[b, :Fb] - want).max()
        print('%s clip %d: err %.3e bound %.3e' % (name, b, err, tol))
        assert err <= tol
        z = got[b].view(np.float32).view(np.int32).reshape(got.shape[1], -1, 2)
        assert (z[Fb:] == 0).all()                      # exact +0 frames
        assert (z[:, 0, 1] == 0).all() and (z[:, -1, 1] == 0).all()


def test_stft_without_lengths_is_full_lengths(hip_lib):
    res = R.SHAPES['tile33'][:3]
    audio = R.make_audio('tile33')
    a = _gl(res).stft(audio)
    b = _gl(res).stft(audio, [audio.shape[1]] * audio.shape[0])
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    one = _gl(res).stft(audio[1])
    assert torch.equal(torch.view_as_real(one), torch.view_as_real(a[1]))


# ----------------------------------------------------------------- wn_istft
@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_istft_of_an_inconsistent_spectrum(hip_lib, name):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    res = (n_fft, hop, win)
    S = R.make_spectrum(name).copy()
    for b, n in enumerate(lengths):
        S[b, R.num_frames(n, hop):] = np.nan            # not read
    got = _gl(res).istft(S, lengths).cpu().numpy()
    assert got.shape == (len(lengths), max(lengths))
    for b, n in enumerate(lengths):
        Sb = S[b, :R.num_frames(n, hop)]
        want = R.istft(Sb, n, *res)
        den, keep = _keep(n, res)
        if hop == win and n % hop == 0:
            assert keep.mean() >= 0.5
        elif hop < win:
            assert keep.all()
        tol = R.TOL_FACTOR * R.yardstick(
            want[keep], [R.istft_f32(Sb, n, *res, k)[keep] for k in KINDS])
        err = np.abs(got[b, :n] - want)[keep].max()
        print('%s clip %d: err %.3e bound %.3e' % (name, b, err, tol))
        assert err <= tol
        assert np.isfinite(got[b]).all()
        assert (got[b, :n][den <= R.DEN_FLOOR] == 0).all()
        assert (got[b, n:].view(np.int32) == 0).all()


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_device_round_trip_returns_the_signal(hip_lib, name):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    res = (n_fft, hop, win)
    gl = _gl(res)
    audio = R.make_audio(name)
    got = gl.istft(gl.stft(audio, lengths), lengths).cpu().numpy()
    for b, n in enumerate(lengths):
        x = audio[b, :n].astype(np.float64)
        den, keep = _keep(n, res)
        rest = [R.istft_f32(R.stft_f32(x, *res, k), n, *res, k)[keep]
                for k in KINDS]
        tol = R.TOL_FACTOR * R.yardstick(x[keep], rest)
        err = np.abs(got[b, :n] - x)[keep].max()
        print('%s clip %d: err %.3e bound %.3e' % (name, b, err, tol))
        assert err <= tol
        assert (got[b, :n][den <= R.DEN_FLOOR] == 0).all()


# ------------------------------------------------------------ wn_gl_project
@pytest.mark.parametrize('name', ['ragged', 'oddhop', 'tile33', 'r1024'])
def test_project_against_the_restatement(hip_lib, name):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    res, nb, B = (n_fft, hop, win), n_fft // 2 + 1, len(lengths)
    F = R.num_frames(T, hop)
    gl = _gl(res)
    alpha = 0.75
    audio = R.make_audio(name)
    rng = np.random.default_rng(R.SEEDS[name] + 7)
    A = rng.uniform(0.1, 2.0, (B, F, nb)).astype(np.float32)
    tp = R.make_spectrum(name).copy()
    for b, n in enumerate(lengths):                     # not read
        A[b, R.num_frames(n, hop):] = np.nan
        tp[b, R.num_frames(n, hop):] = np.nan
    dev = torch.device('cuda')
    x = torch.from_numpy(audio).to(dev)
    Ad = torch.from_numpy(A).to(dev)
    t = torch.view_as_real(torch.from_numpy(tp).to(dev)).contiguous()
    c = torch.empty_like(t)
    nd = torch.tensor(lengths, dtype=torch.int32, device=dev)
    trace = torch.empty((B, 2), dtype=torch.float64, device=dev)
    parts = torch.empty(hip_lib.wn_gl_project_partials(B, T, hop),
                        dtype=torch.float64, device=dev)
    gl._project(x, nd, Ad, t, c, alpha, trace, parts)    # (t in place)
    t2, c2 = t.clone(), torch.empty_like(c)
    t2.copy_(torch.view_as_real(torch.from_numpy(tp).to(dev)))
    gl._project(x, nd, Ad, t2, c2, alpha, None, None)
    assert torch.equal(_bits(t), _bits(t2)) and torch.equal(_bits(c), _bits(c2))
    tg = torch.view_as_complex(t).cpu().numpy()
    cg = torch.view_as_complex(c).cpu().numpy()
    tr = trace.cpu().numpy()
    for b, n in enumerate(lengths):
        xb = audio[b, :n].astype(np.float64)
        S = R.stft(xb, *res)
        Fb = S.shape[0]
        Ab, tpb = A[b, :Fb], tp[b, :Fb]
        wt, wc, wtr = R.project(S, Ab.astype(np.float64),
                                tpb.astype(np.complex128), alpha)
        keep = np.abs(S) >= 1e-3 * np.abs(S).max()
        assert keep.mean() >= 0.95
        rest = [R.project_f32(xb, Ab, tpb, alpha, res, k) for k in KINDS]
        for what, got, want, i in (('t', tg, wt, 0), ('c', cg, wc, 1)):
            tol = R.TOL_FACTOR * R.yardstick(want[keep],
                                             [r[i][keep] for r in rest])
            err = np.abs(got[b, :Fb] - want)[keep].max()
            print('%s clip %d %s: err %.3e bound %.3e' % (name, b, what, err, tol))
            assert err <= tol
            assert (got[b, Fb:].view(np.float32).view(np.int32) == 0).all()
        assert np.isfinite(tg[b]).all() and np.isfinite(cg[b]).all()
        # the sums: each term (|S| - A)^2 moves by at most 2 |g| d + d^2 for
        # a |S| that is off by d = the STFT's own bound; A^2 is exact in
        # float64 and its sum of N terms is off by at most N 2^-53 of itself
        d = R.TOL_FACTOR * R.yardstick(
            S, [R.stft_f32(xb, *res, k) for k in KINDS])
        g = np.abs(np.abs(S) - Ab)
        bound = float((2 * g * d + d * d).sum()) + S.size * 2.0 ** -53 * wtr[0]
        print('%s clip %d trace: %r want %r bound %.3e' % (name, b, tr[b], wtr, bound))
        assert abs(tr[b, 0] - wtr[0]) <= bound
        assert abs(tr[b, 1] - wtr[1]) <= S.size * 2.0 ** -53 * wtr[1]


# ------------------------------------------------------ wn_mel_to_magnitude
@pytest.mark.parametrize('n_mels', [1, 33, 80, 128])
def test_magnitude_against_the_restatement(hip_lib, n_mels):
    gl = _gl((256, 64, 256), n_mels)
    melw = R.filterbank(R.RUN_RATE, 256, n_mels)
    frames = R.logmel_frames(n_mels, 2, 9, n_mels)
    nf = [9, 5]
    frames[1, 5:] = np.nan                              # not read
    got = gl.magnitude(frames, nf).cpu().numpy()
    assert got.shape == (2, 9, 129)
    for b in range(2):
        want = R.magnitude(frames[b, :nf[b]], melw)
        tol = R.TOL_FACTOR * R.yardstick(
            want, [R.magnitude_f32(frames[b, :nf[b]], melw, k) for k in KINDS])
        err = np.abs(got[b, :nf[b]] - want).max()
        print('%d mels clip %d: err %.3e bound %.3e' % (n_mels, b, err, tol))
        assert err <= tol
        assert (got[b, nf[b]:].view(np.int32) == 0).all()
    one = gl.magnitude(frames[0])
    assert torch.equal(_bits(one), _bits(gl.magnitude(frames, nf)[0]))


# --------------------------------------------------------------- wn_gl_init
@pytest.mark.parametrize('init', ['random', 'zero'])
def test_initial_spectrum_bit_for_bit(hip_lib, init):
    gl = _gl((64, 16, 64), seed=2 ** 63 + 12345, init=init)
    rng = np.random.default_rng(3)
    A = rng.uniform(0, 2, (3, 17, 33)).astype(np.float32)
    keys = [5, 0, 2 ** 24 - 1]
    got = gl.initial(torch.from_numpy(A).cuda(), keys).cpu().numpy()
    for b in range(3):
        re, im = gl.reference_initial(A[b], keys[b])
        assert np.array_equal(got[b].real.view(np.int32), re.view(np.int32))
        assert np.array_equal(got[b].imag.view(np.int32), im.view(np.int32))
    if init == 'zero':
        assert np.array_equal(got.real, A) and (got.imag == 0).all()
    else:
        assert (got.imag[:, :, 1:-1] != 0).mean() > 0.9
        assert (got.imag[:, :, 0] == 0).all() and (got.imag[:, :, -1] == 0).all()


# ---------------------------------------------------------------- whole runs
@functools.lru_cache(maxsize=None)
def _run_inputs():
    """(frames float32 [3, F, mels], lengths, melw): raw log-mel of three
    ragged signals from the float64 restatement."""
    res, T, lengths = R.RUN
    melw = R.filterbank(R.RUN_RATE, res[0], R.RUN_MELS)
    F = R.num_frames(T, res[1])
    frames = np.zeros((3, F, R.RUN_MELS), np.float32)
    for b, n in enumerate(lengths):
        S = R.stft(R.signal(40 + b, T)[:n], *res)
        frames[b, :S.shape[0]] = np.log(np.maximum(
            (np.abs(S) ** 2) @ melw.T, 1e-10))
    return frames, list(lengths), melw


def _run_gl(**kw):
    return _gl(R.RUN[0], R.RUN_MELS, **kw)


def test_a_clip_does_not_depend_on_the_batch_or_the_grouping(hip_lib):
    frames, lengths, _ = _run_inputs()
    gl = _run_gl(iterations=6)
    whole, trace = gl(frames, lengths, return_trace=True)
    assert tuple(whole.shape) == (3, 4000) and whole.dtype == torch.float32
    assert tuple(trace.shape) == (7, 3, 2) and gl.last_trace is trace
    again = gl(frames, lengths)
    assert torch.equal(_bits(whole), _bits(again))           # run to run
    per = gl.bytes_per_clip(frames.shape[1])
    for clips in (1, 2):
        small = _run_gl(iterations=6, max_bytes=clips * per + 1)
        got, tr = small(frames, lengths, return_trace=True)
        assert torch.equal(_bits(got), _bits(whole)), clips
        assert torch.equal(_bits(tr), _bits(trace)), clips
    for b, n in enumerate(lengths):
        alone, tr = gl(frames[b], [n], keys=[b], return_trace=True)
        assert tuple(alone.shape) == (n,)
        assert torch.equal(_bits(alone), _bits(whole[b, :n])), b
        assert torch.equal(_bits(tr[:, 0]), _bits(trace[:, b])), b
        assert (_bits(whole[b, n:]) == 0).all()
    # another key, another seed: another waveform
    other = gl(frames[0], [lengths[0]], keys=[1])
    assert not torch.equal(_bits(other), _bits(whole[0]))
    assert not torch.equal(_bits(_run_gl(iterations=6, seed=1)(frames, lengths)),
                           _bits(whole))
    with pytest.raises(ValueError, match=str(per)):
        _run_gl(iterations=6, max_bytes=per - 1)(frames, lengths)


def test_no_iterations_is_the_inverse_of_the_initial_spectrum(hip_lib):
    frames, lengths, _ = _run_inputs()
    gl = _run_gl(iterations=0)
    nf = [R.num_frames(n, R.RUN[0][1]) for n in lengths]
    want = gl.istft(gl.initial(gl.magnitude(frames, nf)), lengths)
    got, trace = gl(frames, lengths, return_trace=True)
    assert torch.equal(_bits(got), _bits(want))
    assert tuple(trace.shape) == (1, 3, 2)
    # nframes alone stands for lengths = nframes * hop
    a = gl(frames, nframes=nf)
    b = gl(frames, [f * R.RUN[0][1] for f in nf])
    assert torch.equal(_bits(a), _bits(b))


def test_a_nan_frame_stays_in_its_clip(hip_lib):
    frames, lengths, _ = _run_inputs()
    gl = _run_gl(iterations=4)
    clean = gl(frames, lengths)
    bad = frames.copy()
    bad[1, 3] = np.nan
    got = gl(bad, lengths)
    for b in (0, 2):
        assert torch.equal(_bits(got[b]), _bits(clean[b]))
    assert not torch.equal(_bits(got[1]), _bits(clean[1]))


def test_one_iteration_against_the_restatement(hip_lib):
    """The whole loop, one iteration, from the device's own magnitudes (a
    clip's A does not depend on the batch, so the run inside computes these
    bits): within 4 x the float32 loops' error."""
    frames, lengths, _ = _run_inputs()
    gl = _run_gl(iterations=1, momentum=0.5, seed=9)
    got = gl(frames, lengths).cpu().numpy()
    res = R.RUN[0]
    for b, n in enumerate(lengths):
        Fb = R.num_frames(n, res[1])
        A = gl.magnitude(frames[b, :Fb]).cpu().numpy().astype(np.float64)
        want, _ = R.griffin_lim(A, n, res, 1, 0.5, seed=9, key=b)
        rest = [R.griffin_lim_f32(A, n, res, 1, 0.5, seed=9, key=b, order=k)[0]
                for k in KINDS]
        tol = R.TOL_FACTOR * R.yardstick(want, rest)
        err = np.abs(got[b, :n] - want).max()
        print('clip %d: err %.3e bound %.3e' % (b, err, tol))
        assert err <= tol


def test_the_trace_falls_without_momentum(hip_lib):
    """alpha = 0: the inconsistency sqrt(sum (|S| - A)^2 / sum A^2) does not
    rise from one iteration to the next.  Margin: 4 x the worst upward step of
    the float32 restatements (gl_ref.griffin_lim_f32, both orders) on these
    three clips over 32 iterations, measured on a CPU -- they show NONE: their
    smallest DOWNWARD steps are 3.2e-4, 7.9e-4 and 5.9e-4 -- so the margin is
    zero."""
    frames, lengths, _ = _run_inputs()
    gl = _run_gl(iterations=32, momentum=0.0)
    _, trace = gl(frames, lengths, return_trace=True)
    ratio = R.ratio(trace.cpu().numpy())                  # [33, 3]
    print(ratio[[0, 8, 32]])
    assert np.isfinite(ratio).all()
    assert (np.diff(ratio, axis=0) <= 0.0).all()
    assert (ratio[0] > 0.5).all() and (ratio[-1] < 0.3).all()


@pytest.mark.parametrize('alpha', [0.0, 0.99])
def test_the_final_inconsistency_against_the_float64_loop(hip_lib, alpha):
    """Device and restatement do not share a trajectory: only the ordering --
    the device after 32 iterations lies below the float64 loop after 8 (on a
    CPU: 0.216 / 0.237 / 0.197 against 0.246 / 0.275 / 0.268 at alpha = 0,
    0.199 / 0.198 / 0.174 against 0.223 / 0.246 / 0.221 at 0.99)."""
    frames, lengths, melw = _run_inputs()
    gl = _run_gl(iterations=32, momentum=alpha)
    _, trace = gl(frames, lengths, return_trace=True)
    final = R.ratio(trace.cpu().numpy())[-1]
    res = R.RUN[0]
    for b, n in enumerate(lengths):
        A = R.magnitude(frames[b, :R.num_frames(n, res[1])], melw)
        quarter = R.ratio(R.griffin_lim(A, n, res, 8, alpha, key=b)[1])[-1]
        print('alpha %g clip %d: device %.4f, float64 after 8: %.4f'
              % (alpha, b, final[b], quarter))
        assert final[b] < quarter
