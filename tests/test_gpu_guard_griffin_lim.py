"""Guard bands (tests/guard.py) around the operands of the entries of
include/wavenet_griffin_lim.h that write through a pointer: no launch reads or
writes outside them -- poisoned margins round the audio (padded rows: the gap
columns belong to the band), the lengths, the tables, the spectra, the scratch
and every output; what lies behind n[b] INSIDE the audio and behind a clip's
last frame INSIDE the spectra is poison too, so no output depends on it.
tests/test_griffin_lim_host.py holds ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard
import gl_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_griffin_lim.h that write through a pointer
ENTRIES = ('wn_stft', 'wn_istft', 'wn_mel_to_magnitude', 'wn_gl_init',
           'wn_gl_project')

# (shape of gl_ref.SHAPES, ld - T, bytes off alignment)
CASES = [('ragged', 5, 0), ('oddhop', 0, 4), ('nooverlap', 3, 0),
         ('tile33', 7, 4), ('r1024', 1, 0)]


def _gl(name, n_mels=20):
    from wavenet import features, griffin_lim
    n_fft, hop, win = R.SHAPES[name][:3]
    return griffin_lim.GriffinLim(features.MelSpec(
        R.RUN_RATE, n_fft=n_fft, hop=hop, n_mels=n_mels, win_length=win))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _common(ar, name, gl, skew):
    """lengths, window and basis into the arena."""
    T, lengths = R.SHAPES[name][3:]
    window, basis, _ = gl.spec.device_tables(torch.device('cuda'))
    # (band values that are lengths themselves: T, then 1)
    ar.place('lengths', np.asarray(lengths, np.int32), torch.int32,
             fill=(T, 1), skew_bytes=skew)
    ar.place('window', window.cpu(), torch.float32, skew_bytes=skew)
    # (bands of a tile of basis rows, not of the whole table)
    ar.place('basis', basis.cpu(), torch.float32, tile_ld=64)


def _written(bits, *names):
    for key in names:
        pat = guard.BODY32 if bits[key].dtype == torch.int32 else guard.BODY64
        bad = bits[key] == guard._signed(pat, 32 if pat == guard.BODY32 else 64)
        assert not bad.any(), key


@pytest.mark.parametrize('name,gap,skew', CASES)
def test_stft_stays_inside_its_operands(hip_lib, name, gap, skew):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    B, F, nb = len(lengths), R.num_frames(T, hop), n_fft // 2 + 1
    gl = _gl(name)
    audio = R.make_audio(name).copy()
    want = torch.view_as_real(gl.stft(audio, lengths)).cpu().view(torch.int32)
    for b, n in enumerate(lengths):                # poison behind the clip's end
        audio[b, n:] = np.nan
    ar = guard.Arena('cuda')
    ar.place('x', audio, torch.float32, ld=T + gap if gap else None,
             skew_bytes=skew)
    _common(ar, name, gl, skew)
    ar.place('out', (B, F, nb * 2), torch.float32, role='out')

    def run():
        code = hip_lib.wn_stft(ar.ptr('x'), T + gap, B, T, ar.ptr('lengths'),
                               ar.ptr('window'), ar.ptr('basis'), n_fft, hop,
                               nb, ar.ptr('out'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    _written(bits, 'out')
    assert torch.equal(bits['out'].cpu().reshape(want.shape), want)


@pytest.mark.parametrize('name,gap,skew', CASES)
def test_istft_stays_inside_its_operands(hip_lib, name, gap, skew):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    B, F, nb = len(lengths), R.num_frames(T, hop), n_fft // 2 + 1
    gl = _gl(name)
    S = R.make_spectrum(name).copy()
    # (istft cuts its result to max(lengths) = T here)
    want = gl.istft(S, lengths).cpu().view(torch.int32)
    for b, n in enumerate(lengths):                # poison behind the last frame
        S[b, R.num_frames(n, hop):] = np.nan + 1j * np.nan
    ar = guard.Arena('cuda')
    ar.place('spec', S.view(np.float32).reshape(B, F, nb * 2), torch.float32)
    _common(ar, name, gl, skew)
    nbytes = hip_lib.wn_istft_scratch_bytes(B, T, n_fft, hop)
    assert nbytes == 4 * B * F * n_fft
    ar.place('scratch', (B * F, n_fft), torch.float32, role='out',
             skew_bytes=skew)
    ar.place('x', (B, T), torch.float32, ld=T + gap if gap else None,
             role='out', skew_bytes=skew)

    def run():
        code = hip_lib.wn_istft(ar.ptr('spec'), B, T, ar.ptr('lengths'),
                                ar.ptr('window'), ar.ptr('basis'), n_fft, hop,
                                nb, ar.ptr('scratch'), ar.ptr('x'), T + gap,
                                _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    _written(bits, 'x')
    assert torch.equal(bits['x'].cpu(), want)


@pytest.mark.parametrize('name,gap,skew', CASES)
@pytest.mark.parametrize('in_place', [False, True])
def test_project_stays_inside_its_operands(hip_lib, name, gap, skew, in_place):
    n_fft, hop, win, T, lengths = R.SHAPES[name]
    B, F, nb = len(lengths), R.num_frames(T, hop), n_fft // 2 + 1
    gl = _gl(name)
    audio = R.make_audio(name).copy()
    rng = np.random.default_rng(R.SEEDS[name])
    A = rng.uniform(0.1, 2.0, (B, F, nb)).astype(np.float32)
    tp = R.make_spectrum(name).copy()
    for b, n in enumerate(lengths):
        audio[b, n:] = np.nan
        A[b, R.num_frames(n, hop):] = np.nan
        tp[b, R.num_frames(n, hop):] = np.nan + 1j * np.nan
    ar = guard.Arena('cuda')
    ar.place('x', audio, torch.float32, ld=T + gap if gap else None,
             skew_bytes=skew)
    _common(ar, name, gl, skew)
    ar.place('A', A, torch.float32, skew_bytes=skew)
    ar.place('t_prev', tp.view(np.float32).reshape(B, F, nb * 2),
             torch.float32, role='inout' if in_place else 'in')
    if not in_place:
        ar.place('t_out', (B, F, nb * 2), torch.float32, role='out')
    ar.place('c_out', (B, F, nb * 2), torch.float32, role='out')
    ar.place('trace', (B, 2), torch.float64, role='out')
    parts = hip_lib.wn_gl_project_partials(B, T, hop)
    assert parts == 2 * B * -(-F // 32)
    ar.place('partials', (parts,), torch.float64, role='out')
    t_out = 't_prev' if in_place else 't_out'

    def run():
        code = hip_lib.wn_gl_project(
            ar.ptr('x'), T + gap, B, T, ar.ptr('lengths'), ar.ptr('window'),
            ar.ptr('basis'), n_fft, hop, nb, ar.ptr('A'), ar.ptr('t_prev'),
            0.75, ar.ptr(t_out), ar.ptr('c_out'), ar.ptr('trace'),
            ar.ptr('partials'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    _written(bits, t_out, 'c_out', 'trace', 'partials')
    # the same bits as from clean, contiguous operands through the package
    dev = torch.device('cuda')
    t = torch.view_as_real(torch.from_numpy(R.make_spectrum(name)).to(dev)) \
        .contiguous()
    c = torch.empty_like(t)
    trace = torch.empty((B, 2), dtype=torch.float64, device=dev)
    gl._project(torch.from_numpy(R.make_audio(name)).to(dev),
                torch.tensor(lengths, dtype=torch.int32, device=dev),
                torch.from_numpy(np.nan_to_num(A)).to(dev), t, c, 0.75, trace,
                torch.empty(parts, dtype=torch.float64, device=dev))
    assert torch.equal(bits[t_out].cpu().reshape(-1), t.cpu().view(torch.int32).reshape(-1))
    assert torch.equal(bits['c_out'].cpu().reshape(-1), c.cpu().view(torch.int32).reshape(-1))
    assert torch.equal(bits['trace'].cpu(), trace.cpu().view(torch.int64))


@pytest.mark.parametrize('n_mels,n_fft,F', [(1, 64, 3), (33, 256, 70),
                                            (80, 1024, 5), (128, 2048, 2)])
def test_mel_to_magnitude_stays_inside_its_operands(hip_lib, n_mels, n_fft, F):
    from wavenet import features, griffin_lim
    gl = griffin_lim.GriffinLim(features.MelSpec(R.RUN_RATE, n_fft=n_fft,
                                                 hop=n_fft // 4, n_mels=n_mels))
    nb = n_fft // 2 + 1
    frames = R.logmel_frames(n_mels + F, 3, F, n_mels)
    nf = np.array([F, (F + 1) // 2, 0], np.int32)
    want = gl.magnitude(frames, nf).cpu().view(torch.int32)
    for b in range(3):
        frames[b, nf[b]:] = np.nan
    ar = guard.Arena('cuda')
    ar.place('frames', frames, torch.float32, skew_bytes=4)
    ar.place('nframes', nf, torch.int32, fill=(F, 0), skew_bytes=4)
    ar.place('pinv', gl.pinv, torch.float32, skew_bytes=4)
    ar.place('out', (3, F, nb), torch.float32, role='out', skew_bytes=4)

    def run():
        code = hip_lib.wn_mel_to_magnitude(
            ar.ptr('frames'), 3, F, n_mels, ar.ptr('nframes'), ar.ptr('pinv'),
            nb, ar.ptr('out'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    _written(bits, 'out')
    assert torch.equal(bits['out'].cpu(), want)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('n_fft,F', [(64, 3), (256, 33)])
def test_gl_init_stays_inside_its_operands(hip_lib, mode, n_fft, F):
    from wavenet import features, griffin_lim
    gl = griffin_lim.GriffinLim(
        features.MelSpec(R.RUN_RATE, n_fft=n_fft, hop=n_fft // 4, n_mels=8),
        seed=31, init=griffin_lim.INITS[mode])
    nb = n_fft // 2 + 1
    A = np.random.default_rng(F).uniform(0, 2, (3, F, nb)).astype(np.float32)
    keys = np.array([7, 0, 2 ** 24 - 1], np.int64)
    ar = guard.Arena('cuda')
    ar.place('A', A, torch.float32, skew_bytes=4)
    ar.place('keys', keys, torch.int64, fill=(1, 2))
    ar.place('tab', gl.tab, torch.float32)
    ar.place('c0', (3, F, nb * 2), torch.float32, role='out')

    def run():
        code = hip_lib.wn_gl_init(ar.ptr('A'), 3, F, nb, ar.ptr('keys'), 31,
                                  mode, ar.ptr('tab'), ar.ptr('c0'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    _written(bits, 'c0')
    got = bits['c0'].cpu().numpy().view(np.float32).reshape(3, F, nb, 2)
    for b in range(3):
        re, im = gl.reference_initial(A[b], int(keys[b]))
        assert np.array_equal(got[b, :, :, 0].view(np.int32), re.view(np.int32))
        assert np.array_equal(got[b, :, :, 1].view(np.int32), im.view(np.int32))
