"""Guard bands (tests/guard.py) around the operands of the entries of
include/wavenet_lpc.h that write through a pointer: wn_lpc_from_mel,
wn_lpc_analysis and wn_lpc_synthesis read and write nothing outside them --
poisoned margins round the frames, the tables, the audio (padded rows: the gap
columns belong to the band), the coefficients, the lengths and the outputs;
what lies behind n[b] INSIDE the audio and behind the last frame INSIDE the
frames and the coefficients is poison too, so no output depends on it.
tests/test_lpc_host.py holds ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard
import lpc_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_lpc.h that write through a pointer
ENTRIES = ('wn_lpc_from_mel', 'wn_lpc_analysis', 'wn_lpc_synthesis')


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize('name,skew', [('o16', 0), ('o32m8', 4), ('o1', 4),
                                       ('o17m128', 0)])
def test_from_mel_stays_inside_its_operands(hip_lib, name, skew):
    lp, fr = R.case_lp(name), R.case_frames(name)
    F = fr.shape[0]
    nf = np.array([F, F // 3, 0], np.int32)
    frames = np.stack([fr, fr[::-1], fr]).copy()
    want = lp.coefficients(frames, nf).cpu().view(torch.int32)
    for b in range(3):                       # poison behind the real frames
        frames[b, nf[b]:] = np.nan
    ar = guard.Arena('cuda')
    ar.place('frames', frames, torch.float32, skew_bytes=skew)
    ar.place('nframes', nf, torch.int32, fill=(F, 0), skew_bytes=skew)
    ar.place('pinv', np.ascontiguousarray(lp.pinv.T), torch.float32,
             skew_bytes=skew)
    ar.place('ctab', lp.ctab, torch.float64)
    ar.place('lagwin', lp.lagwin, torch.float64)
    ar.place('out', (3, F, lp.order), torch.float32, role='out',
             skew_bytes=skew)

    def run():
        code = hip_lib.wn_lpc_from_mel(
            ar.ptr('frames'), 3, F, lp.n_mels, ar.ptr('nframes'),
            ar.ptr('pinv'), lp.n_bins, ar.ptr('ctab'), ar.ptr('lagwin'),
            lp.order, ar.ptr('out'), _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    assert not (bits['out'] == guard._signed(guard.BODY32, 32)).any()
    assert torch.equal(bits['out'].cpu(), want)


def _filter_problem(order, hop, lengths, gain):
    from test_gpu_lpc import _lp, _problem
    lp = _lp(order, hop, gain)
    x, cf, n = _problem(order, hop, lengths, 7 * order + hop)
    return lp, x, cf, n


# (order, hop, lengths, ld_in - T, ld_out - T, skew bytes)
FILTER_CASES = [(16, 256, (1500, 1024, 1, 700), 3, 5, 0),
                (16, 256, (1025, 1023, 64), 0, 0, 4),
                (32, 7, (1100, 33, 500), 1, 0, 4),
                (17, 1, (1030, 400), 4, 8, 0),
                (1, 256, (65, 2), 0, 7, 8)]


@pytest.mark.parametrize('entry', ['wn_lpc_analysis', 'wn_lpc_synthesis',
                                   'in place'])
@pytest.mark.parametrize('order,hop,lengths,gap_in,gap_out,skew', FILTER_CASES)
def test_filters_stay_inside_their_operands(hip_lib, entry, order, hop,
                                            lengths, gap_in, gap_out, skew):
    lp, x, cf, n = _filter_problem(order, hop, lengths, 8.0)
    B, T = x.shape
    F = cf.shape[1]
    if entry == 'wn_lpc_analysis':
        src, g = x, float(lp.gain32)
        want = lp.reference_analysis(x, cf, n)
    else:
        src, g = lp.reference_analysis(x, cf, n), float(lp.inv_gain32)
        want = lp.reference_synthesis(src, cf, n)
    src, cf = src.copy(), cf.copy()
    for b in range(B):               # poison behind n[b] and the last frame
        src[b, n[b]:] = np.nan
        cf[b, -(-int(n[b]) // hop):] = np.nan
    in_place = entry == 'in place'
    if in_place:
        gap_out = gap_in
    ar = guard.Arena('cuda')
    ar.place('in', src, torch.float32, ld=T + gap_in if gap_in else None,
             skew_bytes=skew, role='inout' if in_place else 'in')
    ar.place('coeffs', cf, torch.float32, skew_bytes=skew)
    ar.place('lengths', n.astype(np.int32), torch.int32, fill=(T, 1),
             skew_bytes=skew)
    if not in_place:
        ar.place('out', (B, T), torch.float32, role='out',
                 ld=T + gap_out if gap_out else None, skew_bytes=skew)
    dst = 'in' if in_place else 'out'
    fn = hip_lib.wn_lpc_analysis if entry == 'wn_lpc_analysis' else \
        hip_lib.wn_lpc_synthesis

    def run():
        code = fn(ar.ptr('in'), T + gap_in, ar.ptr('coeffs'), F, order, hop,
                  ar.ptr('lengths'), B, T, g, ar.ptr(dst), T + gap_out,
                  _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    got = bits[dst].cpu()
    assert not (got == guard._signed(guard.BODY32, 32)).any()
    assert torch.equal(got, torch.from_numpy(
        np.ascontiguousarray(want).view(np.int32)))


def test_filters_without_lengths(hip_lib):
    lp, x, cf, _ = _filter_problem(16, 256, (1300, 1300), 1.0)
    B, T = x.shape
    e = lp.reference_analysis(x, cf)
    for fn, src, g, want in (
            (hip_lib.wn_lpc_analysis, x, 1.0, e),
            (hip_lib.wn_lpc_synthesis, e, 1.0,
             lp.reference_synthesis(e, cf))):
        ar = guard.Arena('cuda')
        ar.place('in', src, torch.float32, ld=T + 2, skew_bytes=4)
        ar.place('coeffs', cf, torch.float32)
        ar.place('out', (B, T), torch.float32, role='out', ld=T + 6)

        def run():
            code = fn(ar.ptr('in'), T + 2, ar.ptr('coeffs'), cf.shape[1], 16,
                      256, None, B, T, g, ar.ptr('out'), T + 6, _stream())
            assert code == 0, code
        bits = guard.read_check(ar, run)
        ar.check()
        assert torch.equal(bits['out'].cpu(), torch.from_numpy(
            np.ascontiguousarray(want).view(np.int32)))
