"""Guard bands (tests/guard.py) around the operands of the entries of
include/wavenet_pitch_path.h that write through a pointer: wn_pitch_path
reads and writes nothing outside them -- f0, aper, lag, cost and the
predecessor workspace as outputs, the c' rows, the tracker's lags, nframes and
the two tables as inputs whose bands hold NaNs in one run and zeros in the
other -- at N = 5 (one wave, most lanes behind the last state) and N = 257
(four waves), with ragged nframes.  tests/test_pitch_path_host.py holds
ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard
import pitch_path_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_pitch_path.h that write through a pointer
ENTRIES = ('wn_pitch_path',)

# (tau_min, tau_max, F, nframes)
CASES = [(2, 7, 9, [9, 4, 0]), (2, 7, 5, None), (3, 260, 9, [1, 9, 6]),
         (3, 260, 4, None)]


def _build(tau_min, tau_max, F, nframes, skew=0):
    """(arena, run) of one call on three clips of random rows."""
    from wavenet import pitch
    path = pitch.PitchPath(R.tracker_with_lags(pitch, tau_min, tau_max))
    B, N = 3, tau_max - tau_min
    clips = [R.random_rows(20 + b, F, tau_max) for b in range(B)]
    pen, bias = path.tables()
    ar = guard.Arena('cuda')
    ar.place('cmnd', np.stack([c for c, _ in clips]), torch.float32,
             skew_bytes=skew)
    # (band values that are lags / frame counts themselves)
    ar.place('lag_in', np.stack([l for _, l in clips]), torch.int32,
             fill=(0, 1), skew_bytes=skew)
    if nframes is not None:
        ar.place('nframes', np.asarray(nframes, np.int32), torch.int32,
                 fill=(F, 0), skew_bytes=skew)
    ar.place('pen', pen, torch.float32, skew_bytes=skew)
    ar.place('bias', bias, torch.float32, skew_bytes=skew)
    words = -(-2 * B * F * (N + 1) // 4)
    ar.place('workspace', (words,), torch.int32, role='out', skew_bytes=skew)
    ar.place('f0', (B, F), torch.float32, role='out', skew_bytes=skew)
    ar.place('aper', (B, F), torch.float32, role='out', skew_bytes=skew)
    ar.place('lag', (B, F), torch.int32, role='out', skew_bytes=skew)
    ar.place('cost', (B,), torch.float64, role='out',
             skew_bytes=2 * skew)

    def run(lib):
        assert lib.wn_pitch_path_workspace_bytes(B, F, tau_min, tau_max) \
            <= 4 * words
        code = lib.wn_pitch_path(
            ar.ptr('cmnd'), ar.ptr('lag_in'),
            ar.ptr('nframes' if nframes is not None else None), B, F,
            tau_min, tau_max, ar.ptr('pen'), ar.ptr('bias'), path.switch,
            path.unvoiced, path.tracker.sample_rate, ar.ptr('workspace'),
            ar.ptr('f0'), ar.ptr('aper'), ar.ptr('lag'), ar.ptr('cost'),
            torch.cuda.current_stream().cuda_stream)
        assert code == 0, code
    return ar, run, path, clips


@pytest.mark.parametrize('tau_min,tau_max,F,nframes', CASES)
def test_path_stays_inside_its_operands(hip_lib, tau_min, tau_max, F,
                                        nframes):
    ar, run, path, clips = _build(tau_min, tau_max, F, nframes)
    run(hip_lib)
    torch.cuda.synchronize()
    ar.check()
    bits = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    # (every word of f0, aper and cost was written)
    for key in ('f0', 'aper'):
        assert not (bits[key] == guard._signed(guard.BODY32, 32)).any(), key
    assert not (bits['cost'] == guard._signed(guard.BODY64, 64)).any()
    # and the bits are the rule's
    for b, (c, lag) in enumerate(clips):
        nf = F if nframes is None else nframes[b]
        want = np.zeros(F, np.int32)
        if nf:
            want[:nf] = path.reference(c[:nf], lag[:nf])[0].lag
        assert np.array_equal(bits['lag'][b].cpu().numpy(), want), b


@pytest.mark.parametrize('tau_min,tau_max,F,nframes', [CASES[0], CASES[2]])
def test_path_four_bytes_off_alignment(hip_lib, tau_min, tau_max, F, nframes):
    ar0, run0, _, _ = _build(tau_min, tau_max, F, nframes)
    want = guard.read_check(ar0, lambda: run0(hip_lib))
    ar, run, _, _ = _build(tau_min, tau_max, F, nframes, skew=4)
    assert ar.ptr('cmnd') % 16 == 4 and ar.ptr('f0') % 16 == 4 and \
        ar.ptr('cost') % 16 == 8
    got = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    assert sorted(got) == sorted(want)
    for key in want:
        assert torch.equal(got[key], want[key]), key
