"""Guard bands (tests/guard.py) around the operands of the entries of
include/wavenet_pitch.h that write through a pointer: wn_pitch_track reads
and writes nothing outside them -- with padded rows (ld > T: the gap columns
belong to the band), with and without the cmnd output, with lengths, and with
every operand four bytes off its alignment.  tests/test_pitch_host.py holds
ENTRIES against the header, the rule tests/test_guard_host.py keeps for
wavenet_hip.h."""
import numpy as np
import pytest
import torch

import guard
import pitch_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_pitch.h that write through a pointer
ENTRIES = ('wn_pitch_track',)

# (shape of pitch_ref.SHAPES, ld - T, cmnd)
CASES = [('a', 5, 1), ('a', 1, 0), ('b', 3, 1), ('b', 0, 0), ('c', 7, 1),
         ('c', 2, 0)]


def _build(name, gap, cmnd, skew=0):
    """(arena, run) of one call on the audio of shape `name`."""
    from wavenet import pitch
    t = pitch.PitchTracker(**R.settings(name))
    x, lengths = R.make_audio(name)
    B, T = x.shape
    F = t.num_frames(T)
    ar = guard.Arena('cuda')
    ar.place('audio', x, torch.float32, ld=T + gap if gap else None,
             skew_bytes=skew)
    if lengths is not None:
        # (band values that are lengths themselves: T, then 1)
        ar.place('lengths', np.asarray(lengths, np.int32), torch.int32,
                 fill=(T, 1), skew_bytes=skew)
    ar.place('f0', (B, F), torch.float32, role='out', skew_bytes=skew)
    ar.place('aper', (B, F), torch.float32, role='out', skew_bytes=skew)
    ar.place('lag', (B, F), torch.int32, role='out', skew_bytes=skew)
    if cmnd:
        ar.place('cmnd', (B, F, t.tau_max + 1), torch.float32, role='out',
                 skew_bytes=skew)

    def run(lib):
        code = lib.wn_pitch_track(
            ar.ptr('audio'), ar.ptr('lengths' if lengths is not None
                                    else None), T + gap, B, T, t.hop,
            t.window, t.tau_min, t.tau_max, t.threshold, t.silence,
            t.sample_rate, ar.ptr('f0'), ar.ptr('aper'), ar.ptr('lag'),
            ar.ptr('cmnd' if cmnd else None),
            torch.cuda.current_stream().cuda_stream)
        assert code == 0, code
    return ar, run


@pytest.mark.parametrize('name,gap,cmnd', CASES)
def test_track_stays_inside_its_operands(hip_lib, name, gap, cmnd):
    ar, run = _build(name, gap, cmnd)
    run(hip_lib)
    torch.cuda.synchronize()
    ar.check()
    bits = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    # (every word of every output was written)
    for key, b in bits.items():
        assert not (b == guard.BODY32).any(), key


@pytest.mark.parametrize('name,gap,cmnd', [('a', 5, 1), ('b', 3, 1),
                                           ('c', 7, 0)])
def test_track_four_bytes_off_alignment(hip_lib, name, gap, cmnd):
    ar0, run0 = _build(name, gap, cmnd)
    want = guard.read_check(ar0, lambda: run0(hip_lib))
    ar, run = _build(name, gap, cmnd, skew=4)
    assert ar.ptr('audio') % 16 == 4 and ar.ptr('f0') % 16 == 4
    got = guard.read_check(ar, lambda: run(hip_lib))
    ar.check()
    assert sorted(got) == sorted(want)
    for key in want:
        assert torch.equal(got[key], want[key]), key
