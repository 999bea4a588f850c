"""Guard bands (tests/guard.py) around the operands of the entry of
include/wavenet_resample.h that writes through a pointer: wn_resample reads
and writes nothing outside them -- poisoned margins round the audio (padded
rows: the gap columns belong to the band), the lengths, the tap table and the
output; what lies behind n[b] INSIDE the audio is poison too, so no output
depends on it.  tests/test_resample_host.py holds ENTRIES against the
header."""
import numpy as np
import pytest
import torch

import guard

pytestmark = pytest.mark.gpu

# the entries of wavenet_resample.h that write through a pointer
ENTRIES = ('wn_resample',)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# (up, down, half_width, lengths, ld_x - T, ld_out - T_out, skew bytes): the
# whole table, the phase rows, taps from memory, input from memory, a copy
CASES = [(5, 8, 10, (1300, 410, 0, 1, 777), 3, 5, 0),
         (5, 4, 10, (500, 499, 205), 0, 0, 4),
         (100, 441, 1, (2400, 1200, 17), 1, 7, 8),
         (1000, 1001, 10, (300, 257), 4, 0, 4),
         (300, 301, 32, (520, 3), 0, 3, 0),
         (1, 13, 10, (4000, 3999), 5, 2, 4),
         (1, 1, 10, (300, 0, 299), 2, 1, 4)]


@pytest.mark.parametrize('up,down,half_width,lengths,gap_in,gap_out,skew',
                         CASES)
def test_resample_stays_inside_its_operands(hip_lib, up, down, half_width,
                                            lengths, gap_in, gap_out, skew):
    from wavenet import resample
    rs = resample.Resampler(down * 100, up * 100, half_width=half_width)
    B, T = len(lengths), max(lengths)
    To = rs.out_length(T)
    rng = np.random.default_rng(up + down)
    x = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    n = np.array(lengths, np.int32)
    want = rs.reference(x, n)
    for b in range(B):                       # poison behind n[b]
        x[b, n[b]:] = np.nan
    ar = guard.Arena('cuda')
    ar.place('x', x, torch.float32, ld=T + gap_in if gap_in else None,
             skew_bytes=skew)
    ar.place('lengths', n, torch.int32, fill=(T, 0), skew_bytes=skew)
    ar.place('tab', rs.table, torch.float32, skew_bytes=skew)
    ar.place('out', (B, To), torch.float32, role='out',
             ld=To + gap_out if gap_out else None, skew_bytes=skew)

    def run():
        code = hip_lib.wn_resample(
            ar.ptr('x'), T + gap_in, ar.ptr('lengths'), B, T, up, down,
            rs.Hh, ar.ptr('tab'), ar.ptr('out'), To + gap_out, _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    got = bits['out'].cpu()
    assert not (got == guard._signed(guard.BODY32, 32)).any()
    assert torch.equal(got, torch.from_numpy(
        np.ascontiguousarray(want).view(np.int32)))


def test_resample_without_lengths(hip_lib):
    from wavenet import resample
    rs = resample.Resampler(16000, 10000)
    B, T = 2, 900
    To = rs.out_length(T)
    x = np.random.default_rng(1).uniform(-1, 1, (B, T)).astype(np.float32)
    ar = guard.Arena('cuda')
    ar.place('x', x, torch.float32, ld=T + 2, skew_bytes=4)
    ar.place('tab', rs.table, torch.float32)
    ar.place('out', (B, To), torch.float32, role='out', ld=To + 6)

    def run():
        code = hip_lib.wn_resample(ar.ptr('x'), T + 2, None, B, T, 5, 8, 80,
                                   ar.ptr('tab'), ar.ptr('out'), To + 6,
                                   _stream())
        assert code == 0, code
    bits = guard.read_check(ar, run)
    ar.check()
    assert torch.equal(bits['out'].cpu(), torch.from_numpy(
        np.ascontiguousarray(rs.reference(x)).view(np.int32)))
