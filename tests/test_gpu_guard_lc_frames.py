"""Guard bands (tests/guard.py) around the operands of the entries of
include/wavenet_lc_frames.h that write through a pointer: wn_lc_frames reads
and writes nothing outside them -- out as the output (its padding columns and
the columns the call does not own are band), mel, f0, shift, scale and nframes
as inputs whose bands hold NaNs in one run and zeros in the other -- with
padded leading dimensions, ragged nframes, and padding frames of mel and f0
poisoned so that a read behind nframes[b] shows.  On the vector path (M, both
leading dimensions multiples of 4) and on the scalar one, across a chunk seam.
tests/test_lc_frames_host.py holds ENTRIES against the header."""
import numpy as np
import pytest
import torch

import guard
import lc_frames_ref as R

pytestmark = pytest.mark.gpu

# the entries of wavenet_lc_frames.h that write through a pointer
ENTRIES = ('wn_lc_frames',)

FMIN, FMAX = 60.0, 500.0
SPAN = float(np.log2(FMAX / FMIN))

# (M, ld_mel, ld_out, c0, F, nframes, normalise): F and nframes in frames
# or, as ('CH', k), k frames behind the chunk
CASES = [(8, 12, 16, 8, 9, [9, 4, 0], True),
         (8, 12, 16, 10, 9, None, False),
         (5, 7, 9, 5, 11, [1, 11, 6], True),
         (80, 84, 88, 80, ('CH', 3), [('CH', 0), ('CH', 3), 2], True),
         (3, 3, 5, 3, ('CH', 1), None, False)]


def _n(v, CH):
    return v if isinstance(v, int) else CH + v[1]


def _build(lib, M, ld_mel, ld_out, c0, F, nframes, norm, mode, skew=0):
    """(arena, run, want) of one call on three clips."""
    CH = lib.wn_lc_frames_chunk()
    F = _n(F, CH)
    n = None if nframes is None else [_n(v, CH) for v in nframes]
    B = 3
    rng = np.random.default_rng(M + F)
    mel = rng.standard_normal((B, F, M)).astype(np.float32) * 3 - 8
    f0 = np.stack([R.track(F, runs, seed=b) for b, runs in enumerate((
        [(1, 3), (F - 2, F)], [(0, 1)], [(2, F - 3)]))])
    nn = [F] * B if n is None else n
    for b in range(B):                  # poisoned padding frames
        mel[b, nn[b]:] = np.nan
        f0[b, nn[b]:] = 333.0
    shift = rng.standard_normal(M).astype(np.float32) - 8
    scale = rng.uniform(0.2, 2.0, M).astype(np.float32)
    ar = guard.Arena('cuda')
    ar.place('mel', mel, torch.float32, ld=ld_mel, skew_bytes=skew)
    ar.place('f0', f0, torch.float32, skew_bytes=skew)
    if norm:
        ar.place('shift', shift, torch.float32, skew_bytes=skew)
        ar.place('scale', scale, torch.float32, skew_bytes=skew)
    if n is not None:
        ar.place('nframes', np.asarray(n, np.int32), torch.int32,
                 fill=(F, 0), skew_bytes=skew)
    # out: [B * F rows][ld_out]; the columns the call owns are the operand's,
    # the others are checked as "untouched" below
    ar.place('out', (B * F, ld_out), torch.float32, role='out',
             skew_bytes=skew)

    def run():
        code = lib.wn_lc_frames(
            ar.ptr('mel'), ld_mel, M, ar.ptr('shift' if norm else None),
            ar.ptr('scale' if norm else None), -2.5, 2.5, ar.ptr('f0'), mode,
            FMIN, SPAN, ar.ptr('nframes' if n is not None else None), B, F,
            ar.ptr('out'), ld_out, c0,
            torch.cuda.current_stream().cuda_stream)
        assert code == 0, code

    from wavenet import features
    want = np.zeros((B, F, M + 2), np.float32)
    m = np.where(np.isnan(mel), 0, mel)
    want[..., :M] = features.Normalizer(shift, scale, -2.5, 2.5).reference(
        m, n) if norm else np.where(
            np.arange(F)[None, :, None] < np.asarray(nn)[:, None, None], m, 0)
    ch0, flag = R.batch_channels(f0, nn, mode, FMIN, FMAX)
    want[..., M], want[..., M + 1] = ch0, flag
    return ar, run, want, (B, F)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('M,ld_mel,ld_out,c0,F,nframes,norm', CASES)
def test_lc_frames_stays_inside_its_operands(hip_lib, M, ld_mel, ld_out, c0,
                                             F, nframes, norm, mode):
    ar, run, want, (B, F) = _build(hip_lib, M, ld_mel, ld_out, c0, F, nframes,
                                   norm, mode)
    run()
    torch.cuda.synchronize()
    ar.check()
    bits = guard.read_check(ar, run)
    ar.check()
    out = bits['out'].view(torch.float32).cpu().numpy().reshape(B, F, ld_out)
    raw = bits['out'].cpu().numpy().reshape(B, F, ld_out)
    owned = np.zeros(ld_out, bool)
    owned[:M] = owned[c0] = owned[c0 + 1] = True
    # every owned word was written, no other column was
    body = guard._signed(guard.BODY32, 32)
    assert not (raw[..., owned] == body).any()
    assert (raw[..., ~owned] == body).all()
    # and the bits are the rule's: the mel channels exactly, the flag
    # exactly, the F0 channel within one rounding flip
    assert np.array_equal(out[..., :M], want[..., :M])
    assert np.array_equal(out[..., c0 + 1], want[..., M + 1])
    assert np.abs(out[..., c0].astype(np.float64) - want[..., M]).max() \
        <= 2.0 ** -23


@pytest.mark.parametrize('M,ld_mel,ld_out,c0,F,nframes,norm',
                         [CASES[0], CASES[2]])
def test_lc_frames_four_bytes_off_alignment(hip_lib, M, ld_mel, ld_out, c0, F,
                                            nframes, norm):
    ar0, run0, _, _ = _build(hip_lib, M, ld_mel, ld_out, c0, F, nframes, norm,
                             1)
    want = guard.read_check(ar0, run0)
    ar, run, _, _ = _build(hip_lib, M, ld_mel, ld_out, c0, F, nframes, norm,
                           1, skew=4)
    assert ar.ptr('mel') % 16 == 4 and ar.ptr('out') % 16 == 4
    got = guard.read_check(ar, run)
    ar.check()
    assert torch.equal(got['out'], want['out'])
