"""wn_lc_frames on the device (include/wavenet_lc_frames.h, wavenet/
frontend.py) against the float64 restatement of tests/lc_frames_ref.py and
features.Normalizer.reference, with CH = wn_lc_frames_chunk(): F on and around
the chunk seams, tracks whose voiced runs and gaps end on, start on and span
them, ragged nframes, padded leading dimensions, both modes; the mel channels
bit for bit, the voicing flag exactly, the F0 channel within 2^-23; in place,
NULL operands, a clip alone against the clip in a batch; and MelPitchSpec on
two short synthetic clips against its parts."""
import numpy as np
import pytest
import torch

import lc_frames_ref as R

pytestmark = pytest.mark.gpu

FMIN, FMAX = 60.0, 500.0
SPAN = float(np.log2(FMAX / FMIN))
# Two correct float64 evaluations of the F0 channel differ by ~1e-16.  That
# can flip the single rounding to float32 by one float32 ulp, at most 2^-24
# on [0, 1]; the bound is twice that.
BOUND = 2.0 ** -23
LO, HI = -2.5, 2.5


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)) \
        .cuda()


def _call(lib, mel, M, shift, scale, f0, mode, nframes, B, F, out, c0):
    """One launch on device tensors (mel and out [B, F, ld])."""
    code = lib.wn_lc_frames(
        None if mel is None else mel.data_ptr(),
        0 if mel is None else mel.shape[-1], M,
        None if shift is None else shift.data_ptr(),
        None if scale is None else scale.data_ptr(), LO, HI,
        None if f0 is None else f0.data_ptr(), mode, FMIN, SPAN,
        None if nframes is None else nframes.data_ptr(), B, F,
        out.data_ptr(), out.shape[-1], c0,
        torch.cuda.current_stream().cuda_stream)
    assert code == 0, code


@pytest.fixture(scope='module')
def CH(hip_lib):
    return hip_lib.wn_lc_frames_chunk()


_cache = {}


def _case(CH, Fk, B, M):
    """The inputs and the expected frames of one shape, computed once and
    left unchanged: (mel [B, F, M], f0 [B, F], n [B], shift, scale,
    {(mode, norm): (mel part float32, ch0 float64, flag)})."""
    F = {'1': 1, '2': 2, 'CH-1': CH - 1, 'CH': CH, 'CH+1': CH + 1,
         '2CH+1': 2 * CH + 1}[Fk]
    key = (F, B, M)
    if key not in _cache:
        from wavenet import features
        rng = np.random.default_rng(1000 * B + M + F)
        mel = (rng.standard_normal((B, F, M)) * 4 - 8).astype(np.float32)
        mel[0, 0, 0] = np.nan                       # (a NaN stays a NaN)
        tracks = R.seam_tracks(F, CH)
        f0 = tracks[(np.arange(B) * 3 + F + M) % len(tracks)]
        if B == 5:
            # (a fixed choice; test_every_seam_track runs all of them)
            f0 = tracks[[15, 9, 5, 13, 12]]
        f0 = f0.copy()
        f0[0, F // 3] = np.nan
        f0[-1, F // 2] = -50.0
        n = np.array([F, 0, max(F - 1, 0), F // 2, F][:B] if B > 1 else [F],
                     np.int32)
        shift = (rng.standard_normal(M) - 8).astype(np.float32)
        scale = rng.uniform(0.2, 2.0, M).astype(np.float32)
        norm = features.Normalizer(shift, scale, LO, HI)
        real = np.arange(F)[None, :, None] < n[:, None, None]
        want = {}
        for mode in (0, 1):
            ch0, flag = R.batch_channels(f0, n, mode, FMIN, FMAX)
            want[mode, True] = (norm.reference(mel, n), ch0, flag)
            want[mode, False] = (np.where(real, mel, np.float32(0)), ch0,
                                 flag)
        _cache[key] = (mel, f0, n, shift, scale, want)
    return (F,) + _cache[key]


def _same_bits(got, want):
    """Bit for bit; a NaN of any payload where the other holds a NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(gn, wn) and \
        np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn])


def _check(out, M, c0, want, what=''):
    got = out.cpu().numpy()
    melw, ch0, flag = want
    assert _same_bits(got[..., :M], melw), what
    assert np.array_equal(got[..., c0 + 1], flag), what
    err = np.abs(got[..., c0].astype(np.float64) - ch0)
    differ = int((got[..., c0] != ch0.astype(np.float32)).sum())
    print('%s: F0 channel max error %.3g, %d of %d elements differ from the '
          'rounded restatement' % (what, err.max(), differ, ch0.size))
    assert err.max() <= BOUND, what


@pytest.mark.parametrize('M,pad_in,pad_out,gap', [(1, 0, 0, 0), (1, 2, 1, 1),
                                                  (80, 4, 2, 0), (80, 1, 3, 2),
                                                  (128, 0, 6, 4)])
@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('Fk', ['1', '2', 'CH-1', 'CH', 'CH+1', '2CH+1'])
def test_frames_against_the_restatement(hip_lib, CH, Fk, B, M, pad_in,
                                        pad_out, gap):
    """Both modes, with and without a normaliser and nframes; ld_mel = M +
    pad_in, c0 = M + gap, ld_out = c0 + 2 + pad_out.  Columns the call does
    not own keep their contents."""
    F, mel, f0, n, shift, scale, want = _case(CH, Fk, B, M)
    c0 = M + gap
    ld_out = c0 + 2 + pad_out
    melp = np.full((B, F, M + pad_in), np.float32(7e7))
    melp[..., :M] = mel
    d_mel, d_f0, d_n = _dev(melp), _dev(f0), _dev(n)
    d_shift, d_scale = _dev(shift), _dev(scale)
    owned = np.zeros(ld_out, bool)
    owned[:M] = owned[c0] = owned[c0 + 1] = True
    for mode in (0, 1):
        for norm in (True, False):
            out = torch.full((B, F, ld_out), -77.0, device='cuda')
            _call(hip_lib, d_mel, M, d_shift if norm else None,
                  d_scale if norm else None, d_f0, mode, d_n, B, F, out, c0)
            _check(out, M, c0, want[mode, norm],
                   'F %d B %d M %d mode %d norm %d' % (F, B, M, mode, norm))
            assert (out.cpu().numpy()[..., ~owned] == -77.0).all()
    # nframes NULL: every frame is real
    out = torch.full((B, F, ld_out), -77.0, device='cuda')
    _call(hip_lib, d_mel, M, None, None, d_f0, 1, None, B, F, out, c0)
    ch0, flag = R.batch_channels(f0, None, 1, FMIN, FMAX)
    _check(out, M, c0, (mel, ch0, flag), 'F %d B %d M %d, all real'
           % (F, B, M))


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('Fk', ['CH+1', '2CH+1'])
def test_every_seam_track(hip_lib, CH, Fk, mode):
    """Every row of seam_tracks(F, CH) in one batch: a voiced frame exactly
    at a chunk's first and at its last frame, runs and gaps that end on,
    start on and span the seams, a gap over two seams.  Flag exact, F0
    channel within 2^-23; with all frames real and with ragged nframes that
    cut clips on and beside the seams."""
    F = {'CH+1': CH + 1, '2CH+1': 2 * CH + 1}[Fk]
    f0 = R.seam_tracks(F, CH)
    B = f0.shape[0]
    assert B == 16
    # (the handovers: voiced at a chunk's first frame / at its last)
    assert (f0[:, CH] > 0).any() and (f0[:, CH - 1] > 0).any()
    d_f0 = _dev(f0)
    cuts = np.array([F, CH, CH + 1, CH - 1, F - 1, 1, 0, 2, F, CH, CH + 1,
                     CH - 1, F, F - 1, 3, F], np.int32)
    for n in (None, cuts):
        out = torch.full((B, F, 3), -77.0, device='cuda')
        _call(hip_lib, None, 0, None, None, d_f0, mode, _dev(n), B, F, out, 1)
        got = out.cpu().numpy()
        ch0, flag = R.batch_channels(f0, n, mode, FMIN, FMAX)
        assert (got[..., 0] == -77.0).all()
        assert np.array_equal(got[..., 2], flag)
        err = np.abs(got[..., 1].astype(np.float64) - ch0)
        print('F %d mode %d %s: max error %.3g per track %s'
              % (F, mode, 'all real' if n is None else 'ragged', err.max(),
                 np.array2string(err.max(1), precision=2)))
        assert err.max() <= BOUND


# (80, 2): ld = 84, every 16-byte condition holds -- the wide path, in place
@pytest.mark.parametrize('M,pad', [(80, 4), (80, 2), (5, 3)])
def test_in_place_null_operands_and_batch_independence(hip_lib, CH, M, pad):
    B, Fk = 5, '2CH+1'
    F, mel, f0, n, shift, scale, want = _case(CH, Fk, B, 80)
    mel, shift, scale = mel[..., :M], shift[:M], scale[:M]
    ld = M + 2 + pad
    c0 = M + pad // 2
    if (M, pad) == (80, 2):
        assert M % 4 == 0 and ld % 4 == 0 and c0 >= M
    buf = np.full((B, F, ld), np.float32(-5.0))
    buf[..., :M] = mel
    d_f0, d_n = _dev(f0), _dev(n)
    d_shift, d_scale = _dev(shift), _dev(scale)
    src = _dev(buf)
    # out of place, then in place: the same bits
    out = torch.full((B, F, ld), -5.0, device='cuda')
    _call(hip_lib, src, M, d_shift, d_scale, d_f0, 1, d_n, B, F, out, c0)
    inp = src.clone()
    _call(hip_lib, inp, M, d_shift, d_scale, d_f0, 1, d_n, B, F, inp, c0)
    assert torch.equal(out.view(torch.int32), inp.view(torch.int32))
    from wavenet import features
    assert _same_bits(
        out.cpu().numpy()[..., :M],
        features.Normalizer(shift, scale, LO, HI).reference(
            np.ascontiguousarray(mel), n))
    # NULL mel: its columns keep their contents, the pitch channels are the
    # full call's; NULL f0: the other way round
    a = torch.full((B, F, ld), 3.0, device='cuda')
    _call(hip_lib, None, M, None, None, d_f0, 1, d_n, B, F, a, c0)
    assert (a[..., :M] == 3.0).all()
    assert torch.equal(a[..., c0:c0 + 2], out[..., c0:c0 + 2])
    b = torch.full((B, F, ld), 3.0, device='cuda')
    _call(hip_lib, src, M, d_shift, d_scale, None, 0, d_n, B, F, b, c0)
    assert (b[..., M:] == 3.0).all()
    assert torch.equal(b[..., :M].view(torch.int32).contiguous(),
                       out[..., :M].view(torch.int32).contiguous())
    # a clip alone is the clip in the batch, bit for bit
    for k in range(B):
        one = torch.full((1, F, ld), -5.0, device='cuda')
        _call(hip_lib, src[k:k + 1].contiguous(), M, d_shift, d_scale,
              d_f0[k:k + 1].contiguous(), 1, d_n[k:k + 1].contiguous(), 1, F,
              one, c0)
        assert torch.equal(one[0].view(torch.int32),
                           out[k].view(torch.int32)), k


@pytest.fixture(scope='module')
def clips():
    """Two tones with a silent gap, 4000 samples at 16 kHz: [2, 4000], and
    their lengths (the second is shorter: ragged)."""
    x = np.stack([R.tone_with_gap(150.0, seed=1),
                  R.tone_with_gap(260.0, gap=(900, 2000), seed=2)])
    return x, np.array([4000, 3500])


@pytest.mark.parametrize('use_path', [False, True], ids=['tracker', 'path'])
def test_spec_is_its_parts(hip_lib, clips, use_path):
    """MelPitchSpec(audio) against mel(audio) plus the normaliser (bit for
    bit) and tracker.channels (mode 0, 2^-23); the interpolated channel
    against the restatement on the device's own track."""
    from wavenet import features, frontend, pitch
    x, lengths = clips
    rng = np.random.default_rng(4)
    norm = features.Normalizer(rng.standard_normal(20) - 8,
                               rng.uniform(0.2, 1.0, 20), -3.0, 3.0)
    mel = features.MelSpec(16000, n_fft=256, hop=64, n_mels=20)
    # (a window short enough that whole frames fall into the silent gaps)
    t = pitch.PitchTracker(16000, hop=64, fmin=100.0, window=256)
    path = pitch.PitchPath(t) if use_path else None
    nf = -(-lengths // 64)
    p = (path or t)(x, lengths)
    f0 = p.f0.cpu().numpy()
    print('voiced frames per clip: %s of %s' % ((f0 > 0).sum(1), nf))
    assert ((f0 > 0).sum(1) > 10).all()
    assert all((f0[b, :nf[b]] == 0).sum() >= 3 for b in range(2))
    for normalizer in (None, norm):
        raw = mel(x, lengths)
        want_mel = raw if normalizer is None else normalizer(raw, nf)
        for interp in (False, True):
            spec = frontend.MelPitchSpec(mel.with_normalizer(normalizer), t,
                                         path, interp)
            got = spec(x, lengths)
            assert got.shape == (2, 63, 22) and got.dtype == torch.float32
            assert torch.equal(got[..., :20].view(torch.int32).contiguous(),
                               want_mel.view(torch.int32))
            ch = t.channels(p, nf)
            assert torch.equal(got[..., 21], ch[..., 1])
            if not interp:
                assert (got[..., 20] - ch[..., 0]).abs().max().item() <= BOUND
            ch0, flag = R.batch_channels(f0, nf, int(interp), t.fmin, t.fmax)
            g = got.cpu().numpy()
            assert np.array_equal(g[..., 21], flag)
            assert np.abs(g[..., 20].astype(np.float64) - ch0).max() <= BOUND
            assert (g[1, nf[1]:] == 0).all()
            # one clip [T] is the batch's first
            one = spec(x[0])
            assert one.shape == (63, 22)
            assert torch.equal(one.view(torch.int32),
                               got[0].view(torch.int32))
    # the numpy rule of the whole front end, on the device's track
    ref = spec.reference_channels(f0, nf)
    assert np.abs(ref[..., 0] - g[..., 20]).max() <= BOUND
    assert np.array_equal(ref[..., 1], g[..., 21])
