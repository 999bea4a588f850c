"""Linear prediction on the device (csrc/wn_lpc.hip) against wavenet/lpc.py's
numpy rules and the float64 restatement of tests/lpc_ref.py: the coefficients
within the float32 yardstick measured on the CPU as the test runs, the two
filters bit for bit at every length where the kernels take another path."""
import functools

import numpy as np
import pytest
import torch

import lpc_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def _same(got, want, what=''):
    got = got.cpu().numpy() if hasattr(got, 'cpu') else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), '%s: %d of %d words differ, first at %s: %r / %r' % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][0],
        want[bad][0])


# ------------------------------------------------------------ coefficients
@pytest.mark.parametrize('name', [c[0] for c in R.CASES])
def test_coefficients_within_the_yardstick(hip_lib, name):
    """Every frame within four times (the larger error of two float32
    restatements against float64 over the case + one float32 ulp of the
    frame's largest coefficient); ragged nframes, the padding exact zeros."""
    lp, fr = R.case_lp(name), R.case_frames(name)
    c64, tol = R.yardstick(lp, fr)
    F = fr.shape[0]
    batch = np.stack([fr, fr[::-1]])
    nf = [F, F // 2 - 1]
    got = lp.coefficients(batch, nf)
    assert got.shape == (2, F, lp.order) and got.dtype == torch.float32
    got = got.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    err0 = np.abs(got[0] - c64).max(axis=1)
    err1 = np.abs(got[1, :nf[1]] - c64[::-1][:nf[1]]).max(axis=1)
    rule = np.abs(got[0] - lp.reference_coefficients(fr)).max()
    print('%s: worst error / tolerance %.3g (tolerance %.3g .. %.3g), against '
          'the numpy rule %.3g' % (name, max((err0 / tol).max(),
                                            (err1 / tol[::-1][:nf[1]]).max()),
                                   tol.min(), tol.max(), rule))
    assert (err0 <= tol).all(), (err0 / tol).max()
    assert (err1 <= tol[::-1][:nf[1]]).all()
    assert not got[1, nf[1]:].any()
    assert (_bits(got[1, nf[1]:].astype(np.float32)) == 0).all()


def test_one_frame_and_a_frame_in_a_batch():
    """F = 1; a frame alone against the frame in a batch, bit for bit."""
    lp, fr = R.make_lp(), R.vowel_frames()
    whole = lp.coefficients(fr[None, :40]).cpu().numpy()[0]
    for f in (0, 7, 39):
        one = lp.coefficients(fr[f:f + 1])
        assert one.shape == (1, 16)
        _same(one, whole[f:f + 1], 'frame %d alone' % f)
    two = lp.coefficients(np.stack([fr[10:20], fr[30:40]]), [10, 3])
    _same(two[0], whole[10:20], 'clip 0')
    _same(two[1, :3], whole[30:33], 'clip 1')
    assert (_bits(two[1, 3:].cpu().numpy()) == 0).all()


def test_nan_and_inf_frames_give_zeros_and_touch_no_neighbour():
    lp = R.make_lp()
    bad, clean = R.broken_frames(), R.vowel_frames()[20:30]
    got = lp.coefficients(bad).cpu().numpy()
    want = lp.coefficients(clean).cpu().numpy()
    assert np.isfinite(got).all()
    assert not got[R.NAN_FRAME].any() and not got[R.INF_FRAME].any()
    assert want[R.NAN_FRAME].any() and want[R.INF_FRAME].any()
    keep = [f for f in range(10) if f not in (R.NAN_FRAME, R.INF_FRAME)]
    _same(got[keep], want[keep], 'neighbours')
    # any bits at all: finite coefficients
    rng = np.random.default_rng(1)
    wild = rng.integers(-2 ** 31, 2 ** 31, (3, 50, 80), dtype=np.int64) \
        .astype(np.int32).view(np.float32)
    assert torch.isfinite(lp.coefficients(wild)).all()


# ----------------------------------------------------------------- filters
@functools.lru_cache(maxsize=None)
def _lp(order, hop, gain):
    if hop == 256:
        return R.make_lp(order, gain=gain)
    return R.make_lp(order, 8, 64, hop, gain=gain)


def _problem(order, hop, lengths, seed):
    """(x [B, T], coeffs [B, F, order], lengths): random clips, coefficients
    with sum |a| < 0.9 (the recursion stays bounded whatever the frames do)."""
    rng = np.random.default_rng(seed)
    n = np.asarray(lengths, np.int64)
    B, T = n.shape[0], int(n.max())
    F = -(-T // hop)
    x = rng.uniform(-1, 1, (B, T)).astype(np.float32)
    cf = (rng.uniform(-1, 1, (B, F, order)) * 0.9 / order).astype(np.float32)
    return x, cf, n


def _tile():
    from wavenet import lpc
    return lpc.LinearPrediction.analysis_tile()


# (order, hop, gain, lengths): T = 1, T < order, either side of a multiple of
# 64, of a frame edge and of the analysis tile; hops of 1 read the
# coefficients from memory once a tile needs more than 8192 of them
FILTER_CASES = [
    (1, 1, 1.0, (1, 2, 63, 64, 65)),
    (16, 256, 1.0, (1, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257)),
    (16, 256, 8.0, (1023, 1024, 1025, 2047, 2048, 2049, 2100)),
    (17, 7, 8.0, (3, 13, 14, 15, 16, 17, 18, 127, 128, 129, 1030)),
    (32, 7, 1.0, (1, 31, 32, 33, 700)),
    (32, 256, 8.0, (1024 + 31, 1024 + 32, 1024 + 33, 512)),
    (16, 1, 1.0, (100, 1024, 1025)),
    (32, 1, 1.0, (300, 1100, 2049)),
]


@pytest.mark.parametrize('order,hop,gain,lengths', FILTER_CASES)
def test_filters_bit_for_bit(hip_lib, order, hop, gain, lengths):
    """One ragged batch with padded leading dimensions: analysis and synthesis
    (out of place and in place) against reference_*; zeros behind n[b]; then
    every clip alone, without lengths, against its row of the batch."""
    assert _tile() == 1024
    lp = _lp(order, hop, gain)
    x, cf, n = _problem(order, hop, lengths, 100 * order + hop)
    B, T = x.shape
    want_e = lp.reference_analysis(x, cf, n)
    want_y = lp.reference_synthesis(want_e, cf, n)
    dev = torch.device('cuda')
    xin = torch.full((B, T + 5), float('nan'), device=dev)[:, :T]
    xin.copy_(torch.from_numpy(x))
    # (poison behind n[b]: not read)
    for b in range(B):
        xin[b, n[b]:] = float('nan')
    cfd = torch.from_numpy(cf).to(dev)
    out = torch.full((B, T + 3), float('nan'), device=dev)[:, :T]
    got = lp.analysis(xin, cfd, n, out=out)
    assert got is out
    _same(out, want_e, 'analysis')
    ein = torch.full((B, T + 8), float('nan'), device=dev)[:, :T]
    ein.copy_(torch.from_numpy(want_e))
    for b in range(B):
        ein[b, n[b]:] = float('nan')
    y = lp.synthesis(ein, cfd, n)
    _same(y, want_y, 'synthesis')
    back = lp.synthesis(ein, cfd, n, out=ein)           # in place
    assert back is ein
    _same(ein, want_y, 'synthesis in place')
    # a clip alone (numpy in, no lengths, contiguous) against its row
    for b in range(B):
        nb = int(n[b])
        fb = -(-nb // hop)
        _same(lp.analysis(x[b, :nb], cf[b, :fb]), want_e[b, :nb],
              'analysis, clip %d alone' % b)
        _same(lp.synthesis(want_e[b, :nb], cf[b, :fb]), want_y[b, :nb],
              'synthesis, clip %d alone' % b)


def test_a_nan_sample_stays_in_its_clip(hip_lib):
    lp = _lp(16, 256, 1.0)
    x, cf, n = _problem(16, 256, (1500, 1500, 900), 3)
    clean_e = lp.analysis(x, cf, n).cpu().numpy()
    clean_y = lp.synthesis(clean_e, cf, n).cpu().numpy()
    x2 = x.copy()
    x2[1, 700] = np.nan
    e = lp.analysis(x2, cf, n).cpu().numpy()
    for b in (0, 2):
        _same(e[b], clean_e[b], 'analysis clip %d' % b)
    assert np.isnan(e[1, 700:717]).all() and not np.isnan(e[1, :700]).any()
    assert not np.isnan(e[1, 717:]).any()
    e2 = clean_e.copy()
    e2[1, 700] = np.nan
    y = lp.synthesis(e2, cf, n).cpu().numpy()
    for b in (0, 2):
        _same(y[b], clean_y[b], 'synthesis clip %d' % b)
    _same(y[1, :700], clean_y[1, :700], 'in front of the NaN')
    assert np.isnan(y[1, 700:1500]).all()


@pytest.mark.parametrize('order', [16, 32])
def test_zero_coefficients_are_the_identity_times_the_gain(hip_lib, order):
    lp = _lp(order, 256, 8.0)
    x = np.array(R.white()[:3000])
    cf = np.zeros((12, order), np.float32)
    e = lp.analysis(x, cf)
    _same(e, x * np.float32(8), 'analysis')
    _same(lp.synthesis(e, cf), x, 'synthesis')


def test_round_trip_on_the_vowel(hip_lib):
    """The device's own coefficients of the vowel's frames, analysis, then
    synthesis: x comes back within the bound measured on the CPU."""
    lp = R.make_lp()
    lo = 8192
    x = np.array(R.vowel()[lo:lo + 12288])
    cf = lp.coefficients(R.vowel_frames()[lo // 256:])
    e = lp.analysis(x, cf)
    y = lp.synthesis(e, cf).cpu().numpy()
    err = np.abs(y.astype(np.float64) - x).max()
    bound = R.round_trip_bound(x, cf.cpu().numpy(), 256)
    print('round trip: error %.3g, bound %.3g, max |e| %.3g'
          % (err, bound, float(e.abs().max())))
    assert err <= bound
    # and the filters are the numpy rules' on these coefficients too
    _same(e, lp.reference_analysis(x, cf.cpu().numpy()), 'analysis')


def test_coefficients_of_audio_and_ragged_synthesis(hip_lib):
    """coefficients_of = coefficients(raw_frames); synthesis_ragged gives
    every clip the bits of its own call."""
    lp = R.make_lp()
    x = R.vowel()
    clips = [np.array(x[:3000]), np.array(x[4000:5100]), np.array(x[100:101])]
    cfs = [lp.coefficients_of(c) for c in clips]
    for c, cf in zip(clips, cfs):
        assert cf.shape == (-(-c.shape[0] // 256), 16)
        _same(cf, lp.coefficients(lp.raw_frames(c)).cpu().numpy(), 'of')
    es = [lp.analysis(c, cf) for c, cf in zip(clips, cfs)]
    ys = lp.synthesis_ragged(es, cfs)
    for c, cf, e, y in zip(clips, cfs, es, ys):
        _same(y, lp.synthesis(e, cf).cpu().numpy(), 'ragged')
        assert y.shape == c.shape
