"""The pitch tracker on the device (csrc/wn_pitch.hip through
wavenet/pitch.py) against the float64 oracle of tests/pitch_ref.py at every
shape of pitch_ref.SHAPES: c' within four times the shape's float32 yardstick;
lag and voicing exact, f0 within the derived tolerance and aper within the
bound on the decisive frames (tests/test_pitch_host.py holds them to 95 % of
the frames on the oracle alone); silent and padding frames exactly as the rule
states them; rows that are ties exactly; and, bit for bit, a clip alone
against the clip in a batch of NaN, a padded and skewed operand, cmnd on or
off, and the conditioning channels against the CPU."""
import numpy as np
import pytest
import torch

import guard
import pitch_ref as R

pytestmark = pytest.mark.gpu

NAN = float('nan')
_ORACLE, _DEVICE = {}, {}


def _oracle(name):
    """The oracle's results for the clips of shape `name`: computed once,
    shared, never written to."""
    if name not in _ORACLE:
        _ORACLE[name] = [R.track(c, **R.settings(name))
                         for c in R.clips(name)]
    return _ORACLE[name]


def _tracker(name):
    from wavenet import pitch
    return pitch.PitchTracker(**R.settings(name))


def _device(name):
    """Pitch of make_audio(name) with cmnd, as numpy: one launch per shape."""
    if name not in _DEVICE:
        x, lengths = R.make_audio(name)
        p = _tracker(name)(x, lengths, return_cmnd=True)
        torch.cuda.synchronize()
        _DEVICE[name] = tuple(t.cpu().numpy() for t in p)
    return _DEVICE[name]


def _bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int32)


@pytest.mark.parametrize('name', sorted(R.SHAPES))
def test_against_the_oracle(hip_lib, name):
    kw = R.settings(name)
    t = _tracker(name)
    B, T, lengths = R.CLIPS[name]
    f0, aper, lag, cmnd = _device(name)
    F = t.num_frames(T)
    assert f0.shape == aper.shape == lag.shape == (B, F)
    assert cmnd.shape == (B, F, t.tau_max + 1)
    assert f0.dtype == aper.dtype == cmnd.dtype == np.float32
    assert lag.dtype == np.int32
    m = R.shape_tol(name)
    worst = 0.0
    for b, ref in enumerate(_oracle(name)):
        nF = ref['f0'].shape[0]
        # padding frames: exact zeros in every output
        assert not f0[b, nF:].any() and not aper[b, nF:].any()
        assert not lag[b, nF:].any() and not cmnd[b, nF:].any()
        err = float(np.abs(cmnd[b, :nF].astype(np.float64) -
                           ref['cmnd']).max())
        worst = max(worst, err)
        assert (cmnd[b, :nF, 0] == 1.0).all()
        # silent frames, exactly
        s = ref['silent']
        assert (f0[b, :nF][s] == 0).all() and (aper[b, :nF][s] == 1).all()
        assert (lag[b, :nF][s] == 0).all() and (cmnd[b, :nF][s] == 1).all()
        dec = R.decisive_frames(ref, m, **kw)
        assert np.array_equal(lag[b, :nF][dec], ref['lag'][dec])
        assert np.array_equal(f0[b, :nF][dec] > 0, ref['voiced'][dec])
        assert np.abs(aper[b, :nF].astype(np.float64) -
                      ref['aper'])[dec].max(initial=0.0) <= m
        tol = R.f0_tol(ref, m, kw['sample_rate'])
        v = dec & ref['voiced']
        assert (np.abs(f0[b, :nF].astype(np.float64) - ref['f0'])[v] <=
                tol[v]).all()
        assert (f0[b, :nF][~(f0[b, :nF] > 0)] == 0).all()
        # (whatever the frame: aper is c' at the lag that was picked)
        loud = np.nonzero(~s)[0]
        assert np.array_equal(aper[b, loud], cmnd[b, loud, lag[b, loud]])
    print('%s: max |c\' - float64| = %.3g, bound %.3g' % (name, worst, m))
    assert worst <= m


@pytest.mark.parametrize('key', sorted(R.TIES))
def test_ties_are_exact(hip_lib, key):
    """Rows of which every c' is exactly 1 in the oracle (d = 0, or d the
    same for every lag) are exactly that on the device: c' all 1, unvoiced,
    the first lag of the range."""
    from wavenet import pitch
    t = pitch.PitchTracker(16000)
    kw = dict(R.DEFAULTS, sample_rate=16000)
    x = R.TIES[key]
    ref = R.track(x, **kw)
    p = t(x, return_cmnd=True)
    f0, aper, lag, cmnd = (v.cpu().numpy() for v in p)
    tie = (ref['cmnd'] == 1.0).all(1) & ~ref['silent']
    assert tie.sum() >= 1
    assert (cmnd[tie] == 1.0).all() and (f0[tie] == 0).all()
    assert (aper[tie] == 1.0).all() and (lag[tie] == t.tau_min).all()
    # the other rows (the clip's edges): y is 0 or 0.25, every d a sum of at
    # most 1024 times 1 / 16 and exact in float32 in any order, so c' is the
    # float64 quotient rounded to float32
    assert (np.abs(cmnd.astype(np.float64) - ref['cmnd']) <=
            2.0 ** -23 * np.abs(ref['cmnd'])).all()


@pytest.mark.parametrize('name', ['a', 'd1', 'c'])
def test_clip_in_a_batch_of_nan_equals_the_clip_alone(hip_lib, name):
    t = _tracker(name)
    x, lengths = R.make_audio(name)
    B, T = x.shape
    batch = _device(name)
    for b in range(B):
        n = T if lengths is None else lengths[b]
        alone = t(x[b, :n], return_cmnd=True)
        nF = t.num_frames(n)
        poisoned = np.full((B + 1, T), NAN, np.float32)
        poisoned[b, :n] = x[b, :n]
        ln = np.full(B + 1, T, np.int64)
        ln[b] = n
        inside = t(poisoned, ln, return_cmnd=True)
        for k in range(4):
            a = _bits(alone[k])
            assert np.array_equal(a, _bits(inside[k][b, :nF])), (b, k)
            assert np.array_equal(a, _bits(batch[k][b, :nF])), (b, k)
            assert not _bits(inside[k][b, nF:]).any()


@pytest.mark.parametrize('name', ['a', 'b'])
def test_padded_skewed_operand_and_cmnd_off(hip_lib, name):
    """ld = T + 3 with NaN in the gap columns and a base four bytes off a
    16-byte boundary; cmnd NULL: the same bits as the plain call."""
    t = _tracker(name)
    x, lengths = R.make_audio(name)
    B, T = x.shape
    F = t.num_frames(T)
    want = _device(name)
    ar = guard.Arena('cuda')
    audio = ar.place('audio', x, torch.float32, ld=T + 3, skew_bytes=4)
    assert audio.data_ptr() % 16 == 4 and audio.stride(0) == T + 3
    ln = None if lengths is None else ar.place(
        'lengths', np.asarray(lengths, np.int32), torch.int32, fill=(T, 1))
    out = [ar.place(n, (B, F), d, role='out') for n, d in
           (('f0', torch.float32), ('aper', torch.float32),
            ('lag', torch.int32))]
    cm = ar.place('cmnd', (B, F, t.tau_max + 1), torch.float32, role='out')
    for with_cmnd in (True, False):
        ar.reset()
        code = hip_lib.wn_pitch_track(
            audio.data_ptr(), None if ln is None else ln.data_ptr(), T + 3, B,
            T, t.hop, t.window, t.tau_min, t.tau_max, t.threshold, t.silence,
            t.sample_rate, out[0].data_ptr(), out[1].data_ptr(),
            out[2].data_ptr(), cm.data_ptr() if with_cmnd else None,
            torch.cuda.current_stream().cuda_stream)
        assert code == 0
        torch.cuda.synchronize()
        ar.check()
        for k in range(3):
            assert np.array_equal(_bits(out[k]), _bits(want[k])), k
        if with_cmnd:
            assert np.array_equal(_bits(cm), _bits(want[3]))
        else:                  # not written: what the arena placed there
            assert (_bits(cm) == guard.BODY32).all()
    # the front end's own switch
    p = t(x, lengths)
    assert p.cmnd is None
    for k in range(3):
        assert np.array_equal(_bits(p[k]), _bits(want[k]))


def test_one_clip_without_a_batch_dimension(hip_lib):
    t = _tracker('a')
    x, _ = R.make_audio('a')
    p = t(torch.from_numpy(x[0]).cuda().double(), return_cmnd=True)
    assert p.f0.shape == (24,) and p.cmnd.shape == (24, 268)
    assert p.f0.device.type == 'cuda' and p.voiced.dtype == torch.bool
    want = _device('a')
    for k in range(4):
        assert np.array_equal(_bits(p[k]), _bits(want[k][0]))


def test_channels_on_the_device_equal_the_cpu(hip_lib):
    from wavenet import pitch
    t = _tracker('a')
    x, lengths = R.make_audio('a')
    p = t(x, lengths)
    nf = [t.num_frames(n) for n in lengths]
    for nframes in (None, nf):
        dev = t.channels(p, nframes)
        assert dev.device.type == 'cuda' and dev.shape == (3, 24, 2)
        cpu = t.channels(pitch.Pitch(p.f0.cpu(), None, None, None), nframes)
        assert np.array_equal(_bits(dev), _bits(cpu))
        want = R.channels(p.f0.cpu().numpy(), t.fmin, t.fmax, nframes)
        assert np.allclose(dev.cpu().numpy(), want, rtol=1e-9, atol=0)
    assert float(dev[..., 1].sum()) >= 5 and float(dev[..., 0].max()) > 0.1
    # f0_error on the device: a track against itself, and against the CPU
    e = pitch.f0_error(p, p, nf)
    assert e.frames.device.type == 'cuda'
    s = e.summary()
    assert s['f0_rmse_cents'] == 0.0 and s['gross_pitch_error'] == 0.0
    assert s['vuv_error'] == 0.0 and s['frames'] == sum(nf)
    assert s['voiced_frames'] == int((p.f0 > 0).sum())
