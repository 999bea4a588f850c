"""The pitch path on the device (csrc/wn_pitch_path.hip) against
PitchPath.reference, bit for bit: lag, f0, aper and cost at the scan's edges
(G1), batch invariance (G2), the octave case end to end (G3), the max_bytes
grouping (G4) and NaN / Inf rows in one clip of a batch (G5)."""
import numpy as np
import pytest
import torch

import pitch_path_ref as R

pytestmark = pytest.mark.gpu

# (tau_min, tau_max): N = 2, 3, 4, 5 (inside one lane, across two), 63, 64,
# 65 (a wave's lanes), 255, 256, 257 (one wave / four waves), 1022 (the most)
LAGS = [(2, 4), (2, 5), (2, 6), (2, 7), (2, 65), (2, 66), (2, 67), (3, 258),
        (3, 259), (3, 260), (2, 1024)]
# (B, F, nframes)
BATCHES = [(1, 1, None), (3, 2, [2, 0, 1]), (1, 3, None), (3, 3, [1, 3, 2]),
           (3, 70, [70, 0, 33]), (1, 70, [69])]
TIES = dict(jump=0.0, octave_bias=0.0, switch=0.25, unvoiced=0.25)
# an unvoiced state dear enough that the path stays voiced at every N, so the
# voiced predecessors of both one-sided minima are walked at the small N too
WEIGHTS = {'ties': TIES, 'voiced': dict(unvoiced=1.9)}


def _path(tau_min=None, tau_max=None, **kw):
    from wavenet import pitch
    return pitch.PitchPath(R.tracker_with_lags(pitch, tau_min, tau_max), **kw)


def _rows(kind, seed, F, tau_max):
    if kind in ('random', 'voiced'):
        return R.random_rows(seed, F, tau_max, silent=0.2)
    if kind == 'ties':
        return R.random_rows(seed, F, tau_max, silent=0.2, quantum=0.25)
    c, lag = R.random_rows(seed, F, tau_max, silent=0.0)
    if kind == 'silent':
        lag[:] = 0
    else:                                       # alternating
        lag[::2] = 0
    c[lag == 0] = 1.0
    return c, lag


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]).numpy()


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and \
        np.array_equal(a.view('i%d' % a.itemsize), b.view('i%d' % b.itemsize))


def _expect(path, c, lag, nf):
    """Reference outputs of one clip with nf real frames of F."""
    F = c.shape[0]
    f0, aper = np.zeros(F, np.float32), np.zeros(F, np.float32)
    out, cost = np.zeros(F, np.int32), np.float64(0)
    if nf:
        p, cost = path.reference(c[:nf], lag[:nf])
        f0[:nf], aper[:nf], out[:nf] = p.f0, p.aper, p.lag
    return f0, aper, out, cost


# -------------------------------------------------------------------- G1
@pytest.mark.parametrize('kind', ['random', 'voiced', 'ties', 'silent',
                                  'alternating'])
@pytest.mark.parametrize('tau_min,tau_max', LAGS,
                         ids=['N%d' % (b - a) for a, b in LAGS])
def test_decode_is_the_reference_bit_for_bit(hip_lib, tau_min, tau_max, kind):
    path = _path(tau_min, tau_max, **WEIGHTS.get(kind, {}))
    runs = []
    for B, F, nfs in BATCHES:                   # launch all, then compare
        clips = [_rows(kind, 10 * F + b, F, tau_max) for b in range(B)]
        c = torch.from_numpy(np.stack([x[0] for x in clips])).cuda()
        lag = torch.from_numpy(np.stack([x[1] for x in clips])).cuda()
        p, cost = path.decode(c, lag, nfs, return_cost=True)
        assert cost is path.last_cost and p.cmnd is None
        runs.append((clips, F, nfs, p, cost))
    torch.cuda.synchronize()
    voiced = 0
    for clips, F, nfs, p, cost in runs:
        assert p.f0.shape == p.aper.shape == p.lag.shape == (len(clips), F)
        assert p.f0.dtype == torch.float32 and p.lag.dtype == torch.int32
        assert cost.dtype == torch.float64 and cost.shape == (len(clips),)
        for b, (cb, lb) in enumerate(clips):
            nf = F if nfs is None else nfs[b]
            f0, aper, out, J = _expect(path, cb, lb, nf)
            what = (kind, tau_max - tau_min, F, b, nf)
            assert np.array_equal(p.lag[b].cpu().numpy(), out), what
            assert _same(p.f0[b].cpu().numpy(), f0), what
            assert _same(p.aper[b].cpu().numpy(), aper), what
            assert _same(cost[b].cpu().numpy(), np.float64(J)), what
            voiced += int((out > 0).sum())
    if kind == 'silent':
        assert voiced == 0
    if kind == 'voiced':
        assert voiced >= 60


def test_one_clip_tensors_and_device_nframes(hip_lib):
    """[F] in, [F] out; nframes as a device tensor is clamped by the kernel
    to [0, F]."""
    path = _path(2, 40)
    c, lag = R.random_rows(3, 9, 40)
    cd, ld = torch.from_numpy(c).cuda(), torch.from_numpy(lag).cuda()
    p = path.decode(cd, ld)
    assert p.f0.shape == (9,) and path.last_cost.shape == (1,)
    f0, aper, out, J = _expect(path, c, lag, 9)
    assert np.array_equal(p.lag.cpu().numpy(), out)
    assert _same(p.f0.cpu().numpy(), f0) and _same(p.aper.cpu().numpy(), aper)
    both = torch.stack([cd, cd]), torch.stack([ld, ld])
    q = path.decode(*both, nframes=torch.tensor([-3, 12]).cuda())
    assert not q.lag[0].any() and not q.f0[0].any() and not q.aper[0].any()
    assert np.array_equal(q.lag[1].cpu().numpy(), out)
    assert path.last_cost.cpu().tolist() == [0.0, float(J)]


# -------------------------------------------------------------------- G2
@pytest.mark.parametrize('tau_min,tau_max', [(2, 42), (3, 260)])
def test_batch_invariance_bit_for_bit(hip_lib, tau_min, tau_max):
    path = _path(tau_min, tau_max)
    F = 20
    clips = [R.random_rows(50 + b, F, tau_max) for b in range(3)]
    c = torch.from_numpy(np.stack([x[0] for x in clips])).cuda()
    lag = torch.from_numpy(np.stack([x[1] for x in clips])).cuda()
    nfs = [F, 7, 13]
    full, cost = path.decode(c, lag, return_cost=True)
    cut, ccost = path.decode(c, lag, nfs, return_cost=True)
    for b in range(3):
        alone, acost = path.decode(c[b:b + 1], lag[b:b + 1], return_cost=True)
        for k in range(3):
            assert np.array_equal(_bits(alone[k][0]), _bits(full[k][b])), b
        assert np.array_equal(_bits(acost), _bits(cost[b:b + 1]))
        k = nfs[b]
        short, scost = path.decode(c[b:b + 1, :k].contiguous(),
                                   lag[b:b + 1, :k].contiguous(),
                                   return_cost=True)
        for j in range(3):
            assert np.array_equal(_bits(short[j][0]), _bits(cut[j][b, :k])), b
            assert not cut[j][b, k:].any()
        assert np.array_equal(_bits(scost), _bits(ccost[b:b + 1]))


# -------------------------------------------------------------------- G3
def test_octave_case_end_to_end(hip_lib):
    from wavenet import pitch
    tracker = pitch.PitchTracker(16000)
    path = pitch.PitchPath(tracker)
    x = R.octave_signal().astype(np.float32)
    raw = tracker(x, return_cmnd=True)
    p = path(x)
    assert p.cmnd is None and p.f0.shape == raw.f0.shape == (63,)
    rl, pl = raw.lag.cpu().numpy(), p.lag.cpu().numpy()
    up = int(((rl > 0) & (rl < 120)).sum())
    print('device raw track: %d frames an octave up; path: %d'
          % (up, ((pl > 0) & (pl < 120)).sum()))
    assert up >= 10
    assert not ((pl > 0) & (pl < 120)).any()
    # the device's own c' rows and lags through the numpy rule
    want, J = path.reference(raw.cmnd.cpu().numpy(), rl)
    assert np.array_equal(pl, want.lag)
    assert _same(p.f0.cpu().numpy(), want.f0)
    assert _same(p.aper.cpu().numpy(), want.aper)
    assert _same(path.last_cost.cpu().numpy(), np.array([J]))
    # and the conditioning channels take it as it stands
    ch = tracker.channels(p)
    assert ch.shape == (63, 2)
    assert torch.equal(ch[:, 1] > 0, p.f0 > 0)


# -------------------------------------------------------------------- G4
def test_max_bytes_grouping(hip_lib, monkeypatch):
    from wavenet import _lib, pitch
    tracker = pitch.PitchTracker(16000)
    rng = np.random.default_rng(8)
    t = np.arange(5000) / 16000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * f * t) for f in (110., 180., 260.)])
    x = (x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
    lengths = [5000, 3100, 4097]
    whole = pitch.PitchPath(tracker)
    F = tracker.num_frames(5000)
    one = pitch.PitchPath(tracker, max_bytes=whole.clip_bytes(F))
    two = pitch.PitchPath(tracker, max_bytes=2 * whole.clip_bytes(F) + 1)
    for n in (None, lengths):
        a = whole(x, n)
        ca = whole.last_cost
        for other in (one, two):
            b = other(x, n)
            assert b.cmnd is None and b.f0.shape == (3, F)
            for k in range(3):
                assert np.array_equal(_bits(a[k]), _bits(b[k]))
            assert np.array_equal(_bits(ca), _bits(other.last_cost))

    def boom(*a, **k):
        raise AssertionError('a launch')
    monkeypatch.setattr(_lib, 'call', boom)
    low = pitch.PitchPath(tracker, max_bytes=whole.clip_bytes(F) - 1)
    with pytest.raises(ValueError) as e:
        low(x)
    assert str(whole.clip_bytes(F)) in str(e.value)
    assert str(whole.clip_bytes(F) - 1) in str(e.value)


# -------------------------------------------------------------------- G5
@pytest.mark.parametrize('tau_min,tau_max', [(2, 42), (3, 260)])
def test_nan_and_inf_rows_stay_in_their_clip(hip_lib, tau_min, tau_max):
    path = _path(tau_min, tau_max)
    F = 16
    clips = [R.random_rows(70 + b, F, tau_max) for b in range(3)]
    c = np.stack([x[0] for x in clips])
    lag = torch.from_numpy(np.stack([x[1] for x in clips])).cuda()
    clean, cost = path.decode(torch.from_numpy(c).cuda(), lag,
                              return_cost=True)
    bad = c.copy()
    bad[1, 2] = np.nan
    bad[1, 5, ::3] = np.inf
    bad[1, 6, 1::2] = -np.inf
    bad[1, 9, tau_min + 1] = np.nan
    # (_lib.call raises on any code but WN_OK)
    got, gcost = path.decode(torch.from_numpy(bad).cuda(), lag,
                             return_cost=True)
    torch.cuda.synchronize()
    for b in (0, 2):
        for k in range(3):
            assert np.array_equal(_bits(got[k][b]), _bits(clean[k][b])), b
        assert np.array_equal(_bits(gcost[b:b + 1]), _bits(cost[b:b + 1]))
