"""wn_stoi on the device against the float64 restatement (tests/stoi_ref.py):
kept frames and segments exactly, a clip's scores within 4 x the larger of the
largest distance of two float32 numpy evaluations from float64 and one float32
ulp -- for M = 29, 30, 31 and 65 kept frames with frames removed at the start,
in the middle and at the end, at 16 kHz and at 10 kHz; ragged batches clip by
clip, generated is original, a NaN's confinement, StoiSums.cat and summary()."""
import numpy as np
import pytest
import torch

import stoi_ref as S

pytestmark = pytest.mark.gpu

_meters, _cases = {}, {}


def _meter(rate):
    from wavenet import stoi
    if rate not in _meters:
        _meters[rate] = stoi.Stoi(rate)
    return _meters[rate]


def _case(M, rate):
    """(generated, original, the restatement's result, the bounds): computed
    once, shared and left unchanged."""
    key = (M, rate)
    if key not in _cases:
        meter = _meter(rate)
        x = S.fixture(M, rate)
        y = S.degraded(x, 0.1, seed=M)
        want = S.stoi64(y, x, meter.resampler)
        assert want['kept'] == M and S.decisive(want['margin'])
        tol = {}
        if want['segments']:
            ref = meter.reference(y, x)
            assert ref['kept'] == M
            alt = S.alt32(y, x, meter.resampler, want['keep'])
            for key_, other in (('stoi', alt[0]), ('estoi', alt[1])):
                tol[key_] = S.bound(want[key_], [
                    ref[key_ + '_sum'] / ref['segments'], other])
        _cases[key] = (y, x, want, tol)
    return _cases[key]


def _host(sums):
    return [t.cpu().numpy() for t in sums]


def _bits(sums):
    st, es, sg, kp = _host(sums)
    return (st.view(np.int64).tolist(), es.view(np.int64).tolist(),
            sg.tolist(), kp.tolist())


def _check_clip(st, es, sg, kp, want, tol, what):
    assert (int(kp), int(sg)) == (want['kept'], want['segments']), what
    if not want['segments']:
        assert st.tobytes() == es.tobytes() == np.float64(0.0).tobytes()
        return 0.0
    worst = 0.0
    for key, got in (('stoi', float(st) / int(sg)),
                     ('estoi', float(es) / int(sg))):
        err = abs(got - want[key])
        print('%s %s: device %.9f, float64 %.9f, error %.3e, bound %.3e, '
              'ratio %.3f' % (what, key, got, want[key], err, tol[key],
                              err / tol[key]))
        assert err <= tol[key], (what, key)
        worst = max(worst, err / tol[key])
    return worst


@pytest.mark.parametrize('M,rate', [(29, 16000), (30, 16000), (31, 16000),
                                    (65, 16000), (31, 10000)])
def test_scores_against_the_restatement(hip_lib, M, rate):
    y, x, want, tol = _case(M, rate)
    sums = _meter(rate)(y, x)
    st, es, sg, kp = _host(sums)
    assert st.shape == es.shape == sg.shape == kp.shape == (1,)
    assert st.dtype == np.float64 and sg.dtype == np.int32
    _check_clip(st[0], es[0], sg[0], kp[0], want, tol, 'M %d at %d' % (M, rate))
    assert sums.frames.tolist() == [want['frames']]


def test_ragged_batch_clip_by_clip(hip_lib):
    meter = _meter(16000)
    cases = [_case(65, 16000), _case(31, 16000), _case(29, 16000)]
    n = [len(c[0]) for c in cases] + [0, 1]
    T = max(n) + 37
    g = np.full((5, T), np.nan, np.float32)      # poison behind n[b]
    o = np.full((5, T), np.nan, np.float32)
    for b, c in enumerate(cases):
        g[b, :n[b]], o[b, :n[b]] = c[0], c[1]
    g[4, 0], o[4, 0] = 0.25, 0.5
    sums = meter(g, o, n)
    st, es, sg, kp = _host(sums)
    for b, c in enumerate(cases):
        _check_clip(st[b], es[b], sg[b], kp[b], c[2], c[3], 'clip %d' % b)
    assert sg[3:].tolist() == [0, 0] and kp[3:].tolist() == [0, 0]
    assert not st[3:].view(np.int64).any() and not es[3:].view(np.int64).any()
    assert sums.frames.tolist() == [c[2]['frames'] for c in cases] + [0, 0]
    # each clip alone, at its own T, and in another order: the same bits
    whole = _bits(sums)
    for b in (0, 1, 2, 4):
        alone = _bits(meter(g[b, :n[b]], o[b, :n[b]]))
        assert [v[0] for v in alone] == [v[b] for v in whole], b
    order = [2, 0, 4, 1]
    again = _bits(meter(g[order], o[order], [n[b] for b in order]))
    assert again == tuple([v[b] for b in order] for v in whole)


def test_generated_is_original(hip_lib):
    for rate in (16000, 10000):
        _, x, want, _ = _case(31, rate)
        t = torch.from_numpy(x).cuda()
        st, es, sg, kp = _host(_meter(rate)(t, t))
        assert (int(kp[0]), int(sg[0])) == (31, 2)
        assert abs(st[0] / sg[0] - 1) < 1e-12 and abs(es[0] / sg[0] - 1) < 1e-12


def test_a_nan_stays_in_its_clip(hip_lib):
    meter = _meter(16000)
    cases = [_case(31, 16000), _case(65, 16000), _case(30, 16000)]
    n = [len(c[0]) for c in cases]
    T = max(n)
    g = np.zeros((3, T), np.float32)
    o = np.zeros((3, T), np.float32)
    for b, c in enumerate(cases):
        g[b, :n[b]], o[b, :n[b]] = c[0], c[1]
    clean = _bits(meter(g, o, n))
    g2, o2 = g.copy(), o.copy()
    g2[1, n[1] // 2] = np.nan
    o2[1, n[1] // 3] = np.nan
    dirty = _bits(meter(g2, o2, n))
    for b in (0, 2):
        assert [v[b] for v in dirty] == [v[b] for v in clean]


def test_cat_and_summary(hip_lib):
    from wavenet import stoi
    meter = _meter(16000)
    cases = [_case(65, 16000), _case(29, 16000), _case(31, 16000),
             _case(30, 16000)]
    parts = []
    for group in ([0, 1], [2], [3]):
        n = [len(cases[b][0]) for b in group]
        g = np.zeros((len(group), max(n)), np.float32)
        o = np.zeros_like(g)
        for j, b in enumerate(group):
            g[j, :n[j]], o[j, :n[j]] = cases[b][0], cases[b][1]
        parts.append(meter(g, o, n))
    got = stoi.StoiSums.cat(parts).summary()
    want = S.corpus([c[2] for c in cases])
    assert set(got) == set(want) == {
        'stoi', 'estoi', 'clips', 'skipped_clips', 'segments', 'kept_frames',
        'frames', 'sample_rate'}
    for k in want:
        if k not in ('stoi', 'estoi'):
            assert got[k] == want[k], k
    for k in ('stoi', 'estoi'):
        tol = max(c[3][k] for c in cases if c[3])
        print('corpus %s: device %.9f, float64 %.9f, bound %.3e'
              % (k, got[k], want[k], tol))
        assert abs(got[k] - want[k]) <= tol
    assert (got['clips'], got['skipped_clips']) == (3, 1)
    with pytest.raises(ValueError):
        parts[0].__class__(*(t[1:] for t in parts[0]),
                           frames=parts[0].frames[1:]).summary()
