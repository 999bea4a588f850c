"""The frame-context convolution in front of the learned LC upsampler without
a GPU: argument errors before any library or device is touched, the bucket
segment, view, name, L2 mask and identity initialisation, the float64
restatement (tests/lc_ctx_ref.py) against a brute-force loop, the staging
window and the CLIs' flags."""
import inspect
import sys

import numpy as np
import pytest
import torch

import lc_ctx_ref
from util import ROOT

sys.path.insert(0, ROOT)


def _net(lc=8, scales=(4, 5), p=2, **kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=2, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args, local_condition_channels=lc,
                        local_condition_upsample_scales=scales,
                        local_condition_context=p)


def test_keyword_only_with_default_none():
    from wavenet import WaveNetModel
    p = inspect.signature(WaveNetModel.__init__).parameters[
        'local_condition_context']
    assert p.kind == p.KEYWORD_ONLY and p.default is None
    assert WaveNetModel.LC_CONTEXT_MAX == 8


@pytest.mark.parametrize('scales, p, what', [
    (None, 2, 'needs local_condition_upsample_scales'),
    (None, 0, 'needs local_condition_upsample_scales'),
    ((4, 5), -1, 'from 0 to 8'),
    ((4, 5), 9, 'from 0 to 8'),
    ((4, 5), True, 'from 0 to 8'),
    ((4, 5), False, 'from 0 to 8'),
    ((4, 5), 2.0, 'from 0 to 8'),
    ((4, 5), '2', 'from 0 to 8'),
    ((4, 5), np.bool_(True), 'from 0 to 8'),
])
def test_bad_arguments_raise_at_construction(scales, p, what, monkeypatch):
    from wavenet import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    with pytest.raises(ValueError, match=what):
        _net(scales=scales, p=p, device=None)


def test_good_values_accepted():
    for p in (0, 1, 8, np.int64(3)):
        net = _net(p=p)
        assert net.local_condition_context == int(p)
        assert type(net.local_condition_context) is int
    assert _net(p=None).local_condition_context is None


def test_bucket_layout():
    from wavenet import parallel
    for biases in (True, False):
        for Lc, p in ((8, 2), (5, 0), (80, 8)):
            a = _net(lc=Lc, p=None, use_biases=biases)
            b = _net(lc=Lc, p=p, use_biases=biases)
            lo, n = b.segments['lc_ctx']
            assert n == (2 * p + 1) * Lc * Lc
            up = b.segments['lc_up']
            assert up == a.segments['lc_up']
            assert lo >= up[0] + up[1] and lo < up[0] + up[1] + 32
            assert b.segments['skip_w'][0] >= lo + n
            assert b.segments['skip_w'][0] < lo + n + 32
            assert parallel.tail_start(b) == b.segments['skip_w'][0]
            assert 'lc_ctx' not in a.segments
            for k in ('causal', 'layers', 'lc_w', 'lc_up'):
                assert a.segments[k] == b.segments[k]
            # skip_w and what follows keep their sizes and order
            tail = ['skip_w', 'skip_b', 'post1_w', 'post2_w', 'post1_b',
                    'post2_b']
            d = b.segments['skip_w'][0] - a.segments['skip_w'][0]
            for k in tail:
                assert b.segments[k] == (a.segments[k][0] + d,
                                         a.segments[k][1])
            assert b.params.numel() == a.params.numel() + d
    # models without the argument keep every offset
    assert _net(p=None).segments == _net(p=None).segments


def test_view_name_identity_init_and_l2_mask():
    net = _net(lc=6, p=2)
    w = net.variables['lc_context']['filter']
    assert tuple(w.shape) == (5, 6, 6)
    want = torch.zeros(5, 6, 6)
    want[2] = torch.eye(6)
    assert torch.equal(w, want)
    names = [n for n, _ in net.named_variables()]
    assert 'wavenet/lc_context/filter' in names
    i = names.index('wavenet/lc_context/filter')
    assert names[i - 1].startswith('wavenet/lc_upsample/')
    assert names[i + 1].startswith('wavenet/postprocessing/')
    # a view into the bucket in [K][Cin][Cout] order
    lo, n = net.segments['lc_ctx']
    with torch.no_grad():
        w[3, 1, 4] = 7.0
    assert float(net.params[lo + (3 * 6 + 1) * 6 + 4]) == 7.0
    g = net.gradients['lc_context']['filter']
    assert g.data_ptr() == net.grads[lo:].data_ptr()
    # L2 mask: a filter, so in
    m = net._views(net._l2_mask())
    assert bool((m['lc_context']['filter'] == 1).all())


def test_no_rng_consumed_and_state_dict_round_trip():
    plain = _net(p=None)
    net = _net(p=3)
    vp = dict(plain.named_variables())
    names = set()
    for n, v in net.named_variables():
        names.add(n)
        if n != 'wavenet/lc_context/filter':
            assert torch.equal(v, vp[n]), n
    assert names - set(vp) == {'wavenet/lc_context/filter'}
    with torch.no_grad():
        net.variables['lc_context']['filter'].normal_()
    sd = net.state_dict()
    assert tuple(sd['wavenet/lc_context/filter'].shape) == (7, 8, 8)
    other = _net(p=3)
    other.load_state_dict(sd)
    assert torch.equal(other.params, net.params)


@pytest.mark.parametrize('p', [0, 1, 2, 4])
def test_ref_matches_brute_force(p):
    rng = np.random.default_rng(p)
    Lc = 5
    for nf in (1, 3, 2 * p + 4):
        frames = rng.standard_normal((2, nf, Lc))
        W = rng.standard_normal((2 * p + 1, Lc, Lc))
        got = lc_ctx_ref.context(torch.as_tensor(frames),
                                 torch.as_tensor(W)).numpy()
        for b in range(2):
            want = lc_ctx_ref.brute_force(frames[b], W)
            assert np.abs(got[b] - want).max() < 1e-12, (p, nf)


def test_ref_identity_is_the_frames():
    frames = torch.as_tensor(np.random.default_rng(0).standard_normal(
        (2, 7, 4)))
    W = torch.zeros(5, 4, 4, dtype=torch.float64)
    W[2] = torch.eye(4, dtype=torch.float64)
    assert torch.equal(lc_ctx_ref.context(frames, W), frames)


def _staged(net, fr, off, T, Fx):
    """local_condition.stage over the window of offsets `off` (no frame
    cover check: the window runs past the clip on purpose)."""
    from wavenet import local_condition
    win = local_condition.window(net, off, fr.shape[1], T)
    dst = torch.full((fr.shape[0], Fx, fr.shape[2]), -1.0)
    dst_off = torch.zeros(fr.shape[0], dtype=torch.int32)
    local_condition.stage(net, local_condition.Frames(fr, off, T, *win), dst,
                          dst_off)
    return dst, dst_off, win


def test_stage_frames_fill_rules():
    """Both fill rules of the staging window: zero rows outside the clip
    with context (p = 0 included), the clamp to frame F - 1 without."""
    from wavenet import local_condition
    net = _net(lc=3, scales=(2, 5), p=2)          # hop 10
    fr = torch.arange(2 * 12 * 3, dtype=torch.float32).view(2, 12, 3) + 1
    T = 35
    Fw = local_condition.frame_window(net, T)
    assert Fw == 5                                 # (35 + 8) // 10 + 1
    # clip 0 near offset 0: window frames -2 .. 6; clip 1 near its last
    # frame: offset 87 -> frames 6 .. 14 of 12
    dst, off, (idx, inside) = _staged(net, fr, np.array([0, 87]), T, Fw + 4)
    assert off.tolist() == [0, 7]
    assert idx.tolist() == [list(range(-2, 7)), list(range(6, 15))]
    assert inside[0].tolist() == [False] * 2 + [True] * 7
    assert inside[1].tolist() == [True] * 6 + [False] * 3
    assert torch.equal(dst[0, :2], torch.zeros(2, 3))
    assert torch.equal(dst[0, 2:], fr[0, 0:7])
    assert torch.equal(dst[1, :6], fr[1, 6:12])
    assert torch.equal(dst[1, 6:], torch.zeros(3, 3))
    # p = 0: the window without context, zero rows past the clip (no clamp)
    net0 = _net(lc=3, scales=(2, 5), p=0)
    dst0, _, _ = _staged(net0, fr, np.array([0, 87]), T, Fw)
    assert torch.equal(dst0[0], fr[0, :5])
    assert torch.equal(dst0[1, :4], fr[1, 8:12])
    assert torch.equal(dst0[1, 4], torch.zeros(3))
    # a model without context keeps its clamp: clip 1 takes frames 8 .. 11
    # (12 frames: the window's last entry is clamped)
    plain = _net(lc=3, scales=(2, 5), p=None)
    dstp, offp, _ = _staged(plain, fr, np.array([0, 87]), T, Fw)
    assert offp.tolist() == [0, 7]
    assert torch.equal(dstp[0], fr[0, :5])
    assert torch.equal(dstp[1, :4], fr[1, 8:12])
    assert torch.equal(dstp[1, 4], fr[1, 11])


def test_train_cli_flag():
    import train
    base = ['--synthetic', '--lc_channels', '8', '--lc_upsample_scales',
            '4,5,10']
    assert train.get_arguments(base).lc_context is None
    assert train.lc_context(train.get_arguments(base)) is None
    assert train.lc_context(train.get_arguments(
        base + ['--lc_context', '2'])) == 2
    with pytest.raises(ValueError, match='needs --lc_upsample_scales'):
        train.lc_context(train.get_arguments(
            ['--synthetic', '--lc_channels', '8', '--lc_context', '2']))
    with pytest.raises(ValueError, match='from 0 to 8'):
        train.lc_context(train.get_arguments(base + ['--lc_context', '9']))


def test_train_main_refuses_context_without_upsampler(capsys, tmp_path):
    import os
    import train
    assert train.main(['--synthetic', '--lc_channels', '8', '--lc_hop', '10',
                       '--lc_context', '1',
                       '--logdir', str(tmp_path / 'run')]) == 1
    assert 'needs --lc_upsample_scales' in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / 'run'))


def test_generate_cli_flag_and_mismatch_message():
    import generate
    a = generate.get_arguments(['ck', '--lc_path', 'f.npy',
                                '--lc_upsample_scales', '2,5',
                                '--lc_context', '2'])
    assert a.lc_context == 2
    assert generate.get_arguments(['ck']).lc_context is None
    sd = _net(lc=8, scales=(2, 5), p=2).state_dict()
    assert generate.context_mismatch(_net(lc=8, scales=(2, 5), p=2),
                                     sd) is None
    msg = generate.context_mismatch(_net(lc=8, scales=(2, 5), p=1), sd)
    assert 'lc_context' in msg and 'P = 2' in msg and 'P = 1' in msg
    msg = generate.context_mismatch(_net(lc=8, scales=(2, 5), p=None), sd)
    assert 'lc_context' in msg and 'none' in msg
    sd0 = _net(lc=8, scales=(2, 5), p=None).state_dict()
    msg = generate.context_mismatch(_net(lc=8, scales=(2, 5), p=0), sd0)
    assert 'none' in msg and 'P = 0' in msg
    assert generate.context_mismatch(_net(lc=8, scales=(2, 5), p=None),
                                     sd0) is None


def test_generate_refuses_context_without_upsampler(capsys, tmp_path):
    import generate
    np.save(str(tmp_path / 'f.npy'), np.zeros((3, 8), np.float32))
    assert generate.main(['ck', '--lc_path', str(tmp_path / 'f.npy'),
                          '--fast_generation', 'false', '--lc_hop', '10',
                          '--lc_context', '1']) == 1
    assert 'needs --lc_upsample_scales' in capsys.readouterr().out
