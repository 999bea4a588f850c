"""The learned local-conditioning upsampler without a GPU: argument errors
before any library or device is touched, the bucket segment, views, names,
L2 mask and initial values, the float64 restatement (tests/lc_up_ref.py)
against a brute-force loop and repetition, the reader's frames mode, the
frames / offset validation and the CLIs' flags."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_up_ref
from util import ROOT

sys.path.insert(0, ROOT)


def _net(lc=8, scales=(4, 5), **kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=2, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args, local_condition_channels=lc,
                        local_condition_upsample_scales=scales)


def test_keyword_only_and_defaults():
    from wavenet import WaveNetModel
    for fn, name, default in [
            (WaveNetModel.__init__, 'local_condition_upsample_scales', None),
            (WaveNetModel.loss, 'local_condition_offset', 0),
            (WaveNetModel.loss_from_codes, 'local_condition_offset', 0)]:
        p = inspect.signature(fn).parameters[name]
        assert p.kind == p.KEYWORD_ONLY and p.default == default, (fn, name)
    p = inspect.signature(WaveNetModel.upsample_local_condition).parameters
    assert list(p) == ['self', 'frames', 'num_samples', 'offset']
    assert p['offset'].default == 0


@pytest.mark.parametrize('lc, scales, exc, what', [
    (None, (4, 5), ValueError, 'needs local_condition_channels'),
    (8, (), ValueError, '1 to 8'),
    (8, (1,), ValueError, '>= 2'),
    (8, (4, 1, 5), ValueError, '>= 2'),
    (8, (2.0,), ValueError, 'ints'),
    (8, (True, 2), ValueError, 'ints'),
    (8, (2,) * 9, ValueError, '1 to 8'),
    (8, (64, 128), ValueError, 'at most 4096'),
    (8, 5, ValueError, 'tuple'),
    (8, ('4',), ValueError, 'ints'),
    (513, (4, 5), NotImplementedError, 'at most 512'),
])
def test_bad_arguments_raise_at_construction(lc, scales, exc, what,
                                             monkeypatch):
    from wavenet import _lib
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    with pytest.raises(exc, match=what):
        _net(lc=lc, scales=scales, device=None)


def test_good_scales_accepted():
    for sc in [(2,), (4096,), (2,) * 8, [4, 5, 10], (np.int64(3), 7)]:
        net = _net(scales=sc)
        assert net.lc_hop == int(np.prod(sc))
        assert net.local_condition_upsample_scales == tuple(int(s) for s in sc)
    assert _net(lc=512).Lc == 512


def test_bucket_layout():
    from wavenet import parallel
    plain = _net(scales=None)
    for biases in (True, False):
        a = _net(scales=None, use_biases=biases)
        b = _net(scales=(4, 5, 10), use_biases=biases)
        lo, n = b.segments['lc_up']
        assert n == 3 * 19 + (3 if biases else 0)
        assert lo == b.segments['lc_w'][0] + b.segments['lc_w'][1]
        assert b.segments['skip_w'][0] >= lo + n
        assert b.segments['skip_w'][0] < lo + n + 32
        assert parallel.tail_start(b) == b.segments['skip_w'][0]
        assert 'lc_up' not in a.segments
        for k in ('causal', 'layers', 'lc_w'):
            assert a.segments[k] == b.segments[k]
    # models without the argument keep every offset
    assert plain.segments == _net(scales=None).segments


def test_views_names_init_and_l2_mask():
    net = _net(scales=(4, 5, 10))
    up = net.variables['lc_upsample']
    assert [tuple(c['filter'].shape) for c in up] == [(4, 3), (5, 3), (10, 3)]
    assert all(tuple(c['bias'].shape) == (1,) for c in up)
    names = [n for n, _ in net.named_variables() if '/lc_upsample/' in n]
    assert names == ['wavenet/lc_upsample/layer%d/%s' % (i, k)
                     for i in range(3) for k in ('filter', 'bias')]
    for c in up:
        f = c['filter']
        assert torch.equal(f, torch.tensor([[0.0, 1.0, 0.0]]).expand_as(f))
        assert float(c['bias']) == 0.0
    # views into the flat bucket
    lo, n = net.segments['lc_up']
    with torch.no_grad():
        up[1]['filter'][2, 0] = 7.0
        up[2]['bias'][0] = -3.0
    seg = net.params[lo:lo + n]
    assert float(seg[3 * 4 + 3 * 2]) == 7.0
    assert float(seg[-1]) == -3.0
    # L2 mask: filters in, biases out
    m = net._views(net._l2_mask())
    for c in m['lc_upsample']:
        assert bool((c['filter'] == 1).all()) and float(c['bias']) == 0.0
    # no biases: no bias views, names or floats
    nb = _net(scales=(2, 3), use_biases=False)
    assert all('bias' not in c for c in nb.variables['lc_upsample'])
    assert nb.segments['lc_up'][1] == 15


def test_no_rng_consumed_and_state_dict_round_trip():
    plain = _net(scales=None)
    net = _net(scales=(2, 5, 4))
    vp = dict(plain.named_variables())
    for n, v in net.named_variables():
        if '/lc_upsample/' not in n:
            assert torch.equal(v, vp[n]), n
    with torch.no_grad():
        for c in net.variables['lc_upsample']:
            c['filter'].normal_()
            c['bias'].normal_()
    sd = net.state_dict()
    assert 'wavenet/lc_upsample/layer2/filter' in sd
    other = _net(scales=(2, 5, 4))
    other.load_state_dict(sd)
    assert torch.equal(other.params, net.params)


def _ref_weights(scales, seed, biases=True):
    rng = np.random.default_rng(seed)
    f = [rng.standard_normal((s, 3)) for s in scales]
    b = [rng.standard_normal(1) for _ in scales] if biases else None
    return f, b


@pytest.mark.parametrize('scales', [(2,), (4, 5), (2, 5, 4, 5), (3, 2, 2)])
def test_ref_matches_brute_force(scales):
    hop = int(np.prod(scales))
    Lc, T = 6, 3 * hop + 7
    rng = np.random.default_rng(len(scales))
    offs = [0, hop - 1]
    frames = rng.standard_normal((2, (hop + T - 2) // hop + 1, Lc))
    for biases in (True, False):
        f, b = _ref_weights(scales, hop, biases)
        got = lc_up_ref.rows(torch.as_tensor(frames), offs, T, scales,
                             [torch.as_tensor(x) for x in f],
                             None if b is None else
                             [torch.as_tensor(x) for x in b]).numpy()
        for i in range(2):
            want = lc_up_ref.brute_force(frames[i], offs[i], T, scales, f,
                                         None if b is None else
                                         [float(x[0]) for x in b])
            assert np.abs(got[i] - want).max() < 1e-12


def test_ref_at_initialisation_is_repetition():
    from wavenet.audio_reader import upsample_lc
    scales, Lc = (2, 5, 4), 7
    net = _net(lc=Lc, scales=scales)
    from util import tree_to_numpy
    var = tree_to_numpy(net.variables)
    frames = np.random.default_rng(0).standard_normal((2, 9, Lc)).astype(
        np.float32)
    T, offs = 250, [13, 39]
    got = lc_up_ref.rows_np(frames, offs, T, scales, var['lc_upsample'])
    for b in range(2):
        want = upsample_lc(frames[b], 40, offs[b] + T)[offs[b]:]
        assert np.array_equal(got[b], want.astype(np.float64))


def test_frames_and_offset_validation():
    net = _net(lc=8, scales=(4, 5))           # hop 20
    B, T = 2, 100
    ok = np.zeros((B, 6, 8), np.float32)     # covers offsets 0 .. 20
    fr, off = net._lc_frames(ok, 19, B, T, 'loss')
    assert off.tolist() == [19, 19]
    fr, off = net._lc_frames(ok, [0, 5], B, T, 'loss')
    assert off.dtype == np.int64
    for bad, offset, what in [
            (None, 0, r'\[B, F, Lc\] = \[2, F, 8\]'),
            (np.zeros((B, 6, 7), np.float32), 0, r'\[B, F, Lc\] = \[2, F, 8\]'),
            (np.zeros((3, 6, 8), np.float32), 0, 'shape'),
            (np.zeros((B, 6, 8), np.int32), 0, 'float'),
            (ok, 21, 'do not cover'),
            (ok, [0, 25], 'do not cover'),
            (ok, -1, 'non-negative'),
            (ok, [1, 2, 3], 'int or 2 ints'),
            (ok, 1.5, 'int or 2 ints'),
            (ok, True, 'int or 2 ints')]:
        with pytest.raises(ValueError, match=what):
            net._lc_frames(bad, offset, B, T, 'loss')
    # a model without the upsampler refuses an offset
    plain = _net(scales=None)
    with pytest.raises(ValueError, match='local_condition_upsample_scales'):
        plain._lc_input(np.zeros((B, T, 8), np.float32), 3, B, T, 'loss')


def _corpus(tmp_path, Lc, hop):
    rng = np.random.default_rng(1)
    sr = 16000
    for i, n in enumerate([21000, 9000, 30000]):
        audio = np.zeros(n, np.float32)
        lo, hi = 2600 + 500 * i, n - 3100
        audio[lo:hi] = 0.3 * rng.standard_normal(hi - lo)
        wavfile.write(str(tmp_path / ('c%d.wav' % i)), sr, audio)
        # (the last frame falls short of the clip by less than one hop)
        frames = n // hop
        np.save(str(tmp_path / ('c%d.npy' % i)),
                rng.standard_normal((frames, Lc)).astype(np.float32))


def test_reader_frames_mode_matches_row_mode(tmp_path):
    from wavenet.audio_reader import AudioReader, upsample_lc
    Lc, hop = 5, 40
    _corpus(tmp_path, Lc, hop)
    kw = dict(sample_rate=16000, gc_enabled=False, sample_size=4000,
              silence_threshold=0.01, seed=3, lc_channels=Lc, lc_hop=hop)
    rows = list(AudioReader(str(tmp_path), None, **kw).iter_pieces())
    frames = list(AudioReader(str(tmp_path), None, lc_frames=True,
                              **kw).iter_pieces())
    assert len(rows) == len(frames) > 6
    some_trim = False
    for (pa, _, lr), (pb, _, (fr, off)) in zip(rows, frames):
        n = pa.shape[0]
        assert np.array_equal(pa, pb)
        up = upsample_lc(fr, hop, off + n)[off:off + n]
        assert np.array_equal(up, lr)
        some_trim |= off % 4000 != 0
    assert some_trim


def test_reader_frames_dequeue(tmp_path):
    from wavenet.audio_reader import AudioReader
    Lc, hop = 5, 40
    _corpus(tmp_path, Lc, hop)
    r = AudioReader(str(tmp_path), None, 16000, False, sample_size=4000,
                    silence_threshold=0.01, seed=3, lc_channels=Lc,
                    lc_hop=hop, lc_frames=True)
    r.start_threads()
    try:
        audio = r.dequeue(3)
        fr, off = r.dequeue_lc_frames(3)
    finally:
        r.coord.request_stop()
    assert audio.shape[0] == 3 and fr.shape[0] == 3 and fr.shape[2] == Lc
    assert off.dtype == torch.int64 and off.shape == (3,)
    for i in range(3):
        assert (int(off[i]) + audio.shape[1] - 1) // hop < fr.shape[1]
    with pytest.raises(ValueError, match='dequeue_lc_frames'):
        r.dequeue_lc(3)


def test_train_cli_scales():
    import train
    args = train.get_arguments(['--synthetic', '--lc_channels', '8',
                                '--lc_upsample_scales', '4,5,10'])
    assert train.lc_upsample_scales(args) == ((4, 5, 10), 200)
    args = train.get_arguments(['--synthetic', '--lc_channels', '8',
                                '--lc_upsample_scales', '4,5,10',
                                '--lc_hop', '200'])
    assert train.lc_upsample_scales(args) == ((4, 5, 10), 200)
    args = train.get_arguments(['--synthetic', '--lc_channels', '8'])
    assert train.lc_upsample_scales(args) == (None, None)
    for argv, what in [
            (['--lc_hop', '100'], 'disagrees'),
            (['--lc_upsample_scales', '4,x'], 'comma-separated'),
            (['--lc_channels', None], 'needs --lc_channels')]:
        base = ['--synthetic', '--lc_channels', '8', '--lc_upsample_scales',
                '4,5,10']
        if argv[0] == '--lc_channels':
            base = base[:1] + base[3:]
            argv = []
        elif argv[0] == '--lc_upsample_scales':
            base = base[:3]
        with pytest.raises(ValueError, match=what):
            train.lc_upsample_scales(train.get_arguments(base + argv))


def test_train_main_refuses_disagreeing_hop(capsys, tmp_path):
    import train
    assert train.main(['--synthetic', '--lc_channels', '8',
                       '--lc_upsample_scales', '2,5', '--lc_hop', '7',
                       '--logdir', str(tmp_path / 'run')]) == 1
    assert 'disagrees' in capsys.readouterr().out
    assert not os.path.exists(str(tmp_path / 'run'))


def test_synthetic_reader_frames():
    import train
    r = train.SyntheticReader(300, lc_channels=6, lc_hop=20)
    r.dequeue(4)
    fr, off = r.dequeue_lc_frames(4)
    assert fr.shape[0] == 4 and fr.shape[2] == 6 and off.shape == (4,)
    assert int(off.min()) >= 0 and int(off.max()) < 80
    assert (int(off.max()) + 299) // 20 < fr.shape[1]


def test_generate_cli_flag_and_mismatch_message():
    import generate
    a = generate.get_arguments(['ck', '--lc_path', 'f.npy',
                                '--lc_upsample_scales', '2,5'])
    assert a.lc_upsample_scales == '2,5'
    net = _net(lc=8, scales=(2, 5))
    sd = net.state_dict()
    assert generate.upsampler_mismatch(net, sd) is None
    msg = generate.upsampler_mismatch(_net(lc=8, scales=(10,)), sd)
    assert 'lc_upsample' in msg and '2,5' in msg and '10' in msg
    msg = generate.upsampler_mismatch(_net(lc=8, scales=None), sd)
    assert 'none' in msg
