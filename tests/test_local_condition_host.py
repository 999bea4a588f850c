"""Local conditioning without a GPU: constructor / shape errors before any
device is touched, the flat bucket's LC segment, the reader's upsampling /
trimming / piece alignment, CLI parsing, argument validation of the new entry
points, and the float64 restatement (tests/lc_ref.py) against the project's
oracle where there is no LC."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ref
from util import O, ROOT, TINY, cfg_with, flat_named

sys.path.insert(0, ROOT)


def _net(lc=None, **kw):
    from wavenet import WaveNetModel
    args = dict(batch_size=2, dilations=[1, 2, 4, 8], filter_width=2,
                residual_channels=32, dilation_channels=32, skip_channels=64,
                quantization_channels=256, use_biases=True, device='cpu')
    args.update(kw)
    return WaveNetModel(**args, local_condition_channels=lc)


def test_keyword_only_and_default_none():
    from wavenet import WaveNetModel
    import inspect
    for fn, name in [(WaveNetModel.__init__, 'local_condition_channels'),
                     (WaveNetModel.loss, 'local_condition_batch'),
                     (WaveNetModel.loss_from_codes, 'local_condition_batch'),
                     (WaveNetModel.predict_proba, 'local_condition')]:
        p = inspect.signature(fn).parameters[name]
        assert p.kind == p.KEYWORD_ONLY and p.default is None, (fn, name)


@pytest.mark.parametrize('kw, what', [
    (dict(residual_channels=64), 'more than 32'),
    (dict(dilation_channels=48), 'more than 32'),
    (dict(filter_width=3), 'filter_width 3'),
    (dict(scalar_input=True), 'scalar_input'),
])
def test_unsupported_family_raises_at_construction(kw, what, monkeypatch):
    from wavenet import _lib
    # nothing may reach the library or a device first
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('library touched'))
    monkeypatch.setattr(_lib, 'require_gpu',
                        lambda: pytest.fail('device touched'))
    with pytest.raises(NotImplementedError, match=what) as e:
        _net(lc=8, device=None, **kw)
    assert 'filter_width 2' in str(e.value) and 'channels <= 32' in str(e.value)


@pytest.mark.parametrize('bad', [0, -3, 2.5, True, 'x'])
def test_bad_channel_count(bad):
    with pytest.raises((ValueError, TypeError)):
        _net(lc=bad)


def test_bucket_segments_with_and_without_lc():
    a, b = _net(), _net(lc=5)
    L = 4
    assert b.Lc == 5 and b.Lcp == 8 and a.Lc == 0
    # layer blocks unchanged; the LC segment sits between them and skip_w
    assert a.layer_stride == b.layer_stride
    for k in ('causal', 'layers'):
        assert a.segments[k] == b.segments[k]
    lo, n = b.segments['lc_w']
    assert n == 8 * L * 64
    assert lo == a.segments['skip_w'][0]
    assert b.segments['skip_w'][0] == lo + n
    assert 'lc_w' not in a.segments
    assert b.params.numel() == a.params.numel() + n
    for k in ('skip_w', 'skip_b', 'post1_w', 'post2_w', 'post1_b', 'post2_b'):
        assert b.segments[k][0] == a.segments[k][0] + n
    # (the data-parallel tail all-reduce starts at skip_w: LC is in the head)
    from wavenet import parallel
    assert parallel.tail_start(b) == lo + n
    # views: [Lc, D] filter | gate columns of layer l, padding zero
    lcw = b._seg(b.params, 'lc_w').view(8, L, 64)
    for l, cur in enumerate(b.variables['dilated_stack']):
        assert tuple(cur['lc_filtweights'].shape) == (5, 32)
        assert cur['lc_filtweights'].data_ptr() == lcw[0, l, 0].data_ptr()
        assert cur['lc_gateweights'].data_ptr() == lcw[0, l, 32].data_ptr()
        assert float(cur['lc_filtweights'].abs().max()) > 0
    assert int(torch.count_nonzero(lcw[5:])) == 0
    # same seed: every shared variable has the values of the model without LC
    va = dict(a.named_variables())
    names = [n for n, _ in b.named_variables()]
    assert 'wavenet/dilated_stack/layer2/lc_filter' in names
    assert 'wavenet/dilated_stack/layer2/lc_gate' in names
    for n, v in b.named_variables():
        if n in va:
            assert torch.equal(v, va[n]), n
    assert len(names) == len(va) + 2 * L


def test_l2_mask_covers_lc_weights():
    b = _net(lc=3)
    b.tf_bias_name_quirk = False
    m = b._l2_mask()
    o, n = b.segments['lc_w']
    assert float(m[o:o + n].min()) == 1.0
    tree = b._views(m)
    assert float(tree['dilated_stack'][0]['filter_bias'].max()) == 0.0


def test_shape_errors_before_any_launch():
    net = _net(lc=4)
    net._check_supported = lambda: None        # (a CPU model: stop before launches)
    with pytest.raises(ValueError, match='required'):
        net._lc_rows(None, 2, 10, 'loss')
    with pytest.raises(ValueError, match=r'\[2, 10, 4\]'):
        net._lc_rows(np.zeros((2, 10, 5), np.float32), 2, 10, 'loss')
    with pytest.raises(ValueError, match='shape'):
        net._lc_rows(np.zeros((2, 9, 4), np.float32), 2, 10, 'loss')
    plain = _net()
    with pytest.raises(ValueError, match='without local'):
        plain._lc_rows(np.zeros((2, 10, 4), np.float32), 2, 10, 'loss')
    # the public calls: the checks run before the workspace / device
    for call in (lambda: net.loss(np.zeros((2, 10), np.float32)),
                 lambda: net.predict_proba(np.zeros((2, 10), np.int32)),
                 lambda: net.predict_proba(np.zeros((2, 10), np.int32),
                                           local_condition=np.zeros((2, 3, 4)))):
        with pytest.raises(ValueError):
            call()
    plain._check_supported = lambda: None
    with pytest.raises(ValueError, match='without local'):
        plain.loss(np.zeros((2, 10), np.float32),
                   local_condition_batch=np.zeros((2, 10, 4), np.float32))
    net.stack_bwd = False
    with pytest.raises(NotImplementedError, match='stack_fwd / stack_bwd'):
        net.loss(np.zeros((2, 10), np.float32),
                 local_condition_batch=np.zeros((2, 10, 4), np.float32))


def test_fast_generation_refuses_lc_models_before_the_device():
    net = _net(lc=4, batch_size=1)
    for c in (lambda: net.generate(10), lambda: net.reset_generator(),
              lambda: net.predict_proba_incremental([3]),
              lambda: net.prime_generator([1, 2]),
              lambda: net.continue_generation(4, 3),
              lambda: net.generate_batch(4, [1, 2]),
              lambda: net.continue_generation_batch(4, [1, 2], [1, 2])):
        with pytest.raises(NotImplementedError, match='predict_proba'):
            c()


def test_restatement_matches_oracle_without_lc():
    """tests/lc_ref.py with lc=None is the project's float64 oracle: plainly,
    with residual_postproc, and with L2 under either bias-name setting (loss,
    every gradient and the logits)."""
    cfg = cfg_with(TINY, batch_size=2)
    var = O.create_variables(cfg, seed=3, dtype=np.float64, bias_scale=0.1)
    # (the model holds float32: the oracle gets the same rounded weights)
    r32 = lambda t: ({k: r32(v) for k, v in t.items()} if isinstance(t, dict)
                     else [r32(v) for v in t] if isinstance(t, list)
                     else np.asarray(t, np.float32).astype(np.float64))
    var = r32(var)
    audio = np.random.default_rng(5).uniform(-1, 1, (2, 50)).astype(np.float32)
    net = _net(batch_size=2, dilations=cfg['dilations'], residual_channels=8,
               dilation_channels=8, skip_channels=16, quantization_channels=16)
    net.load_nested(var)
    codes = O.mu_law_encode(audio, 16)
    # (residual_postproc, l2, tf_bias_name_quirk)
    for rp, l2, quirk in ((False, None, True), (True, None, True),
                          (False, 0.05, True), (False, 0.05, False),
                          (True, 0.05, False)):
        c = cfg_with(cfg, residual_postproc=rp)
        ref_loss, ref_g = O.loss_and_grads(c, var, audio, l2=l2,
                                           dtype=np.float64,
                                           tf_bias_name_quirk=quirk)
        ref_logits = O.loss(c, var, audio, dtype=np.float64,
                            keep=True)[1]['logits']
        loss, g, lg = lc_ref.loss_and_grads(
            lc_ref.model_tree(net), cfg['dilations'], np.asarray(codes), None,
            use_biases=True, quantization_channels=16, residual_postproc=rp,
            l2=l2, tf_bias_name_quirk=quirk, return_logits=True)
        assert abs(loss - ref_loss) < 1e-9, (rp, l2, quirk)
        got = dict(flat_named(g))
        for n, r in flat_named(ref_g):
            assert np.abs(got[n] - r).max() <= 1e-9 * max(1.0, np.abs(r).max()), \
                (rp, l2, quirk, n)
        assert np.abs(lg - ref_logits).max() < 1e-9
        fwd = lc_ref.logits(lc_ref.model_tree(net), cfg['dilations'],
                            np.asarray(codes), None, use_biases=True,
                            quantization_channels=16, residual_postproc=rp)
        assert np.array_equal(fwd, lg)
    # the L2 term itself: with the quirk off the biases leave it
    la = lc_ref.loss_and_grads(lc_ref.model_tree(net), cfg['dilations'],
                               np.asarray(codes), None, use_biases=True,
                               quantization_channels=16, l2=0.05)[0]
    lb = lc_ref.loss_and_grads(lc_ref.model_tree(net), cfg['dilations'],
                               np.asarray(codes), None, use_biases=True,
                               quantization_channels=16, l2=0.05,
                               tf_bias_name_quirk=False)[0]
    nb = sum((a ** 2).sum() / 2 for n, a in flat_named(var)
             if 'bias' in n.split('/')[-1])
    assert nb > 0 and abs((la - lb) - 0.05 * nb) < 1e-12


# ---- entry points: argument validation without launching -------------------
def test_lc_entry_points_validate_arguments(hip_lib):
    from wavenet import _lib
    lib = hip_lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.addressof(buf)
    p16 = p + (-p) % 16
    flags = (ctypes.c_uint * 64)()
    fp = ctypes.addressof(flags)
    v32 = _lib.stack_variant(rows=32)
    v16 = _lib.stack_variant(rows=16)
    fwd = lambda lc, stride, L=2, variant=v32, B=1, T=32: lib.wn_stack_fwd_lc(
        p16, p16, None, p16, None, 0, 0, fp, fp, fp, None, L, B, T, 0,
        variant, lc, stride, None)
    bwd = lambda lc, stride, L=2, variant=v32: lib.wn_stack_bwd_lc(
        p16, p16, p16, p16, p16, 0, p16, p16, p16, 1 << 20, None, fp, fp, fp,
        None, L, 1, 32, variant, lc, stride, None)
    for f in (fwd, bwd):
        assert f(None, 128) == -5                    # WN_ERR_NULL
        assert f(p16 + 4, 128) == -3                 # misaligned
        assert f(p16, 127) == -1                     # stride < 64 L
        assert f(p16, 130) == -1                     # stride % 4
        assert f(p16, 128, L=0) == -1
        assert f(p16, 128, variant=v16) == -2        # 16-row tiles: unsupported


# ---- reader ----------------------------------------------------------------
def _write_clip(d, name, audio, feats, sr=16000):
    wavfile.write(os.path.join(d, name + '.wav'), sr,
                  (audio * 32767).astype(np.int16))
    np.save(os.path.join(d, name + '.npy'), feats)


def test_reader_upsampling_and_trimming_keep_features_beside_samples(tmp_path):
    from wavenet.audio_reader import (load_lc, trim_bounds, trim_silence,
                                      trim_silence_lc)
    hop, frames, Lc = 40, 250, 3
    T = hop * frames
    t = np.arange(T)
    audio = (0.5 * np.sin(2 * np.pi * 440 * t / 16000)).astype(np.float32)
    audio[:3000] = 0.0            # leading silence (trimmed)
    audio[-2500:] = 0.0           # trailing silence
    feats = np.arange(frames * Lc, dtype=np.float32).reshape(frames, Lc)
    _write_clip(str(tmp_path), 'a', audio, feats)
    up = load_lc(str(tmp_path / 'a.npy'), hop, T, Lc)
    assert up.shape == (T, Lc)
    for i in (0, 39, 40, 41, T - 1):
        assert np.array_equal(up[i], feats[i // hop])
    a2, l2 = trim_silence_lc(audio, up, 0.01)
    lo, hi = trim_bounds(audio, 0.01)
    assert 0 < lo < hi < T
    assert np.array_equal(a2, trim_silence(audio, 0.01))
    assert np.array_equal(a2, audio[lo:hi]) and np.array_equal(l2, up[lo:hi])
    # features shorter than the audio by less than one frame: the last frame
    # is repeated; more is an error, as is a channel mismatch
    u2 = load_lc(str(tmp_path / 'a.npy'), hop, T + 17, Lc)
    assert u2.shape == (T + 17, Lc) and np.array_equal(u2[-1], feats[-1])
    with pytest.raises(ValueError):
        load_lc(str(tmp_path / 'a.npy'), hop, T + hop + 1, Lc)
    with pytest.raises(ValueError):
        load_lc(str(tmp_path / 'a.npy'), hop, T, Lc + 1)


def test_reader_pieces_carry_their_own_feature_rows(tmp_path):
    from wavenet import AudioReader
    hop, frames, Lc, piece = 16, 200, 2, 500
    T = hop * frames
    rng = np.random.default_rng(0)
    audio = rng.uniform(-0.9, 0.9, T).astype(np.float32)
    # feature column 0 = the frame index, column 1 = its square
    fi = np.arange(frames, dtype=np.float32)
    _write_clip(str(tmp_path), 'clip', audio, np.stack([fi, fi ** 2], 1))
    reader = AudioReader(str(tmp_path), None, sample_rate=16000,
                         gc_enabled=False, sample_size=piece,
                         silence_threshold=None, lc_channels=Lc, lc_hop=hop)
    pieces = list(reader.iter_pieces())
    assert [p.shape[0] for p, _, _ in pieces] == [500] * 6 + [200]
    start = 0
    for wav, _, lc in pieces:
        n = wav.shape[0]
        idx = np.arange(start, start + n)
        assert lc.shape == (n, Lc)
        assert np.allclose(wav.reshape(-1), audio[idx], atol=1e-4)
        assert np.array_equal(lc[:, 0], (idx // hop).astype(np.float32))
        assert np.array_equal(lc[:, 1], ((idx // hop) ** 2).astype(np.float32))
        start += n
    # the queue: dequeue, then dequeue_lc for the same pieces
    reader.start_threads()
    try:
        a = reader.dequeue(2)
        lc = reader.dequeue_lc(2)
        assert tuple(lc.shape) == (2, a.shape[1], Lc)
        with pytest.raises(ValueError):
            reader.dequeue_lc(2)
    finally:
        reader.coord.request_stop()
        reader.coord.join(reader.threads)
    with pytest.raises(ValueError, match='lc_hop'):
        AudioReader(str(tmp_path), None, 16000, False, lc_channels=2)
    os.remove(str(tmp_path / 'clip.npy'))
    with pytest.raises(ValueError, match='no features'):
        AudioReader(str(tmp_path), None, 16000, False, lc_channels=2, lc_hop=4)


# ---- CLI --------------------------------------------------------------------
def test_cli_parsing():
    import train
    import generate
    a = train.get_arguments(['--synthetic', '--lc_channels', '80',
                             '--lc_hop', '200'])
    assert a.lc_channels == 80 and a.lc_hop == 200
    a = train.get_arguments(['--synthetic'])
    assert a.lc_channels is None
    g = generate.get_arguments(['ckpt', '--fast_generation', 'false',
                                '--lc_path', 'f.npy', '--lc_hop', '80'])
    assert g.lc_path == 'f.npy' and g.lc_hop == 80 and not g.fast_generation
    g = generate.get_arguments(['ckpt'])
    assert g.lc_path is None


def test_generate_needs_naive_path_for_lc(tmp_path, capsys):
    import generate
    np.save(str(tmp_path / 'f.npy'), np.zeros((4, 3), np.float32))
    rc = generate.main([str(tmp_path / 'model.ckpt-1'), '--lc_path',
                        str(tmp_path / 'f.npy')])
    assert rc != 0
    assert '--fast_generation false' in capsys.readouterr().out
