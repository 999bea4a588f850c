"""The learned local-conditioning upsampler on the GPU: bitwise repetition at
initialisation, loss and every gradient against the float64 restatement
(tests/lc_up_ref.py), window invariance of the rows, determinism and
launch-plan replay, generation on upsampled rows, learning, the CLIs and two
data-parallel ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ref
import lc_up_ref
from util import ROOT

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TOL = 2e-5     # of each variable's largest entry (the project's bar)
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2]


def _model(B, Lc, scales, dil=DIL, biases=True, gc=None, seed=0, S=64, Q=64):
    from wavenet import WaveNetModel
    kw = {}
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    if scales is not None:
        kw['local_condition_upsample_scales'] = tuple(scales)
    net = WaveNetModel(B, dil, 2, 32, 32, S, quantization_channels=Q,
                       use_biases=biases, seed=seed,
                       local_condition_channels=Lc, **kw)
    return net


def _randomise(net, seed, up=True):
    """Non-zero biases, LC weights large enough that the rows matter and
    (up) random upsampler weights."""
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_upsample/' in n:
                if up:
                    v.copy_((0.6 * torch.randn(v.shape, generator=g,
                                               dtype=torch.float64)).float())
            elif 'bias' in last:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
            elif last.startswith('lc_'):
                v.copy_(0.3 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())


def _frames(B, T, Lc, hop, offs, seed, extra=2):
    rng = np.random.default_rng(seed)
    F = int((max(offs) + T - 1) // hop + 1 + extra)
    return rng.standard_normal((B, F, Lc)).astype(np.float32)


def _codes(B, T, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, T)).astype(np.int32)


def test_bitwise_repetition_at_initialisation(hip_lib):
    """An untrained upsampler is repetition: the loss and every shared
    gradient are bitwise those of the plain LC model fed repeated rows on the
    same launches (B = 2, offsets 0 and hop - 1, T not a multiple of the
    hop, GC and biases), eager and replayed."""
    from wavenet.audio_reader import upsample_lc
    B, T, Lc, scales = 2, 1003, 80, (4, 5)
    hop = 20
    up = _model(B, Lc, scales, gc=3, seed=4)
    plain = _model(B, Lc, None, gc=3, seed=4)
    vp = dict(plain.named_variables())
    for n, v in up.named_variables():
        if '/lc_upsample/' not in n:
            assert torch.equal(v, vp[n]), n
    _randomise(up, 1, up=False)
    _randomise(plain, 1, up=False)
    offs = [0, hop - 1]
    frames = _frames(B, T, Lc, hop, offs, seed=3)
    rows = np.stack([upsample_lc(frames[b], hop, offs[b] + T)[offs[b]:]
                     for b in range(B)])
    q = torch.as_tensor(_codes(B, T, 64, 2)).cuda()
    ids = [0, 2]
    for _ in range(3):      # eager, recorded, replayed
        a = up.loss_from_codes(q, ids, local_condition_batch=frames,
                               local_condition_offset=offs)
        b = plain.loss_from_codes(q, ids, local_condition_batch=rows)
        torch.cuda.synchronize()
        assert float(a) == float(b)
        gu = dict(up.named_variables(up.gradients))
        for n, g in plain.named_variables(plain.gradients):
            assert torch.equal(g, gu[n]), n
        assert torch.equal(up._ws[(B, T, True)].lc, plain._ws[(B, T, True)].lc)
    r = up.upsample_local_condition(frames, T, offs).cpu().numpy()
    assert np.array_equal(r, rows)


CASES = [
    # (scales, Lc, B, T, offsets, biases, gc)
    ((2,), 5, 2, 700, [0, 3], True, None),
    ((4, 5), 80, 2, 613, [7, 131], True, 3),
    ((2, 5, 4, 5), 80, 2, 900, [0, 417], False, None),
    ((2, 5, 4, 5), 5, 3, 450, [199, 5, 0], True, None),
    ((4, 5), 5, 1, 800, [33], False, 2),
]


@pytest.mark.parametrize('case', CASES, ids=['s2_lc5', 's4x5_lc80_gc',
                                             's2x5x4x5_lc80_nob',
                                             's2x5x4x5_lc5_B3', 's4x5_lc5_B1'])
def test_random_weights_match_float64(hip_lib, case):
    scales, Lc, B, T, offs, biases, gc = case
    hop = int(np.prod(scales))
    net = _model(B, Lc, scales, biases=biases, gc=gc, seed=Lc + B)
    _randomise(net, Lc + len(scales))
    frames = _frames(B, T, Lc, hop, offs, seed=T)
    codes = _codes(B, T, 64, B + T)
    ids = None if gc is None else np.arange(B) % gc
    loss = float(net.loss_from_codes(torch.as_tensor(codes).cuda(), ids,
                                     local_condition_batch=frames,
                                     local_condition_offset=offs))
    torch.cuda.synchronize()
    ref_loss, ref_g = lc_up_ref.loss_and_grads(
        lc_ref.model_tree(net), DIL, codes, frames, offs, scales, gc_ids=ids,
        use_biases=biases, quantization_channels=64,
        relu_masks=lc_ref.device_relu_masks(net, B, T))
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
    ref = dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    assert any('lc_upsample' in k for k in got)
    bad = []
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        if not err <= TOL * max(scale, 1e-30):
            bad.append((k, float(err), float(scale)))
        if 'lc_upsample' in k and 'filter' in k:
            assert scale > 0, k
    assert not bad, bad[:6]
    # the rows themselves
    rows = net.upsample_local_condition(frames, T, offs).cpu().numpy()
    want = lc_up_ref.rows_np(frames, offs, T, scales,
                             lc_ref.model_tree(net)['lc_upsample'])
    assert np.abs(rows - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def test_window_invariance(hip_lib):
    """upsample_local_condition(frames, n, offset=p) is bitwise rows p .. p + n
    - 1 of the whole-clip result, whatever B, n and p."""
    scales, Lc = (2, 5, 4), 37
    hop = 40
    net = _model(1, Lc, scales, seed=2)
    _randomise(net, 5)
    F = 60
    frames = np.random.default_rng(9).standard_normal((4, F, Lc)).astype(
        np.float32)
    whole = net.upsample_local_condition(frames, F * hop).cpu().numpy()
    for B in (1, 2, 4):
        for n, p in ((1, 0), (39, 1), (1000, 123), (333, F * hop - 333)):
            offs = [(p + 17 * b) % (F * hop - n + 1) for b in range(B)]
            got = net.upsample_local_condition(frames[:B], n, offs)
            got = got.cpu().numpy()
            for b in range(B):
                assert np.array_equal(got[b], whole[b, offs[b]:offs[b] + n]), \
                    (B, n, offs[b])
    one = net.upsample_local_condition(frames[0], 77, 5).cpu().numpy()
    assert one.shape == (77, Lc)
    assert np.array_equal(one, whole[0, 5:82])


def test_determinism_and_replay(hip_lib):
    """Two identical calls give the same bucket bitwise; calls replaying the
    recorded launch plan with new frames and offsets match float64."""
    scales, Lc, B, T = (4, 5), 24, 2, 900
    net = _model(B, Lc, scales, gc=3, seed=8)
    _randomise(net, 8)
    assert net.use_launch_plans
    q = torch.as_tensor(_codes(B, T, 64, 1)).cuda()
    fr = _frames(B, T, Lc, 20, [3, 50], seed=1)
    buckets = []
    for _ in range(2):
        net.loss_from_codes(q, [0, 1], local_condition_batch=fr,
                            local_condition_offset=[3, 50])
        torch.cuda.synchronize()
        buckets.append(net.grads.clone())
    assert torch.equal(buckets[0], buckets[1])
    for s in range(3):
        offs = [11 * s, 400 + 7 * s]
        frames = _frames(B, T, Lc, 20, offs, seed=100 + s)
        codes = _codes(B, T, 64, 200 + s)
        ids = np.array([s % 3, (s + 1) % 3])
        loss = float(net.loss_from_codes(torch.as_tensor(codes).cuda(), ids,
                                         local_condition_batch=frames,
                                         local_condition_offset=offs))
        torch.cuda.synchronize()
        ref_loss, ref_g = lc_up_ref.loss_and_grads(
            lc_ref.model_tree(net), DIL, codes, frames, offs, scales,
            gc_ids=ids, use_biases=True, quantization_channels=64,
            relu_masks=lc_ref.device_relu_masks(net, B, T))
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
        got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
        for k, r in lc_ref.flatten(ref_g):
            assert np.abs(got[k] - r).max() <= TOL * max(np.abs(r).max(),
                                                         1e-30), (s, k)
    ws = net._ws[(B, T, True)]
    assert any(isinstance(p, list) and len(p) > 5 for p in ws.plans.values())


def _softmax(x):
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(-1, keepdims=True)


def test_generation_on_upsampled_rows(hip_lib):
    """predict_proba and teacher-forced fast generation on
    upsample_local_condition rows match float64 (rows and network)."""
    scales, Lc = (2, 5), 16
    net = _model(1, Lc, scales, gc=3, seed=3)
    _randomise(net, 3)
    T = 400
    frames = _frames(1, T, Lc, 10, [0], seed=4)[0]
    rows = net.upsample_local_condition(frames, T - 1)
    var = lc_ref.model_tree(net)
    want = lc_up_ref.rows_np(frames[None], [0], T - 1, scales,
                             var['lc_upsample'])[0]
    codes = _codes(1, T, 64, 5)[0]
    ref = _softmax(lc_ref.logits(var, DIL, codes[None, :T - 1], want[None],
                                 [2], True, 64))[0]
    out, p = net.generate(0, seed_samples=codes, return_proba_every=1,
                          global_condition=[2], local_condition=rows)
    assert np.array_equal(out.cpu().numpy(), codes)
    assert np.abs(p.cpu().numpy() - ref).max() < 1e-5
    for n in (T - 1, 200, 37):
        pp = net.predict_proba(codes[:n], [2],
                               local_condition=rows[:n]).cpu().numpy()
        assert np.abs(pp - ref[n - 1]).max() < 1e-5, n


def test_training_moves_the_upsampler(hip_lib):
    from wavenet import optimizer_factory
    scales, Lc, B, T = (2, 4), 4, 4, 256
    net = _model(B, Lc, scales, dil=[1, 2, 4, 8], seed=1, Q=16)
    up0 = net._seg(net.params, 'lc_up').clone()
    opt = optimizer_factory['adam'](learning_rate=0.01, momentum=0.9)
    rng = np.random.default_rng(0)
    losses = []
    for step in range(40):
        cls = rng.integers(0, Lc, (B, T // 8 + 2))
        frames = np.eye(Lc, dtype=np.float32)[cls]
        offs = rng.integers(0, 8, B)
        rows_cls = np.stack([np.repeat(cls[b], 8)[offs[b]:offs[b] + T]
                             for b in range(B)])
        codes = np.empty((B, T), np.int32)
        codes[:, 0] = 0
        codes[:, 1:] = 3 * rows_cls[:, :-1] + 1
        loss = net.loss_from_codes(torch.as_tensor(codes).cuda(),
                                   local_condition_batch=frames,
                                   local_condition_offset=offs)
        opt.minimize(loss)
        losses.append(float(loss))
    torch.cuda.synchronize()
    assert np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses
    moved = (net._seg(net.params, 'lc_up') - up0).abs().max()
    assert float(moved) > 1e-3


SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}


def test_cli_train_and_generate(hip_lib, tmp_path, capsys):
    import generate
    import train
    params = str(tmp_path / 'params.json')
    json.dump(SMALL, open(params, 'w'))
    logdir = str(tmp_path / 'run')
    assert train.main(['--synthetic', '--lc_channels', '8',
                       '--lc_upsample_scales', '2,5', '--sample_size', '2000',
                       '--batch_size', '2', '--wavenet_params', params,
                       '--logdir', logdir, '--checkpoint_every', '3',
                       '--num_steps', '4', '--learning_rate', '0.002']) == 0
    assert 'step 3 - loss = ' in capsys.readouterr().out
    ck = train.latest_checkpoint(logdir)
    sd = torch.load(ck, map_location='cpu')['variables']
    assert tuple(sd['wavenet/lc_upsample/layer1/filter'].shape) == (5, 3)
    frames = 30
    feats = np.random.default_rng(0).standard_normal((frames, 8)).astype(
        np.float32)
    np.save(str(tmp_path / 'f.npy'), feats)
    for fast in ('false', 'true'):
        wav = str(tmp_path / ('out_%s.wav' % fast))
        extra = ['--fast_generation', 'false'] if fast == 'false' else \
            ['--lc_fast_generation', 'true']
        assert generate.main([ck, '--wavenet_params', params,
                              '--lc_path', str(tmp_path / 'f.npy'),
                              '--lc_upsample_scales', '2,5',
                              '--wav_out_path', wav,
                              '--logdir', str(tmp_path / 'gen')] + extra) == 0
        rate, data = wavfile.read(wav)
        assert rate == 16000 and data.shape == (1 + 10 * frames,)
        assert np.isfinite(data).all()
    capsys.readouterr()
    # a scales flag that does not match the checkpoint
    assert generate.main([ck, '--wavenet_params', params, '--fast_generation',
                          'false', '--lc_path', str(tmp_path / 'f.npy'),
                          '--lc_upsample_scales', '10',
                          '--wav_out_path', str(tmp_path / 'x.wav')]) == 1
    assert 'lc_upsample' in capsys.readouterr().out


def test_two_ranks_keep_identical_upsampler_weights(hip_lib, tmp_path):
    """Two data-parallel ranks (gloo, sharing this GPU), each on its shard of
    frames and offsets: after three Adam steps both hold the same parameters,
    upsampler included, and the upsampler moved."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'rank%d.npz')
    spec = dict(mode='frames', B=4, T=300, steps=3, lc=12, scales=[4, 5],
                lr=1e-2, overlap=True, out=out)
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2',
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0', WN_SHARE_GPU='1',
                   WN_DIST_BACKEND='gloo')
        procs.append(subprocess.Popen(
            [sys.executable, os.path.join(HERE, 'dp_worker.py'),
             json.dumps(spec)], env=env, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        outs.append(o.decode(errors='replace'))
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = np.load(out % 0), np.load(out % 1)
    assert np.array_equal(a['params'], b['params'])
    assert np.array_equal(a['lc_up'], b['lc_up'])
    from wavenet import WaveNetModel
    init = WaveNetModel(2, [1], 2, 32, 32, 64, use_biases=True, device='cpu',
                        local_condition_channels=12,
                        local_condition_upsample_scales=(4, 5))
    up0 = init._seg(init.params, 'lc_up').numpy()
    assert np.abs(a['lc_up'] - up0).max() > 1e-4
