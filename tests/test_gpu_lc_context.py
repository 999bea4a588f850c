"""The frame-context convolution in front of the learned LC upsampler on the
GPU: identity at initialisation (bitwise the model without context), loss,
rows and every gradient against the float64 restatement
(tests/lc_ctx_ref.py), window invariance, determinism and launch-plan replay,
learning what only context gives, generation, the CLIs and two data-parallel
ranks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ctx_ref
import lc_ref
from util import ROOT

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TOL = 2e-5     # of each variable's largest entry (the project's bar)
DIL = [1, 2, 4, 8, 16, 32, 64, 128, 1, 2]


def _model(B, Lc, scales, p, dil=DIL, biases=True, gc=None, seed=0, S=64,
           Q=64):
    from wavenet import WaveNetModel
    kw = {}
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    if p is not None:
        kw['local_condition_context'] = p
    return WaveNetModel(B, dil, 2, 32, 32, S, quantization_channels=Q,
                        use_biases=biases, seed=seed,
                        local_condition_channels=Lc,
                        local_condition_upsample_scales=tuple(scales), **kw)


def _randomise(net, seed, ctx=True):
    """Non-zero biases, LC weights large enough that the rows matter, random
    upsampler weights and (ctx) a random context filter; the draws of every
    other variable do not depend on whether the model has context."""
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_context/' in n:
                continue
            if '/lc_upsample/' in n:
                v.copy_((0.6 * torch.randn(v.shape, generator=g,
                                           dtype=torch.float64)).float())
            elif 'bias' in last:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
            elif last.startswith('lc_'):
                v.copy_(0.3 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
        if ctx and net.lc_ctx is not None:
            w = net.variables['lc_context']['filter']
            gc_ = torch.Generator().manual_seed(seed + 11)
            w.copy_((torch.randn(w.shape, generator=gc_, dtype=torch.float64)
                     / np.sqrt(w.shape[0] * w.shape[1])).float())


def _frames(B, T, Lc, hop, offs, seed, extra=0):
    """Exactly the frames the offsets need (extra = 0): the last frame's
    right context is the zero padding."""
    rng = np.random.default_rng(seed)
    F = int((max(offs) + T - 1) // hop + 1 + extra)
    return rng.standard_normal((B, F, Lc)).astype(np.float32)


def _codes(B, T, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, T)).astype(np.int32)


def test_identity_at_initialisation(hip_lib):
    """An untrained context filter is the identity: the loss, the rows and
    every gradient but the context filter's are bitwise those of the same
    model without context (B = 2, offsets 0 and near the clip's end, GC and
    biases), eager, recorded and replayed."""
    B, T, Lc, scales, hop = 2, 1003, 80, (4, 5), 20
    ctx = _model(B, Lc, scales, 2, gc=3, seed=4)
    plain = _model(B, Lc, scales, None, gc=3, seed=4)
    vp = dict(plain.named_variables())
    for n, v in ctx.named_variables():
        if '/lc_context/' not in n:
            assert torch.equal(v, vp[n]), n
    _randomise(ctx, 1)
    _randomise(plain, 1)
    with torch.no_grad():
        w = ctx.variables['lc_context']['filter']
        w.zero_()
        w[2] = torch.eye(Lc)
    offs = [0, 3 * hop + 7]
    frames = _frames(B, T, Lc, hop, offs, seed=3)
    q = torch.as_tensor(_codes(B, T, 64, 2)).cuda()
    ids = [0, 2]
    for _ in range(3):      # eager, recorded, replayed
        a = ctx.loss_from_codes(q, ids, local_condition_batch=frames,
                                local_condition_offset=offs)
        b = plain.loss_from_codes(q, ids, local_condition_batch=frames,
                                  local_condition_offset=offs)
        torch.cuda.synchronize()
        assert float(a) == float(b)
        gc_ = dict(ctx.named_variables(ctx.gradients))
        for n, g in plain.named_variables(plain.gradients):
            assert torch.equal(g, gc_[n]), n
        assert torch.equal(ctx._ws[(B, T, True)].lc,
                           plain._ws[(B, T, True)].lc)
        assert float(gc_['wavenet/lc_context/filter'].abs().max()) > 0
    r = ctx.upsample_local_condition(frames, T, offs)
    assert torch.equal(r, plain.upsample_local_condition(frames, T, offs))


def _bad_grads(got, ref):
    """Variables off by more than TOL of their largest entry.  An upsampler
    layer's one-float bias gradient is the plain sum of the d rows its filter
    gradient weighs, which can cancel far below them: it is held to its
    layer's largest entry."""
    bad = []
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        if k.startswith('/lc_upsample/') and k.endswith('/bias'):
            scale = max(scale, np.abs(ref[k[:-len('bias')] + 'filter']).max())
        err = np.abs(got[k] - ref[k]).max()
        if not err <= TOL * max(scale, 1e-30):
            bad.append((k, float(err), float(scale)))
    return bad


CASES = [
    # (p, scales, Lc, B, T, offsets, biases, gc)
    (0, (2,), 5, 2, 700, [0, 3], True, None),
    (1, (4, 5), 80, 2, 613, [7, 131], True, 3),
    (2, (2, 5, 4, 5), 80, 3, 900, [0, 417, 199], False, None),
    (8, (2, 5), 5, 1, 450, [33], True, None),
    (2, (4, 5), 200, 2, 500, [0, 19], True, 2),
    (8, (4, 5), 80, 2, 400, [5, 1], False, 3),
]


@pytest.mark.parametrize('case', CASES, ids=['p0_lc5', 'p1_lc80_gc',
                                             'p2_lc80_B3_nob', 'p8_lc5_B1',
                                             'p2_lc200_gc', 'p8_lc80_nob'])
def test_random_weights_match_float64(hip_lib, case):
    p, scales, Lc, B, T, offs, biases, gc = case
    hop = int(np.prod(scales))
    net = _model(B, Lc, scales, p, biases=biases, gc=gc, seed=Lc + B)
    _randomise(net, Lc + p)
    frames = _frames(B, T, Lc, hop, offs, seed=T)
    codes = _codes(B, T, 64, B + T)
    ids = None if gc is None else np.arange(B) % gc
    loss = float(net.loss_from_codes(torch.as_tensor(codes).cuda(), ids,
                                     local_condition_batch=frames,
                                     local_condition_offset=offs))
    torch.cuda.synchronize()
    ref_loss, ref_g = lc_ctx_ref.loss_and_grads(
        lc_ref.model_tree(net), DIL, codes, frames, offs, scales, gc_ids=ids,
        use_biases=biases, quantization_channels=64,
        relu_masks=lc_ref.device_relu_masks(net, B, T))
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
    ref = dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    assert '/lc_context/filter' in got
    assert np.abs(ref['/lc_context/filter']).max() > 0
    bad = _bad_grads(got, ref)
    assert not bad, bad[:6]
    rows = net.upsample_local_condition(frames, T, offs).cpu().numpy()
    want = lc_ctx_ref.rows_np(frames, offs, T, scales, lc_ref.model_tree(net))
    assert np.abs(rows - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


def test_window_invariance(hip_lib):
    """upsample_local_condition(frames, n, offset) is bitwise the matching
    slice of the whole-clip result, at both clip edges, whatever B; a clip
    inside a zero-padded batch gives the rows it gives alone."""
    scales, Lc, p = (2, 5, 4), 37, 3
    hop = 40
    net = _model(1, Lc, scales, p, seed=2)
    _randomise(net, 5)
    F = 30
    frames = np.random.default_rng(9).standard_normal((4, F, Lc)).astype(
        np.float32)
    whole = net.upsample_local_condition(frames, F * hop).cpu().numpy()
    for B in (1, 2, 4):
        for n, q in ((1, 0), (39, 1), (1000, 123), (333, F * hop - 333),
                     (1, F * hop - 1), (hop + 1, 0)):
            offs = [(q + 17 * b) % (F * hop - n + 1) for b in range(B)]
            if q in (0, F * hop - 333, F * hop - 1):
                offs[0] = q
            got = net.upsample_local_condition(frames[:B], n, offs)
            got = got.cpu().numpy()
            for b in range(B):
                assert np.array_equal(got[b], whole[b, offs[b]:offs[b] + n]), \
                    (B, n, offs[b])
    # clip 1 has 12 frames; padded with zeros to the batch's 30
    short = frames[1, :12]
    alone = net.upsample_local_condition(short, 12 * hop - 5, 5).cpu().numpy()
    padded = np.zeros((2, F, Lc), np.float32)
    padded[0] = frames[0]
    padded[1, :12] = short
    both = net.upsample_local_condition(padded, 12 * hop - 5,
                                        [100, 5]).cpu().numpy()
    assert np.array_equal(both[1], alone)
    assert np.array_equal(both[0], whole[0, 100:100 + 12 * hop - 5])


def test_determinism_and_replay(hip_lib):
    """Two identical calls give the same bucket bitwise; replays of the
    recorded launch plan fed new frames and offsets give the bits of a
    fresh model and match float64."""
    scales, Lc, B, T, p = (4, 5), 24, 2, 900, 2
    net = _model(B, Lc, scales, p, gc=3, seed=8)
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
        fresh = _model(B, Lc, scales, p, gc=3, seed=8)
        fresh.load_state_dict(net.state_dict())
        floss = float(fresh.loss_from_codes(torch.as_tensor(codes).cuda(),
                                            ids, local_condition_batch=frames,
                                            local_condition_offset=offs))
        torch.cuda.synchronize()
        assert loss == floss
        assert torch.equal(net.grads, fresh.grads), s
        ref_loss, ref_g = lc_ctx_ref.loss_and_grads(
            lc_ref.model_tree(net), DIL, codes, frames, offs, scales,
            gc_ids=ids, use_biases=True, quantization_channels=64,
            relu_masks=lc_ref.device_relu_masks(net, B, T))
        assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
        got = dict(lc_ref.flatten(lc_ref.model_tree(net, grads=True)))
        bad = _bad_grads(got, dict(lc_ref.flatten(ref_g)))
        assert not bad, (s, bad[:6])
    ws = net._ws[(B, T, True)]
    assert any(isinstance(pl, list) and len(pl) > 5 for pl in ws.plans.values())


def _softmax(x):
    x = x - x.max(-1, keepdims=True)
    e = np.exp(x)
    return e / e.sum(-1, keepdims=True)


def test_generation_on_context_rows(hip_lib):
    """predict_proba and teacher-forced fast generation on
    upsample_local_condition rows of a context model match float64."""
    scales, Lc, p = (2, 5), 16, 2
    net = _model(1, Lc, scales, p, gc=3, seed=3)
    _randomise(net, 3)
    T = 400
    frames = _frames(1, T, Lc, 10, [0], seed=4, extra=1)[0]
    rows = net.upsample_local_condition(frames, T - 1)
    var = lc_ref.model_tree(net)
    want = lc_ctx_ref.rows_np(frames[None], [0], T - 1, scales, var)[0]
    assert np.abs(rows.cpu().numpy() - want).max() < 1e-5 * max(
        1.0, np.abs(want).max())
    codes = _codes(1, T, 64, 5)[0]
    ref = _softmax(lc_ref.logits(var, DIL, codes[None, :T - 1], want[None],
                                 [2], True, 64))[0]
    out, pr = net.generate(0, seed_samples=codes, return_proba_every=1,
                           global_condition=[2], local_condition=rows)
    assert np.array_equal(out.cpu().numpy(), codes)
    assert np.abs(pr.cpu().numpy() - ref).max() < 1e-5
    for n in (T - 1, 200, 37):
        pp = net.predict_proba(codes[:n], [2],
                               local_condition=rows[:n]).cpu().numpy()
        assert np.abs(pp - ref[n - 1]).max() < 1e-5, n


def _next_frame_batch(rng, B, T, Lc, hop):
    """One-hot frames of random classes; the sample at timeline position
    u + 1 encodes the class of frame u // hop + 1 (the NEXT frame): the
    first prediction of every frame can only come from context."""
    offs = rng.integers(0, 2 * hop, B)
    F = (int(offs.max()) + T) // hop + 2
    cls = rng.integers(0, Lc, (B, F))
    frames = np.eye(Lc, dtype=np.float32)[cls]
    codes = np.zeros((B, T), np.int32)
    for b in range(B):
        u = offs[b] + np.arange(T - 1)
        codes[b, 1:] = 3 * cls[b, u // hop + 1] + 1
    return frames, offs, codes


def test_context_learns_the_next_frame(hip_lib):
    from wavenet import optimizer_factory
    scales, Lc, B, T, hop = (2,), 4, 4, 256, 2
    losses = {}
    moved = None
    for p in (None, 1):
        net = _model(B, Lc, scales, p, dil=[1, 2, 4, 8], seed=1, Q=16)
        w0 = None if p is None else net._seg(net.params, 'lc_ctx').clone()
        opt = optimizer_factory['adam'](learning_rate=0.01, momentum=0.9)
        rng = np.random.default_rng(0)
        ls = []
        for step in range(80):
            frames, offs, codes = _next_frame_batch(rng, B, T, Lc, hop)
            loss = net.loss_from_codes(torch.as_tensor(codes).cuda(),
                                       local_condition_batch=frames,
                                       local_condition_offset=offs)
            opt.minimize(loss)
            ls.append(float(loss))
        torch.cuda.synchronize()
        assert np.isfinite(ls).all()
        losses[p] = float(np.mean(ls[-10:]))
        if p is not None:
            moved = float((net._seg(net.params, 'lc_ctx') - w0).abs().max())
    # without context the first sample of every frame (half of them) stays
    # a guess among Lc classes
    assert losses[1] < 0.5 * losses[None], losses
    assert moved > 1e-2


SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}


def test_cli_train_resume_and_generate(hip_lib, tmp_path, capsys):
    import generate
    import train
    params = str(tmp_path / 'params.json')
    json.dump(SMALL, open(params, 'w'))
    logdir = str(tmp_path / 'run')
    base = ['--synthetic', '--lc_channels', '8', '--lc_upsample_scales', '2,5',
            '--lc_context', '2', '--sample_size', '2000', '--batch_size', '2',
            '--wavenet_params', params, '--logdir', logdir,
            '--checkpoint_every', '3', '--learning_rate', '0.002']
    assert train.main(base + ['--num_steps', '4']) == 0
    assert 'step 3 - loss = ' in capsys.readouterr().out
    ck = train.latest_checkpoint(logdir)
    sd = torch.load(ck, map_location='cpu')['variables']
    assert tuple(sd['wavenet/lc_context/filter'].shape) == (5, 8, 8)
    # resume: picks up the checkpoint (context filter included)
    assert train.main(base + ['--num_steps', '7']) == 0
    out = capsys.readouterr().out
    assert 'step 6 - loss = ' in out and 'step 0 - loss' not in out
    ck = train.latest_checkpoint(logdir)
    sd2 = torch.load(ck, map_location='cpu')['variables']
    assert not torch.equal(sd2['wavenet/lc_context/filter'],
                           sd['wavenet/lc_context/filter'])
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
                              '--lc_context', '2',
                              '--wav_out_path', wav,
                              '--logdir', str(tmp_path / 'gen')] + extra) == 0
        rate, data = wavfile.read(wav)
        assert rate == 16000 and data.shape == (1 + 10 * frames,)
        assert np.isfinite(data).all()
    capsys.readouterr()
    # a context flag that does not match the checkpoint
    for flag in (['--lc_context', '1'], []):
        assert generate.main([ck, '--wavenet_params', params,
                              '--fast_generation', 'false',
                              '--lc_path', str(tmp_path / 'f.npy'),
                              '--lc_upsample_scales', '2,5',
                              '--wav_out_path', str(tmp_path / 'x.wav')]
                             + flag) == 1
        assert 'lc_context' in capsys.readouterr().out


def test_two_ranks_keep_identical_context_weights(hip_lib, tmp_path):
    """Two data-parallel ranks (gloo, sharing this GPU), each on its shard of
    frames and offsets: after three Adam steps both hold the same parameters,
    context filter included, and the filter moved off the identity."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'rank%d.npz')
    spec = dict(mode='frames', B=4, T=300, steps=3, lc=12, scales=[4, 5], p=2,
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
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            pr.kill()
            o, _ = pr.communicate()
        outs.append(o.decode(errors='replace'))
    for pr, o in zip(procs, outs):
        assert pr.returncode == 0, o[-3000:]
    a, b = np.load(out % 0), np.load(out % 1)
    assert np.array_equal(a['params'], b['params'])
    assert np.array_equal(a['lc_ctx'], b['lc_ctx'])
    eye = np.zeros((5, 12, 12), np.float32)
    eye[2] = np.eye(12)
    assert np.abs(a['lc_ctx'].reshape(5, 12, 12) - eye).max() > 1e-4
