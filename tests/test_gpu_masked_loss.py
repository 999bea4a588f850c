"""The masked loss on the GPU (`lengths` on WaveNetModel.loss /
loss_from_codes, csrc/wn_loss.hip's xent_masked_kernel): parity with the
float64 masked reference (tests/masked_ref.py) on every kind of model, full
lengths bitwise the unmasked loss, the padding's content irrelevant, the last
real row's target not the padding, launch-plan replay with new lengths,
loss_denominator, determinism, and train.py --mask_padding end to end.

Bars: those of tests/test_gpu_local_condition.py -- the loss within 1e-5
relative, every gradient within TOL = 2e-5 of its variable's largest entry."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import lc_ctx_ref
import lc_ref
import masked_ref
from util import O, ROOT, TINY, cfg_with, build_pair, flat_named, tree_to_numpy

sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5     # of each variable's largest entry (the project's bar)
DIL = [1, 2, 4, 8, 16, 32, 64, 1, 2, 4]


def _model(B, Q=256, biases=True, gc=None, Lc=None, R=32, S=64, dil=DIL,
           seed=0, rows=None, **extra):
    from wavenet import WaveNetModel, _lib
    kw = dict(extra)
    if gc:
        kw.update(global_condition_channels=gc, global_condition_cardinality=gc)
    net = WaveNetModel(B, dil, 2, R, R, S, quantization_channels=Q,
                       use_biases=biases, seed=seed,
                       local_condition_channels=Lc, **kw)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for n, v in net.named_variables():
            last = n.split('/')[-1]
            if '/lc_upsample/' in n or '/lc_context/' in n:
                v.copy_((0.5 * torch.randn(v.shape, generator=g,
                                           dtype=torch.float64)
                         / np.sqrt(max(v.shape[0], 1))).float())
            elif 'bias' in last:
                v.copy_(0.1 * torch.randn(v.shape, generator=g,
                                          dtype=torch.float64).float())
    if rows is not None:
        net.stack_variant = _lib.stack_variant(rows=rows)
    return net


def _codes(B, T, Q, seed):
    return np.random.default_rng(seed).integers(0, Q, (B, T)).astype(np.int32)


def _assert_close(tag, loss, grads, ref_loss, ref_g):
    """The bars of this file's docstring; prints every figure first."""
    got, ref = dict(lc_ref.flatten(grads)), dict(lc_ref.flatten(ref_g))
    assert sorted(got) == sorted(ref)
    print('%s: loss %.9g reference %.9g relative error %.3g'
          % (tag, loss, ref_loss, abs(loss - ref_loss) / max(1.0, abs(ref_loss))))
    worst = (0.0, None)
    for k in sorted(ref):
        scale = max(np.abs(ref[k]).max(), 1e-30)
        worst = max(worst, (np.abs(got[k] - ref[k]).max() / scale, k))
    print('%s: worst gradient error %.3g of the largest entry (%s), bar %g'
          % (tag, worst[0], worst[1], TOL))
    assert abs(loss - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss)), \
        (loss, ref_loss)
    assert max(np.abs(a).max() for a in ref.values()) > 0
    for k in sorted(ref):
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        assert err <= TOL * max(scale, 1e-30), (tag, k, err, scale)


def _assert_rows(net, B, T, rows):
    ws = net._ws[(B, T, True)]
    assert ws.stack_bwd and ws.stack_rows == rows, (ws.stack_rows, rows)


# ---- parity with the float64 masked reference --------------------------------
# (name, model keywords, T, lengths, tile rows of the stack launches or None,
#  float audio through loss() instead of codes through loss_from_codes())
CASES = [
    ('q256_bias_rows16', dict(Q=256, biases=True, rows=16), 300,
     [300, 141, 1], 16, False),
    ('q64_nobias_gc_rows32_audio', dict(Q=64, biases=False, gc=3, rows=32),
     330, [330, 2, 200], 32, True),
    ('q256_nobias_rows32', dict(Q=256, biases=False, rows=32), 400,
     [77, 400], 32, False),
    ('lc_rows_gc_bias', dict(Q=256, biases=True, gc=2, Lc=20), 400,
     [123, 400, 1], 32, False),
    ('lc_rows_q64_nobias', dict(Q=64, biases=False, Lc=80), 260,
     [260, 2], 32, True),
    # more than 32 channels: the channel-block kernels (wavenet/blocked.py)
    ('blocked_r64', dict(Q=64, biases=True, R=64, S=32,
                         dil=[1, 2, 4, 8, 16, 1, 2]), 150, [150, 77], None,
     False),
]


@pytest.mark.parametrize('name, kw, T, lengths, rows, audio', CASES,
                         ids=[c[0] for c in CASES])
def test_masked_loss_and_gradients_match_float64(hip_lib, name, kw, T, lengths,
                                                 rows, audio):
    B = len(lengths)
    assert max(lengths) == T and min(lengths) < T
    net = _model(B, seed=T, **kw)
    Q, Lc, gc = net.Q, kw.get('Lc'), kw.get('gc')
    dil = kw.get('dil', DIL)
    rng = np.random.default_rng(T + B)
    lc = rng.standard_normal((B, T, Lc)).astype(np.float32) if Lc else None
    ids = None if gc is None else np.arange(B) % gc
    if audio:
        a = rng.uniform(-1, 1, (B, T)).astype(np.float32)
        codes = O.mu_law_encode(a, Q)
        loss = net.loss(a, ids, local_condition_batch=lc, lengths=lengths)
    else:
        codes = _codes(B, T, Q, T)
        loss = net.loss_from_codes(torch.as_tensor(codes).cuda(), ids,
                                   local_condition_batch=lc,
                                   lengths=np.asarray(lengths))
    loss = float(loss)
    torch.cuda.synchronize()
    if rows is not None:
        _assert_rows(net, B, T, rows)
    else:
        assert net.blocked
    ref_loss, ref_g = masked_ref.loss_and_grads(
        lc_ref.model_tree(net), dil, codes, lengths, lc, gc_ids=ids,
        use_biases=net.use_biases, quantization_channels=Q,
        relu_masks=lc_ref.device_relu_masks(net, B, T))
    _assert_close(name, loss, lc_ref.model_tree(net, grads=True), ref_loss,
                  ref_g)
    # forward only: the same loss, nothing else
    fwd = float(net.loss_from_codes(torch.as_tensor(codes).cuda(), ids,
                                    backward=False, local_condition_batch=lc,
                                    lengths=lengths))
    assert abs(fwd - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    # padded rows of dlogits are exact zeros (the logits buffer holds them)
    ws = net._ws[(B, T, True)]
    net.loss_from_codes(torch.as_tensor(codes).cuda(), ids,
                        local_condition_batch=lc, lengths=lengths)
    # (the backward GEMMs read dlogits in place: still there after the step)
    dl = ws.logits.reshape(B, T, Q)
    for b, n in enumerate(lengths):
        assert int(torch.count_nonzero(dl[b, n:])) == 0
        assert float(dl[b, :n].abs().max()) > 0


def test_scalar_input_matches_the_clips_alone(hip_lib):
    """scalar_input (float audio in, loss()): the reference is assembled from
    the project's float64 oracle run on every clip alone and unpadded, with
    the device's ReLU decisions of that clip's rows."""
    cfg = cfg_with(TINY, batch_size=3, scalar_input=True,
                   initial_filter_width=4)
    B, T, lengths = 3, 70, [31, 70, 2]
    net, var = build_pair(cfg)
    audio = np.random.default_rng(2).uniform(-1, 1, (B, T)).astype(np.float32)
    loss = float(net.loss(audio, lengths=lengths))
    torch.cuda.synchronize()
    masks = lc_ref.device_relu_masks(net, B, T)
    one = cfg_with(cfg, batch_size=1)
    per = [O.loss_and_grads(one, var, audio[b:b + 1, :n], dtype=np.float64,
                            relu_masks=masked_ref.clip_masks(masks, b, n))
           for b, n in enumerate(lengths)]
    ref_loss, ref_g = masked_ref.assemble(per, lengths)
    _assert_close('scalar_input', loss, tree_to_numpy(net.gradients), ref_loss,
                  ref_g)


def test_lc_frames_with_offsets_and_context_match_the_clips_alone(hip_lib):
    """Learned upsampling of frames at nonzero offsets behind a context
    convolution: assembled from tests/lc_ctx_ref.py on every clip alone.  (No
    biases: an upsampler layer's one-float bias gradient cancels far below
    its layer's entries, tests/test_gpu_lc_context.py holds it to another
    scale; the bar here is the plain one.)"""
    B, T, Lc, scales, p, hop = 3, 500, 20, (4, 5), 2, 20
    lengths, offs = [237, 500, 1], [7, 131, 45]
    net = _model(B, Q=64, biases=False, gc=3, Lc=Lc, seed=4,
                 local_condition_upsample_scales=scales,
                 local_condition_context=p)
    rng = np.random.default_rng(8)
    F = (max(offs) + T - 1) // hop + 1
    frames = rng.standard_normal((B, F, Lc)).astype(np.float32)
    codes = _codes(B, T, 64, 3)
    ids = np.array([0, 2, 1])
    loss = float(net.loss_from_codes(
        torch.as_tensor(codes).cuda(), ids, local_condition_batch=frames,
        local_condition_offset=offs, lengths=lengths))
    torch.cuda.synchronize()
    masks = lc_ref.device_relu_masks(net, B, T)
    var = lc_ref.model_tree(net)
    per = [lc_ctx_ref.loss_and_grads(
        var, DIL, codes[b:b + 1, :n], frames[b:b + 1], offs[b:b + 1], scales,
        gc_ids=ids[b:b + 1], use_biases=False, quantization_channels=64,
        relu_masks=masked_ref.clip_masks(masks, b, n))
        for b, n in enumerate(lengths)]
    ref_loss, ref_g = masked_ref.assemble(per, lengths)
    grads = lc_ref.model_tree(net, grads=True)
    assert np.abs(dict(lc_ref.flatten(ref_g))['/lc_context/filter']).max() > 0
    _assert_close('lc_frames_ctx', loss, grads, ref_loss, ref_g)


# ---- identities ------------------------------------------------------------------
def _bucket(net):
    torch.cuda.synchronize()
    return net.grads.clone()


@pytest.mark.parametrize('Q', [256, 64])
def test_full_lengths_are_bitwise_the_unmasked_loss(hip_lib, Q):
    B, T = 3, 500
    net = _model(B, Q=Q, gc=2, Lc=16, seed=1)
    q = torch.as_tensor(_codes(B, T, Q, 1)).cuda()
    lc = np.random.default_rng(1).standard_normal((B, T, 16)).astype(np.float32)
    for l2 in (None, 1e-4):
        for _ in range(3):          # eager, recorded, replayed
            a = net.loss_from_codes(q, [0, 1, 0], l2, local_condition_batch=lc)
            ga = _bucket(net)
            b = net.loss_from_codes(q, [0, 1, 0], l2, local_condition_batch=lc,
                                    lengths=[T] * B)
            gb = _bucket(net)
            assert torch.equal(a, b), (float(a), float(b))
            assert torch.equal(ga, gb)
            assert float(ga.abs().max()) > 0


def _pad_variants(rng, codes, lc, lengths, Q):
    """The same real samples with the padding zero, random codes, random codes
    and random LC rows."""
    B, T = codes.shape
    out = []
    for fill_codes, fill_lc in ((False, False), (True, False), (True, True)):
        c, r = codes.copy(), lc.copy()
        for b, n in enumerate(lengths):
            c[b, n:] = rng.integers(0, Q, T - n) if fill_codes else 0
            r[b, n:] = rng.standard_normal(r[b, n:].shape) if fill_lc else 0
        out.append((c, r))
    return out


def test_padding_content_is_irrelevant(hip_lib):
    B, T, Q, Lc = 3, 400, 256, 12
    lengths = [400, 123, 1]
    net = _model(B, Q=Q, gc=3, Lc=Lc, seed=2)
    rng = np.random.default_rng(5)
    codes = _codes(B, T, Q, 6)
    lc = rng.standard_normal((B, T, Lc)).astype(np.float32)
    res = []
    for c, r in _pad_variants(rng, codes, lc, lengths, Q):
        loss = net.loss_from_codes(torch.as_tensor(c).cuda(), [0, 1, 2],
                                   local_condition_batch=r, lengths=lengths)
        res.append((loss.clone(), _bucket(net)))
    assert float(res[0][1].abs().max()) > 0
    for loss, g in res[1:]:
        assert torch.equal(loss, res[0][0])
        assert torch.equal(g, res[0][1])
    # without lengths the padding does matter (the test can see it)
    a = net.loss_from_codes(torch.as_tensor(codes).cuda(), [0, 1, 2],
                            local_condition_batch=lc)
    assert not torch.equal(a, res[0][0])


def test_padding_content_is_irrelevant_float_audio_and_frames(hip_lib):
    # scalar input: the padding's float audio
    cfg = cfg_with(TINY, batch_size=2, scalar_input=True,
                   initial_filter_width=4)
    net, _ = build_pair(cfg)
    rng = np.random.default_rng(3)
    T, lengths = 90, [90, 40]
    audio = rng.uniform(-1, 1, (2, T)).astype(np.float32)
    a2 = audio.copy()
    audio[1, 40:] = 0
    res = []
    for a in (audio, a2):
        loss = net.loss(a, lengths=lengths)
        res.append((loss.clone(), _bucket(net)))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    # frames: those behind the last frame the clip's rows (and its context)
    # reach
    B, T, Lc, scales, p, hop = 2, 300, 10, (4, 5), 1, 20
    lengths, offs = [300, 90], [25, 3]
    net = _model(B, Q=64, Lc=Lc, seed=6,
                 local_condition_upsample_scales=scales,
                 local_condition_context=p)
    F = (max(offs) + T - 1) // hop + 1
    frames = rng.standard_normal((B, F, Lc)).astype(np.float32)
    last = (offs[1] + lengths[1] - 1) // hop + p
    assert last + 1 < F
    f0, f1 = frames.copy(), frames.copy()
    f0[1, last + 1:] = 0
    q = torch.as_tensor(_codes(B, T, 64, 7)).cuda()
    res = []
    for f in (f0, f1):
        loss = net.loss_from_codes(q, local_condition_batch=f,
                                   local_condition_offset=offs,
                                   lengths=lengths)
        res.append((loss.clone(), _bucket(net)))
    assert float(res[0][1].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_last_real_row_has_no_target(hip_lib):
    """Only q[b][lengths[b]] (the first padding code, which the unmasked loss
    gives the last real sample as its target) changes: nothing moves."""
    B, T, Q = 3, 300, 256
    lengths = [300, 141, 1]
    net = _model(B, Q=Q, seed=3)
    codes = _codes(B, T, Q, 9)
    c2 = codes.copy()
    for b, n in enumerate(lengths):
        if n < T:
            c2[b, n] = (c2[b, n] + 1 + b) % Q
    assert (codes != c2).sum() == 2
    a = net.loss_from_codes(torch.as_tensor(codes).cuda(), lengths=lengths)
    ga = _bucket(net)
    b = net.loss_from_codes(torch.as_tensor(c2).cuda(), lengths=lengths)
    gb = _bucket(net)
    assert torch.equal(a, b) and torch.equal(ga, gb)


def test_launch_plan_replay_sees_new_lengths(hip_lib):
    """Consecutive calls on ONE workspace (eager, recorded, replayed, replayed)
    with different lengths: each matches its own reference."""
    B, T, Q = 3, 300, 256
    net = _model(B, Q=Q, gc=2, seed=5)
    assert net.use_launch_plans
    codes = _codes(B, T, Q, 4)
    q = torch.as_tensor(codes).cuda()
    ids = [1, 0, 1]
    ws = None
    for i, lengths in enumerate(([300, 141, 1], [17, 300, 299], [300, 2, 150],
                                 [1, 1, 300])):
        loss = float(net.loss_from_codes(q, ids, lengths=lengths))
        torch.cuda.synchronize()
        assert ws is None or ws is net._ws[(B, T, True)]
        ws = net._ws[(B, T, True)]
        ref_loss, ref_g = masked_ref.loss_and_grads(
            lc_ref.model_tree(net), DIL, codes, lengths, gc_ids=ids,
            use_biases=True, quantization_channels=Q,
            relu_masks=lc_ref.device_relu_masks(net, B, T))
        _assert_close('call %d' % i, loss, lc_ref.model_tree(net, grads=True),
                      ref_loss, ref_g)
    assert any(isinstance(p, list) for p in ws.plans.values())   # recorded


def test_loss_denominator_power_of_two(hip_lib):
    """The denominator enters as ONE float32 factor 1 / D on every dlogits
    entry and one division of the loss sum: doubling D halves a float32
    exactly (no subnormals here), so loss and bucket halve bit for bit."""
    B, T, Q = 3, 300, 256
    lengths = [300, 141, 1]
    net = _model(B, Q=Q, seed=3)
    q = torch.as_tensor(_codes(B, T, Q, 9)).cuda()
    a = net.loss_from_codes(q, lengths=lengths).clone()
    ga = _bucket(net)
    same = net.loss_from_codes(q, lengths=lengths,
                               loss_denominator=sum(lengths)).clone()
    assert torch.equal(a, same) and torch.equal(ga, _bucket(net))
    for d in (2 * sum(lengths), 512, 1024.0):
        b = net.loss_from_codes(q, lengths=lengths, loss_denominator=d).clone()
        gb = _bucket(net)
        k = d / float(sum(lengths))
        if d == 2 * sum(lengths):
            assert torch.equal(b * 2, a) and torch.equal(gb * 2, ga)
        else:
            assert abs(float(b) * k - float(a)) <= 1e-6 * float(a)
    h = net.loss_from_codes(q, lengths=lengths, loss_denominator=512).clone()
    gh = _bucket(net)
    d = net.loss_from_codes(q, lengths=lengths, loss_denominator=1024).clone()
    assert torch.equal(d * 2, h) and torch.equal(_bucket(net) * 2, gh)
    assert float(gh.abs().max()) > 0 and float(gh[gh != 0].abs().min()) > 1e-30


def test_masked_call_is_deterministic(hip_lib):
    B, T, Q = 4, 700, 256
    lengths = [700, 350, 699, 2]
    net = _model(B, Q=Q, gc=2, Lc=8, seed=7)
    q = torch.as_tensor(_codes(B, T, Q, 2)).cuda()
    lc = np.random.default_rng(2).standard_normal((B, T, 8)).astype(np.float32)
    res = []
    for _ in range(4):
        loss = net.loss_from_codes(q, [0, 1, 1, 0], local_condition_batch=lc,
                                   lengths=lengths)
        res.append((loss.clone(), _bucket(net)))
    for loss, g in res[1:]:
        assert torch.equal(loss, res[0][0]) and torch.equal(g, res[0][1])


# ---- train.py ----------------------------------------------------------------------
SMALL = {"filter_width": 2, "sample_rate": 16000,
         "dilations": [1, 2, 4, 8, 16, 32, 1, 2, 4, 8, 16, 32],
         "residual_channels": 32, "dilation_channels": 32,
         "quantization_channels": 256, "skip_channels": 64,
         "use_biases": True, "scalar_input": False,
         "initial_filter_width": 32, "residual_postproc": False}
SIZES = [3000, 1700, 2400, 900]


def _corpus(d):
    os.makedirs(d)
    for i, n in enumerate(SIZES):
        t = np.arange(n) / 16000.0
        a = 0.5 * np.sin(2 * np.pi * (220 + 60 * i) * t + 0.3)
        wavfile.write(os.path.join(d, 'clip%d.wav' % i), 16000,
                      (a * 32767).astype(np.int16))


def _train(tmp_path, name, extra, capsys):
    import train
    params = str(tmp_path / 'params.json')
    json.dump(SMALL, open(params, 'w'))
    data = str(tmp_path / 'corpus')
    if not os.path.exists(data):
        _corpus(data)
    logdir = str(tmp_path / name)
    assert train.main(['--data_dir', data, '--batch_size', '2',
                       '--wavenet_params', params, '--logdir', logdir,
                       '--num_steps', '6', '--checkpoint_every', '5',
                       '--silence_threshold', '0', '--learning_rate', '0.002']
                      + extra) == 0
    out = capsys.readouterr().out
    ev = [json.loads(l) for l in open(os.path.join(logdir, 'events.jsonl'))]
    return out, ev, logdir


def test_train_mask_padding(hip_lib, tmp_path, capsys):
    import train
    out, ev, logdir = _train(tmp_path, 'masked', ['--mask_padding', 'true'],
                             capsys)
    assert [e['step'] for e in ev] == list(range(6))
    assert all(np.isfinite(e['loss']) for e in ev)
    assert ev[-1]['loss'] < ev[0]['loss']
    # two whole clips per step: the real samples are the sum of two pieces'
    # sizes (the reader's own pieces: trimming moves the files' ends)
    from wavenet import AudioReader
    sizes = [p.shape[0] for p, _, _ in AudioReader(
        str(tmp_path / 'corpus'), None, sample_rate=16000, gc_enabled=False,
        sample_size=train.SAMPLE_SIZE, silence_threshold=0.0).iter_pieces()]
    assert len(sizes) == len(SIZES) and len(set(sizes)) == len(SIZES)
    pairs = {a + b for a in sizes for b in sizes}
    assert any(e['real_samples'] < 2 * max(sizes) for e in ev)
    for e in ev:
        assert e['real_samples'] in pairs, e
        assert re.search(r'^step %d - loss = \d+\.\d{3}, \(\d+\.\d{3} '
                         r'sec/step\), %d real samples$'
                         % (e['step'], e['real_samples']), out, re.M), e
    assert train.latest_checkpoint(logdir).endswith('model.ckpt-5')
    # off (and absent): the lines and the numbers of a run without the flag
    off, ev_off, _ = _train(tmp_path, 'off', ['--mask_padding', 'false'],
                            capsys)
    absent, ev_abs, _ = _train(tmp_path, 'absent', [], capsys)
    for e in ev_off:
        assert sorted(e) == ['loss', 'sec_per_step', 'step']
        assert re.search(r'^step %d - loss = \d+\.\d{3}, \(\d+\.\d{3} '
                         r'sec/step\)$' % e['step'], off, re.M), e
    assert 'real samples' not in off and 'real samples' not in absent
    assert ['%.3f' % e['loss'] for e in ev_off] == \
        ['%.3f' % e['loss'] for e in ev_abs]
    # and masking changes what is learned from
    assert ['%.3f' % e['loss'] for e in ev_off] != \
        ['%.3f' % e['loss'] for e in ev]
